"""smpq.memo on the host: the LRU, how the evaluation key is composed (with an injected digest
function standing in for the device fingerprints), and the epoch of smpq.batches.ResidentSet up to
the point where a device is needed (the rest: tests/test_gpu_memo.py)."""
import hashlib

import numpy as np
import pytest
import torch


def _digest(net, named):
    """One integer per tensor from its bytes alone (what smpq_fingerprint does on the device)."""
    return [int.from_bytes(hashlib.sha256(t.contiguous().numpy().tobytes()).digest()[:8], "little") for _, t in named]


@pytest.fixture(scope="module")
def net():
    import resnet
    torch.manual_seed(0)
    return resnet.resnet18(num_classes=10).eval()


def test_lru_evicts_least_recently_used_and_a_hit_refreshes():
    from smpq import memo
    lru = memo.LRU(2)
    lru.put("A", 1)
    lru.put("B", 2)
    assert lru.get("A") == 1          # A is now the most recent
    lru.put("C", 3)                   # B goes
    assert lru.get("B") is None and lru.get("A") == 1 and lru.get("C") == 3
    assert lru.evictions == 1 and len(lru.items) == 2
    lru.put("A", 4)                   # replacing keeps the size
    assert len(lru.items) == 2 and lru.get("A") == 4
    lru.drop(lambda k: k == "A")
    assert list(lru.items) == ["C"]


def test_entry_holds_host_numbers():
    from smpq import memo
    e = memo.Entry(torch.tensor([1.5, 2.0, 8.0, 1.0], dtype=torch.float64).tolist(), [torch.zeros(2, 5)])
    assert e.stats == (1.5, 2.0, 8.0, 1.0) and all(type(v) is float for v in e.stats)
    assert e.nbytes() == 40 and memo.Entry([0, 0, 0, 0]).nbytes() == 0


def test_compose_key_depends_on_order_names_dtype_shape_digest():
    from smpq import memo
    ts = [("a.weight", "torch.float32", (4, 3)), ("a.bias", "torch.float32", (4,))]
    base = memo.compose_key(ts, [11, 22], [("a", b"x")], ("tree",), (("k", 1),))
    assert base == memo.compose_key(list(ts), [11, 22], [("a", b"x")], ("tree",), (("k", 1),))
    others = [
        memo.compose_key(ts[::-1], [22, 11], [("a", b"x")], ("tree",), (("k", 1),)),             # order
        memo.compose_key([("b.weight",) + ts[0][1:], ts[1]], [11, 22], [("a", b"x")], ("tree",), (("k", 1),)),
        memo.compose_key([(ts[0][0], "torch.float16", (4, 3)), ts[1]], [11, 22], [("a", b"x")], ("tree",), (("k", 1),)),
        memo.compose_key([(ts[0][0], ts[0][1], (3, 4)), ts[1]], [11, 22], [("a", b"x")], ("tree",), (("k", 1),)),
        memo.compose_key(ts, [11, 23], [("a", b"x")], ("tree",), (("k", 1),)),                   # content
        memo.compose_key(ts, [11, 22], [("a", b"y")], ("tree",), (("k", 1),)),                   # bits mirror
        memo.compose_key(ts, [11, 22], [("a", b"x")], ("tree2",), (("k", 1),)),                  # structure
        memo.compose_key(ts, [11, 22], [("a", b"x")], ("tree",), (("k", 2),)),                   # a setting
        memo.compose_key(ts[:1], [11], [("a", b"x")], ("tree",), (("k", 1),)),                   # a tensor less
    ]
    assert len(set(others + [base])) == len(others) + 1


def test_state_key_is_content_only(net):
    """The same state in another model object, at other addresses, gives the same key; the key
    covers fc and every BN buffer; a _bits_host that disagrees with qbits changes it."""
    import resnet
    from smpq import memo
    k0 = memo.state_key(net, digest=_digest)
    assert k0 == memo.state_key(net, digest=_digest)
    torch.manual_seed(123)
    other = resnet.resnet18(num_classes=10).eval()
    assert memo.state_key(other, digest=_digest) != k0
    other.load_state_dict({k: v.clone() for k, v in net.state_dict().items()})
    assert {t.data_ptr() for t in other.state_dict().values()}.isdisjoint(
        {t.data_ptr() for t in net.state_dict().values()})
    assert memo.state_key(other, digest=_digest) == k0
    for name in ("fc.weight", "fc.bias", "bn1.running_var", "layer3.1.bn2.running_mean",
                 "layer4.0.downsample.1.num_batches_tracked", "layer2.0.conv1.qstep", "layer2.0.conv1.qbits",
                 "conv1.weight"):
        t = other.state_dict()[name]
        keep = t.clone()
        t.view(-1)[0] += 1
        assert memo.state_key(other, digest=_digest) != k0, name
        t.copy_(keep)
        assert memo.state_key(other, digest=_digest) == k0, name
    conv = other.layer1[0].conv2
    conv._bits_host[3] = 4  # qbits still says 0: the packing kind is chosen from this mirror
    assert memo.state_key(other, digest=_digest) != k0
    conv._bits_host[3] = 0
    assert memo.state_key(other, digest=_digest) == k0
    assert conv._bits_host.dtype == np.int16


def test_state_key_sees_structure(net):
    import resnet
    from smpq import memo
    k0 = memo.state_key(net, digest=_digest)
    torch.manual_seed(0)
    twin = resnet.resnet18(num_classes=10).eval()
    assert memo.state_key(twin, digest=_digest) == k0
    twin.layer2[0].conv1.stride = (1, 1)  # same tensors, other geometry
    assert memo.state_key(twin, digest=_digest) != k0
    twin.layer2[0].conv1.stride = (2, 2)
    twin.relu = torch.nn.ReLU6()          # same tensors, other module type
    assert memo.state_key(twin, digest=_digest) != k0


def test_state_key_changes_with_every_setting(net, monkeypatch):
    from smpq import engine, memo, ops
    k0 = memo.state_key(net, digest=_digest)
    names = [n for n, _ in memo.settings()]
    for must in ("range_mode", "act_limbs", "headroom", "chunk", "fused_stem", "concurrent_ds", "streams", "kmajor",
                 "pair_1x1", "fuse_ds", "fuse_ds_max_cin", "pair_stage_entry"):
        assert must in names
    seen = {k0}

    def moved():
        k = memo.state_key(net, digest=_digest)
        assert k not in seen
        seen.add(k)
    monkeypatch.setattr(engine, "_MODE", ["dynamic" if engine.get_range_mode() == "static" else "static"])
    moved()
    monkeypatch.undo()
    monkeypatch.setattr(ops, "_ACT_LIMBS", [2 if ops.get_act_limbs() != 2 else 3])
    moved()
    monkeypatch.undo()
    monkeypatch.setattr(engine, "HEADROOM", engine.HEADROOM * 2)
    moved()
    monkeypatch.undo()
    for owner, knob in ((engine, "FUSED_STEM"), (engine, "CONCURRENT_DS"), (ops, "KMAJOR"), (engine, "PAIR_1X1"),
                        (engine, "FUSE_DS"), (engine, "PAIR_STAGE_ENTRY"), (engine, "USE_GRAPH")):
        monkeypatch.setattr(owner, knob, [not getattr(owner, knob)[0]])
        moved()
        monkeypatch.undo()
    for knob in ("CHUNK", "STREAMS", "FUSE_DS_MAX_CIN"):
        monkeypatch.setattr(engine, knob, [getattr(engine, knob)[0] + 1])
        moved()
        monkeypatch.undo()
    assert memo.state_key(net, digest=_digest) == k0


def test_switches_and_report():
    from smpq import memo, stats
    was = memo.enabled()
    try:
        memo.clear()
        memo.enable(entries=3)
        assert memo.enabled() and memo.report()["capacity"] == 3
        memo.disable()
        assert not memo.enabled()
        r = memo.report()
        for k in ("hits", "misses", "bypasses", "entries", "evictions", "prob_bytes"):
            assert r[k] == 0, k
        assert "memo_hits" in stats and "memo_misses" in stats
    finally:
        memo.enable(entries=4) if was else (memo.enable(entries=4), memo.disable())


def test_memo_is_off_by_default_and_a_plain_loader_is_a_bypass(net):
    """The switch follows SMPQ_EVAL_MEMO as read at import (unset: off, and functions._run_eval
    never consults the memo). A list loader or a CPU device is a counted bypass before any key is
    computed."""
    import os

    import functions
    from smpq import memo
    assert functions.memo is memo
    assert memo.enabled() == (os.environ.get("SMPQ_EVAL_MEMO", "0") == "1")
    memo.clear()
    assert memo.begin(net, torch.device("cpu"), [(torch.zeros(1), torch.zeros(1))], True) is None
    assert memo.report()["bypasses"] == 1 and memo.report()["entries"] == 0
    memo.clear()


def test_resident_set_epoch_moves_on_invalidate():
    """The epoch on the host side: it starts at 0, is reported, and invalidate() moves it (that a
    completed filling pass moves it needs a device: tests/test_gpu_memo.py)."""
    from smpq.batches import ResidentSet
    rs = ResidentSet([(torch.zeros(2, 3, 8, 8), torch.zeros(2, dtype=torch.long))])
    assert rs.report()["epoch"] == 0
    rs.invalidate()
    assert rs.report()["epoch"] == 1
    rs.invalidate()
    assert rs.report()["epoch"] == 2 and not rs.report()["resident"]
