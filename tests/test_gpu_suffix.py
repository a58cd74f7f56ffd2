"""smpq.suffix on the GPU: sensitivity tables whose trials forward only the blocks from the patched
conv on (suffix=True) against the same tables through the replay route (suffix=False), bit for bit;
that a resumed forward really is shorter; the byte budget; what a table leaves behind; the failure
path. Unless a test says otherwise every block is resumed (suffix.MIN_SKIPPED = 0), block 0 too."""
import gc

import numpy as np
import pytest
import torch

from test_gpu import build_model
from test_gpu_sensitivity import _batches, _operands, knobs  # noqa: F401  (knobs: a fixture)

pytestmark = pytest.mark.gpu

ZERO = {"calibrations": 0, "graph_captures": 0, "repack": 0}
CAL = {"resnet18": "r18_u8_cal", "resnet50": "r50_mixed_cal"}
R18_CHANNELS = {1: [0, 63], 8: [5, 127], 16: [0, 511]}
R50_CHANNELS = {4: [0], 5: [63], 6: [255], 24: [0], 40: [255], 46: [511], 47: [0], 48: [2047]}


@pytest.fixture
def every_block(monkeypatch):
    from smpq import suffix
    monkeypatch.setattr(suffix, "MIN_SKIPPED", [0.0])


def _set(graph, limbs):
    from smpq import engine, ops
    engine.USE_GRAPH[0] = graph
    ops.set_act_limbs(limbs)


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _counts(rep):
    return {k: v for k, v in rep.items() if k not in ("suffix", "baseline_s", "trials_s")}


_OFF = {}


def _delta_off(gpu, arch, graph, limbs, sizes, channels, bits):
    """The replay route's table of one case, computed once and shared (never written to)."""
    key = (arch, graph, limbs, sizes, repr(channels), bits)
    if key not in _OFF:
        _set(graph, limbs)
        net = build_model(gpu, arch, None, CAL[arch])
        _OFF[key] = _delta(net, _mixed_batches(gpu, sizes), channels, bits, suffix=False)
    return _OFF[key]


def _mixed_batches(gpu, sizes):
    """One batch per entry of ``sizes``, cut from _batches' images and labels of the largest size."""
    _, dev = _batches(gpu, n=max(sizes), count=len(sizes))
    return [(x[:n].contiguous(), y[:n].contiguous()) for (x, y), n in zip(dev, sizes)]


def _delta(net, batches, channels, bits, **kw):
    from smpq import sensitivity
    return sensitivity.delta_loss_table(net, batches, bits=bits, lnums=sorted(channels), channels=channels, **kw)


def _assert_same_delta_tables(on, off):
    assert on.bits == off.bits and on.lnum.tolist() == off.lnum.tolist() and on.cnum.tolist() == off.cnum.tolist()
    for bit in off.bits:
        assert np.isfinite(off.stats[bit]).all()
        assert _same_bits(on.stats[bit], off.stats[bit]), (bit, on.stats[bit], off.stats[bit])
        assert _same_bits(on.delta[bit], off.delta[bit]), bit
    assert _same_bits(on.base_loss, off.base_loss) and _same_bits(on.eval_loss, off.eval_loss)
    ron, roff = on.report(), off.report()
    assert _counts(ron) == _counts(roff), (ron, roff)
    assert ron["patched"] == ron["trials"] and not ron["slow"] and not ron["constant"], ron
    assert ron["during_trials"] == ZERO and roff["during_trials"] == ZERO
    assert roff["suffix"] == {}


def _assert_all_resumed(rep, blocks, batches):
    sfx = rep["suffix"]
    assert [b["block"] for b in sfx["blocks"]] == blocks, sfx
    for b in sfx["blocks"]:
        assert b["used"] and b["resumable"] and b["self_check"] is True, b
        assert b["kept"] == batches and b["full"] == 0 and b["bytes"] > 0 and b["prefix_pass_s"] > 0, b
    assert sfx["resumed_forwards"] == (len(blocks) + rep["trials"]) * batches and sfx["resumed_conv_launches"] > 0


# ---- delta-loss tables, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("graph,limbs", [(True, 3), (False, 3), (True, 2)])
def test_delta_loss_table_equals_the_replay_route_resnet18(gpu, knobs, every_block, graph, limbs):  # noqa: F811
    bits = (8, 4, 2)
    off = _delta_off(gpu, "resnet18", graph, limbs, (8, 8), R18_CHANNELS, bits)
    _set(graph, limbs)
    net = build_model(gpu, "resnet18", None, CAL["resnet18"])
    on = _delta(net, _mixed_batches(gpu, (8, 8)), R18_CHANNELS, bits, suffix=True)
    _assert_same_delta_tables(on, off)
    _assert_all_resumed(on.report(), [0, 3, 7], 2)
    assert [b["name"] for b in on.report()["suffix"]["blocks"]] == ["layer1.0", "layer2.1", "layer4.1"]


@pytest.mark.parametrize("graph,limbs", [(True, 3), (False, 3), (True, 2)])
def test_delta_loss_table_equals_the_replay_route_resnet50(gpu, knobs, every_block, graph, limbs):  # noqa: F811
    # layer 1 after the stage entry (block 1), a stride-2 stage entry's neighbourhood (lnum 24: the
    # last conv before layer3.0; lnum 40: layer4.0's first), all three convs of the last block
    off = _delta_off(gpu, "resnet50", graph, limbs, (4, 4), R50_CHANNELS, (4,))
    _set(graph, limbs)
    net = build_model(gpu, "resnet50", None, CAL["resnet50"])
    on = _delta(net, _mixed_batches(gpu, (4, 4)), R50_CHANNELS, (4,), suffix=True)
    _assert_same_delta_tables(on, off)
    _assert_all_resumed(on.report(), [1, 7, 13, 15], 2)


def test_uneven_slices_and_two_batch_shapes(gpu, knobs, every_block):  # noqa: F811
    # a batch of 5 runs as slices of 3 + 2, the batch of 8 as 4 + 4: two shapes in one table
    from smpq import suffix
    assert suffix.slices(5) == [(0, 3), (3, 5)] and suffix.slices(8) == [(0, 4), (4, 8)]
    bits = (8, 4, 2)
    off = _delta_off(gpu, "resnet18", True, 3, (5, 8), R18_CHANNELS, bits)
    _set(True, 3)
    net = build_model(gpu, "resnet18", None, CAL["resnet18"])
    on = _delta(net, _mixed_batches(gpu, (5, 8)), R18_CHANNELS, bits, suffix=True)
    _assert_same_delta_tables(on, off)
    _assert_all_resumed(on.report(), [0, 3, 7], 2)


def test_default_cut_keeps_the_replay_for_shallow_blocks(gpu, knobs):  # noqa: F811
    from smpq import prefix, suffix
    bits = (8, 4, 2)
    off = _delta_off(gpu, "resnet18", True, 3, (8, 8), R18_CHANNELS, bits)
    _set(True, 3)
    net = build_model(gpu, "resnet18", None, CAL["resnet18"])
    first = suffix.first_block(net)
    assert 0 < first <= len(prefix.block_names(net))
    on = _delta(net, _mixed_batches(gpu, (8, 8)), R18_CHANNELS, bits, suffix=True)
    _assert_same_delta_tables(on, off)
    sfx = on.report()["suffix"]
    assert sfx["first_block"] == first and [b["block"] for b in sfx["blocks"]] == [0, 3, 7]
    for b in sfx["blocks"]:
        assert b["used"] == (b["block"] >= first)
        assert (b["kept"], b["self_check"]) == ((2, True) if b["used"] else (0, None)), b


def test_switch_off_is_the_parents_table(gpu, knobs):  # noqa: F811
    off = _delta_off(gpu, "resnet18", True, 3, (8, 8), R18_CHANNELS, (8, 4, 2))
    _set(True, 3)
    net = build_model(gpu, "resnet18", None, CAL["resnet18"])
    default = _delta(net, _mixed_batches(gpu, (8, 8)), R18_CHANNELS, (8, 4, 2))  # SMPQ_TRIAL_SUFFIX unset: off
    _assert_same_delta_tables(default, off)
    assert default.report()["suffix"] == {}


# ---- semilayer tables, bit for bit ----------------------------------------------------------------------
SEMILAYERS = {"resnet18": [(8, range(0, 128, 2), 4), (16, range(0, 512, 2), 4)],
              "resnet50": [(24, range(0, 512, 2), 4), (48, range(0, 2048, 2), 4)]}


@pytest.mark.parametrize("with_reference", [True, False])
@pytest.mark.parametrize("arch,n,blocks", [("resnet18", 8, [3, 7]), ("resnet50", 4, [7, 15])])
def test_semilayer_table_equals_the_replay_route(gpu, knobs, every_block, arch, n, blocks, with_reference):  # noqa: F811
    import functions
    from smpq import sensitivity
    _set(True, 3)
    _, dev = _batches(gpu, n=n)
    tables = {}
    refs = None
    for sfx in (False, True):
        net = build_model(gpu, arch, None, CAL[arch])
        if with_reference:  # (on both models, so that both tables start from the same caches)
            outs = [p.clone() for p in functions.evaluate_acc_loss_softmax(net, gpu, dev)[2]]
            refs = outs if refs is None else refs
        tables[sfx] = sensitivity.semilayer_table(net, dev, SEMILAYERS[arch], reference_outputs=refs, suffix=sfx)
    on, off = tables[True], tables[False]
    assert np.isfinite(off.stats).all() and np.isfinite(off.kl_stats).all() and (off.kl > 0).all()
    for name in ("stats", "kl_stats", "loss", "acc", "kl"):
        assert _same_bits(getattr(on, name), getattr(off, name)), (name, getattr(on, name), getattr(off, name))
    assert _same_bits(on.base_loss, off.base_loss) and _same_bits(on.eval_loss, off.eval_loss)
    ron, roff = on.report(), off.report()
    assert _counts(ron) == _counts(roff) and ron["patched"] == 2 and not ron["slow"], (ron, roff)
    assert ron["during_trials"] == ZERO and roff["during_trials"] == ZERO and roff["suffix"] == {}
    _assert_all_resumed(ron, blocks, 2)


# ---- it really is shorter --------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,n,lnum", [("resnet18", 8, 16), ("resnet50", 4, 48)])
def test_a_resumed_forward_runs_only_its_blocks_convs(gpu, knobs, arch, n, lnum):  # noqa: F811
    from smpq import assignments, engine, prefix, sensitivity, stats, suffix
    from smpq.qconv import QConv2d
    _set(True, 3)
    _, dev = _batches(gpu, n=n)
    net = build_model(gpu, arch, None, CAL[arch])
    conv = assignments.conv_for_lnum(net, lnum)
    table = sensitivity.delta_loss_table(net, dev, bits=(4,), lnums=[lnum], channels=[0], suffix=True)  # the default cut
    j = suffix.block_of(net, conv)
    blocks = assignments.blocks_of(net)
    assert j == len(blocks) - 1
    (row,) = table.report()["suffix"]["blocks"]
    assert row["name"] == prefix.block_names(net)[j] and row["used"] and row["resumable"] and row["self_check"] is True
    assert (row["kept"], row["full"]) == (2, 0) and row["bytes"] == 2 * suffix.kept_bytes(net, dev[0][0], j)
    assert table.report()["during_trials"] == ZERO
    # from the module tree: every conv of the blocks from j on, once per slice
    per_slice = sum(isinstance(m, QConv2d) for b in blocks[j:] for m in b.modules())
    assert per_slice == (3 if arch == "resnet50" else 2)
    expected = per_slice * len(suffix.slices(n))
    assert table.report()["suffix"]["resumed_conv_launches"] == expected * table.report()["suffix"]["resumed_forwards"]
    cal = engine.model_state(net).ranges
    x = dev[0][0]
    with torch.no_grad():
        c0 = stats["hip_conv"]
        kept = suffix.fill(net, x, cal, j)
        c1 = stats["hip_conv"]
        logits, flags = suffix.resume(net, kept, cal, j)
        c2 = stats["hip_conv"]
        full, fflags = engine._static_eager(net, x, cal)
        c3 = stats["hip_conv"]
    print("%s block %d: %d conv launches resumed, %d in the prefix pass, %d in a full eager forward"
          % (arch, j, c2 - c1, c1 - c0, c3 - c2))
    assert c2 - c1 == expected
    assert (c2 - c1) + (c1 - c0) == c3 - c2 and c3 - c2 >= 5 * expected
    assert kept.nbytes == suffix.kept_bytes(net, x, j) and [p[:2] for p in kept.parts] == suffix.slices(n)
    assert torch.equal(logits, full) and flags.tolist() == [0, 0] and fflags.tolist() == [0, 0]


# ---- the byte budget --------------------------------------------------------------------------------------
@pytest.mark.parametrize("batches_kept", [0, 1])
def test_budget(gpu, knobs, every_block, batches_kept):  # noqa: F811
    from smpq import suffix
    bits = (8, 4, 2)
    off = _delta_off(gpu, "resnet18", True, 3, (8, 8), R18_CHANNELS, bits)
    _set(True, 3)
    net = build_model(gpu, "resnet18", None, CAL["resnet18"])
    dev = _mixed_batches(gpu, (8, 8))
    one = suffix.kept_bytes(net, dev[0][0], 7)  # the deepest block's batch: the smallest of the three
    assert one == 3 * 8 * 7 * 7 * 512
    on = _delta(net, dev, R18_CHANNELS, bits, suffix=True, suffix_bytes=one * batches_kept)
    _assert_same_delta_tables(on, off)
    rows = {b["block"]: b for b in on.report()["suffix"]["blocks"]}
    assert sorted(rows) == [0, 3, 7]
    for j, b in rows.items():
        kept = batches_kept if j == 7 else 0  # (the shallower blocks' batches are larger than the budget)
        assert (b["kept"], b["full"], b["bytes"], b["resumable"]) == (kept, 2 - kept, one * kept, True), b
        assert b["self_check"] is (True if kept else None)
    # the self-check and every trial of block 7 resumed the first batch only
    assert on.report()["suffix"]["resumed_forwards"] == batches_kept * (1 + 2 * 3)


# ---- what a table leaves behind -----------------------------------------------------------------------------
def test_leaves_nothing_behind(gpu, knobs, every_block):  # noqa: F811
    from smpq import engine, sensitivity
    _set(True, 3)
    _, dev = _batches(gpu)
    net = build_model(gpu, "resnet18", None, CAL["resnet18"])
    sensitivity.delta_loss_table(net, dev, bits=(8, 2), lnums=[2, 15], channels=[3, 60], suffix=False)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ops_before = _operands(net)
    assert len(ops_before) >= 17
    copies = {k: [t.clone() for t in ts] for k, ts in ops_before.items()}
    st = engine.model_state(net)
    ranges, entries = st.ranges, dict(st.graphs.entries)
    assert ranges is not None and entries
    gc.collect()
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    table = sensitivity.delta_loss_table(net, dev, bits=(8, 2), lnums=[2, 15], channels=[3, 60], suffix=True)
    rep = table.report()
    assert rep["patched"] == 8 and rep["during_trials"] == ZERO
    assert rep["baseline"] == {"calibrations": 1, "graph_captures": 0, "repack": 0}, rep
    _assert_all_resumed(rep, [0, 7], 2)
    del table
    gc.collect()
    torch.cuda.synchronize()
    after = torch.cuda.memory_allocated()
    print("memory_allocated before %d after %d" % (before, after))
    assert abs(after - before) <= 8 * 1000 * 4  # within one batch's logits
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    now = _operands(net)
    assert now.keys() == ops_before.keys()
    for k, ts in now.items():
        for t, t0, c in zip(ts, ops_before[k], copies[k]):
            assert t is t0 and torch.equal(t, c), k
    st = engine.model_state(net)
    assert st.ranges is ranges
    assert len(st.graphs.entries) == len(entries) and all(st.graphs.entries[k] is v for k, v in entries.items())


# ---- the failure path -----------------------------------------------------------------------------------------
def test_a_failing_resume_restores_releases_and_invalidates(gpu, knobs, every_block, monkeypatch):  # noqa: F811
    from smpq import assignments, sensitivity, suffix
    _set(True, 3)
    _, dev = _batches(gpu)
    net = build_model(gpu, "resnet18", None, CAL["resnet18"])
    sensitivity.delta_loss_table(net, dev, bits=(4,), lnums=[16], channels=[0], suffix=False)  # operands, graphs
    conv = assignments.conv_for_lnum(net, 16)
    pristine = {k: [t.clone() for t in ts] for k, ts in _operands(net).items()}
    gen = conv._content_gen
    real_resume, real_release = suffix.resume, suffix.Store.release
    calls, stores = [], []

    def resume(*a, **kw):
        calls.append(1)
        if len(calls) == 4:  # 1, 2: the block's self-check; 3: the first trial's first batch; 4: its second
            raise RuntimeError("injected")
        return real_resume(*a, **kw)

    def release(self):
        stores.append(self)
        return real_release(self)

    monkeypatch.setattr(suffix, "resume", resume)
    monkeypatch.setattr(suffix.Store, "release", release)
    with pytest.raises(RuntimeError, match="injected"):
        sensitivity.delta_loss_table(net, dev, bits=(4,), lnums=[16], channels=[0, 5], suffix=True)
    assert len(calls) == 4
    torch.cuda.synchronize()
    now = _operands(net)
    assert now.keys() == pristine.keys()
    for k, ts in now.items():  # the row restore ran
        for t, c in zip(ts, pristine[k]):
            assert torch.equal(t.view(torch.int8), c.view(torch.int8)), k
    assert conv._content_gen == gen + 1  # and the conv is marked for repacking
    assert stores and all(s is stores[0] for s in stores)
    assert stores[0].entries == [] and stores[0].block is None and stores[0].bytes == 0
    # the model still evaluates, and a later table on it is the replay route's
    monkeypatch.setattr(suffix, "resume", real_resume)
    again = sensitivity.delta_loss_table(net, dev, bits=(4,), lnums=[16], channels=[0, 5], suffix=True)
    ref = sensitivity.delta_loss_table(net, dev, bits=(4,), lnums=[16], channels=[0, 5], suffix=False)
    assert _same_bits(again.stats[4], ref.stats[4]) and np.isfinite(ref.stats[4]).all()
