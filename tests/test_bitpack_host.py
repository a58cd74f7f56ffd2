"""Format smpq-packed/1 on the host (include/smpq.h; smpq.ops bitpack_*, smpq.checkpoint snapshot /
restore_ / save_packed / load_packed / packed_report): the native host twins against an
independent numpy packer, bit for bit, and the state round trips on a mixed ResNet-18. CPU only."""
import numpy as np
import pytest
import torch

import bitpack_ref as ref
from bitpack_ref import u32
from test_checkpoint import _mixed_net


def _host_pack(w, qbits, step):
    from smpq import ops
    mode, base, words = ops.bitpack_plan(w, qbits, step)
    off = ops.bitpack_offsets(words)
    payload = ops.bitpack_store(w, mode, base, step, off)
    return mode, base, words, off, payload


def _check_against_numpy(w, qbits, step):
    """plan / store / load of the host twins == the numpy packer, and back to the input bitwise."""
    from smpq import ops
    cout, k = w.shape
    mode, base, words, off, payload = _host_pack(w, qbits, step)
    n_mode, n_base, n_off, n_payload = ref.np_pack(w.numpy(), qbits.numpy(), step.numpy())
    assert mode.dtype == torch.int8 and base.dtype == torch.int32 and off.dtype == torch.int64
    assert np.array_equal(mode.numpy(), n_mode)
    assert np.array_equal(base.numpy(), n_base)
    assert np.array_equal(off.numpy(), n_off) and np.array_equal(np.diff(n_off), words.numpy())
    assert payload.dtype == torch.int8 and payload.numel() == 4 * n_off[-1]
    assert np.array_equal(ref.payload_words(payload), n_payload)
    back = ops.bitpack_load(payload, cout, k, mode, base, step, off)
    assert np.array_equal(u32(back.numpy()), u32(w.numpy()))
    assert np.array_equal(u32(ref.np_unpack(n_payload, cout, k, n_mode, n_base, step.numpy(), n_off)), u32(w.numpy()))
    return mode.numpy()


@pytest.mark.parametrize("k", ref.KS)
def test_host_twins_match_numpy_packer(built_lib, k):
    w, qbits, step = ref.quantized_tensor(k)
    w0 = w.clone()
    mode = _check_against_numpy(w, qbits, step)
    assert torch.equal(w, w0)  # plan / store read only
    # the cap: every quantized channel packs at its recorded width, no raw fallback among them
    q = qbits.numpy()
    assert np.array_equal(mode, q), (mode, q)
    assert (q > 0).sum() == 10 and (q == 0).sum() == 2
    # packed channels cost ceil(k * b / 32) words, raw ones k
    _, _, words, _, _ = _host_pack(w, qbits, step)
    assert words.tolist() == [k if b == 0 else -(-k * int(b) // 32) for b in q]


def test_forced_fallbacks_go_raw_and_round_trip(built_lib):
    w, qbits, step, raw = ref.fallback_tensor()
    mode = _check_against_numpy(w, qbits, step)
    for c, name in enumerate(ref.FALLBACK_NAMES):
        assert (mode[c] == 0) == raw[c], name
    assert mode[0] == 4 and mode[10] == 8
    # the -0.0 survives
    from smpq import ops
    m, b, words = ops.bitpack_plan(w, qbits, step)
    off = ops.bitpack_offsets(words)
    back = ops.bitpack_load(ops.bitpack_store(w, m, b, step, off), w.shape[0], w.shape[1], m, b, step, off)
    assert u32(back.numpy()[1, 4:5])[0] == 0x80000000


def test_quantizer_negative_zero_goes_raw(built_lib):
    """A zero point of 0 makes the quantizer itself write -0.0 (functions.py:41: rint(t / s + 0) - 0
    keeps the sign of a small negative t). Code 0 unpacks to +0.0, so that channel stays raw; the
    same channel with +0.0 packs in one bit per weight."""
    w, qbits, step = ref.zero_point_zero_channel()
    mode = _check_against_numpy(w, qbits, step)
    assert mode.tolist() == [0, 1]


def test_bitpack_ops_reject_bad_operands(built_lib):
    from smpq import ops
    w, qbits, step = ref.quantized_tensor(9)
    with pytest.raises(ValueError):
        ops.bitpack_plan(w.double(), qbits, step)
    with pytest.raises(ValueError):
        ops.bitpack_plan(w, qbits[:-1], step)
    with pytest.raises(ValueError):
        ops.bitpack_plan(w.t(), qbits, step)
    mode, base, words, off, payload = _host_pack(w, qbits, step)
    with pytest.raises(ValueError):
        ops.bitpack_load(payload[:-4], w.shape[0], w.shape[1], mode, base, step, off[:-1])
    with pytest.raises(ValueError):
        ops.bitpack_load(payload, w.shape[0], w.shape[1], mode, base.long(), step, off)


# ---- state round trips ---------------------------------------------------------------------------
def _bits_equal(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _assert_same_state(net, sd0, bits0):
    from smpq import checkpoint
    sd = net.state_dict()
    assert list(sd) == list(sd0)
    for k in sd0:
        assert _bits_equal(sd[k], sd0[k]), k
    assert checkpoint.bit_assignment(net) == bits0


def _expected_packed_bytes(conv, mode):
    k = conv.weight[0].numel()
    q = conv.qbits.numpy().astype(np.int64)
    assert ((mode == 0) | (mode == q)).all()
    return int(4 * np.where(mode == 0, k, -(-k * q // 32)).sum())


def test_snapshot_restore_round_trip(built_lib):
    from smpq import checkpoint
    from smpq.assignments import addressable_convs
    from smpq.quant import quantize_layer_
    net = _mixed_net(built_lib)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}
    bits0 = checkpoint.bit_assignment(net)
    hosts0 = [c._bits_host.copy() for c in addressable_convs(net)]
    st = checkpoint.snapshot(net)
    _assert_same_state(net, sd0, bits0)  # taking a snapshot changes nothing
    assert all(pc.device.type == "cpu" for pc in st.convs.values())
    # the report: the payload follows the ceil(k * b / 32) rule; the numpy planner agrees on which
    # channels pack
    rep = checkpoint.packed_report(st)
    named = dict(net.named_modules())
    for name, pc in st.convs.items():
        conv, row = named[name], rep["convs"][name]
        mode = pc.mode.numpy().astype(np.int64)
        n_mode = ref.np_pack(conv.weight.detach().reshape(pc.cout, -1).numpy(), conv.qbits.numpy(),
                             conv.qstep.numpy())[0]
        assert np.array_equal(mode, n_mode), name
        assert row["packed_bytes"] == _expected_packed_bytes(conv, mode) == pc.payload.numel(), name
        assert row["fp32_bytes"] == 4 * conv.weight.numel()
        assert row["packed_channels"] == int((mode > 0).sum()) and row["raw_channels"] == int((mode == 0).sum())
    tot = rep["total"]
    assert tot["packed_channels"] > 0 and tot["raw_channels"] > 0
    assert tot["packed_bytes"] == sum(r["packed_bytes"] for r in rep["convs"].values()) < tot["fp32_bytes"]
    # the search moves on: more channels quantized, BN and fc touched; then the rollback
    convs = addressable_convs(net)
    gens = [(c._meta_gen, c._content_gen) for c in convs]
    quantize_layer_(convs[2], np.full(convs[2].out_channels, 2))
    quantize_layer_(convs[9], np.full(convs[9].out_channels, 4))
    with torch.no_grad():
        net.bn1.running_mean.add_(1.0)
        net.fc.weight.zero_()
    assert checkpoint.bit_assignment(net) != bits0
    assert checkpoint.restore_(net, st) is net
    _assert_same_state(net, sd0, bits0)
    for c, h, g in zip(convs, hosts0, gens):
        assert np.array_equal(c._bits_host, h) and c._bits_host.dtype == h.dtype
        assert c._meta_gen > g[0] and c._content_gen > g[1]  # the engine's caches are keyed on these
    # the state is reusable: a second rollback gives the same bits
    quantize_layer_(convs[0], np.full(convs[0].out_channels, 2))
    checkpoint.restore_(net, st)
    _assert_same_state(net, sd0, bits0)


def test_restore_rejects_another_net(built_lib):
    import resnet
    from smpq import checkpoint
    st = checkpoint.snapshot(_mixed_net(built_lib))
    with pytest.raises(ValueError):
        checkpoint.restore_(resnet.resnet34(), st)


def test_save_load_packed_round_trip(built_lib, tmp_path):
    import os
    import resnet
    from smpq import checkpoint
    from smpq.assignments import addressable_convs
    net = _mixed_net(built_lib)
    p, plain = tmp_path / "net.smpq", tmp_path / "net.pth"
    checkpoint.save_packed(net, p)
    torch.save(net.state_dict(), plain)
    assert not os.path.exists(checkpoint.sidecar_path(p))
    doc = torch.load(p, weights_only=True)
    assert doc["format"] == "smpq-packed/1"
    assert all(isinstance(v, torch.Tensor) for k, v in doc.items() if k != "format")
    assert os.path.getsize(p) < os.path.getsize(plain)
    torch.manual_seed(5)
    net2 = resnet.resnet18()
    got = checkpoint.load_packed(net2, p)
    _assert_same_state(net2, net.state_dict(), checkpoint.bit_assignment(net))
    assert got == checkpoint.bit_assignment(net)
    for a, b in zip(addressable_convs(net), addressable_convs(net2)):
        assert np.array_equal(a._bits_host, b._bits_host)


def _corrupt(doc, what):
    key = "conv/layer1.0.conv1/"
    if what == "truncated payload":
        doc[key + "payload"] = doc[key + "payload"][:-4].clone()
    elif what == "mode 9":
        doc[key + "mode"][3] = 9
    elif what == "non-monotone word_off":
        off = doc[key + "word_off"]
        off[5], off[6] = off[6].item(), off[5].item()
    elif what == "word_off not from 0":
        doc[key + "word_off"] += 1
    elif what == "format tag":
        doc["format"] = "smpq-packed/2"
    elif what == "another cout":
        doc[key + "shape"][0] += 1
    elif what == "mode against the payload":
        # a raw channel declared packed: the increments no longer fit
        m = doc[key + "mode"]
        i = int((m == 0).nonzero()[0])
        m[i] = 4
    else:
        raise AssertionError(what)


@pytest.mark.parametrize("what", ["truncated payload", "mode 9", "non-monotone word_off", "word_off not from 0",
                                  "format tag", "another cout", "mode against the payload"])
def test_load_packed_rejects_corrupted_files(built_lib, tmp_path, what):
    import resnet
    from smpq import checkpoint
    net = _mixed_net(built_lib)
    p = tmp_path / "bad.smpq"
    checkpoint.save_packed(net, p)
    doc = torch.load(p, weights_only=True)
    _corrupt(doc, what)
    torch.save(doc, p)
    torch.manual_seed(6)
    net2 = resnet.resnet18()
    sd0 = {k: v.clone() for k, v in net2.state_dict().items()}
    with pytest.raises(ValueError):
        checkpoint.load_packed(net2, p)
    for k, v in net2.state_dict().items():  # nothing was written before the validation failed
        assert _bits_equal(v, sd0[k]), k
