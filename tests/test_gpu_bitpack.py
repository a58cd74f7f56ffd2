"""Format smpq-packed/1 on the device (csrc/bitpack.hip): the plan / store / load kernels between
guard regions, bit for bit against the host twins and the numpy packer of tests/bitpack_ref.py,
and snapshot / restore_ as the search's rollback through the engine."""
import numpy as np
import pytest
import torch

import bitpack_ref as ref
from bitpack_ref import u32
from lean_ref import run_guarded

pytestmark = pytest.mark.gpu


def _cases():
    return [("k%d" % k, lambda k=k: ref.quantized_tensor(k)) for k in ref.KS] + \
        [("fallbacks", lambda: ref.fallback_tensor()[:3]), ("zero_point_zero", ref.zero_point_zero_channel)]


@pytest.mark.parametrize("name,make", _cases(), ids=[c[0] for c in _cases()])
def test_device_kernels_match_host_and_numpy(gpu, name, make):
    from smpq import ops
    w, qbits, step = make()
    cout, k = w.shape
    # the host twins and the numpy packer: the expected bits
    h_mode, h_base, h_words = ops.bitpack_plan(w, qbits, step)
    h_off = ops.bitpack_offsets(h_words)
    h_payload = ops.bitpack_store(w, h_mode, h_base, step, h_off)
    n_mode, n_base, n_off, n_payload = ref.np_pack(w.numpy(), qbits.numpy(), step.numpy())
    wd, qd, sd = w.to(gpu), qbits.to(gpu), step.to(gpu)
    w_before = wd.clone()

    mode, base, words = run_guarded(lambda: ops.bitpack_plan(wd, qd, sd), modules=("smpq.ops",))
    assert mode.device == base.device == words.device == wd.device
    assert torch.equal(mode.cpu(), h_mode) and np.array_equal(mode.cpu().numpy(), n_mode)
    assert torch.equal(base.cpu(), h_base) and np.array_equal(base.cpu().numpy(), n_base)
    assert torch.equal(words.cpu(), h_words)
    off = ops.bitpack_offsets(words)
    assert off.dtype == torch.int64 and np.array_equal(off.cpu().numpy(), n_off)
    total = int(n_off[-1])

    # exactly the planned words: the guards on both sides stay, and no byte keeps its fill
    payload = run_guarded(lambda: ops.bitpack_store(wd, mode, base, sd, off, total), modules=("smpq.ops",))
    assert payload.dtype == torch.int8 and payload.numel() == 4 * total
    assert torch.equal(payload.cpu(), h_payload)
    assert np.array_equal(ref.payload_words(payload), n_payload)
    assert torch.equal(wd.view(torch.int32), w_before.view(torch.int32))  # bits: the fallbacks hold a NaN

    # no read past word_off[cout] can be seen from outside, but a wrong word would be: load from a
    # payload that ends exactly at the allocation's last planned word
    exact = payload.clone()
    # (the two fills' outputs are compared as bits: a raw channel may hold a NaN)
    back = run_guarded(lambda: ops.bitpack_load(exact, cout, k, mode, base, sd, off).view(torch.int32),
                       modules=("smpq.ops",)).view(torch.float32)
    assert back.shape == (cout, k) and back.dtype == torch.float32
    assert np.array_equal(u32(back.cpu().numpy()), u32(w.numpy()))
    # and into a caller's tensor in place, from the host twin's payload
    out = torch.full((cout, k), 7.0, device=gpu)
    assert ops.bitpack_load(h_payload.to(gpu), cout, k, mode, base, sd, off, out=out) is out
    assert np.array_equal(u32(out.cpu().numpy()), u32(w.numpy()))


def _r18(gpu, seed=0):
    import resnet
    torch.manual_seed(seed)
    return resnet.resnet18().to(gpu).eval()


def _quantize(net, convs, bits_choice, seed):
    from smpq.assignments import addressable_convs
    from smpq.quant import quantize_layer_
    rng = np.random.default_rng(seed)
    all_convs = addressable_convs(net)
    for i in convs:
        quantize_layer_(all_convs[i], rng.choice(bits_choice, size=all_convs[i].out_channels))


def _state(net):
    return {k: v.clone() for k, v in net.state_dict().items()}


def _assert_state_bits(net, sd0):
    sd = net.state_dict()
    assert list(sd) == list(sd0)
    for k, v in sd0.items():
        a = sd[k]
        assert a.dtype == v.dtype and a.shape == v.shape, k
        if v.dtype == torch.float32:
            a, v = a.contiguous().view(torch.int32), v.contiguous().view(torch.int32)
        assert torch.equal(a.cpu(), v.cpu()), k


def test_rollback_through_the_engine(gpu):
    """The search's accept / reject step: snapshot, quantize further, restore_; the forward after
    the rollback is bitwise the forward before it (first forward and the static-range one after)."""
    from smpq import checkpoint
    net = _r18(gpu)
    _quantize(net, range(0, 6), [0, 4, 6, 8], 1)
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(2)).to(gpu)
    with torch.no_grad():
        a1, a2 = net(x).clone(), net(x).clone()
    sd0 = _state(net)
    bits0 = checkpoint.bit_assignment(net)
    st = checkpoint.snapshot(net)
    assert all(pc.device == x.device for pc in st.convs.values())
    assert all(t.device == x.device for t in st.tensors.values())
    rep = checkpoint.packed_report(st)["total"]
    assert rep["packed_channels"] > 0 and rep["packed_bytes"] < rep["fp32_bytes"]
    _quantize(net, range(4, 12), [2, 4], 3)
    with torch.no_grad():
        b = net(x).clone()
    assert not torch.equal(a1, b)
    checkpoint.restore_(net, st)
    with torch.no_grad():
        c1, c2 = net(x).clone(), net(x).clone()
    assert torch.equal(c1, a1)
    assert torch.equal(c2, a2)
    _assert_state_bits(net, sd0)
    assert checkpoint.bit_assignment(net) == bits0


def test_snapshot_crosses_devices(gpu):
    """A device snapshot restored into a host net and a host snapshot restored into a device net
    give the bits of the net they were taken from; both snapshots hold the same payload."""
    import resnet
    from smpq import checkpoint
    torch.manual_seed(0)
    host = resnet.resnet18()
    from smpq.assignments import addressable_convs
    from smpq.quant import quantize_layer_
    rng = np.random.default_rng(1)
    for conv in addressable_convs(host)[:6]:
        quantize_layer_(conv, rng.choice([0, 2, 4, 6, 8], size=conv.out_channels))
    sd0 = _state(host)
    dev = _r18(gpu, seed=9)
    st_h = checkpoint.snapshot(host)
    checkpoint.restore_(dev, st_h)
    _assert_state_bits(dev, sd0)
    st_d = checkpoint.snapshot(dev)
    for name, pc in st_d.convs.items():
        assert pc.device == gpu
        for f in ("mode", "base", "word_off", "payload", "qbits"):
            assert torch.equal(getattr(pc, f).cpu(), getattr(st_h.convs[name], f)), (name, f)
    torch.manual_seed(11)
    host2 = resnet.resnet18()
    checkpoint.restore_(host2, st_d)
    _assert_state_bits(host2, sd0)
    assert checkpoint.bit_assignment(host2) == checkpoint.bit_assignment(host)


def test_snapshot_surfaces_a_deferred_constant_channel(gpu):
    """A deferred per-channel quantization that met a constant channel (functions.py:40) raises
    from snapshot, before any state exists, as it does from save_checkpoint."""
    import functions
    from smpq import checkpoint, quant
    net = _r18(gpu)
    conv = net.layer2[0].conv2
    with torch.no_grad():
        conv.weight.data[5] = 0.25
    functions.channel_wise_quantizationperchan(conv.weight.data, 4, 5)
    st = None
    with pytest.raises(ZeroDivisionError):
        st = checkpoint.snapshot(net)
    assert st is None
    quant.check_pending()  # cleared by the raise
    assert conv.qbits[5].item() == 0
    st = checkpoint.snapshot(net)  # and the next one goes through
    assert st.convs["layer2.0.conv2"].mode[5].item() == 0
