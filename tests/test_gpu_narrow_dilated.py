"""Dilated narrow-channel 3x3 convs on the HIP path (csrc/conv_narrow_dilated.hip): the kernel against the
float64 emulation of the integer path on the zero-inflated (2d+1) x (2d+1) form of its codes, its item walk,
the QConv2d module path, a width-scaled dilated ResNet-50 through the fused engine, and the refusal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import family_cases
from family_cases import scaled_images, zero_inflate
from lean_ref import check_codes, emit_range_for, expected_overflow, to_code_units
from test_gpu import LIMB_QMAX

pytestmark = pytest.mark.gpu

# (cin, cout, d, H, W): smallest K, one active wave, resident weights, lattices of 5 and 4; padded last K step, a
# partial last workgroup (5 fragments), a partial second row tile, non-square; lattices of 2 and 1; streamed
# weights (23 steps), a second row tile for phase row 0 only; d > H (empty phases, row taps all outside); the
# widest cin narrow_geo(3x3, stride 1) stages in one slab (34 chunks: smpq_weights_narrow_expand_bytes gives
# ceil(9 * 34 / 4) = 77 steps) and the narrowest that takes two (35 = 34 + 1 chunks: 77 + 3 steps, not 79;
# test_narrow_dilated_host.py holds both counts)
SHAPES = [(16, 16, 2, 9, 9), (48, 80, 2, 18, 12), (96, 32, 4, 7, 7), (160, 64, 4, 33, 10), (32, 64, 8, 5, 11),
          (544, 16, 2, 9, 9), (560, 16, 2, 9, 9)]


def nd_case(gpu, shape, wl):
    """family_cases.dilated_case on the narrow operand: pack_weights_narrow at stride 1, conv2d_narrow_dilated_q."""
    from smpq import ops
    cin, cout, d, h, w_ = shape
    g = torch.Generator().manual_seed(cin + cout + d + h + 10 * wl)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.1).to(gpu)
    step = ops.quantize_channels_(w.reshape(cout, -1), [8] * cout) if wl == 1 else None
    codes, offset, wscale, st = ops.pack_weights_narrow(w, step, wl, 1)
    x = torch.randn(2, h, w_, cin, generator=g)
    return family_cases._finish(("narrow_dilated", shape, wl), lambda xq, am, c, o, cs, sh, **kw:
                                ops.conv2d_narrow_dilated_q(xq, am, c, o, d, cs, sh, **kw), gpu, x, codes, offset,
                                wscale, st, wl, True, lambda m: (zero_inflate(m, d), 2 * d + 1, d), 3, 1)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d_o%d_d%d_h%d_w%d" % s)
def test_narrow_dilated_kernel_vs_emulation(gpu, shape, wl, relu):
    case = nd_case(gpu, shape, wl)
    assert wl == 3 or bool((case.offset != 0).any())
    y, bound = case.reference()
    ye = np.maximum(y, 0) if relu else y

    def check_f32(yk, yam):
        yk = yk.cpu().numpy()
        err = np.abs(yk.astype(np.float64) - ye)
        assert (err <= 2e-6 * bound + 1e-30).all(), ("emulation mismatch", float((err / (bound + 1e-30)).max()))
        np.testing.assert_array_equal(yam.cpu().numpy(), np.abs(yk).reshape(2, -1).max(1))

    yk, yam, _, _ = case.launch("fp32", relu=relu, guard=True)
    check_f32(yk, yam)
    for form, factor in (("planes", 2.0), ("planes", 0.5), ("both", 2.0)):  # a range that holds, one that clamps
        rng = emit_range_for(y, relu, factor)
        z, B = to_code_units(y, bound, relu, rng, 3)
        yk, yam, yq, ovf = case.launch(form, relu=relu, emit_range=rng, guard=form == "planes" and factor > 1)
        check_codes(yq, z, B, relu, 3)
        assert int(ovf.item()) == expected_overflow(z, B, 3) == (factor < 1)
        if form == "both":
            check_f32(yk, yam)


def test_narrow_dilated_item_walk_bitwise(gpu):
    """cout 256 is 16 fragments = 4 workgroup columns, so the launch has min(ceil(1024 / 4), items) = 256
    workgroup rows. At d 4 an image of 5 x 65 has lattices of 2 or 1 rows and 17 (pw 0) or 16 columns: every phase
    gets the 3 column tiles of phase 0, 16 * 3 = 48 items per image, and column tile 2 of the 12 phases with pw > 0
    is outside its lattice. 5 images are 240 items (a workgroup each); 6 are 288 > 256, the smallest batch in which
    rows 0 .. 31 walk on to item 256 + y = image 5, item 16 + y. Row 5 skips its first item (image 0, phase 1, tile
    2) and computes the second (phase 7, tile 0); row 1 computes first (phase 0, tile 1) and then skips (phase 5,
    tile 2). Images are independent: the result is bitwise that of per-image launches (a workgroup per item)."""
    from smpq import ops
    n, d = 6, 4
    g = torch.Generator().manual_seed(23)
    w = (torch.randn(256, 48, 3, 3, generator=g) * 0.1).to(gpu)
    step = ops.quantize_channels_(w.reshape(256, -1), [8] * 256)
    codes, offset, wscale, _ = ops.pack_weights_narrow(w, step, 1, 1)
    x = scaled_images(torch.randn(n, 5, 65, 48, generator=g)).to(gpu)
    am = ops.act_absmax(x)
    xq = ops.act_quantize(x, am, 3)
    sh = torch.linspace(-0.1, 0.1, 256, device=gpu).contiguous()

    def run(i0, i1):
        ovf, yam = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(i1 - i0, device=gpu)
        a = (xq[:, i0:i1].contiguous(), am[i0:i1], codes, offset, d, wscale, sh)
        y = ops.conv2d_narrow_dilated_q(*a, relu=True, y_absmax=yam)
        _, yq = ops.conv2d_narrow_dilated_q(*a, relu=True, emit_range=4.0, overflow=ovf, want_f32=False)
        y3, yq3 = ops.conv2d_narrow_dilated_q(*a, relu=True, emit_range=4.0, overflow=ovf)
        return y, yam, yq, y3, yq3
    whole = run(0, n)
    parts = [run(i, i + 1) for i in range(n)]
    for k in range(5):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts], dim=1 if whole[k].dtype == torch.int8 else 0)), k


@pytest.mark.parametrize("free_channel,path", [(False, "hip-exact8"), (True, "hip-fixed")])
def test_narrow_dilated_module_path(gpu, monkeypatch, free_channel, path):
    from smpq import ops, stats
    from smpq.qconv import QConv2d
    torch.manual_seed(5)
    conv = QConv2d(96, 96, 3, padding=2, dilation=2, bias=False).to(gpu)
    bits = np.array([8, 6, 4, 2] * 24)
    if free_channel:
        bits[77] = 0
    step = ops.quantize_channels_(conv.weight.data.reshape(96, -1), bits.tolist())
    conv.record_quant_all(bits, step)
    x = torch.randn(2, 96, 9, 9, generator=torch.Generator().manual_seed(6))
    x[1] *= 7.0
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        yk = conv(x.to(gpu)).double().cpu()
    assert conv.last_path == path and stats["fp32_conv"] == f0 and conv.hip_supported() and conv.narrow_dilated()
    w = conv.weight.detach().double().cpu()
    yt = F.conv2d(x.double(), w, padding=2, dilation=2)
    # test_dilated_module_path's bound: the activation quantization error 0.5 * s_x * sum |w| (+ fp32 noise)
    sx = (x.abs().amax(dim=(1, 2, 3)).double() / LIMB_QMAX[3]).reshape(2, 1, 1, 1)
    qbound = 0.5 * sx * w.abs().sum(dim=(1, 2, 3)).reshape(1, 96, 1, 1) * 1.0001 + 1e-5 * yt.abs() + 1e-6
    assert bool(((yk - yt).abs() <= qbound).all()), float(((yk - yt).abs() / qbound).max())
    for k, switch in enumerate(("DILATED", "NARROW")):  # what SMPQ_DILATED=0 / SMPQ_NARROW=0 set
        with monkeypatch.context() as mp:
            mp.setattr(ops, switch, [False])
            with torch.no_grad():
                conv(x.to(gpu))
            assert conv.last_path == "fp32" and stats["fp32_conv"] == f0 + 1 + k


def test_width_scaled_dilated_resnet50_runs_fused_on_hip(gpu):
    """width_per_group 48 gives layer widths 48, 96, 192, 384: of the 12 dilated conv2s the three of layer 2 (96
    channels, d 2) are this kernel's, the six on 192 = 3 * 64 and the three on 384 the dense dilated kernel's.
    Without this kernel the three on 96 make _dilated_ok() false and the whole model leaves the fused path."""
    import resnet
    from smpq import stats
    from smpq.models import Bottleneck
    torch.manual_seed(11)
    net = resnet.resnet50(width_per_group=48, replace_stride_with_dilation=[True, True, True]).to(gpu).eval()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(gpu)
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        y_cal = net(x)  # calibrates the static ranges
        y_static = net(x)  # the static-range forward, captured
        y_replay = net(x)  # the graph's replay
    dil = [b.conv2 for b in net.modules() if isinstance(b, Bottleneck) and b.conv2.dilation[0] > 1]
    assert stats["fp32_conv"] == f0 and len(dil) == 12
    assert sorted(c.in_channels for c in dil) == [96] * 3 + [192] * 6 + [384] * 3
    assert [c.narrow_dilated() for c in dil] == [c.in_channels == 96 for c in dil]
    assert all(c.last_path.startswith("hip-") for c in dil)
    assert torch.equal(y_static, y_replay)
    net.fused = False
    with torch.no_grad():
        y_mod = net(x)
    assert stats["fp32_conv"] == f0
    for y in (y_cal, y_replay):
        rel = (y - y_mod).abs().max() / y_mod.abs().max()
        assert rel < 1.5e-2, float(rel)


def test_narrow_dilated_refusal(gpu):
    from smpq import _lib, ops
    # the C entry itself on the dense dilated kernel's cin: a clean error before any launch
    xq = torch.zeros(3, 1, 4, 4, 64, dtype=torch.int8, device=gpu)
    codes = torch.zeros(3, 64, 576, dtype=torch.int8, device=gpu)
    am, v = torch.ones(1, device=gpu), torch.ones(64, device=gpu)
    y = torch.full((1, 4, 4, 64), 5.0, device=gpu)
    with pytest.raises(_lib.SmpqError, match="unsupported geometry"):
        ops._launch(gpu, "smpq_conv2d_narrow_dilated_fwd_q", xq, am, 1, 4, 4, 64, codes, codes, 3, None, 64, 3, 3, 1, 2,
                    2, v, v, 0, 3, y, None, None, 0.0, None)
    assert bool((y == 5.0).all())
