"""Grouped 3x3 conv on the HIP path (csrc/conv_grouped.hip): the kernel against the float64 emulation
of the integer path on the dense block-diagonal expansion of its codes, the QConv2d module path, a
ResNeXt-50 32x4d through the fused engine, and the refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from family_cases import GROUPED_SHAPES as SHAPES, grouped_case
from lean_ref import check_codes, emit_range_for, expected_overflow, to_code_units
from test_gpu import LIMB_QMAX

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d_o%d_g%d_s%d_h%d" % s)
def test_grouped_kernel_vs_emulation(gpu, shape, wl, relu):
    from smpq import ops
    case = grouped_case(gpu, shape, wl)
    xq, am, codes, offset, cs, sh = case.operands
    y, bound = case.reference()
    stride = shape[3]
    ye = np.maximum(y, 0) if relu else y
    yam = torch.zeros(2, device=gpu)
    yk = ops.conv2d_grouped_q(xq, am, codes, offset, stride, cs, sh, relu=bool(relu), y_absmax=yam)
    yk = yk.cpu().numpy()
    err = np.abs(yk.astype(np.float64) - ye)
    assert (err <= 2e-6 * bound + 1e-30).all(), ("emulation mismatch", float((err / (bound + 1e-30)).max()))
    np.testing.assert_array_equal(yam.cpu().numpy(), np.abs(yk).reshape(2, -1).max(1))
    for factor in (2.0, 0.5):  # a range that holds, one that clamps
        rng = emit_range_for(y, relu, factor)
        z, B = to_code_units(y, bound, relu, rng, 3)
        ovf = torch.zeros(1, dtype=torch.int32, device=gpu)
        yf, yq = ops.conv2d_grouped_q(xq, am, codes, offset, stride, cs, sh, relu=bool(relu), emit_range=rng,
                                      overflow=ovf, want_f32=False)
        assert yf is None
        check_codes(yq, z, B, relu, 3)
        assert int(ovf.item()) == expected_overflow(z, B, 3) == (factor < 1)


def test_grouped_tile_walk_bitwise(gpu):
    """More tiles (48 images x 25) than the launch has workgroups per channel block (1024): a workgroup
    restages its patch and walks on with its weights in registers. Images are independent, so the
    result is bitwise that of 16-image launches (400 tiles: one tile per workgroup, the path the
    emulation checks above)."""
    from smpq import ops
    g = torch.Generator().manual_seed(21)
    w = (torch.randn(64, 16, 3, 3, generator=g) * 0.1).to(gpu)
    step = ops.quantize_channels_(w.reshape(64, -1), [8] * 64)
    codes, offset, wscale, _ = ops.pack_weights_grouped(w, step, 1, 4)
    x = (torch.randn(48, 40, 40, 64, generator=g) * (1.0 + torch.arange(48) % 5).reshape(48, 1, 1, 1)).to(gpu)
    am = ops.act_absmax(x)
    xq = ops.act_quantize(x, am, 3)
    sh = torch.linspace(-0.1, 0.1, 64, device=gpu).contiguous()

    def run(i0, i1):
        ovf, yam = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(i1 - i0, device=gpu)
        xs = xq[:, i0:i1].contiguous()
        y = ops.conv2d_grouped_q(xs, am[i0:i1], codes, offset, 1, wscale, sh, relu=True, y_absmax=yam)
        _, yq = ops.conv2d_grouped_q(xs, am[i0:i1], codes, offset, 1, wscale, sh, relu=True, emit_range=1.0,
                                     overflow=ovf, want_f32=False)
        return y, yam, yq
    y, yam, yq = run(0, 48)
    parts = [run(i, i + 16) for i in (0, 16, 32)]
    assert torch.equal(y, torch.cat([p[0] for p in parts]))
    assert torch.equal(yam, torch.cat([p[1] for p in parts]))
    assert torch.equal(yq, torch.cat([p[2] for p in parts], dim=1))


def _quantized_conv(gpu, free_channel):
    from smpq import ops
    from smpq.qconv import QConv2d
    torch.manual_seed(5)
    conv = QConv2d(128, 128, 3, padding=1, groups=32, bias=False).to(gpu)
    bits = np.array([8, 6, 4, 2] * 32)
    if free_channel:
        bits[77] = 0
    step = ops.quantize_channels_(conv.weight.data.reshape(128, -1), bits.tolist())
    conv.record_quant_all(bits, step)
    return conv


@pytest.mark.parametrize("free_channel,path", [(False, "hip-exact8"), (True, "hip-fixed")])
def test_grouped_module_path(gpu, monkeypatch, free_channel, path):
    from smpq import ops, stats
    conv = _quantized_conv(gpu, free_channel)
    x = torch.randn(2, 128, 9, 9, generator=torch.Generator().manual_seed(6))
    x[1] *= 7.0
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        yk = conv(x.to(gpu)).double().cpu()
    assert conv.last_path == path and stats["fp32_conv"] == f0 and conv.hip_supported()
    w = conv.weight.detach().double().cpu()
    yt = F.conv2d(x.double(), w, padding=1, groups=32)
    # run_conv_case's second check: the activation quantization error 0.5 * s_x * sum |w| (+ fp32 noise)
    sx = (x.abs().amax(dim=(1, 2, 3)).double() / LIMB_QMAX[3]).reshape(2, 1, 1, 1)
    qbound = 0.5 * sx * w.abs().sum(dim=(1, 2, 3)).reshape(1, 128, 1, 1) * 1.0001 + 1e-5 * yt.abs() + 1e-6
    assert bool(((yk - yt).abs() <= qbound).all()), float(((yk - yt).abs() / qbound).max())
    monkeypatch.setattr(ops, "GROUPED", [False])  # what SMPQ_GROUPED=0 sets
    with torch.no_grad():
        conv(x.to(gpu))
    assert conv.last_path == "fp32" and stats["fp32_conv"] == f0 + 1


def test_resnext50_runs_fused_on_hip(gpu):
    import resnet
    from smpq import stats
    from smpq.models import Bottleneck
    torch.manual_seed(11)
    net = resnet.resnet50(groups=32, width_per_group=4).to(gpu).eval()
    x = torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(gpu)
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        y_fused = net(x)
    blocks = [m for m in net.modules() if isinstance(m, Bottleneck)]
    assert stats["fp32_conv"] == f0 and len(blocks) == 16
    assert all(b.conv2.groups == 32 and b.conv2.last_path.startswith("hip-") for b in blocks)
    net.fused = False
    with torch.no_grad():
        y_mod = net(x)
    assert stats["fp32_conv"] == f0
    rel = (y_fused - y_mod).abs().max() / y_mod.abs().max()
    assert rel < 1.5e-2, float(rel)


def test_grouped_refusals(gpu):
    from smpq import _lib, ops
    from smpq.qconv import QConv2d
    # (cin, cout, groups, k, pad, dilation): groups = 3 on 48 -> 48 as a dilated 5 x 5, then dilation 2 and
    # 5 x 5 each alone on channels the kernel takes, a fragment span of 48 channels, cout / groups = 12
    for cin, cout, groups, k, pad, dil in ((48, 48, 3, 5, 4, 2), (64, 64, 4, 3, 2, 2), (64, 64, 4, 5, 2, 1),
                                           (96, 96, 2, 3, 1, 1), (96, 96, 8, 3, 1, 1)):
        conv = QConv2d(cin, cout, k, padding=pad, dilation=dil, groups=groups, bias=False).to(gpu)
        assert conv.hip_supported() is False and conv.packed() is None
        if dil == 1:
            assert not ops.conv_grouped_supported(cin, cout, groups, k, k, 1, pad, 3, 3)
            with pytest.raises(ValueError):
                ops.pack_weights_grouped(conv.weight.detach(), None, 3, groups)
    # the C entry itself: a clean error before any launch
    xq = torch.zeros(3, 1, 4, 4, 48, dtype=torch.int8, device=gpu)
    am, v = torch.ones(1, device=gpu), torch.ones(48, device=gpu)
    y = torch.full((1, 4, 4, 48), 5.0, device=gpu)
    with pytest.raises(_lib.SmpqError, match="unsupported geometry"):
        ops._launch(gpu, "smpq_conv2d_grouped_fwd_q", xq, am, 1, 4, 4, 48, xq, xq, 3, None, 48, 3, 5, 5, 1, 2, v, v, 0,
                    3, y, None, None, 0.0, None)
    assert bool((y == 5.0).all())
