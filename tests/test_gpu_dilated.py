"""Dilated 3x3 conv on the HIP path (csrc/conv_dilated.hip): the kernel against the float64 emulation of
the integer path on the zero-inflated (2d+1) x (2d+1) form of its codes, the QConv2d module path, dilated
ResNet-50s through the fused engine, and the refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from family_cases import DILATED_SHAPES as SHAPES, dilated_case
from lean_ref import check_codes, emit_range_for, expected_overflow, to_code_units
from test_gpu import LIMB_QMAX

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d_o%d_d%d_h%d_w%d" % s)
def test_dilated_kernel_vs_emulation(gpu, shape, wl, relu):
    from smpq import ops
    case = dilated_case(gpu, shape, wl)
    xq, am, codes, offset, cs, sh = case.operands
    y, bound = case.reference()
    d = shape[2]
    ye = np.maximum(y, 0) if relu else y
    yam = torch.zeros(2, device=gpu)
    yk = ops.conv2d_dilated_q(xq, am, codes, offset, d, cs, sh, relu=bool(relu), y_absmax=yam)
    yk = yk.cpu().numpy()
    err = np.abs(yk.astype(np.float64) - ye)
    assert (err <= 2e-6 * bound + 1e-30).all(), ("emulation mismatch", float((err / (bound + 1e-30)).max()))
    np.testing.assert_array_equal(yam.cpu().numpy(), np.abs(yk).reshape(2, -1).max(1))
    for factor in (2.0, 0.5):  # a range that holds, one that clamps
        rng = emit_range_for(y, relu, factor)
        z, B = to_code_units(y, bound, relu, rng, 3)
        ovf = torch.zeros(1, dtype=torch.int32, device=gpu)
        yf, yq = ops.conv2d_dilated_q(xq, am, codes, offset, d, cs, sh, relu=bool(relu), emit_range=rng, overflow=ovf,
                                      want_f32=False)
        assert yf is None
        check_codes(yq, z, B, relu, 3)
        assert int(ovf.item()) == expected_overflow(z, B, 3) == (factor < 1)


@pytest.mark.parametrize("free_channel,path", [(False, "hip-exact8"), (True, "hip-fixed")])
def test_dilated_module_path(gpu, monkeypatch, free_channel, path):
    from smpq import ops, stats
    from smpq.qconv import QConv2d
    torch.manual_seed(5)
    conv = QConv2d(128, 128, 3, padding=2, dilation=2, bias=False).to(gpu)
    bits = np.array([8, 6, 4, 2] * 32)
    if free_channel:
        bits[77] = 0
    step = ops.quantize_channels_(conv.weight.data.reshape(128, -1), bits.tolist())
    conv.record_quant_all(bits, step)
    x = torch.randn(2, 128, 9, 9, generator=torch.Generator().manual_seed(6))
    x[1] *= 7.0
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        yk = conv(x.to(gpu)).double().cpu()
    assert conv.last_path == path and stats["fp32_conv"] == f0 and conv.hip_supported()
    w = conv.weight.detach().double().cpu()
    yt = F.conv2d(x.double(), w, padding=2, dilation=2)
    # test_grouped_module_path's bound: the activation quantization error 0.5 * s_x * sum |w| (+ fp32 noise)
    sx = (x.abs().amax(dim=(1, 2, 3)).double() / LIMB_QMAX[3]).reshape(2, 1, 1, 1)
    qbound = 0.5 * sx * w.abs().sum(dim=(1, 2, 3)).reshape(1, 128, 1, 1) * 1.0001 + 1e-5 * yt.abs() + 1e-6
    assert bool(((yk - yt).abs() <= qbound).all()), float(((yk - yt).abs() / qbound).max())
    monkeypatch.setattr(ops, "DILATED", [False])  # what SMPQ_DILATED=0 sets
    with torch.no_grad():
        conv(x.to(gpu))
    assert conv.last_path == "fp32" and stats["fp32_conv"] == f0 + 1


@pytest.mark.parametrize("rswd,size", [([False, True, True], 224), ([True, True, True], 64)])
def test_dilated_resnet50_runs_fused_on_hip(gpu, rswd, size):
    import resnet
    from smpq import stats
    from smpq.models import Bottleneck
    torch.manual_seed(11)
    net = resnet.resnet50(replace_stride_with_dilation=rswd).to(gpu).eval()
    x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(3)).to(gpu)
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        y_cal = net(x)  # calibrates the static ranges
        y_static = net(x)  # the static-range forward, captured
        y_replay = net(x)  # the graph's replay
    dil = [b.conv2 for b in net.modules() if isinstance(b, Bottleneck) and b.conv2.dilation[0] > 1]
    assert stats["fp32_conv"] == f0 and len(dil) == (12 if rswd[0] else 8)
    assert all(c.last_path.startswith("hip-") for c in dil)
    assert torch.equal(y_static, y_replay)
    net.fused = False
    with torch.no_grad():
        y_mod = net(x)
    assert stats["fp32_conv"] == f0
    for y in (y_cal, y_replay):
        rel = (y - y_mod).abs().max() / y_mod.abs().max()
        assert rel < 1.5e-2, float(rel)


def test_dilated_refusals(gpu):
    from smpq import _lib, ops
    from smpq.qconv import QConv2d
    # (cout, stride, pad, dilation, groups): stride 2; pad != d; d = 3; cout = 80; dilated + grouped
    for cout, stride, pad, dil, groups in ((64, 2, 2, 2, 1), (64, 1, 1, 2, 1), (64, 1, 3, 3, 1), (80, 1, 2, 2, 1),
                                           (64, 1, 2, 2, 4)):
        conv = QConv2d(64, cout, 3, stride=stride, padding=pad, dilation=dil, groups=groups, bias=False).to(gpu)
        assert conv.hip_supported() is False and conv.packed() is None
    # the C entry itself: a clean error before any launch
    xq = torch.zeros(3, 1, 4, 4, 64, dtype=torch.int8, device=gpu)
    codes = torch.zeros(3, 64, 576, dtype=torch.int8, device=gpu)
    am, v = torch.ones(1, device=gpu), torch.ones(64, device=gpu)
    y = torch.full((1, 4, 4, 64), 5.0, device=gpu)
    with pytest.raises(_lib.SmpqError, match="unsupported geometry"):
        ops._launch(gpu, "smpq_conv2d_dilated_fwd_q", xq, am, 1, 4, 4, 64, codes, None, 3, None, 64, 3, 3, 1, 3, 3, v, v, 0,
                    3, y, None, None, 0.0, None)
    assert bool((y == 5.0).all())
