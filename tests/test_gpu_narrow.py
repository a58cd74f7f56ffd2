"""Narrow-channel dense convs on the HIP path (csrc/conv_narrow.hip): the kernel against the float64
emulation of the integer path on its own codes, the QConv2d module path, width-scaled ResNet-50s
through the fused engine, and the refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from family_cases import NARROW_SHAPES as SHAPES, narrow_case
from lean_ref import check_codes, decode, emit_range_for, expected_overflow, residual_planes, to_code_units
from test_gpu import LIMB_QMAX

pytestmark = pytest.mark.gpu

ONE_BY_ONE = [s for s in SHAPES if s[2] == 1]


def check_forms(gpu, ops_args, y, bound, relu, **res):
    """The general form (fp32 y, y_absmax), then limb planes at a range that holds and one that clamps."""
    from smpq import ops
    ye = np.maximum(y, 0) if relu else y
    yam = torch.zeros(2, device=gpu)
    yk = ops.conv2d_narrow_q(*ops_args, relu=bool(relu), y_absmax=yam, **res).cpu().numpy()
    err = np.abs(yk.astype(np.float64) - ye)
    assert (err <= 2e-6 * bound + 1e-30).all(), ("emulation mismatch", float((err / (bound + 1e-30)).max()))
    np.testing.assert_array_equal(yam.cpu().numpy(), np.abs(yk).reshape(2, -1).max(1))
    if "residual" in res:
        return  # (an fp32 residual: the general form only)
    for factor in (2.0, 0.5):
        rng = emit_range_for(y, relu, factor)
        z, B = to_code_units(y, bound, relu, rng, 3)
        for want_f32 in (False, True):  # the lean epilogue, the general one
            ovf = torch.zeros(1, dtype=torch.int32, device=gpu)
            yf, yq = ops.conv2d_narrow_q(*ops_args, relu=bool(relu), emit_range=rng, overflow=ovf, want_f32=want_f32,
                                         **res)
            assert (yf is None) == (not want_f32)
            check_codes(yq, z, B, relu, 3)
            assert int(ovf.item()) == expected_overflow(z, B, 3) == (factor < 1)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d_o%d_k%d_s%d_h%d_w%d" % s)
def test_narrow_kernel_vs_emulation(gpu, shape, wl, relu):
    case = narrow_case(gpu, shape, wl)
    y, bound = case.reference()
    check_forms(gpu, case.operands, y, bound, relu)


@pytest.mark.parametrize("form", ["fp32", "planes"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape", ONE_BY_ONE, ids=lambda s: "c%d_o%d_k%d_s%d_h%d_w%d" % s)
def test_narrow_1x1_residual(gpu, shape, wl, relu, form):
    case = narrow_case(gpu, shape, wl)
    _, cout, _, _, h, w_ = shape
    if form == "fp32":
        r = torch.randn(2, h, w_, cout, generator=torch.Generator().manual_seed(9)).to(gpu)
        res, rhost = {"residual": r}, r.cpu().numpy().astype(np.float64)
    else:
        rq, rr = residual_planes(gpu, 2, h, w_, cout, 3, 9)
        res = {"residual_q": rq, "residual_range": rr}
        rhost = decode(rq).astype(np.float64) * np.float64(np.float32(rr) / np.float32(LIMB_QMAX[3]))
    y, bound = case.reference(residual=rhost)
    check_forms(gpu, case.operands, y, bound, relu, **res)


@pytest.mark.parametrize("free_channel,path", [(False, "hip-exact8"), (True, "hip-fixed")])
@pytest.mark.parametrize("cin,cout,k", [(96, 96, 3), (48, 128, 1)])
def test_narrow_module_path(gpu, monkeypatch, cin, cout, k, free_channel, path):
    from smpq import ops, stats
    from smpq.qconv import QConv2d
    torch.manual_seed(5)
    conv = QConv2d(cin, cout, k, padding=k // 2, bias=False).to(gpu)
    bits = np.array([8, 6, 4, 2] * (cout // 4))
    if free_channel:
        bits[77] = 0
    step = ops.quantize_channels_(conv.weight.data.reshape(cout, -1), bits.tolist())
    conv.record_quant_all(bits, step)
    x = torch.randn(2, cin, 9, 9, generator=torch.Generator().manual_seed(6))
    x[1] *= 7.0
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        yk = conv(x.to(gpu)).double().cpu()
    assert conv.last_path == path and stats["fp32_conv"] == f0 and conv.hip_supported()
    w = conv.weight.detach().double().cpu()
    yt = F.conv2d(x.double(), w, padding=k // 2)
    # test_dilated_module_path's bound: the activation quantization error 0.5 * s_x * sum |w| (+ fp32 noise)
    sx = (x.abs().amax(dim=(1, 2, 3)).double() / LIMB_QMAX[3]).reshape(2, 1, 1, 1)
    qbound = 0.5 * sx * w.abs().sum(dim=(1, 2, 3)).reshape(1, cout, 1, 1) * 1.0001 + 1e-5 * yt.abs() + 1e-6
    assert bool(((yk - yt).abs() <= qbound).all()), float(((yk - yt).abs() / qbound).max())
    monkeypatch.setattr(ops, "NARROW", [False])  # what SMPQ_NARROW=0 sets
    with torch.no_grad():
        conv(x.to(gpu))
    assert conv.last_path == "fp32" and stats["fp32_conv"] == f0 + 1


@pytest.mark.parametrize("wpg", [32, 48])
def test_width_scaled_resnet50_runs_fused_on_hip(gpu, wpg):
    import resnet
    from smpq import stats
    from smpq.models import Bottleneck
    torch.manual_seed(11)
    net = resnet.resnet50(width_per_group=wpg).to(gpu).eval()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(gpu)
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        y_cal = net(x)  # calibrates the static ranges
        y_static = net(x)  # the static-range forward, captured
        y_replay = net(x)  # the graph's replay
    narrow = [c for b in net.modules() if isinstance(b, Bottleneck) for c in (b.conv2, b.conv3) if c.in_channels % 64]
    assert stats["fp32_conv"] == f0 and len(narrow) == (6 if wpg == 32 else 14)
    assert all(c.last_path.startswith("hip-") for c in narrow)
    assert torch.equal(y_static, y_replay)
    net.fused = False
    with torch.no_grad():
        y_mod = net(x)
    assert stats["fp32_conv"] == f0
    for y in (y_cal, y_replay):
        rel = (y - y_mod).abs().max() / y_mod.abs().max()
        assert rel < 1.5e-2, float(rel)


def test_narrow_refusals(gpu):
    from smpq import _lib, ops
    from smpq.qconv import QConv2d
    # (cin, cout, k, stride): cin % 16 != 0; cout % 16 != 0; 5x5; 1x1 at stride 2
    for cin, cout, k, stride in ((24, 64, 3, 1), (48, 100, 3, 1), (48, 64, 5, 1), (48, 64, 1, 2)):
        conv = QConv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False).to(gpu)
        assert conv.hip_supported() is False and conv.packed() is None
    # the C entry itself: a clean error before any launch
    xq = torch.zeros(3, 1, 4, 4, 48, dtype=torch.int8, device=gpu)
    codes = torch.zeros(3, 64, 48, dtype=torch.int8, device=gpu)
    am, v = torch.ones(1, device=gpu), torch.ones(64, device=gpu)
    y = torch.full((1, 2, 2, 64), 5.0, device=gpu)
    with pytest.raises(_lib.SmpqError, match="unsupported geometry"):
        ops._launch(gpu, "smpq_conv2d_narrow_fwd_q", xq, am, 1, 4, 4, 48, codes, codes, 3, None, 64, 1, 1, 2, 0, v, v, None,
                    0, 3, y, None, None, 0.0, None, None, 0.0)
    assert bool((y == 5.0).all())
