"""3x3 small-channel stem on the HIP path (csrc/conv_stem3.hip): the kernel against the float64 emulation of
the integer path on its own codes, the input planes against act_quantize, the QConv2d module path,
CIFAR-style ResNets through the fused engine, and the refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from family_cases import STEM3_SHAPES as SHAPES, stem3_case
from lean_ref import check_codes, emit_range_for, expected_overflow, to_code_units
from test_gpu import LIMB_QMAX

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d_o%d_h%d_w%d" % s)
def test_stem3_kernel_vs_emulation(gpu, shape, relu):
    from smpq import ops
    case = stem3_case(gpu, shape)
    xq, am, codes, _, cs, sh = case.operands
    y, bound = case.reference()
    ye = np.maximum(y, 0) if relu else y
    yam = torch.zeros(2, device=gpu)
    yk = ops.stem_conv3_q(xq, am, codes, cs, sh, relu=bool(relu), y_absmax=yam).cpu().numpy()
    err = np.abs(yk.astype(np.float64) - ye)
    assert (err <= 2e-6 * bound + 1e-30).all(), ("emulation mismatch", float((err / (bound + 1e-30)).max()))
    np.testing.assert_array_equal(yam.cpu().numpy(), np.abs(yk).reshape(2, -1).max(1))
    for factor in (2.0, 0.5):  # a range that holds, one that clamps
        rng = emit_range_for(y, relu, factor)
        z, B = to_code_units(y, bound, relu, rng, 3)
        ovf = torch.zeros(1, dtype=torch.int32, device=gpu)
        yf, yq = ops.stem_conv3_q(xq, am, codes, cs, sh, relu=bool(relu), emit_range=rng, overflow=ovf, want_f32=False)
        assert yf is None
        check_codes(yq, z, B, relu, 3)
        assert int(ovf.item()) == expected_overflow(z, B, 3) == (factor < 1)


@pytest.mark.parametrize("c", [1, 3, 4])
def test_image_quantize_c4_is_act_quantize(gpu, c):
    from smpq import ops
    x = torch.randn(2, c, 7, 5, generator=torch.Generator().manual_seed(c)).to(gpu)
    x[1] *= 3.0
    am = ops.act_absmax(x)
    nhwc8 = F.pad(x.permute(0, 2, 3, 1), (0, 8 - c)).contiguous()
    assert torch.equal(ops.image_quantize_c4(x, am), ops.act_quantize(nhwc8, am, 3)[..., :4])


def test_stem3_module_path(gpu, monkeypatch):
    from smpq import ops, stats
    from smpq.qconv import QConv2d
    torch.manual_seed(5)
    conv = QConv2d(3, 64, 3, padding=1, bias=False).to(gpu)
    bits = np.array([8, 6, 4, 2] + [0] * 60)
    step = ops.quantize_channels_(conv.weight.data.reshape(64, -1), bits.tolist())
    conv.record_quant_all(bits, step)
    x = torch.randn(2, 3, 9, 19, generator=torch.Generator().manual_seed(6))
    x[1] *= 7.0
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        yk = conv(x.to(gpu)).double().cpu()
    assert conv.last_path == "hip-fixed-c4" and stats["fp32_conv"] == f0
    w = conv.weight.detach().double().cpu()
    yt = F.conv2d(x.double(), w, padding=1)
    # the siblings' bound: the activation quantization error 0.5 * s_x * sum |w| (+ fp32 noise)
    sx = (x.abs().amax(dim=(1, 2, 3)).double() / LIMB_QMAX[3]).reshape(2, 1, 1, 1)
    qbound = 0.5 * sx * w.abs().sum(dim=(1, 2, 3)).reshape(1, 64, 1, 1) * 1.0001 + 1e-5 * yt.abs() + 1e-6
    assert bool(((yk - yt).abs() <= qbound).all()), float(((yk - yt).abs() / qbound).max())
    monkeypatch.setattr(ops, "STEM3", [False])  # what SMPQ_STEM3=0 sets
    with torch.no_grad():
        conv(x.to(gpu))
    assert conv.last_path == "fp32" and stats["fp32_conv"] == f0 + 1


@pytest.mark.parametrize("arch,size,pool", [("resnet18", 32, False), ("resnet50", 32, False), ("resnet18", 64, True)])
def test_small_image_resnet_runs_fused_on_hip(gpu, arch, size, pool):
    import resnet
    from smpq import stats
    from smpq.qconv import QConv2d
    torch.manual_seed(11)
    net = getattr(resnet, arch)()
    net.conv1 = QConv2d(3, 64, 3, padding=1, bias=False)
    if not pool:
        net.maxpool = torch.nn.Identity()
    net = net.to(gpu).eval()
    x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(3)).to(gpu)
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        y_cal = net(x)  # calibrates the static ranges
        y_static = net(x)  # the static-range forward, captured
        y_replay = net(x)  # the graph's replay
    assert stats["fp32_conv"] == f0 and net.conv1.last_path.startswith("hip-")
    assert torch.equal(y_static, y_replay)
    net.fused = False
    with torch.no_grad():
        y_mod = net(x)
    assert stats["fp32_conv"] == f0
    for y in (y_cal, y_replay):
        rel = (y - y_mod).abs().max() / y_mod.abs().max()
        assert rel < 1.5e-2, float(rel)


def test_stem3_refusals(gpu):
    from smpq import _lib, ops
    from smpq.qconv import QConv2d
    # (cin, cout, stride): stride 2; five channels; cout % 64 != 0
    for cin, cout, stride in ((3, 64, 2), (5, 64, 1), (3, 80, 1)):
        conv = QConv2d(cin, cout, 3, stride=stride, padding=1, bias=False).to(gpu)
        with torch.no_grad():
            conv(torch.randn(1, cin, 8, 8, device=gpu))
        assert not conv.c4_stem() and conv.last_path == "fp32"
    # the C entry itself: a clean error before any launch
    xq = torch.zeros(3, 1, 4, 4, 4, dtype=torch.int8, device=gpu)
    codes = torch.zeros(3, 64, 64, dtype=torch.int8, device=gpu)
    am, v = torch.ones(1, device=gpu), torch.ones(64, device=gpu)
    y = torch.full((1, 2, 2, 64), 5.0, device=gpu)
    with pytest.raises(_lib.SmpqError, match="unsupported geometry"):
        ops._launch(gpu, "smpq_stem_conv3_q", xq, am, 1, 4, 4, 3, codes, 3, 64, 3, 3, 2, 1, v, v, 0, 3, y, None, None, 0.0,
                    None)
    assert bool((y == 5.0).all())
