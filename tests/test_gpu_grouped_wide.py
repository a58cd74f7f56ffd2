"""Wide-group 3x3 conv on the HIP path (csrc/conv_grouped_wide.hip: cin / groups >= 128, K streamed in
64-channel chunks): the kernel against the float64 emulation of the integer path on the dense
block-diagonal expansion of its codes, its tile walk, the QConv2d module path and a low-group-count
ResNet-50 through the fused engine."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from family_cases import grouped_case, scaled_images
from lean_ref import check_codes, emit_range_for, expected_overflow, to_code_units
from test_gpu import LIMB_QMAX

pytestmark = pytest.mark.gpu

# (cin, cout, groups, stride, H): two chunks, odd size, partial tiles on both axes; stride 2, even; cg 192 =
# three chunks (an odd count for the two-stage ring), og 64, an image smaller than a tile; og 256 = four
# channel blocks per group, cg != og, stride 2 at an odd size; cg 256 = four chunks, nine tiles
SHAPES = [(256, 256, 2, 1, 9), (256, 256, 2, 2, 10), (384, 128, 2, 1, 5), (256, 512, 2, 2, 9), (512, 128, 2, 1, 17)]


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "c%d_o%d_g%d_s%d_h%d" % s)
def test_grouped_wide_kernel_vs_emulation(gpu, shape, wl, relu):
    case = grouped_case(gpu, shape, wl)
    assert wl == 3 or bool((case.offset != 0).any())
    y, bound = case.reference()
    ye = np.maximum(y, 0) if relu else y

    def check_f32(yk, yam):
        yk = yk.cpu().numpy()
        err = np.abs(yk.astype(np.float64) - ye)
        assert (err <= 2e-6 * bound + 1e-30).all(), ("emulation mismatch", float((err / (bound + 1e-30)).max()))
        np.testing.assert_array_equal(yam.cpu().numpy(), np.abs(yk).reshape(2, -1).max(1))

    yk, yam, _, _ = case.launch("fp32", relu=relu)
    check_f32(yk, yam)
    for form, factor in (("planes", 2.0), ("planes", 0.5), ("both", 2.0)):  # a range that holds, one that clamps
        rng = emit_range_for(y, relu, factor)
        z, B = to_code_units(y, bound, relu, rng, 3)
        yk, yam, yq, ovf = case.launch(form, relu=relu, emit_range=rng)
        check_codes(yq, z, B, relu, 3)
        assert int(ovf.item()) == expected_overflow(z, B, 3) == (factor < 1)
        if form == "both":
            check_f32(yk, yam)


def test_grouped_wide_tile_walk_bitwise(gpu):
    """A stride-1 launch has ceil(1024 / (cout / 64)) workgroups per channel block: 512 at cout 128. 129 images
    of 9 x 9 (4 tiles each) are 516 tiles, the smallest count at this size that makes workgroups walk to a second
    tile, across an odd chunk count (cg 192), so the ring's stage flips between tiles. Images are independent:
    the result is bitwise that of per-image launches (one tile per workgroup, the path checked above)."""
    from smpq import ops
    n = 129
    g = torch.Generator().manual_seed(23)
    w = (torch.randn(128, 192, 3, 3, generator=g) * 0.1).to(gpu)
    step = ops.quantize_channels_(w.reshape(128, -1), [8] * 128)
    codes, offset, wscale, _ = ops.pack_weights_grouped(w, step, 1, 2)
    x = scaled_images(torch.randn(n, 9, 9, 384, generator=g)).to(gpu)
    am = ops.act_absmax(x)
    xq = ops.act_quantize(x, am, 3)
    sh = torch.linspace(-0.1, 0.1, 128, device=gpu).contiguous()

    def run(i0, i1):
        ovf, yam = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(i1 - i0, device=gpu)
        xs = xq[:, i0:i1].contiguous()
        y = ops.conv2d_grouped_q(xs, am[i0:i1], codes, offset, 1, wscale, sh, relu=True, y_absmax=yam)
        _, yq = ops.conv2d_grouped_q(xs, am[i0:i1], codes, offset, 1, wscale, sh, relu=True, emit_range=4.0,
                                     overflow=ovf, want_f32=False)
        return y, yam, yq
    y, yam, yq = run(0, n)
    parts = [run(i, i + 1) for i in range(n)]
    assert torch.equal(y, torch.cat([p[0] for p in parts]))
    assert torch.equal(yam, torch.cat([p[1] for p in parts]))
    assert torch.equal(yq, torch.cat([p[2] for p in parts], dim=1))


@pytest.mark.parametrize("free_channel,path", [(False, "hip-exact8"), (True, "hip-fixed")])
def test_grouped_wide_module_path(gpu, monkeypatch, free_channel, path):
    from smpq import ops, stats
    from smpq.qconv import QConv2d
    torch.manual_seed(5)
    conv = QConv2d(256, 256, 3, padding=1, groups=2, bias=False).to(gpu)
    bits = np.array([8, 6, 4, 2] * 64)
    if free_channel:
        bits[77] = 0
    step = ops.quantize_channels_(conv.weight.data.reshape(256, -1), bits.tolist())
    conv.record_quant_all(bits, step)
    x = torch.randn(2, 256, 9, 9, generator=torch.Generator().manual_seed(6))
    x[1] *= 7.0
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        yk = conv(x.to(gpu)).double().cpu()
    assert conv.last_path == path and stats["fp32_conv"] == f0 and conv.hip_supported()
    w = conv.weight.detach().double().cpu()
    yt = F.conv2d(x.double(), w, padding=1, groups=2)
    # test_grouped_module_path's bound: the activation quantization error 0.5 * s_x * sum |w| (+ fp32 noise)
    sx = (x.abs().amax(dim=(1, 2, 3)).double() / LIMB_QMAX[3]).reshape(2, 1, 1, 1)
    qbound = 0.5 * sx * w.abs().sum(dim=(1, 2, 3)).reshape(1, 256, 1, 1) * 1.0001 + 1e-5 * yt.abs() + 1e-6
    assert bool(((yk - yt).abs() <= qbound).all()), float(((yk - yt).abs() / qbound).max())
    monkeypatch.setattr(ops, "GROUPED", [False])  # what SMPQ_GROUPED=0 sets
    with torch.no_grad():
        conv(x.to(gpu))
    assert conv.last_path == "fp32" and stats["fp32_conv"] == f0 + 1


def test_low_group_count_resnet50_runs_fused_on_hip(gpu):
    """groups 2 x width 32: cin / groups = 32, 64, 128, 256 over the four layers."""
    import resnet
    from smpq import stats
    from smpq.models import Bottleneck
    torch.manual_seed(11)
    net = resnet.resnet50(groups=2, width_per_group=32).to(gpu).eval()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(3)).to(gpu)
    f0 = stats["fp32_conv"]
    with torch.no_grad():
        y_cal = net(x)  # calibrates the static ranges
        y_static = net(x)  # the static-range forward, captured
        y_replay = net(x)  # the graph's replay
    blocks = [m for m in net.modules() if isinstance(m, Bottleneck)]
    assert stats["fp32_conv"] == f0 and len(blocks) == 16
    assert sorted({b.conv2.in_channels // 2 for b in blocks}) == [32, 64, 128, 256]
    assert all(b.conv2.groups == 2 and b.conv2.last_path.startswith("hip-") for b in blocks)
    assert torch.equal(y_static, y_replay)
    net.fused = False
    with torch.no_grad():
        y_mod = net(x)
    assert stats["fp32_conv"] == f0
    for y in (y_cal, y_replay):
        rel = (y - y_mod).abs().max() / y_mod.abs().max()
        assert rel < 1.5e-2, float(rel)
