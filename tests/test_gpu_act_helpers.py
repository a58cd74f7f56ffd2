"""The activation-side helper kernels on their own: absmax_kernel,
act_quantize_kernel, image_quantize_s2d_kernel, maxpool_quantize_kernel and maxpool_limbs_kernel of
csrc/conv.hip, image_quantize_c4_kernel of csrc/conv_stem3.hip, and through them the limb codecs
split_limbs / decode4 / encode4 of csrc/conv_common.h. Every call goes through smpq.ops and the C-ABI.

Every output is allocated between guard regions (lean_ref.run_guarded), every quantized value is
compared to the bit with act_ref.quantize_ref (the kernels' fp32 arithmetic restated in numpy) and
then against the float64 bound of act_ref.quantize_ideal. The shapes are chosen by what they run:

  * every code of every width once (the codecs' carries; at 3 limbs the grid-stride loop of
    act_quantize wraps), fed through maxpool_limbs at 1x1, where encode4(decode4(.)) is the identity;
  * act_absmax with one image's maximum at each side of each loop boundary (unrolled body, remainder
    loop, scalar path): act_ref.absmax_launch says which loops a shape runs, and the tests assert it;
  * the quantizer's edge values (act_ref.edge_images): ties, values past the range, signed zeros, an
    all-zero image, a range so small that QMAX / range is past FLT_MAX, a static range;
  * max pools at h, w of 1 and 2 and with c / 4 not a power of two, one whose loop wraps;
  * the image quantizers at every channel count.

NaN and Inf activations are not defined for any of these kernels and are not tested. The grid-stride
wrap of image_quantize_s2d (65535 blocks of 256 pixels: more than 16.7 M space-to-depth pixels, 800 MB
of input at 3 channels) is out of reach of a few-second test; the fused forward tests run that loop's
body, never its second trip.
"""
import numpy as np
import pytest
import torch

from act_ref import (EDGE_IMAGES, absmax_launch, absmax_positions, c4_ref, check_quantized, edge_images, maxpool_ref,
                     quantize_ref, s2d_ref)
from lean_ref import decode, encode, run_guarded
from test_gpu import LIMB_QMAX

pytestmark = pytest.mark.gpu

HERE = ("smpq.ops", __name__)  # modules whose torch.empty outputs run_guarded puts between guards


def image_ranges(x):
    """fp32 [n] max |x| per image, computed by torch (not by the kernel under test)."""
    return x.reshape(x.shape[0], -1).abs().amax(1).contiguous()


# ---- a. every code ------------------------------------------------------------------------------
@pytest.mark.parametrize("limbs", [1, 2, 3])
def test_every_code_quantizes_and_pools_to_itself(gpu, limbs):
    """x holds every integer of [-QMAX, QMAX] once under absmax = QMAX (scale exactly 1): the planes
    decode to x, their digits are the balanced digits of lean_ref.encode, and maxpool_limbs of the
    planes as [L, n, 1, 1, 16] (a 1x1 image pools to itself: decode4, max over nine copies of the
    centre, encode4, in all four lanes of a dword) returns them bit for bit."""
    from smpq import ops
    qmax = int(LIMB_QMAX[limbs])
    count = 2 * qmax + 1
    total = -(-count // 16) * 16  # zero-padded: a multiple of 8 (act_quantize) and of 16 (maxpool_limbs)
    if limbs == 3:
        assert count == 16646145 and total > 8388608  # more than 4096 blocks x 256 threads x 8: the loop wraps
    x = torch.zeros(total)
    x[:count] = torch.arange(-qmax, qmax + 1, dtype=torch.float32)  # exact: |q| < 2^24
    xd = x.reshape(1, total).to(gpu)
    am = torch.full((1,), float(qmax), device=gpu)
    planes = run_guarded(lambda: ops.act_quantize(xd, am, limbs))
    assert planes.shape == (limbs, 1, total) and planes.dtype == torch.int8
    want = xd.to(torch.int32)
    code = sum(planes[l].to(torch.int32) * 256 ** l for l in range(limbs))  # exact integer arithmetic
    bad = code != want
    assert not bool(bad.any()), "%d codes wrong, first x = %d -> %d" % (
        int(bad.sum()), int(want[bad][0]), int(code[bad][0]))
    del code, bad
    digits = encode(x.numpy().astype(np.int64), limbs).reshape(limbs, 1, total)
    assert np.array_equal(planes.cpu().numpy(), digits), "not the balanced digits"
    cells = planes.reshape(limbs, total // 16, 1, 1, 16)
    pooled = run_guarded(lambda: ops.maxpool_limbs(cells))
    assert pooled.shape == cells.shape
    diff = pooled != cells
    assert not bool(diff.any()), "maxpool_limbs changed %d digits of 1x1 images, first at code %d" % (
        int(diff.sum()), int(want.reshape(-1)[diff.any(0).reshape(-1)][0]))


# ---- b. act_absmax ------------------------------------------------------------------------------
# shape -> the loops absmax_launch reports for it (vector: 4-load bodies, one-load remainder passes)
ABSMAX_SHAPES = {(1024, 9728): ("vector", 2, 2), (300, 16384): ("vector", 1, 0), (3, 2240): ("vector", 0, 1),
                 (2, 4551): ("scalar", 0, 4), (5, 1): ("scalar", 0, 1), (5, 2): ("scalar", 0, 1),
                 (5, 3): ("scalar", 0, 1), (5, 5): ("scalar", 0, 1), (5, 7): ("scalar", 0, 1), (1, 12): ("vector", 0, 1)}


def guarded_absmax(x):
    from smpq import ops

    def fn():
        out = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)  # between guards (HERE)
        out.zero_()
        return ops.act_absmax(x, out=out)
    return run_guarded(fn, modules=HERE)


def test_absmax_shapes_cover_every_loop():
    """Between them the shapes run the unrolled body twice in a thread, the remainder loop twice
    (the second pass partial), the remainder loop alone, and the scalar loop once and four times."""
    got = {s: absmax_launch(*s) for s in ABSMAX_SHAPES}
    assert got == ABSMAX_SHAPES
    assert any(p == "vector" and b >= 2 and r >= 2 for p, b, r in got.values())
    assert any(p == "vector" and b >= 1 and r == 0 for p, b, r in got.values())
    assert any(p == "vector" and b == 0 and r == 1 for p, b, r in got.values())
    assert any(p == "scalar" and r >= 2 for p, b, r in got.values())
    assert 9728 % 1024 == 512  # (1024, 9728): the last remainder pass reaches half of the 256 threads


@pytest.mark.parametrize("shape", sorted(ABSMAX_SHAPES), ids=lambda s: "n%d_per%d" % s)
def test_act_absmax_maximum_at_every_place(gpu, shape):
    """Image k holds |x| < 1 and one value of magnitude 1.5 + k / 1024 (its sign alternating with k)
    at position p_k; over the images (and, where there are more positions than images, over several
    launches) p_k takes 0, per - 1 and both sides of every loop boundary. The result is max |x|
    exactly, per image: a load a loop skips, or an image credited with another's maximum, shows."""
    n, per = shape
    assert absmax_launch(n, per) == ABSMAX_SHAPES[shape]
    pos = absmax_positions(n, per)
    assert pos[0] == 0 and pos[-1] == per - 1
    base = torch.rand(n, per, generator=torch.Generator().manual_seed(per)) * 2 - 1
    k = torch.arange(n)
    peak = (1.5 + k.float() / 1024) * (1 - 2 * (k % 2)).float()
    for first in range(0, len(pos), n):
        p = torch.tensor([pos[(first + i) % len(pos)] for i in range(n)])
        x = base.clone()
        x[k, p] = peak
        xd = x.to(gpu)
        got = guarded_absmax(xd)
        assert torch.equal(got.cpu(), peak.abs()), (p[(got.cpu() != peak.abs())][:8].tolist(), got[:4].tolist())
        assert torch.equal(got, image_ranges(xd))


def test_act_absmax_zeros_and_accumulation(gpu):
    from smpq import ops
    x = torch.zeros(4, 4096)
    x[1] = -0.0
    x[2, 4095] = -0.0
    x[3] = torch.randn(4096, generator=torch.Generator().manual_seed(3))
    xd = x.to(gpu)
    assert bool(torch.signbit(xd[1]).all()) and bool(torch.signbit(xd[2, 4095]))
    got = guarded_absmax(xd).cpu()
    assert got[:3].tolist() == [0.0, 0.0, 0.0] and not bool(torch.signbit(got).any())  # +0.0, never -0.0
    assert got[3] == x[3].abs().max()
    # out= accumulates (smpq/engine.py): a value above the maximum stays, to the bit; one below is raised
    pre = torch.tensor([5.0, 0.0, 7.0, 100.0], device=gpu)
    out = pre.clone()
    assert ops.act_absmax(xd, out=out) is out
    assert torch.equal(out.view(torch.int32), pre.view(torch.int32))
    out = torch.tensor([0.0, 0.0, 0.0, 0.5 * float(got[3])], device=gpu)
    ops.act_absmax(xd, out=out)
    assert torch.equal(out.cpu(), got)


def test_act_absmax_image_count_limit(gpu):
    """One grid row per image: 65535 images run, 65536 are refused on the host (SMPQ_E_SHAPE) before
    any launch."""
    from smpq import _lib, ops
    x = torch.zeros(65536, 8, device=gpu)
    x[65534, 7] = -3.0
    x[0, 0] = 2.0
    got = ops.act_absmax(x[:65535])
    assert torch.equal(got, image_ranges(x[:65535])) and got[65534] == 3.0 and got[0] == 2.0
    out = torch.full((65536,), 1.0, device=gpu)
    with pytest.raises(_lib.SmpqError, match=r"\(%d\).*65535" % _lib.SMPQ_E_SHAPE):
        ops.act_absmax(x, out=out)
    torch.cuda.synchronize()
    assert bool((out == 1.0).all())  # nothing was launched


# ---- c. act_quantize edges ----------------------------------------------------------------------
def assert_edge_codes(codes, x, am, limbs):
    """codes int64 [6, ...] of act_ref.edge_images: both references, then what each image is for."""
    codes, x = codes.reshape(EDGE_IMAGES, -1), x.reshape(EDGE_IMAGES, -1)
    qmax = int(LIMB_QMAX[limbs])
    # the tiny range first: the image a scale of +inf turns into -QMAX everywhere
    assert not codes[4][x[4] == 0].any(), "zeros under absmax 1e-33 code to %s" % sorted(set(codes[4][x[4] == 0]))[:4]
    np.testing.assert_array_equal(codes[4], np.sign(x[4]).astype(np.int64) * qmax)
    check_quantized(codes, x, am, limbs)
    np.testing.assert_array_equal(codes[0], np.rint(x[0].astype(np.float64)).astype(np.int64))  # half to even
    assert set(codes[1][np.abs(x[1]) > 3.0]) == {-qmax, qmax}
    assert np.abs(codes).max() == qmax
    assert not codes[2][x[2] == 0].any() and not codes[3].any()
    assert (np.abs(codes[5]) == qmax).sum() > 1


@pytest.mark.parametrize("limbs", [1, 2, 3])
def test_act_quantize_edges(gpu, limbs):
    from smpq import ops
    x, am = edge_images(64, limbs)
    xd, amd = torch.from_numpy(x).to(gpu), torch.from_numpy(am).to(gpu)
    planes = run_guarded(lambda: ops.act_quantize(xd, amd, limbs))
    assert planes.shape == (limbs, EDGE_IMAGES, 64)
    assert_edge_codes(decode(planes), x, am, limbs)


# ---- d. max pools -------------------------------------------------------------------------------
def signed_images(n, h, w, c, seed):
    x = torch.randn(n, h, w, c, generator=torch.Generator().manual_seed(seed))
    return x * (1.0 + (torch.arange(n) % 5).float()).reshape(n, 1, 1, 1)


POOL_HW = [(1, 1), (1, 7), (2, 2), (2, 9), (17, 22)]


@pytest.mark.parametrize("limbs", [1, 2, 3])
@pytest.mark.parametrize("hw", POOL_HW, ids=lambda s: "%dx%d" % s)
def test_maxpool_quantize_geometry(gpu, hw, limbs):
    """c = 4 (one thread per pixel), 12 (c / 4 = 3: no power of two) and 64, signed inputs."""
    from smpq import ops
    h, w = hw
    for c in (4, 12, 64):
        x = signed_images(3, h, w, c, 100 * h + w + c)
        xd = x.to(gpu)
        am = image_ranges(xd)
        q, f = run_guarded(lambda: ops.maxpool_quantize(xd, am, limbs))
        ref = maxpool_ref(x.numpy())
        assert f.shape == ref.shape == (3, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c)
        np.testing.assert_array_equal(f.cpu().numpy().astype(np.float64), ref)
        assert q.shape == (limbs,) + ref.shape
        check_quantized(decode(q), ref.astype(np.float32), am.cpu().numpy(), limbs)
        q2, f2 = run_guarded(lambda: ops.maxpool_quantize(xd, am, limbs, want_f32=False))
        assert f2 is None and torch.equal(q2, q)


@pytest.mark.parametrize("limbs", [1, 2, 3])
@pytest.mark.parametrize("hw", POOL_HW, ids=lambda s: "%dx%d" % s)
def test_maxpool_limbs_geometry(gpu, hw, limbs):
    """maxpool_limbs(act_quantize(x)) == act_quantize(maxpool_ref(x)) == quantize_ref(maxpool_ref(x)),
    c = 16 and 48, signed inputs (negative codes: the max of two's-complement digits would be wrong)."""
    from smpq import ops
    h, w = hw
    for c in (16, 48):
        x = signed_images(3, h, w, c, 200 * h + w + c)
        xd = x.to(gpu)
        am = image_ranges(xd)
        xq = ops.act_quantize(xd, am, limbs)
        got = run_guarded(lambda: ops.maxpool_limbs(xq))
        ref = maxpool_ref(x.numpy()).astype(np.float32)
        assert got.shape == (limbs,) + ref.shape
        codes = decode(got)
        assert codes.min() < 0 < codes.max()
        np.testing.assert_array_equal(codes, quantize_ref(ref, am.cpu().numpy(), limbs))
        assert torch.equal(got, ops.act_quantize(torch.from_numpy(ref).to(gpu), am, limbs))


def test_maxpool_quantize_loop_wraps(gpu):
    """n = 6, 225 x 225 x 64 -> 113 x 113: 4.9 M outputs, more than the 4096 blocks x 256 threads x 4
    channels of one grid pass, so the grid-stride loop takes a second trip."""
    from smpq import ops
    n, h, c, limbs = 6, 225, 64, 3
    x = signed_images(n, h, h, c, 7)
    ref = maxpool_ref(x.numpy())
    assert ref.size == 6 * 113 * 113 * 64 == 4903296 and ref.size > 4096 * 256 * 4
    xd = x.to(gpu)
    am = image_ranges(xd)
    q, f = run_guarded(lambda: ops.maxpool_quantize(xd, am, limbs))
    np.testing.assert_array_equal(f.cpu().numpy().astype(np.float64), ref)
    check_quantized(decode(q), ref.astype(np.float32), am.cpu().numpy(), limbs)


@pytest.mark.parametrize("limbs", [1, 2, 3])
def test_maxpool_quantize_edges(gpu, limbs):
    """The quantizer's edge values through maxpool_quantize: 1 x 1 images of 64 channels pool to
    themselves."""
    from smpq import ops
    x, am = edge_images(64, limbs)
    xd, amd = torch.from_numpy(x).reshape(EDGE_IMAGES, 1, 1, 64).to(gpu), torch.from_numpy(am).to(gpu)
    q, f = run_guarded(lambda: ops.maxpool_quantize(xd, amd, limbs))
    assert torch.equal(f.view(torch.int32), xd.view(torch.int32))  # to the bit: -0.0 stays -0.0
    assert_edge_codes(decode(q), x, am, limbs)


# ---- e. image quantizers ------------------------------------------------------------------------
IMAGE_HW = [(2, 2), (3, 5), (40, 36)]


def images(n, c, h, w, seed):
    x = torch.randn(n, c, h, w, generator=torch.Generator().manual_seed(seed))
    return x * (1.0 + 2.0 * torch.arange(n).float()).reshape(n, 1, 1, 1)


@pytest.mark.parametrize("limbs", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", IMAGE_HW, ids=lambda s: "%dx%d" % s)
def test_image_quantize_s2d_layout(gpu, hw, n, limbs):
    """c = 1, 2, 4 (3 is test_gpu.py's): every byte of the space-to-depth planes, the zero channels and
    the zero row / column of an odd size included."""
    from smpq import ops
    h, w = hw
    for c in (1, 2, 4):
        x = images(n, c, h, w, 10 * h + c + n)
        xd = x.to(gpu)
        am = image_ranges(xd)
        planes = run_guarded(lambda: ops.image_quantize_s2d(xd, am, limbs))
        codes = quantize_ref(x.numpy(), am.cpu().numpy(), limbs)
        check_quantized(codes, x.numpy(), am.cpu().numpy(), limbs)
        want = s2d_ref(codes, limbs)
        assert planes.shape == want.shape == (limbs, n, (h + 1) // 2, (w + 1) // 2, 16)
        np.testing.assert_array_equal(planes.cpu().numpy(), want)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("hw", IMAGE_HW, ids=lambda s: "%dx%d" % s)
def test_image_quantize_c4_layout(gpu, hw, n):
    from smpq import ops
    h, w = hw
    for c in (1, 3, 4):
        x = images(n, c, h, w, 20 * h + c + n)
        xd = x.to(gpu)
        am = image_ranges(xd)
        planes = run_guarded(lambda: ops.image_quantize_c4(xd, am))
        codes = quantize_ref(x.numpy(), am.cpu().numpy(), 3)
        check_quantized(codes, x.numpy(), am.cpu().numpy(), 3)
        want = c4_ref(codes)
        assert planes.shape == want.shape == (3, n, h, w, 4)
        np.testing.assert_array_equal(planes.cpu().numpy(), want)


def edge_image_batch(c, h, w, limbs):
    x, am = edge_images(c * h * w, limbs)
    return x.reshape(EDGE_IMAGES, c, h, w), am


@pytest.mark.parametrize("limbs", [1, 2, 3])
def test_image_quantize_s2d_edges(gpu, limbs):
    from smpq import ops
    x, am = edge_image_batch(4, 5, 7, limbs)
    xd, amd = torch.from_numpy(x).to(gpu), torch.from_numpy(am).to(gpu)
    planes = run_guarded(lambda: ops.image_quantize_s2d(xd, amd, limbs)).cpu().numpy()
    np.testing.assert_array_equal(planes, s2d_ref(quantize_ref(x, am, limbs), limbs))
    # the codes back out of the layout (s2d_ref is linear in the codes: position by position)
    img = decode(planes).reshape(EDGE_IMAGES, 3, 4, 2, 2, 4).transpose(0, 5, 1, 3, 2, 4).reshape(EDGE_IMAGES, 4, 6, 8)
    assert_edge_codes(np.ascontiguousarray(img[:, :, :5, :7]), x, am, limbs)


@pytest.mark.parametrize("c", [3, 4])
def test_image_quantize_c4_edges(gpu, c):
    from smpq import ops
    x, am = edge_image_batch(c, 5, 7, 3)
    xd, amd = torch.from_numpy(x).to(gpu), torch.from_numpy(am).to(gpu)
    planes = run_guarded(lambda: ops.image_quantize_c4(xd, amd)).cpu().numpy()
    np.testing.assert_array_equal(planes, c4_ref(quantize_ref(x, am, 3)))
    img = decode(planes)[..., :c].transpose(0, 3, 1, 2)
    assert_edge_codes(np.ascontiguousarray(img), x, am, 3)
