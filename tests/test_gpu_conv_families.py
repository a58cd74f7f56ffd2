"""The grouped, dilated, narrow-channel and 3x3-stem conv kernels (csrc/conv_grouped.hip, conv_dilated.hip,
conv_narrow.hip, conv_stem3.hip) where their own test files do not reach:

  A. tile walks: one launch in which workgroups walk three tiles across image borders against launches
     in which no workgroup walks, bit for bit, the latter against the float64 emulation;
  B. one and three images (and, for dilated, grids of 4, 12 and 20 blocks: the tail of the XCD remap);
  C. every output form (fp32 + y_absmax, limb planes, both at once) in guarded buffers
     (lean_ref.run_guarded: an unwritten byte or a store next to the tensor shows);
  D. exact codes launched without offsets;
  E. the dilated kernel's two weight layouts, and the wrappers' image chunks;
  F. (CPU) the two weight transformations the grouped and dilated references stand on.

Every reference is family_cases' float64 emulation on the kernel's own codes; the tolerances are the
project's (2e-6 * bound for fp32, check_codes' 0.5 + 2e-6 B for codes, bitwise between two launches).
The static ranges are 2.0 and 0.5 times the reference's own maximum: the largest |z| is QMAX / 2 or
2 QMAX, so expected_overflow never meets an element inside its tolerance band.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from family_cases import (DILATED_SHAPES, GROUPED_SHAPES, NARROW_SHAPES, STEM3_SHAPES, block_diagonal, dilated_case,
                          grouped_case, narrow_case, stem3_case, zero_inflate)
from lean_ref import check_codes, decode, emit_range_for, expected_overflow, residual_planes, to_code_units
from test_gpu import LIMB_QMAX, emulate_limbs

gpu_test = pytest.mark.gpu
FACTORS = (2.0, 0.5)  # a range that holds, one that clamps
WEIGHTS = ["x8_off", "x8_bare", "w3"]  # exact codes with offsets, exact codes without, 3 weight limbs


def _ids(fmt):
    """Parameter ids: a shape tuple through fmt, anything else as it prints."""
    return lambda v: fmt % v if isinstance(v, tuple) else str(v)


G_ID, D_ID = _ids("c%d_o%d_g%d_s%d_h%d"), _ids("c%d_o%d_d%d_h%d_w%d")
N_ID, S_ID = _ids("c%d_o%d_k%d_s%d_h%d_w%d"), _ids("c%d_o%d_h%d_w%d")


def _weights(name):
    """(weight limbs, keep the offsets) of a WEIGHTS name."""
    return (3, True) if name == "w3" else (1, name == "x8_off")


def _residual(gpu, case, kind, shape_out, seed=9):
    """(keywords of conv2d_narrow_q, the residual in real units on the host) for n images of shape_out."""
    n = case.n
    if kind is None:
        return None, None
    if kind == "fp32":
        r = torch.randn(n, *shape_out, generator=torch.Generator().manual_seed(seed)).to(gpu)
        return {"residual": r}, r.cpu().numpy().astype(np.float64)
    rq, rr = residual_planes(gpu, n, *shape_out, 3, seed)
    return ({"residual_q": rq, "residual_range": rr},
            decode(rq).astype(np.float64) * np.float64(np.float32(rr) / np.float32(LIMB_QMAX[3])))


def full_check(case, relu, guard=True, images=None, res=None, rhost=None):
    """The three output forms of images [i0, i1) against the emulation: fp32 within 2e-6 * bound, y_absmax
    the kernel's own maximum, the codes of both epilogues through check_codes, the overflow word as the
    reference fixes it, and the fp32 of the everything-at-once form bitwise that of the fp32 form."""
    i0, i1 = images or (0, case.n)
    y, bound = case.reference(images, None if rhost is None else rhost[i0:i1])
    ye = np.maximum(y, 0) if relu else y
    yk, yam, _, _ = case.launch("fp32", relu, images=images, guard=guard, res=res)
    ykn = yk.cpu().numpy()
    assert ykn.shape == y.shape
    err = np.abs(ykn.astype(np.float64) - ye)
    assert (err <= 2e-6 * bound + 1e-30).all(), ("emulation mismatch", float((err / (bound + 1e-30)).max()))
    np.testing.assert_array_equal(yam.cpu().numpy(), np.abs(ykn).reshape(i1 - i0, -1).max(1))
    for factor in FACTORS:
        rng = emit_range_for(y, relu, factor)
        z, B = to_code_units(y, bound, relu, rng, 3)
        want = expected_overflow(z, B, 3)
        assert want == (factor < 1)
        _, _, yq, ovf = case.launch("planes", relu, rng, images=images, guard=guard, res=res)
        check_codes(yq, z, B, relu, 3)
        assert int(ovf.item()) == want, ("planes", int(ovf.item()), want)
        y3, yam3, yq3, ovf3 = case.launch("both", relu, rng, images=images, guard=guard, res=res)
        _same(y3, yk, "fp32 of the form with everything vs the fp32 form")
        _same(yam3, yam, "y_absmax of the form with everything vs the fp32 form")
        check_codes(yq3, z, B, relu, 3)
        assert int(ovf3.item()) == want, ("both", int(ovf3.item()), want)
    return yk


# ---- A. tile walks ---------------------------------------------------------------------------------------
def _same(a, b, what):
    """Two launches' outputs, bit for bit (the message counts; a tensor's repr says nothing)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        raise AssertionError("%s: %d of %d elements differ" % (what, int((a != b).sum()), a.numel()))


def _thirds(n):
    a, b = (n + 2) // 3, (2 * n + 2) // 3
    return [(0, a), (a, b), (b, n)]


def walk_check(case, tiles_img, gx, budget, relu=True, res=None, rhost=None):
    """One launch over all images == the launches over thirds of them, bit for bit, in the general form with
    everything at once and in the lean form, at both ranges; then the first two images alone == the first
    third's, and against the emulation (full_check). ``budget``: the launch code's workgroup target (gy =
    ceil(budget / gx), capped at the tile count)."""
    n, parts = case.n, _thirds(case.n)
    gy = (budget + gx - 1) // gx
    # the walk, its third tile, the image crossing, and sub-launches that do not walk
    assert n * tiles_img > 2 * gy and gy % tiles_img != 0
    assert all((i1 - i0) * tiles_img <= gy for i0, i1 in parts)
    y2, _ = case.reference((0, 2), None if rhost is None else rhost[0:2])
    first = {}
    for form in ("both", "planes"):
        for factor in FACTORS:
            rng = emit_range_for(y2, relu, factor)
            whole = case.launch(form, relu, rng, res=res)
            ps = [case.launch(form, relu, rng, images=p, res=res) for p in parts]
            what = "walk vs thirds, form %s, range factor %s: " % (form, factor)
            if form == "both":
                _same(whole[0], torch.cat([p[0] for p in ps]), what + "y")
                _same(whole[1], torch.cat([p[1] for p in ps]), what + "y_absmax")
            _same(whole[2], torch.cat([p[2] for p in ps], dim=1), what + "yq")
            assert int(whole[3].item()) == max(int(p[3].item()) for p in ps), what + "overflow"
            assert factor > 1 or int(whole[3].item()) == 1
            first[(form, factor)] = ps[0]
    # the chain's end: two images of a launch that does not walk, against the emulation
    full_check(case, relu, guard=False, images=(0, 2), res=res, rhost=rhost)
    for (form, factor), p in first.items():
        two = case.launch(form, relu, emit_range_for(y2, relu, factor), images=(0, 2), res=res)
        _same(two[2], p[2][:, :2], "two images vs the first third: yq")
        if form == "both":
            _same(two[0], p[0][:2], "two images vs the first third: y")
            _same(two[1], p[1][:2], "two images vs the first third: y_absmax")


# narrow: 8 x 8 tiles, gx = ceil(cout / 64), gy = ceil(1024 / gx). (shape, n, residual):
NARROW_WALKS = [
    # resident 3x3 (7 steps): 17 x 17 -> 9 tiles / image, gx 1, gy 1024; 228 images = 2052 tiles > 2048;
    # thirds of 76 images = 684 tiles; 1024 % 9 = 7
    ((48, 64, 3, 1, 17, 17), 228, None),
    # streaming, one slab (23 steps): 9 tiles / image, gx 2, gy 512; 114 images = 1026 tiles > 1024; thirds of
    # 38 images = 342 tiles; 512 % 9 = 8
    ((160, 128, 3, 1, 17, 17), 114, None),
    # two slabs (11 + 2 chunks), stride 2: 18 x 33 -> 9 x 17 -> 6 tiles / image, gx 4, gy 256; 86 images = 516
    # tiles > 512; thirds of at most 29 images = 174 tiles; 256 % 6 = 4
    ((208, 256, 3, 2, 18, 33), 86, None),
    # five fragments: the second workgroup column has three idle waves; 9 tiles / image, gx 2, gy 512; 114
    # images = 1026 tiles; thirds of 342 tiles; 512 % 9 = 8
    ((48, 80, 3, 1, 17, 17), 114, None),
    # 1x1 (resident, 2 steps) with the limb-plane residual: 9 tiles / image, gx 2, gy 512; 114 images = 1026
    # tiles; thirds of 342 tiles; 512 % 9 = 8
    ((96, 128, 1, 1, 17, 17), 114, "planes"),
]


def _narrow_out(shape):
    cin, cout, k, stride, h, w_ = shape
    return (h + 2 * (k // 2) - k) // stride + 1, (w_ + 2 * (k // 2) - k) // stride + 1, cout


@gpu_test
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("shape,n,residual", NARROW_WALKS, ids=N_ID)
def test_narrow_tile_walk_bitwise(gpu, shape, n, residual, weights):
    wl, offsets = _weights(weights)
    case = narrow_case(gpu, shape, wl, n=n, offsets=offsets)
    ho, wo, cout = _narrow_out(shape)
    res, rhost = _residual(gpu, case, residual, (ho, wo, cout))
    walk_check(case, ((ho + 7) // 8) * ((wo + 7) // 8), (cout // 16 + 3) // 4, 1024, res=res, rhost=rhost)


# stem3: 8-row x 16-column tiles, gx = cout / 64, gy = ceil(512 / gx). (shape, n):
STEM3_WALKS = [
    # 17 x 17 -> 3 x 2 = 6 tiles / image, gx 1, gy 512; 171 images = 1026 tiles > 1024 (a workgroup's third tile
    # is staged where its first was); thirds of 57 images = 342 tiles; 512 % 6 = 2
    ((3, 64, 17, 17), 171),
    # gx 2, gy 256; 86 images = 516 tiles > 512; thirds of at most 29 images = 174 tiles; 256 % 6 = 4
    ((3, 128, 17, 17), 86),
]


@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape,n", STEM3_WALKS, ids=S_ID)
def test_stem3_tile_walk_bitwise(gpu, shape, n, relu):
    c, cout, h, w_ = shape
    walk_check(stem3_case(gpu, shape, n=n), ((h + 7) // 8) * ((w_ + 15) // 16), cout // 64, 512, relu=relu)


# grouped: 8 x 8 tiles, gx = ceil(cout / 64), gy = ceil(1024 / gx). (shape, wl, n):
GROUPED_WALKS = [
    # stride 2: 33 x 33 -> 17 x 17 -> 9 tiles / image, gx 2, gy 512; 114 images = 1026 tiles > 1024; thirds of 38
    # images = 342 tiles; 512 % 9 = 8
    ((128, 128, 16, 2, 33), 1, 114),
    # 3 weight limbs: 9 tiles / image, gx 1, gy 1024; 228 images = 2052 tiles > 2048; thirds of 76 images = 684
    # tiles; 1024 % 9 = 7
    ((64, 64, 16, 1, 17), 3, 228),
    # 48 channels in 3 groups (the fourth wave idle between the walk's barriers): as the case above
    ((48, 48, 3, 1, 17), 1, 228),
]


@gpu_test
@pytest.mark.parametrize("shape,wl,n", GROUPED_WALKS, ids=G_ID)
def test_grouped_tile_walks_bitwise(gpu, shape, wl, n):
    cin, cout, groups, stride, h = shape
    ho = (h - 1) // stride + 1
    walk_check(grouped_case(gpu, shape, wl, n=n), ((ho + 7) // 8) ** 2, (cout // 16 + 3) // 4, 1024)


# ---- B. one and three images; the dilated remap's tail ---------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", [GROUPED_SHAPES[0], GROUPED_SHAPES[3]], ids=G_ID)
def test_grouped_odd_batches(gpu, shape, n, wl, relu):
    full_check(grouped_case(gpu, shape, wl, n=n), relu)


# one channel tile, one 8 x 8 lattice tile per phase (lattices of 5 and 4), d^2 = 4 phases: 4 n blocks. n = 1: 4
# blocks (full = 0, the remap never applies); n = 3: 12 blocks (the remap on blocks 0 .. 7, where it is the
# identity, blocks 8 .. 11 its tail); n = 5: 20 blocks (a remap that permutes blocks 0 .. 15, a tail of 4).
# The second shape: the same counts with two input chunks.
@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 5])
@pytest.mark.parametrize("shape", [(64, 64, 2, 9, 9), (128, 64, 2, 9, 9)], ids=D_ID)
def test_dilated_odd_batches_and_remap_tail(gpu, shape, n, wl, relu):
    cin, cout, d, h, w_ = shape
    assert n * d * d * ((-(-h // d) + 7) // 8) * ((-(-w_ // d) + 7) // 8) * (cout // 64) == 4 * n
    full_check(dilated_case(gpu, shape, wl, n=n), relu)


@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape,residual", [(NARROW_SHAPES[2], None), (NARROW_SHAPES[3], "planes")],
                         ids=N_ID)
def test_narrow_odd_batches(gpu, shape, residual, n, wl, relu):
    case = narrow_case(gpu, shape, wl, n=n)
    res, rhost = _residual(gpu, case, residual, _narrow_out(shape))
    full_check(case, relu, res=res, rhost=rhost)


@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("n", [1, 3])
def test_stem3_odd_batches(gpu, n, relu):
    full_check(stem3_case(gpu, STEM3_SHAPES[1], n=n), relu)


# ---- C. guarded outputs at the families' partial-tile shapes ---------------------------------------------------
@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape", GROUPED_SHAPES, ids=G_ID)
def test_grouped_guarded_forms(gpu, shape, wl, relu):
    full_check(grouped_case(gpu, shape, wl), relu)


# two images give every shape a grid that is a multiple of 8 blocks (the remap covers it all); the last two
# entries are B's grids of 12 and 4 blocks, where a tile the remap loses shows as unwritten bytes
@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape,n", [(s, 2) for s in DILATED_SHAPES] + [((64, 64, 2, 9, 9), 3),
                                                                        ((128, 64, 2, 9, 9), 1)], ids=D_ID)
def test_dilated_guarded_forms(gpu, shape, n, wl, relu):
    full_check(dilated_case(gpu, shape, wl, n=n), relu)


@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape", NARROW_SHAPES, ids=N_ID)
def test_narrow_guarded_forms(gpu, shape, wl, relu):
    full_check(narrow_case(gpu, shape, wl), relu)


@gpu_test
@pytest.mark.parametrize("residual", ["fp32", "planes"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("wl", [1, 3])
def test_narrow_guarded_forms_residual(gpu, wl, relu, residual):
    shape = NARROW_SHAPES[3]  # the 1x1
    case = narrow_case(gpu, shape, wl)
    res, rhost = _residual(gpu, case, residual, _narrow_out(shape))
    full_check(case, relu, res=res, rhost=rhost)


# (the last stem shape is the two-tile walk of test_gpu_stem3.py: 16 MB of output, walked above at 17 x 17)
@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("shape", STEM3_SHAPES[:-1], ids=S_ID)
def test_stem3_guarded_forms(gpu, shape, relu):
    full_check(stem3_case(gpu, shape), relu)


# ---- D. exact codes without offsets (the <LW = 1, OFF = false> instantiations) ---------------------------------
@gpu_test
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("family,shape", [("grouped", GROUPED_SHAPES[0]), ("grouped", GROUPED_SHAPES[3]),
                                          ("grouped", GROUPED_SHAPES[6]), ("dilated", DILATED_SHAPES[1]),
                                          ("dilated", DILATED_SHAPES[2]), ("narrow", NARROW_SHAPES[2]),
                                          ("narrow", NARROW_SHAPES[3]), ("narrow", NARROW_SHAPES[6])],
                         ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else v)
def test_exact_codes_without_offsets(gpu, family, shape, relu):
    builder = {"grouped": grouped_case, "dilated": dilated_case, "narrow": narrow_case}[family]
    case = builder(gpu, shape, 1, offsets=False)
    assert case.offset is None and case.operands[3] is None
    full_check(case, relu)


# ---- E. layouts and image chunks -------------------------------------------------------------------------------
def _all_forms(case, relu, rng, **kw):
    return [t for form in ("fp32", "planes", "both") for t in case.launch(form, relu, rng, **kw) if t is not None]


@gpu_test
@pytest.mark.parametrize("wl", [1, 3])
@pytest.mark.parametrize("shape", [DILATED_SHAPES[1], DILATED_SHAPES[2]], ids=D_ID)
def test_dilated_weight_layouts_bitwise(gpu, monkeypatch, shape, wl):
    from smpq import ops
    case = dilated_case(gpu, shape, wl, n=3)
    assert ops.KMAJOR[0] and getattr(case.codes, "_smpq_km", None) is not None
    rng = emit_range_for(case.reference()[0], True, 2.0)
    kmajor = _all_forms(case, True, rng)
    monkeypatch.setattr(ops, "KMAJOR", [False])  # what SMPQ_KMAJOR=0 sets: the kernel stages the dense pack
    dense = _all_forms(case, True, rng)
    assert len(kmajor) == len(dense) == 8
    for i, (a, b) in enumerate(zip(kmajor, dense)):
        _same(a, b, "K-major vs dense pack, output %d" % i)


def _chunk_cases(gpu):
    narrow = narrow_case(gpu, NARROW_SHAPES[3], 1, n=3)
    return {"grouped": (grouped_case(gpu, GROUPED_SHAPES[0], 1, n=3), None),
            "dilated": (dilated_case(gpu, DILATED_SHAPES[0], 1, n=3), None),
            "narrow": (narrow, _residual(gpu, narrow, "planes", _narrow_out(NARROW_SHAPES[3]))[0]),
            "stem3": (stem3_case(gpu, STEM3_SHAPES[1], n=3), None)}


@gpu_test
@pytest.mark.parametrize("form", ["fp32", "planes", "both"])
@pytest.mark.parametrize("family", ["grouped", "dilated", "narrow", "stem3"])
def test_image_chunks_bitwise(gpu, monkeypatch, family, form):
    """PLANE_LIMIT lowered so that three images run as 2 + 1: every output, a y_absmax and an out passed in, the
    limb planes copied together and the shared overflow word equal the single launch's."""
    from smpq import ops
    case, res = _chunk_cases(gpu)[family]
    seen = []
    chunks_of = ops._image_chunks

    def spy(n, per_img, what):
        seen.append((n, per_img, chunks_of(n, per_img, what)))
        return seen[-1][2]
    monkeypatch.setattr(ops, "_image_chunks", spy)
    yref = case.reference()[0]
    rng = emit_range_for(yref, True, 0.5)  # clamps: the overflow word is set

    def run():
        ovf, yam = torch.zeros(1, dtype=torch.int32, device=gpu), torch.zeros(3, device=gpu)
        out = None if form == "planes" else torch.full(yref.shape, float("nan"), device=gpu)
        r = case.launch(form, True, rng, res=res, out=out, y_absmax=yam, overflow=ovf)
        assert r[0] is out and (r[1] is None or r[1] is yam) and (r[3] is None or r[3] is ovf)
        return [t for t in r if t is not None]
    single = run()
    assert len(seen) == 1 and seen[0][0] == 3 and seen[0][2] is None
    per_img = seen[0][1]
    del seen[:]
    monkeypatch.setattr(ops, "PLANE_LIMIT", 2 * per_img + per_img // 2)
    chunked = run()
    assert [c[2] for c in seen] == [[(0, 2), (2, 3)], None, None]
    assert len(single) == len(chunked) == {"fp32": 2, "planes": 2, "both": 4}[form]
    for i, (a, b) in enumerate(zip(single, chunked)):
        _same(a, b, "one launch vs chunks of 2 + 1, output %d" % i)
    if form != "fp32":
        assert int(single[-1].item()) == 1


# ---- F. the reference's weight transformations (CPU) -----------------------------------------------------------
def _ints(g, *shape):
    return torch.randint(-9, 10, shape, generator=g).double()


def _emulated(x_nchw, dense, k, stride, pad):
    """emulate_limbs as the GPU tests call it, on one 'limb' of small integers with unit scales: the exact
    conv of x with the dense weight [cout, k, k, cin] -> NCHW."""
    n, cout = x_nchw.shape[0], dense.shape[0]
    y, _ = emulate_limbs(x_nchw.permute(0, 2, 3, 1).numpy()[None], dense[None], k, stride, pad, np.ones(n),
                         np.ones(cout), np.zeros(cout), None, False)
    return torch.from_numpy(y).permute(0, 3, 1, 2)


def test_reference_weight_transformations_are_exact():
    g = torch.Generator().manual_seed(0)
    # (cin, cout, groups, stride, H, W): cg == og; cg != og either way, stride 2, odd and even sizes
    for cin, cout, groups, stride, h, w_ in ((8, 8, 4, 1, 5, 6), (6, 12, 3, 2, 7, 4), (12, 4, 2, 2, 6, 9),
                                             (4, 6, 2, 1, 1, 3)):
        w, x = _ints(g, cout, cin // groups, 3, 3), _ints(g, 2, cin, h, w_)
        dense = block_diagonal(w.permute(0, 2, 3, 1).numpy()[None], groups)[0]
        assert dense.shape == (cout, 3, 3, cin)
        want = F.conv2d(x, w, stride=stride, padding=1, groups=groups)
        assert torch.equal(F.conv2d(x, torch.from_numpy(dense).permute(0, 3, 1, 2), stride=stride, padding=1), want)
        assert torch.equal(_emulated(x, dense, 3, stride, 1), want)
    # (cin, cout, d, H, W): d smaller than, equal to and larger than the image
    for cin, cout, d, h, w_ in ((3, 4, 2, 5, 6), (2, 3, 4, 4, 9), (2, 2, 8, 5, 11), (1, 2, 8, 3, 2)):
        w, x = _ints(g, cout, cin, 3, 3), _ints(g, 2, cin, h, w_)
        big = zero_inflate(w.permute(0, 2, 3, 1).numpy()[None], d)[0]
        assert big.shape == (cout, 2 * d + 1, 2 * d + 1, cin) and np.count_nonzero(big) <= 9 * cout * cin
        want = F.conv2d(x, w, dilation=d, padding=d)
        assert want.shape == (2, cout, h, w_)
        assert torch.equal(F.conv2d(x, torch.from_numpy(big).permute(0, 3, 1, 2), padding=d), want)
        assert torch.equal(_emulated(x, big, 2 * d + 1, 1, d), want)
