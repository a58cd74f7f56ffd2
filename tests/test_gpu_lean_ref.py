"""The lean static-range epilogue (int8 limb planes only: almost every conv of the static-range
forward) of every kernel family against a float64 reference of the same operation, to the code:
the LDS-DMA tiles (64- and 128-wide K steps, exact codes and the downsamples' 3 weight limbs), the
halo 3x3 kernel, the weight-stationary 1x1 tiles, and the Bottleneck pair / fused-downsample
launches (tests/lean_ref.py: lean_reference, check_codes, expected_overflow).

Every launch runs twice with its outputs inside pre-filled guard regions (run_guarded): a byte the
kernel leaves unwritten or a store next to the tensor fails the test, which a comparison of two
launches into recycled allocations cannot see. Each case runs in range (factor 2.0 of the
reference's own maximum) and overflowing (0.5), with per-image scales that really differ; launches
of more than 256 images (the per-image scale table of csrc/conv_resident.hip ends there) and the
non-temporal store path are covered too. Every call goes through the C-ABI."""
import os
import subprocess
import sys

import pytest
import torch

import lean_ref
from lean_ref import FACTORS, ChainDsCase, ConvCase, PairCase, run_guarded

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _cfgs(kinds, limbs, wl, cout, cin, k):
    return lean_ref._kind_cfgs(kinds, limbs, wl, cout, cin, k)


def _sweep(case, cfgs, family, layouts=("auto",)):
    """Every config x layout x range factor: guarded launch, codes and flag against the reference.
    (A tensor bitwise equal to one that already passed is not compared element by element again.)"""
    for f in FACTORS:
        passed = []
        for layout in layouts:
            for c in cfgs:
                yq, ovf = case.launch(c, f, layout)
                if not any(torch.equal(yq, p) for p in passed):
                    case.check(yq, ovf, f, family)
                    passed.append(yq)
                else:
                    assert int(ovf.item()) == case.reference(f)[2], (c, f, layout)
        assert int(case.reference(f)[2]) == (1 if f < 1 else 0)


# ---- a. LDS-DMA tiles -------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("limbs", [2, 3])
@pytest.mark.parametrize("shape", [(64, 80, 3, 1, 9), (128, 64, 3, 2, 17), (256, 48, 1, 1, 7), (64, 256, 1, 1, 20)],
                         ids=lambda s: "c%d_o%d_k%d_s%d_h%d" % s)
def test_lds_dma_lean_vs_reference(gpu, shape, limbs, residual, relu):
    """Exact 8-bit codes with weight offsets: partial pixel tiles, partial channel tiles (cout 80,
    48), 1 .. 18 K steps, tiles spanning images; every LDS-DMA config that takes the shape and the
    default tile, row-major and K-major weights."""
    from smpq import ops
    cin, cout, k, s, h = shape
    case = ConvCase(gpu, cin, cout, k, s, h, h, 3, limbs, seed=cin + 3 * cout + limbs, residual=residual, relu=relu,
                    need_offsets=True)
    cfgs = _cfgs((ops.TILE_LDS_DMA, ops.TILE_LDS_DMA_K128), limbs, 1, cout, cin, k)
    assert any(ops.tile_kind(c) == ops.TILE_LDS_DMA for c in cfgs)
    assert cin % 128 != 0 or any(ops.tile_kind(c) == ops.TILE_LDS_DMA_K128 for c in cfgs)
    _sweep(case, [-1] + cfgs, "LDS-DMA, exact codes", layouts=("auto", "rowmajor"))


@pytest.mark.parametrize("shape", [(64, 256, 1, 1, 9), (256, 512, 1, 2, 9)], ids=lambda s: "c%d_o%d_k%d_s%d_h%d" % s)
def test_lds_dma_lean_three_weight_limbs_vs_reference(gpu, shape):
    """The downsample form: 24-bit fixed-point weights (3 limbs, the three lowest limb-pair products
    skipped), 3 activation limbs, no ReLU."""
    from smpq import ops
    cin, cout, k, s, h = shape
    case = ConvCase(gpu, cin, cout, k, s, h, h, 3, 3, wl=3, seed=cin + cout, relu=False)
    cfgs = _cfgs((ops.TILE_LDS_DMA, ops.TILE_LDS_DMA_K128), 3, 3, cout, cin, k)
    assert cfgs
    _sweep(case, [-1] + cfgs, "LDS-DMA, 3 weight limbs", layouts=("auto", "rowmajor"))


# ---- b. halo 3x3 -------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("offsets", [True, False])
@pytest.mark.parametrize("limbs", [2, 3])
@pytest.mark.parametrize("shape", [(64, 64, 13, 17, 3), (128, 64, 5, 6, 3), (512, 512, 7, 7, 3)],
                         ids=lambda s: "c%d_o%d_%dx%d_n%d" % s)
def test_halo_lean_vs_reference(gpu, shape, limbs, offsets, residual):
    from smpq import ops
    cin, cout, h, w, n = shape
    case = ConvCase(gpu, cin, cout, 3, 1, h, w, n, limbs, seed=cin + cout + w + limbs, residual=residual, relu=True,
                    offsets=offsets, need_offsets=True)
    cfgs = _cfgs((ops.TILE_HALO3X3,), limbs, 1, cout, cin, 3)
    assert cfgs
    _sweep(case, cfgs, "halo 3x3", layouts=("auto", "rowmajor"))


# ---- c. weight-stationary 1x1 tiles -----------------------------------------------------------
RES_SHAPES = [(64, 256, 3, 5, 1), (64, 256, 5, 9, 2), (256, 512, 2, 9, 2), (512, 64, 1, 7, 1), (1024, 256, 2, 7, 1)]


@pytest.mark.parametrize("form", ["wl3", "res_relu", "offsets_relu"])
@pytest.mark.parametrize("cin,cout,n,h,stride", RES_SHAPES)
def test_resident_lean_vs_reference(gpu, cin, cout, n, h, stride, form):
    """3 weight limbs (the downsamples: no ReLU, no residual), exact codes with a limb-plane
    residual + ReLU, and exact codes with weight offsets + ReLU, on every resident config that
    takes the shape (1024 -> 256 with 3 weight limbs is over the register budget: none)."""
    from smpq import ops
    wl = 3 if form == "wl3" else 1
    cfgs = _cfgs((ops.TILE_RESIDENT1X1,), 3, wl, cout, cin, 1)
    if not cfgs:
        assert wl == 3 and cin == 1024
        return
    kw ={"wl3": dict(wl=3, relu=False), "res_relu": dict(residual=True, offsets=False, bits=(6, 4)),
          "offsets_relu": dict(need_offsets=True)}[form]
    case = ConvCase(gpu, cin, cout, 1, stride, h, h, n, 3, seed=cin + cout + 7 * n + h, **kw)
    _sweep(case, cfgs, "resident 1x1")


# ---- d. pair and chain launches ---------------------------------------------------------------
PAIR_FACTORS = ((2.0, 2.0), (0.5, 2.0), (2.0, 0.5))


@pytest.mark.parametrize("cout2,n,h", [(64, 3, 9), (128, 1, 3)])
def test_pair_lean_vs_reference(gpu, cout2, n, h):
    """conv3 against the reference; the chained conv1 against the reference fed with the kernel's
    own conv3 codes, its per-image input scales differing between the images."""
    case = PairCase(gpu, n, h, cout2, seed=31 + h)
    for f1, f2 in PAIR_FACTORS:
        p1, p2, ovf = case.launch(f1, f2)
        case.check(p1, p2, ovf, f1, f2, "pair")
        assert int(ovf.item()) == (1 if min(f1, f2) < 1 else 0)


@pytest.mark.parametrize("offsets", [False, True])
@pytest.mark.parametrize("cin,cout,ds_cin,st,n,h,hd", [(64, 256, 64, 1, 3, 9, 9), (128, 512, 256, 2, 3, 5, 9),
                                                       (256, 1024, 512, 2, 1, 3, 5)])
def test_chain_downsample_lean_vs_reference(gpu, cin, cout, ds_cin, st, n, h, hd, offsets):
    """The fused launch never writes the downsample's codes: conv3's reference takes the separate
    downsample launch's (checked against the reference here too)."""
    case = ChainDsCase(gpu, cin, cout, ds_cin, st, n, h, hd, offsets, seed=5 * h + n + cin)
    for fd, f1 in PAIR_FACTORS:
        yd, ovd = case.downsample(fd, f1)
        p1, ovf = case.launch(fd, f1)
        case.check(yd, ovd, p1, ovf, fd, f1, "chain with fused downsample")
        assert int(ovf.item()) == (1 if min(fd, f1) < 1 else 0)


# ---- e. more than 256 images ------------------------------------------------------------------
def _scales_differ_past_256(am, n):
    a = am.cpu()
    assert n > 256 and len(set(a[256:].tolist())) == n - 256 and not set(a[256:].tolist()) & set(a[:256].tolist())


@pytest.mark.parametrize("cin,cout,n,h,stride,form", [(64, 256, 260, 3, 1, "wl3"), (64, 256, 258, 3, 1, "res_relu"),
                                                      (256, 512, 257, 5, 2, "wl3")])
def test_resident_more_than_256_images(gpu, cin, cout, n, h, stride, form):
    """Past the LDS scale table the per-image scale comes from memory inside the tile loop: against
    the reference, and bitwise the default LDS-DMA tile's planes and flag."""
    from smpq import ops
    kw = dict(wl=3, relu=False) if form == "wl3" else dict(residual=True, offsets=False, bits=(6, 4))
    case = ConvCase(gpu, cin, cout, 1, stride, h, h, n, 3, seed=n + cin, **kw)
    _scales_differ_past_256(case.am, n)
    cfgs = _cfgs((ops.TILE_RESIDENT1X1,), 3, kw.get("wl", 1), cout, cin, 1)
    assert cfgs
    for f in FACTORS:
        y0, o0 = case.launch(-1, f)
        case.check(y0, o0, f, "more than 256 images")
        for c in cfgs:
            yq, ovf = case.launch(c, f)
            assert torch.equal(yq, y0) and torch.equal(ovf, o0), (c, f)


def test_pair_more_than_256_images(gpu):
    case = PairCase(gpu, 259, 3, 64, seed=77)
    _scales_differ_past_256(case.am, 259)
    for f1, f2 in PAIR_FACTORS:
        am1 = case.ranges(f1, f2)[2].cpu()
        assert len(set(am1.tolist())) == 3 and am1[256] != am1[257] != am1[258]
        p1, p2, ovf = case.launch(f1, f2)
        case.check(p1, p2, ovf, f1, f2, "more than 256 images")
        y1, y2, o0 = case.separate(f1, f2)
        assert torch.equal(p1, y1) and torch.equal(p2, y2) and torch.equal(ovf, o0), (f1, f2)


@pytest.mark.parametrize("cin,cout,ds_cin,st,n,h,hd", [(64, 256, 64, 1, 261, 3, 3), (128, 512, 256, 2, 257, 3, 5)])
def test_chain_downsample_more_than_256_images(gpu, cin, cout, ds_cin, st, n, h, hd):
    case = ChainDsCase(gpu, cin, cout, ds_cin, st, n, h, hd, True, seed=n + cin)
    _scales_differ_past_256(case.am, n)
    _scales_differ_past_256(case.amb, n)
    for fd, f1 in PAIR_FACTORS:
        yd, ovd = case.downsample(fd, f1)
        p1, ovf = case.launch(fd, f1)
        case.check(yd, ovd, p1, ovf, fd, f1, "more than 256 images")
        y1, o0 = case.separate(fd, f1)
        assert torch.equal(p1, y1) and torch.equal(ovf, o0), (fd, f1)


# ---- f. non-temporal stores -------------------------------------------------------------------
def test_non_temporal_stores_bitwise(gpu, tmp_path):
    """One case of every family in a child process started with SMPQ_NT_MIN_MB=0 (checked against
    the reference and guarded there) gives the planes and flags of this process, whose outputs are
    all below the default 64 MB threshold, bit for bit. That the child's launches take the
    non-temporal store is known from reading csrc/conv.hip (conv_args_q: nt_store = yq &&
    limbs * M * cout >= nt_min, nt_min read once per process from SMPQ_NT_MIN_MB; the chain launches
    build their arguments with the same function): with the threshold at 0 the comparison holds for
    every call. There is no runtime observable for it."""
    assert os.environ.get("SMPQ_NT_MIN_MB") is None
    out = os.path.join(str(tmp_path), "nt.pt")
    env = dict(os.environ, SMPQ_NT_MIN_MB="0", PYTHONUNBUFFERED="1")
    if env.get("SMPQ_LEAN_REF_STATS"):
        env["SMPQ_LEAN_REF_STATS"] += ".nt"
    p = subprocess.Popen([sys.executable, os.path.join(HERE, "lean_nt_worker.py"), out], env=env)
    try:
        rc = p.wait(timeout=300)
    finally:
        if p.poll() is None:
            p.kill()
    assert rc == 0, rc
    got = torch.load(out, weights_only=True)
    want = lean_ref.nt_cases(gpu)
    assert sorted(got) == sorted(want) and len(want) >= 14
    for name in want:
        assert len(got[name]) == len(want[name])
        for a, b in zip(got[name], want[name]):
            assert torch.equal(a, b), name


# ---- g. the stem and the max pool under the same guard ----------------------------------------
@pytest.mark.parametrize("limbs", [1, 2, 3])
@pytest.mark.parametrize("nhw", [(3, 40, 36), (1, 32, 64)])
def test_stem_pool_guarded(gpu, limbs, nhw):
    """conv1 + bn1 + relu + maxpool in one launch, guarded: equal to stem_conv_s2d + maxpool_limbs
    (both guarded too), in range and overflowing."""
    from smpq import ops
    n, h, w = nhw
    g = torch.Generator().manual_seed(31 + limbs + h)
    wt = (torch.randn(64, 3, 7, 7, generator=g) * 0.1).to(gpu)
    x = torch.randn(n, 3, h, w, generator=g).to(gpu)
    x[0] *= 3.0
    am = ops.act_absmax(x)
    codes, wscale = ops.pack_weights_s2d(wt, max(2, limbs))
    cs = (wscale * torch.linspace(-1.0, 2, 64, device=gpu)).contiguous()
    cs[5] = 0.0
    sh = torch.linspace(-1, 1, 64, device=gpu).contiguous()
    xs = ops.image_quantize_s2d(x, am, limbs)
    assert ops.stem_pool_supported(xs, codes, h, w)
    y = ops.stem_conv_s2d(xs, am, codes, h, w, cs, sh, relu=True)
    for frac, want_ovf in ((1.5, 0), (0.3, 1)):
        rng = float(y.abs().max()) * frac

        def two():
            o = torch.zeros(1, dtype=torch.int32, device=gpu)
            _, yq = ops.stem_conv_s2d(xs, am, codes, h, w, cs, sh, relu=True, emit_range=rng, overflow=o,
                                      want_f32=False)
            return ops.maxpool_limbs(yq), yq, o

        def fused():
            o = torch.zeros(1, dtype=torch.int32, device=gpu)
            return ops.stem_pool_s2d(xs, am, codes, h, w, cs, sh, emit_range=rng, overflow=o), o
        ref, _, o2 = run_guarded(two)
        got, o1 = run_guarded(fused)
        assert got.shape == ref.shape == (limbs, n, h // 4, w // 4, 64)
        assert torch.equal(got, ref), (frac, (got != ref).sum().item())
        assert int(o1.item()) == int(o2.item()) == want_ovf


@pytest.mark.parametrize("limbs", [1, 2, 3])
def test_maxpool_limbs_guarded(gpu, limbs):
    import torch.nn.functional as F
    from smpq import ops
    g = torch.Generator().manual_seed(5 + limbs)
    x = torch.relu(torch.randn(3, 17, 22, 32, generator=g)).to(gpu)
    rng = torch.full((3,), float(x.abs().max()) * 1.3, device=gpu)
    xq = ops.act_quantize(x, rng, limbs)
    pooled = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(run_guarded(lambda: ops.maxpool_limbs(xq)), ops.act_quantize(pooled, rng, limbs))
