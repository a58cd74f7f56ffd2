"""Slab groups in the fused-downsample chains (csrc/conv_resident.hip, SG > 1;
smpq_conv2d_chain_fwd_sg): a workgroup of 8 waves holds two slabs of conv3's channels and stages each
activation tile once for both. For every instantiation built (256 -> 1024 + ds 512 / 2 with and
without conv3 weight offsets, 128 -> 512 + ds 256 / 2 without), the launch with two slab groups is
bit for bit the launch with one and the separate launches (downsample, then conv3 + residual + ReLU),
overflow flag included, with every output between pre-filled guard regions (lean_ref.run_guarded).

Shapes (n, output h, stage-input h): 75 pixels with a partial last 16-pixel tile and tiles that
straddle images; one pixel (one tile, fewer tiles than workgroups); 257 images (per-image scales
read from memory past the 256-entry LDS table); 147 pixels = 10 tiles (layer 3: one whole round of 8
tile walkers in the XCD order and a tail of 2); and the smallest at which a workgroup walks more than
one tile (both stages, the deferred copy-out): more tiles than 256 CUs / super-slabs, 37 for layer 3
and 147 for layer 2. Column scales are negative in part and zero for one channel of each conv."""
import pytest
import torch

from lean_ref import acts, run_guarded, weights

pytestmark = pytest.mark.gpu

L3, L2 = (256, 1024, 512), (128, 512, 256)
INSTANCES = [(L3, False), (L3, True), (L2, False)]
SHAPES = [(3, 5, 10), (1, 1, 2), (257, 1, 2), (3, 7, 13)]
MANY_TILES = {L3: (3, 14, 28), L2: (3, 28, 56)}


def _decode(yq):
    return yq[0].long() + 256 * yq[1].long() + 65536 * yq[2].long()


class Case:
    def __init__(self, gpu, chans, offsets, n, h, hd):
        cin, cout, ds_cin = chans
        seed = 7 * n + h + cin
        self.gpu, self.n, self.chans = gpu, n, chans
        self.xq, self.am = acts(gpu, n, h, h, cin, 3, seed + 1)
        self.codes1, off, s1 = weights(gpu, cin, cout, 1, 1, seed, bits=(8,))
        self.off = off if offsets else None
        assert not offsets or bool((off != 0).any())
        self.xbq, self.amb = acts(gpu, n, hd, hd, ds_cin, 3, seed + 5)
        self.dcodes, _, sd = weights(gpu, ds_cin, cout, 1, 3, seed + 6)
        # negative scales in the lower third of the channels of both convs, and a zero scale
        self.cs1 = (s1 * torch.linspace(-0.75, 1.5, cout, device=gpu)).contiguous()
        self.cs1[5] = 0.0
        self.dcs = (sd * torch.linspace(1.4, -0.7, cout, device=gpu)).contiguous()
        self.dcs[cout - 3] = 0.0
        self.sh1 = torch.linspace(-0.3, 0.3, cout, device=gpu).contiguous()
        self.dsh = torch.linspace(-0.2, 0.2, cout, device=gpu).contiguous()
        # the outputs' magnitudes, from the separate launches with wide ranges
        yd, y1, ovf = self.separate(1e4, 1e4)
        assert int(ovf.item()) == 0
        self.md = float(_decode(yd).abs().max()) * 1e4 / 8323072 + 1e-3
        self.m1 = float(_decode(y1).abs().max()) * 1e4 / 8323072 + 1e-3
        self._sep = {}

    def separate(self, rng_d, rng1):
        from smpq import ops
        ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
        _, yd = ops.conv2d_q(self.xbq, self.amb, self.dcodes, None, 1, 1, 2, 0, self.dcs, self.dsh, relu=False,
                             emit_range=rng_d, overflow=ovf, want_f32=False)
        _, y1 = ops.conv2d_q(self.xq, self.am, self.codes1, self.off, 1, 1, 1, 0, self.cs1, self.sh1, relu=True,
                             emit_range=rng1, overflow=ovf, want_f32=False, residual_q=yd, residual_range=rng_d)
        return yd, y1, ovf

    def reference(self, fd, f1):
        """(conv3's planes, the flag) of the separate launches, computed once per range pair."""
        if (fd, f1) not in self._sep:
            self._sep[(fd, f1)] = self.separate(self.md * fd, self.m1 * f1)[1:]
        return self._sep[(fd, f1)]

    def chain(self, fd, f1, sg):
        from smpq import ops
        am1 = torch.full((self.n,), self.m1 * f1, device=self.gpu)

        def fn():
            ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
            p1, p2 = ops.conv_chain_q(self.xq, self.am, self.codes1, self.off, self.cs1, self.sh1, self.m1 * f1, am1,
                                      ovf, ds=(self.xbq, self.amb, self.dcodes, self.dcs, self.dsh, self.md * fd, 2),
                                      sg=sg)
            assert p2 is None
            return p1, ovf
        return run_guarded(fn)


# (downsample range factor, conv3 range factor): in range, and each output past its range
FACTORS = ((2.0, 2.0), (0.5, 3.0), (2.0, 0.5))


def _check(case):
    from smpq import ops
    cin, cout, ds_cin = case.chans
    assert ops.conv_chain_sg_supported(cin, cout, ds_cin, 2, case.off is not None, 2)
    for fd, f1 in FACTORS:
        y1, ovf0 = case.reference(fd, f1)
        assert int(ovf0.item()) == (1 if min(fd, f1) < 1 else 0), (fd, f1)
        a1, o1 = case.chain(fd, f1, 1)
        a2, o2 = case.chain(fd, f1, 2)
        for what, got, flag in (("one slab group", a1, o1), ("two slab groups", a2, o2)):
            assert torch.equal(got, y1), (what, fd, f1, int((got != y1).sum()))
            assert torch.equal(flag, ovf0), (what, fd, f1)


@pytest.mark.parametrize("n,h,hd", SHAPES)
@pytest.mark.parametrize("chans,offsets", INSTANCES)
def test_two_slab_groups_bitwise(gpu, chans, offsets, n, h, hd):
    case = Case(gpu, chans, offsets, n, h, hd)
    if n > 256:  # the scales past the LDS table differ from those in it and from each other
        a = case.am.cpu()
        assert a[256] != a[0] and a[256] != a[255]
    _check(case)


@pytest.mark.parametrize("chans,offsets", INSTANCES)
def test_two_slab_groups_many_tiles_per_workgroup(gpu, chans, offsets):
    case = Case(gpu, chans, offsets, *MANY_TILES[chans])
    _check(case)
    # repeated launches: no race between the tiles, the stages or the slab groups
    y1, ovf0 = case.reference(2.0, 2.0)
    for _ in range(3):
        a2, o2 = case.chain(2.0, 2.0, 2)
        assert torch.equal(a2, y1) and torch.equal(o2, ovf0)


def test_slab_groups_not_built_are_refused(gpu):
    from smpq import ops
    case = Case(gpu, L2, True, 1, 1, 2)  # layer 2 with weight offsets: two groups would spill
    assert not ops.conv_chain_sg_supported(*L2, 2, True, 2)
    am1 = torch.full((1,), 1.0, device=gpu)
    ovf = torch.zeros(1, dtype=torch.int32, device=gpu)
    ds = (case.xbq, case.amb, case.dcodes, case.dcs, case.dsh, 1.0, 2)
    for sg in (2, 4):
        with pytest.raises(ValueError, match="slab groups not built"):
            ops.conv_chain_q(case.xq, case.am, case.codes1, case.off, case.cs1, case.sh1, 1.0, am1, ovf, ds=ds, sg=sg)
    ops.conv_chain_q(case.xq, case.am, case.codes1, case.off, case.cs1, case.sh1, 1.0, am1, ovf, ds=ds)  # (the table: 1)
