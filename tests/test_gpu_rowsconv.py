"""The one-row trial conv on the GPU (csrc/trial_conv.hip, ops.trial_rows_conv) against the conv it
stands in for: ops.conv2d_q in its static limb-plane mode on the same inputs, BITWISE. After the call
the held planes equal the conv's output in the listed channels and the pre-filled baseline in all
others, the guard regions around the planes and the save area are intact, the overflow word equals
the conv's, and after the restore the planes are the baseline again. Shapes: the smallest that reach
a partial pixel tile, unsorted rows, two 64-byte K steps, both limb counts, 3x3 border and interior
pixels, rows patched at 4 bits inside a 3-limb operand, and a range the conv itself overflows."""
import numpy as np
import pytest
import torch

import lean_ref
from lean_ref import GUARD

pytestmark = pytest.mark.gpu

FILL = 0xA5


def _guarded(gpu, nbytes, content):
    """An int8 view of ``nbytes`` bytes holding ``content`` between two guard regions: (buffer, view)."""
    buf = torch.full((2 * GUARD + nbytes,), FILL, dtype=torch.uint8, device=gpu)
    view = buf[GUARD:GUARD + nbytes].view(torch.int8)
    view.copy_(content.reshape(-1))
    return buf, view


def _guards_intact(buf, nbytes):
    return bool((buf[:GUARD] == FILL).all()) and bool((buf[GUARD + nbytes:] == FILL).all())


class Case:
    def __init__(self, gpu, k, L, LW, n, h, w, cin, cout, seed, patch=None):
        from smpq import ops
        self.gpu, self.k, self.pad, self.L = gpu, k, k // 2, L
        self.xq, self.am = lean_ref.acts(gpu, n, h, w, cin, L, seed + 1)
        wt = (torch.randn(cout, cin, k, k, generator=torch.Generator().manual_seed(seed)) * 0.1).to(gpu)
        self.codes, _, wscale, _ = ops.pack_weights_ex(wt, None, LW)
        bn_a = torch.linspace(0.5, 1.5, cout, device=gpu).contiguous()
        self.cs = (wscale * bn_a).contiguous()
        self.sh = torch.linspace(-0.3, 0.3, cout, device=gpu).contiguous()
        if patch:  # rows re-quantized in place, as a sensitivity trial leaves them (both code layouts)
            rows, bits = patch
            save = torch.empty(ops.trial_rows_save_bytes(LW, cin * k * k, len(rows)), dtype=torch.int8, device=gpu)
            status = torch.zeros(len(rows), dtype=torch.int32, device=gpu)
            before = self.codes.clone()
            ops.trial_rows_patch(wt, rows, bits, bn_a, self.codes, wscale, self.cs, save, status,
                                 km=getattr(self.codes, "_smpq_km", None))
            assert status.tolist() == [0] * len(rows) and not torch.equal(before, self.codes)
        self.rq, self.rr = lean_ref.residual_planes(gpu, n, h, w, cout, L, seed + 2)
        y, _ = lean_ref.lean_real(self.xq, self.codes, None, k, 1, self.pad, self.am, self.cs, self.sh, self.rq, self.rr)
        self.ymax = lean_ref.real_max(y, True)

    def conv(self, emit_range):
        """The oracle: the whole conv on the built-in tile; (planes, overflow word)."""
        from smpq import ops
        ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
        y, yq = ops.conv2d_q(self.xq, self.am, self.codes, None, self.k, self.k, 1, self.pad, self.cs, self.sh,
                             relu=True, tile_cfg=-1, emit_range=emit_range, overflow=ovf, want_f32=False,
                             residual_q=self.rq, residual_range=self.rr)
        assert y is None
        return yq, ovf

    def check(self, rows, factor=2.0):
        from smpq import ops
        emit_range = float(np.float32(self.ymax * factor))
        assert emit_range != self.rr  # the residual's range is not the output's
        ref, ref_ovf = self.conv(emit_range)
        L, n, h, w, cout = ref.shape
        M = n * h * w
        g = torch.Generator().manual_seed(3)
        base = torch.randint(-128, 128, ref.shape, generator=g, dtype=torch.int8).to(self.gpu)
        ybuf, yflat = _guarded(self.gpu, base.numel(), base)
        yq = yflat.view(ref.shape)
        nsave = ops.trial_rows_conv_save_bytes(L, M, len(rows))
        sbuf, save = _guarded(self.gpu, nsave, torch.full((nsave,), 0x11, dtype=torch.int8))
        # the conv flags an overflow of ANY channel: the expected word is the listed channels' alone
        qmax = lean_ref.LIMB_QMAX[L]
        ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
        tr = ops.trial_rows_conv(self.xq, self.am, self.codes, self.k, self.k, 1, self.pad, self.cs, self.sh, rows, yq,
                                 emit_range, ovf, save, residual_q=self.rq, residual_range=self.rr)
        torch.cuda.synchronize()
        assert _guards_intact(ybuf, base.numel()) and _guards_intact(sbuf, nsave)
        want = base.clone()
        want[..., rows] = ref[..., rows]
        assert torch.equal(yq, want), "%d bytes differ" % int((yq != want).sum())
        slots = save.view(len(rows), L, M)
        for i, c in enumerate(rows):
            assert torch.equal(slots[i], base.view(L, M, cout)[:, :, c])
        clamped = int((lean_ref.decode(ref[..., rows]) == qmax).sum())
        if factor >= 1:
            assert ref_ovf.item() == 0 and ovf.item() == 0 and clamped == 0
        else:
            # the listed channels hold clamped codes, so both words are set; bitwise equal codes above
            assert clamped > 0 and ref_ovf.item() == 1 and ovf.item() == 1
        ops.trial_rows_conv_restore(tr, yq, save)
        torch.cuda.synchronize()
        assert torch.equal(yq, base) and _guards_intact(ybuf, base.numel())
        return ovf


def test_1x1_partial_tile_unsorted_rows(gpu):
    Case(gpu, 1, 3, 3, 3, 5, 5, 64, 32, seed=201).check([31, 0, 17])  # 75 pixels: one full tile and 11 pixels


def test_1x1_two_k_steps(gpu):
    Case(gpu, 1, 3, 3, 2, 7, 7, 128, 64, seed=202).check([5])


def test_1x1_two_limbs(gpu):
    Case(gpu, 1, 2, 2, 1, 4, 4, 64, 16, seed=203).check([15])


def test_1x1_three_activation_two_weight_limbs(gpu):
    Case(gpu, 1, 3, 2, 2, 3, 3, 64, 16, seed=204).check([9])  # SMIN = 1: one skipped pass


def test_3x3_border_and_interior(gpu):
    Case(gpu, 3, 3, 3, 2, 5, 5, 64, 32, seed=205).check([1, 30])  # K = 576


def test_3x3_every_pixel_at_the_border(gpu):
    Case(gpu, 3, 3, 3, 1, 2, 2, 64, 16, seed=206).check([12])  # 2 x 2: five of nine taps fall outside, for every pixel


def test_rows_patched_at_4_bits_inside_a_three_limb_operand(gpu):
    c = Case(gpu, 1, 3, 3, 2, 5, 5, 64, 32, seed=207, patch=([4, 29], 4))
    c.check([29, 4])
    c.check([7])  # and a row the patch left alone


def test_the_convs_own_overflow(gpu):
    c = Case(gpu, 1, 3, 3, 2, 5, 5, 64, 32, seed=208)
    y, _ = lean_ref.lean_real(c.xq, c.codes, None, 1, 1, 0, c.am, c.cs, c.sh, c.rq, c.rr)
    row = int(np.maximum(y, 0).reshape(-1, 32).max(0).argmax())  # the channel that holds the largest output
    c.check([row], factor=0.5)
    # a channel that stays inside the range leaves the word alone although the conv as a whole overflows
    quiet = int(np.maximum(y, 0).reshape(-1, 32).max(0).argmin())
    from smpq import ops
    rng = float(np.float32(c.ymax * 0.5))
    assert float(np.maximum(y[..., quiet], 0).max()) < 0.9 * rng
    ref, ref_ovf = c.conv(rng)
    yq = ref.clone()
    yq[..., quiet] = 0
    ovf = torch.zeros(1, dtype=torch.int32, device=gpu)
    save = torch.empty(ops.trial_rows_conv_save_bytes(3, 50, 1), dtype=torch.int8, device=gpu)
    ops.trial_rows_conv(c.xq, c.am, c.codes, 1, 1, 1, 0, c.cs, c.sh, [quiet], yq, rng, ovf, save, residual_q=c.rq,
                        residual_range=c.rr)
    assert ref_ovf.item() == 1 and ovf.item() == 0 and torch.equal(yq, ref)
