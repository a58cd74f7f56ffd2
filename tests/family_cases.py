"""Helpers of tests/test_gpu_grouped.py, test_gpu_dilated.py, test_gpu_narrow.py, test_gpu_stem3.py and
test_gpu_conv_families.py (not a test module): one deterministic case builder per conv family
(csrc/conv_grouped.hip, conv_dilated.hip, conv_narrow.hip, conv_stem3.hip).

A case holds the operands on the GPU, ``launch(form, ...)`` (one call of the family's smpq.ops wrapper in
one of three output forms) and ``reference(images)``: the float64 emulation of the integer path
(test_gpu.emulate_limbs) on the kernel's own codes, as a dense conv: block_diagonal() of the codes for
grouped, zero_inflate() for dilated. tests/test_gpu_conv_families.py checks both constructions on the CPU.
"""
import numpy as np
import torch

from lean_ref import run_guarded
from test_gpu import LIMB_QMAX, emulate_limbs

# (cin, cout, groups, stride, H): 4 groups / fragment, odd size; stride 2, even; one group / fragment;
# a fragment is half a group, stride 2, odd; cg 64, og 128; cg != og; three fragments, the workgroup's fourth
# wave idle
GROUPED_SHAPES = [(64, 64, 16, 1, 9), (128, 128, 16, 2, 10), (64, 64, 4, 1, 7), (128, 128, 4, 2, 9),
                  (128, 256, 2, 1, 5), (64, 128, 4, 1, 6), (48, 48, 3, 1, 5)]
# (cin, cout, d, H, W): odd size (lattices of 5 and 4); two input chunks, a partial second row tile, non-square;
# two channel tiles, lattices of 2 and 1; a second row tile for phase row 0 only; d > H (empty phases, row
# taps all outside)
DILATED_SHAPES = [(64, 64, 2, 9, 9), (128, 64, 2, 18, 12), (64, 128, 4, 7, 7), (128, 64, 4, 33, 10), (64, 64, 8, 5, 11)]
# (cin, cout, k, stride, H, W): smallest K, padded last step, one active wave; stride 2, odd and non-square;
# partial last workgroup, partial column tile; 1x1 with K = 1.5 steps; streamed weights (23 steps); at stride 2
# the widest cin staged in one slab (11 chunks) and the narrowest that takes two (13 = 11 + 2)
NARROW_SHAPES = [(16, 16, 3, 1, 9, 9), (32, 64, 3, 2, 9, 11), (48, 80, 3, 1, 7, 18), (96, 32, 1, 1, 5, 13),
                 (160, 64, 3, 1, 10, 8), (176, 16, 3, 2, 9, 9), (208, 16, 3, 2, 9, 9)]
# (c, cout, H, W) on 8-row x 16-column tiles: whole rows of a tile; partial tiles on both axes, two tiles per
# axis; one channel, two channel tiles, an image smaller than a tile; all four channels, a last row tile of one
# row; 2 * 17 * 16 = 544 tiles for the 512 workgroups of the launch (the smallest walk of two tiles, the last
# tiles partial on both axes: it replaces (3, 64, 33, 34), which gives every tile its own workgroup)
STEM3_SHAPES = [(3, 64, 8, 8), (3, 64, 9, 19), (1, 128, 5, 3), (4, 64, 17, 16), (3, 64, 129, 250)]

# per-image input factors (image i: IMAGE_SCALES[i % 5]), so that no two neighbouring images share a range
IMAGE_SCALES = (1.0, 7.0, 3.0, 5.0, 2.0)
FORMS = ("fp32", "planes", "both")  # fp32 y + y_absmax; limb planes only (the lean epilogue); everything at once
_CASES = {}


# ---- the reference's weight transformations --------------------------------------------------------
def block_diagonal(m, groups):
    """Grouped codes [wl, cout, kh, kw, cin / groups] -> the dense weight [wl, cout, kh, kw, cin] of the same
    conv: a row's values on the input channels of its own group, 0 outside."""
    wl, cout, kh, kw, cg = m.shape
    og = cout // groups
    dense = np.zeros((wl, cout, kh, kw, cg * groups), dtype=m.dtype)
    for c in range(cout):
        dense[:, c, :, :, (c // og) * cg:(c // og + 1) * cg] = m[:, c]
    return dense


def zero_inflate(m, d):
    """3x3 codes [wl, cout, 3, 3, cin] of a conv with dilation d -> the (2d+1) x (2d+1) weight of the same
    conv without dilation (padding d): the values at pitch d, 0 elsewhere."""
    wl, cout, kh, kw, cin = m.shape
    assert (kh, kw) == (3, 3)
    big = np.zeros((wl, cout, 2 * d + 1, 2 * d + 1, cin), dtype=m.dtype)
    big[:, :, ::d, ::d, :] = m
    return big


# ---- a case ------------------------------------------------------------------------------------------
def scaled_images(x):
    """x[i] *= IMAGE_SCALES[i % 5] (in place): per-image ranges that really differ."""
    n = x.shape[0]
    x *= torch.tensor(IMAGE_SCALES)[torch.arange(n) % 5].reshape((n,) + (1,) * (x.dim() - 1))
    return x


class FamilyCase:
    """One conv of a family: ``operands`` = (xq, am, codes, offset or None, cs, sh) on the GPU; ``weight`` the
    dense int64 weight [wl, cout, k, k, cin] the reference convolves with (code + offset)."""

    def __init__(self, call, xq, am, codes, offset, cs, sh, weight, k, stride, pad):
        self.call, self.xq, self.am, self.codes, self.offset, self.cs, self.sh = call, xq, am, codes, offset, cs, sh
        self.weight, self.k, self.stride, self.pad = weight, k, stride, pad
        self.n = xq.shape[1]
        self.operands = (xq, am, codes, offset, cs, sh)
        self._ref = {}

    def reference(self, images=None, residual=None):
        """(y, bound) of images [i0, i1) (default: all) in real units before ReLU, float64 on the host;
        ``residual``: those images' residual in real units (float64 [i1 - i0, ho, wo, cout])."""
        i0, i1 = images or (0, self.n)
        if residual is None and (i0, i1) in self._ref:
            return self._ref[(i0, i1)]
        rscale = (self.am[i0:i1].cpu().numpy() * np.float32(1.0 / LIMB_QMAX[3])).astype(np.float64)
        r = emulate_limbs(self.xq[:, i0:i1].cpu().numpy(), self.weight, self.k, self.stride, self.pad, rscale,
                          self.cs.cpu().numpy().astype(np.float64), self.sh.cpu().numpy().astype(np.float64), residual,
                          False)
        if residual is None:
            self._ref[(i0, i1)] = r
        return r

    def launch(self, form, relu=True, emit_range=None, images=None, guard=False, res=None, out=None, y_absmax=None,
               overflow=None):
        """One call of the family's wrapper on images [i0, i1) (default: all) -> (y, y_absmax, yq, overflow),
        None where the form has none. ``res``: the whole batch's residual keywords of conv2d_narrow_q;
        ``guard``: under lean_ref.run_guarded; ``out`` / ``y_absmax`` / ``overflow``: the caller's tensors."""
        assert form in FORMS
        i0, i1 = images or (0, self.n)
        whole = (i0, i1) == (0, self.n)
        xq = self.xq if whole else self.xq[:, i0:i1].contiguous()
        am = self.am[i0:i1]
        fixed = {}
        for key, v in (res or {}).items():
            if key == "residual":
                v = v[i0:i1]
            elif key == "residual_q" and not whole:
                v = v[:, i0:i1].contiguous()
            fixed[key] = v
        if out is not None:
            fixed["out"] = out

        def fn():
            kw, yam, ovf = dict(fixed), None, None
            if form != "planes":
                yam = torch.zeros(i1 - i0, device=xq.device) if y_absmax is None else y_absmax
                kw["y_absmax"] = yam
            if form != "fp32":
                ovf = torch.zeros(1, dtype=torch.int32, device=xq.device) if overflow is None else overflow
                kw.update(emit_range=emit_range, overflow=ovf, want_f32=form == "both")
            r = self.call(xq, am, relu=bool(relu), **kw)
            y, yq = (r, None) if form == "fp32" else r
            assert (y is None) == (form == "planes") and (yq is None) == (form == "fp32")
            return y, yam, yq, ovf
        return run_guarded(fn) if guard else fn()


def _exact_or_fixed(ops, w2d, wl):
    """Quantizes w2d in place to 8-bit steps for exact codes (wl = 1); the step, or None for 24-bit fixed point."""
    return ops.quantize_channels_(w2d, [8] * w2d.shape[0]) if wl == 1 else None


def _finish(key, call, gpu, x, codes, offset, wscale, st, wl, offsets, weight_of, k, stride):
    """The part the NHWC families share: status and offsets asserted, activations quantized, column vectors,
    the reference's weight: weight_of(code + offset [wl, cout, k, k, c]) -> (dense weight, its k, its padding)."""
    from smpq import ops
    cout = codes.shape[1]
    assert st.cpu().tolist() == ([0, 0, 0] if wl == 1 else [0, 0, cout])
    assert wl == 3 or bool((offset != 0).any())
    offset = offset if wl == 1 and offsets else None
    xd = scaled_images(x).to(gpu)
    am = ops.act_absmax(xd)
    assert x.shape[0] == 1 or am[0].item() != am[1].item()
    xq = ops.act_quantize(xd, am, 3)
    cs = (wscale * torch.linspace(0.5, 1.5, cout, device=gpu)).contiguous()
    sh = torch.linspace(-0.1, 0.1, cout, device=gpu).contiguous()
    m = codes.cpu().numpy().astype(np.int64)
    m = m.reshape(m.shape[0], cout, k, k, -1)
    if offset is not None:
        m = m + offset.cpu().numpy().astype(np.int64).reshape(1, cout, 1, 1, 1)
    weight, kk, pp = weight_of(m)
    _CASES[key] = FamilyCase(lambda xq_, am_, **kw: call(xq_, am_, codes, offset, cs, sh, **kw), xq, am, codes, offset,
                             cs, sh, weight, kk, stride, pp)
    return _CASES[key]


def grouped_case(gpu, shape, wl, n=2, offsets=True):
    """(cin, cout, groups, stride, H) with wl weight limbs on n images; offsets=False drops the exact codes'
    offsets (the reference then convolves with the bare codes). Built once per argument set."""
    key = ("grouped", shape, wl, n, offsets)
    if key in _CASES:
        return _CASES[key]
    from smpq import ops
    cin, cout, groups, stride, h = shape
    g = torch.Generator().manual_seed(cin + cout + groups + 10 * wl)
    w = (torch.randn(cout, cin // groups, 3, 3, generator=g) * 0.1).to(gpu)
    step = _exact_or_fixed(ops, w.reshape(cout, -1), wl)
    codes, offset, wscale, st = ops.pack_weights_grouped(w, step, wl, groups)
    x = torch.randn(n, h, h, cin, generator=g)
    return _finish(key, lambda xq, am, c, o, cs, sh, **kw: ops.conv2d_grouped_q(xq, am, c, o, stride, cs, sh, **kw),
                   gpu, x, codes, offset, wscale, st, wl, offsets, lambda m: (block_diagonal(m, groups), 3, 1), 3,
                   stride)


def dilated_case(gpu, shape, wl, n=2, offsets=True):
    """(cin, cout, d, H, W); the other arguments as in grouped_case."""
    key = ("dilated", shape, wl, n, offsets)
    if key in _CASES:
        return _CASES[key]
    from smpq import ops
    cin, cout, d, h, w_ = shape
    g = torch.Generator().manual_seed(cin + cout + d + h + 10 * wl)
    w = (torch.randn(cout, cin, 3, 3, generator=g) * 0.1).to(gpu)
    step = _exact_or_fixed(ops, w.reshape(cout, -1), wl)
    codes, offset, wscale, st = ops.pack_weights_ex(w, step, wl)
    x = torch.randn(n, h, w_, cin, generator=g)
    return _finish(key, lambda xq, am, c, o, cs, sh, **kw: ops.conv2d_dilated_q(xq, am, c, o, d, cs, sh, **kw), gpu, x,
                   codes, offset, wscale, st, wl, offsets, lambda m: (zero_inflate(m, d), 2 * d + 1, d), 3, 1)


def narrow_case(gpu, shape, wl, n=2, offsets=True):
    """(cin, cout, k, stride, H, W); the other arguments as in grouped_case."""
    key = ("narrow", shape, wl, n, offsets)
    if key in _CASES:
        return _CASES[key]
    from smpq import ops
    cin, cout, k, stride, h, w_ = shape
    g = torch.Generator().manual_seed(cin + cout + k + h + 10 * wl)
    w = (torch.randn(cout, cin, k, k, generator=g) * 0.1).to(gpu)
    step = _exact_or_fixed(ops, w.reshape(cout, -1), wl)
    codes, offset, wscale, st = ops.pack_weights_narrow(w, step, wl, stride)
    x = torch.randn(n, h, w_, cin, generator=g)
    return _finish(key, lambda xq, am, c, o, cs, sh, **kw: ops.conv2d_narrow_q(xq, am, c, o, cs, sh, **kw), gpu, x,
                   codes, offset, wscale, st, wl, offsets, lambda m: (m, k, k // 2), k, stride)


def stem3_case(gpu, shape, n=2):
    """(c, cout, H, W): 24-bit fixed-point codes (the stem is never quantized to exact codes); offset is None."""
    key = ("stem3", shape, n)
    if key in _CASES:
        return _CASES[key]
    from smpq import ops
    c, cout, h, w_ = shape
    g = torch.Generator().manual_seed(c + cout + h + w_)
    w = (torch.randn(cout, c, 3, 3, generator=g) * 0.1).to(gpu)
    codes, wscale, st = ops.pack_weights_stem3(w)
    assert st.cpu().tolist() == [0, 0, cout] and not bool(codes[:, :, 36:].any())
    xd = scaled_images(torch.randn(n, c, h, w_, generator=g)).to(gpu)
    am = ops.act_absmax(xd)
    assert n == 1 or am[0].item() != am[1].item()
    xq = ops.image_quantize_c4(xd, am)
    cs = (wscale * torch.linspace(0.5, 1.5, cout, device=gpu)).contiguous()
    sh = torch.linspace(-0.1, 0.1, cout, device=gpu).contiguous()
    m = codes[:, :, :36].cpu().numpy().astype(np.int64).reshape(3, cout, 3, 3, 4)
    _CASES[key] = FamilyCase(lambda xq_, am_, **kw: ops.stem_conv3_q(xq_, am_, codes, cs, sh, **kw), xq, am, codes,
                             None, cs, sh, m, 3, 1, 1)
    return _CASES[key]
