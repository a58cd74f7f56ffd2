"""Helpers of tests/test_gpu_lean_ref.py, tests/test_lean_ref_host.py and tests/lean_nt_worker.py
(not a test module).

  * lean_reference: the float64 reference of the lean static-range epilogue (limb planes in, codes
    out) on top of test_gpu.emulate_limbs, and check_codes / expected_overflow: what a kernel's
    limb planes and overflow flag must be, to the code;
  * guarded / run_guarded: every output a smpq.ops wrapper allocates sits between two guard
    regions of a pre-filled buffer, so an unwritten byte or a store next to the tensor shows;
  * the deterministic case builders the GPU tests and the non-temporal-store child share.
"""
import atexit
import json
import os
import sys

import numpy as np
import torch

from test_gpu import LIMB_QMAX, emulate_limbs, make_layer

EPS_FP32 = 2e-6  # the project's bound of the fp32 epilogue relative to the terms' magnitudes (test_gpu.py)


# ---- limb planes <-> codes ---------------------------------------------------------------------
def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def decode(planes):
    """int64 codes of balanced int8 limb planes [L, ...]."""
    p = _np(planes).astype(np.int64)
    return sum(p[l] * 256 ** l for l in range(p.shape[0]))


def encode(codes, limbs):
    """Balanced base-256 digits (each in [-128, 127]) of integer codes -> int8 [limbs, ...]."""
    q = np.asarray(codes).astype(np.int64)
    out = []
    for _ in range(limbs - 1):
        lo = ((q + 128) & 255) - 128
        out.append(lo)
        q = (q - lo) >> 8
    out.append(q)
    assert -128 <= q.min() and q.max() <= 127, "code does not fit its limbs"
    return np.stack(out).astype(np.int8)


def f32(v):
    return np.float32(v)


def yq_inv(emit_range, limbs):
    """The kernel's QMAX / range, rounded as the C side rounds it."""
    return np.float64(f32(LIMB_QMAX[limbs]) / f32(emit_range))


# ---- the reference -----------------------------------------------------------------------------
def lean_real(xq, wq, w_off, k, stride, pad, x_absmax, col_scale, col_shift, res_q=None, residual_range=None):
    """The conv in real units, before ReLU and the output quantizer, in float64: (y, bound), both
    [n, ho, wo, cout]. xq int8 [L, n, h, w, cin]; wq int8 [LW, cout, K] or [cout, K] (K in (kh, kw,
    cin) order); w_off int32 [cout] or None (LW = 1 only: the weight is code + offset); res_q int8
    [L, n, ho, wo, cout] with its range. Products with la + lw < max(0, L + LW - 4) are skipped, as
    the kernels skip them (emulate_limbs). Only the kernel's fp32 constants are rounded to fp32."""
    xq = _np(xq)
    limbs = xq.shape[0]
    cin = xq.shape[-1]
    wq = _np(wq).astype(np.int64)
    if wq.ndim == 2:
        wq = wq[None]
    lw, cout = wq.shape[:2]
    wq = wq.reshape(lw, cout, k, k, cin)
    if w_off is not None:
        assert lw == 1, "weight offsets: exact codes (one weight limb) only"
        wq = wq + _np(w_off).astype(np.int64).reshape(1, cout, 1, 1, 1)
    rscale = (_np(x_absmax).astype(np.float32) * f32(f32(1.0) / f32(LIMB_QMAX[limbs]))).astype(np.float64)
    residual = None
    if res_q is not None:
        res_scale = np.float64(f32(residual_range) / f32(LIMB_QMAX[limbs]))
        residual = decode(res_q).astype(np.float64) * res_scale
    return emulate_limbs(xq, wq, k, stride, pad, rscale, _np(col_scale).astype(np.float64),
                         _np(col_shift).astype(np.float64), residual, False)


def to_code_units(y, bound, relu, emit_range, limbs):
    inv = yq_inv(emit_range, limbs)
    z = y * inv
    if relu:
        z = np.maximum(z, 0.0)
    return z, bound * inv


def lean_reference(xq, wq, w_off, k, stride, pad, x_absmax, col_scale, col_shift, res_q=None, residual_range=None,
                   relu=False, emit_range=1.0):
    """(z, B): the lean epilogue's output in code units (after ReLU, before rounding and clamping)
    and the sum of its terms' magnitudes in code units."""
    y, bound = lean_real(xq, wq, w_off, k, stride, pad, x_absmax, col_scale, col_shift, res_q, residual_range)
    return to_code_units(y, bound, relu, emit_range, xq.shape[0])


def real_max(y, relu):
    """max |output| in real units: what the range factors multiply."""
    return float(np.maximum(y, 0.0).max() if relu else np.abs(y).max())


def emit_range_for(y, relu, factor):
    r = float(f32(real_max(y, relu) * factor))
    assert r > 0
    return r


def ideal_codes(z, relu, limbs):
    qmax = LIMB_QMAX[limbs]
    return np.clip(np.rint(z), 0.0 if relu else -qmax, qmax).astype(np.int64)


# observed figures per kernel family (never asserted on): the largest (|code - z| - 0.5) / B and the
# share of codes equal to rint(z); SMPQ_LEAN_REF_STATS=<path> writes them there when the process ends
OBSERVED = {}


def _observe(family, excess, exact, count):
    o = OBSERVED.setdefault(family, {"max_excess_over_B": -1.0, "exact": 0, "codes": 0})
    o["max_excess_over_B"] = max(o["max_excess_over_B"], float(excess))
    o["exact"] += int(exact)
    o["codes"] += int(count)


@atexit.register
def _dump_observed():
    path = os.environ.get("SMPQ_LEAN_REF_STATS")
    if path and OBSERVED:
        for o in OBSERVED.values():
            o["exact_share"] = o["exact"] / max(o["codes"], 1)
        with open(path, "w") as f:
            json.dump(OBSERVED, f, indent=1, sort_keys=True)


def check_codes(yq, z, B, relu, limbs, family=None):
    """A kernel's limb planes yq [limbs, n, ho, wo, cout] against the reference (z, B): every limb a
    balanced digit, every code within 0.5 (the rounding) + 2e-6 B (the fp32 epilogue) of the clamped
    reference, no negative code under ReLU, every element compared."""
    yq = _np(yq)
    assert yq.dtype == np.int8 and yq.shape == (limbs,) + z.shape == (limbs,) + B.shape, (yq.shape, z.shape, B.shape)
    p = yq.astype(np.int64)
    assert p.min() >= -128 and p.max() <= 127
    code = decode(yq)
    qmax = LIMB_QMAX[limbs]
    lo = 0.0 if relu else -qmax
    assert np.isfinite(z).all() and np.isfinite(B).all()
    zc = np.clip(z, lo, qmax)
    err = np.abs(code - zc)
    tol = 0.5 + EPS_FP32 * B
    bad = err > tol
    excess = ((err - 0.5) / (B + 1e-300)).max()
    if family is not None:
        _observe(family, excess, (code == ideal_codes(z, relu, limbs)).sum(), code.size)
    assert bad.size == code.size == z.size
    if bad.any():
        i = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError("%d of %d codes off: worst at %s code %d, reference %.3f, bound %.3f" % (
            bad.sum(), bad.size, i, code[i], zc[i], tol[i]))
    if relu:
        assert code.min() >= 0
    return excess


def expected_overflow(z, B, limbs):
    """The overflow flag the reference fixes: 1 if some |rint(z)| is past QMAX by more than the
    codes' tolerance, 0 if every one is inside by more than it. An input with neither (the flag would
    hang on an element inside the tolerance band) fails here."""
    qmax = LIMB_QMAX[limbs]
    tol = 0.5 + EPS_FP32 * B
    a = np.abs(z)
    if (a - tol > qmax).any():
        return 1
    assert (a + tol < qmax).all(), "the reference leaves the overflow flag to an element inside the tolerance band"
    return 0


# ---- guard regions -----------------------------------------------------------------------------
GUARD = 64 * 1024  # bytes per side; a multiple of 4 KiB, so the view keeps the allocation's alignment


class guarded:
    """Context manager: every torch.empty of int8 or float32 that a module in ``modules`` makes on a
    device of ``device_types`` is a contiguous view in the middle of a larger byte buffer filled with
    ``fill`` (GUARD bytes before, GUARD bytes right after the tensor's last byte)."""

    def __init__(self, fill, device_types=("cuda",), modules=("smpq.ops",)):
        self.fill, self.device_types, self.modules = int(fill), tuple(device_types), tuple(modules)
        self.bufs = []

    def _empty(self, *size, **kw):
        dtype = kw.get("dtype") or torch.get_default_dtype()
        device = torch.device(kw.get("device") or "cpu")
        caller = sys._getframe(1).f_globals.get("__name__")
        if (dtype not in (torch.int8, torch.float32) or device.type not in self.device_types
                or caller not in self.modules or set(kw) - {"dtype", "device"}):
            return self._orig(*size, **kw)
        shape = tuple(size[0]) if len(size) == 1 and not isinstance(size[0], int) else tuple(size)
        nbytes = int(np.prod(shape, dtype=np.int64)) * (1 if dtype == torch.int8 else 4)
        buf = torch.full((2 * GUARD + nbytes,), self.fill, dtype=torch.uint8, device=device)
        self.bufs.append((buf, nbytes))
        return buf[GUARD:GUARD + nbytes].view(dtype).view(shape)

    def __enter__(self):
        self._orig = torch.empty
        torch.empty = self._empty
        return self

    def __exit__(self, *exc):
        torch.empty = self._orig
        return False

    def assert_guards_intact(self):
        for k, (buf, nbytes) in enumerate(self.bufs):
            for name, g, base in (("before", buf[:GUARD], -GUARD), ("after", buf[GUARD + nbytes:], nbytes)):
                hit = g != self.fill
                if bool(hit.any()):
                    at = int(hit.nonzero()[0].item()) + base
                    raise AssertionError("guard %s allocation %d (%d bytes) overwritten at byte offset %d of the "
                                         "tensor" % (name, k, nbytes, at))


def run_guarded(fn, device_types=("cuda",), modules=("smpq.ops",)):
    """fn() -> tensor or tuple of tensors (None allowed), run with its outputs guarded under fill
    0x5A and again under 0xA5: the results must agree bit for bit (a byte the op never wrote keeps
    the fill, which differs) and every guard byte must be untouched. Returns the first run's outputs."""
    runs = []
    for fill in (0x5A, 0xA5):
        with guarded(fill, device_types, modules) as g:
            r = fn()
            if "cuda" in device_types and torch.cuda.is_available():
                torch.cuda.synchronize()
        assert g.bufs, "the op allocated no guarded output"
        g.assert_guards_intact()
        runs.append(r if isinstance(r, (tuple, list)) else (r,))
    assert len(runs[0]) == len(runs[1])
    for i, (a, b) in enumerate(zip(*runs)):
        assert (a is None) == (b is None)
        if a is not None:
            assert a.shape == b.shape and a.dtype == b.dtype
            if not torch.equal(a, b):
                raise AssertionError("output %d: %d elements differ between the two fills (unwritten bytes)"
                                     % (i, int((a != b).sum())))
    r = runs[0]
    return r if len(r) > 1 else r[0]


# ---- deterministic cases (shared with tests/lean_nt_worker.py) ----------------------------------
FACTORS = (2.0, 0.5)


def acts(gpu, n, h, w, c, limbs, seed, signed=False):
    """Activation limb planes with per-image ranges that really differ (x[i] *= 1 + i % 5)."""
    from smpq import ops
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, h, w, c, generator=g)
    if not signed:
        x = torch.relu(x)
    x *= (1.0 + (torch.arange(n) % 5).float()).reshape(n, 1, 1, 1)
    xd = x.to(gpu)
    am = ops.act_absmax(xd)
    assert n == 1 or am[0].item() != am[1].item()
    return ops.act_quantize(xd, am, limbs), am


def residual_planes(gpu, n, ho, wo, cout, limbs, seed):
    from smpq import ops
    r = torch.randn(n, ho, wo, cout, generator=torch.Generator().manual_seed(seed)).to(gpu)
    rr = float(f32(float(r.abs().max()) * 1.25))
    return ops.act_quantize(r, torch.full((n,), rr, device=gpu), limbs), rr


def weights(gpu, cin, cout, k, wl, seed, bits=(8,)):
    """(codes [wl, cout, K] with the K-major copy attached, offset or None, column scale). wl = 1:
    exact codes of make_layer's quantized weight; wl = 3: 24-bit fixed point (the downsample form)."""
    from smpq import ops
    if wl == 1:
        wd, step, _, _ = make_layer(gpu, cin, cout, k, seed, bits_choice=bits)
        codes, offset, wscale, st = ops.pack_weights_ex(wd, step, 1)
        assert st.cpu().tolist() == [0, 0, 0]
        return codes, offset, wscale
    w = (torch.randn(cout, cin, k, k, generator=torch.Generator().manual_seed(seed)) * 0.1).to(gpu)
    codes, _, wscale, _ = ops.pack_weights_ex(w, None, wl)
    return codes, None, wscale


class ConvCase:
    """One conv of the lean static-range epilogue: operands on the GPU, the reference on the host."""

    def __init__(self, gpu, cin, cout, k, stride, h, w, n, limbs, wl=1, seed=0, residual=False, relu=True,
                 offsets=True, bits=(8,), need_offsets=False):
        self.gpu, self.k, self.stride, self.pad, self.limbs, self.relu = gpu, k, stride, k // 2, limbs, relu
        self.xq, self.am = acts(gpu, n, h, w, cin, limbs, seed + 1)
        self.codes, off, scale = weights(gpu, cin, cout, k, wl, seed, bits)
        if need_offsets:
            assert off is not None and bool((off != 0).any())
        self.off = off if offsets else None
        self.cs = (scale * torch.linspace(0.5, 1.5, cout, device=gpu)).contiguous()
        self.sh = torch.linspace(-0.3, 0.3, cout, device=gpu).contiguous()
        ho, wo = (h + 2 * self.pad - k) // stride + 1, (w + 2 * self.pad - k) // stride + 1
        self.rq, self.rr = residual_planes(gpu, n, ho, wo, cout, limbs, seed + 2) if residual else (None, None)
        self.y, self.bound = lean_real(self.xq, self.codes, self.off, k, stride, self.pad, self.am, self.cs, self.sh,
                                       self.rq, self.rr)
        self._ref = {}

    def emit_range(self, factor):
        return emit_range_for(self.y, self.relu, factor)

    def reference(self, factor):
        if factor not in self._ref:
            z, B = to_code_units(self.y, self.bound, self.relu, self.emit_range(factor), self.limbs)
            self._ref[factor] = (z, B, expected_overflow(z, B, self.limbs))
        return self._ref[factor]

    def launch(self, cfg, factor, layout="auto"):
        """(limb planes, overflow flag) of one guarded launch on tile config cfg."""
        from smpq import ops

        def fn():
            ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
            y, yq = ops.conv2d_q(self.xq, self.am, self.codes, self.off, self.k, self.k, self.stride, self.pad,
                                 self.cs, self.sh, relu=self.relu, tile_cfg=cfg, emit_range=self.emit_range(factor),
                                 overflow=ovf, want_f32=False, residual_q=self.rq, residual_range=self.rr,
                                 weight_layout=layout)
            assert y is None
            return yq, ovf
        return run_guarded(fn)

    def check(self, yq, ovf, factor, family):
        z, B, want = self.reference(factor)
        check_codes(yq, z, B, self.relu, self.limbs, family)
        assert int(ovf.item()) == want, (int(ovf.item()), want)


def am1_for(gpu, n, rng1):
    """The chained conv's per-image input scale: it differs between images (in a forward it is the
    static range of every image; the kernels take any per-image table)."""
    return (rng1 * (1.0 + 0.25 * (torch.arange(n) % 3).float())).to(gpu)


class PairCase:
    """conv3 64 -> 256 (+ limb-plane identity, ReLU) chained with the next conv1 256 -> cout2 (ReLU)."""

    def __init__(self, gpu, n, h, cout2, seed):
        self.gpu, self.n, self.limbs = gpu, n, 3
        self.xq, self.am = acts(gpu, n, h, h, 64, 3, seed + 1)
        self.codes1, _, s1 = weights(gpu, 64, 256, 1, 1, seed, bits=(6, 4))
        self.codes2, _, s2 = weights(gpu, 256, cout2, 1, 1, seed + 3, bits=(6, 4))
        self.cs1 = (s1 * torch.linspace(0.5, 1.5, 256, device=gpu)).contiguous()
        self.sh1 = torch.linspace(-0.3, 0.3, 256, device=gpu).contiguous()
        self.cs2 = (s2 * torch.linspace(1.5, 0.5, cout2, device=gpu)).contiguous()
        self.sh2 = torch.linspace(-0.2, 0.4, cout2, device=gpu).contiguous()
        self.rq, self.rr = residual_planes(gpu, n, h, h, 256, 3, seed + 2)
        self.y1, self.b1 = lean_real(self.xq, self.codes1, None, 1, 1, 0, self.am, self.cs1, self.sh1, self.rq, self.rr)
        self._rng = {}

    def ranges(self, f1, f2):
        """Both static ranges from the reference alone: the second stage's from the reference's own
        first-stage codes."""
        if (f1, f2) not in self._rng:
            rng1 = emit_range_for(self.y1, True, f1)
            z1, _ = to_code_units(self.y1, self.b1, True, rng1, 3)
            y1q = encode(ideal_codes(z1, True, 3), 3)
            am1 = am1_for(self.gpu, self.n, rng1)
            y2, _ = lean_real(y1q, self.codes2, None, 1, 1, 0, am1, self.cs2, self.sh2)
            self._rng[(f1, f2)] = (rng1, emit_range_for(y2, True, f2), am1)
        return self._rng[(f1, f2)]

    def launch(self, f1, f2):
        from smpq import ops
        rng1, rng2, am1 = self.ranges(f1, f2)

        def fn():
            ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
            p1, p2 = ops.conv_pair_q(self.xq, self.am, self.codes1, self.cs1, self.sh1, self.rq, self.rr, rng1, am1,
                                     self.codes2, self.cs2, self.sh2, rng2, ovf)
            return p1, p2, ovf
        return run_guarded(fn)

    def separate(self, f1, f2):
        from smpq import ops
        rng1, rng2, am1 = self.ranges(f1, f2)
        ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
        _, y1 = ops.conv2d_q(self.xq, self.am, self.codes1, None, 1, 1, 1, 0, self.cs1, self.sh1, relu=True,
                             emit_range=rng1, overflow=ovf, want_f32=False, residual_q=self.rq, residual_range=self.rr)
        _, y2 = ops.conv2d_q(y1, am1, self.codes2, None, 1, 1, 1, 0, self.cs2, self.sh2, relu=True, emit_range=rng2,
                             overflow=ovf, want_f32=False)
        return y1, y2, ovf

    def check(self, p1, p2, ovf, f1, f2, family):
        rng1, rng2, am1 = self.ranges(f1, f2)
        z1, B1 = to_code_units(self.y1, self.b1, True, rng1, 3)
        check_codes(p1, z1, B1, True, 3, family)
        # stage 2 on the kernel's own stage-1 codes
        z2, B2 = lean_reference(p1, self.codes2, None, 1, 1, 0, am1, self.cs2, self.sh2, relu=True, emit_range=rng2)
        check_codes(p2, z2, B2, True, 3, family)
        want = max(expected_overflow(z1, B1, 3), expected_overflow(z2, B2, 3))
        assert int(ovf.item()) == want, (int(ovf.item()), want)


class ChainDsCase:
    """The first block of a stage: conv3 cin -> cout (exact codes, ReLU) whose identity is the 1x1
    downsample ds_cin -> cout (24-bit fixed point, no ReLU, stride hd -> h) computed in the same
    tiles; its codes are never written."""

    def __init__(self, gpu, cin, cout, ds_cin, st, n, h, hd, offsets, seed):
        self.gpu, self.n, self.st, self.limbs = gpu, n, st, 3
        assert (hd - 1) // st + 1 == h
        self.xq, self.am = acts(gpu, n, h, h, cin, 3, seed + 1)
        self.codes1, off, s1 = weights(gpu, cin, cout, 1, 1, seed, bits=(8,))
        self.off = off if offsets else None
        assert not offsets or bool((off != 0).any())
        self.cs1 = (s1 * torch.linspace(0.5, 1.5, cout, device=gpu)).contiguous()
        self.sh1 = torch.linspace(-0.3, 0.3, cout, device=gpu).contiguous()
        self.xbq, self.amb = acts(gpu, n, hd, hd, ds_cin, 3, seed + 5)
        self.dcodes, _, ds_ = weights(gpu, ds_cin, cout, 1, 3, seed + 6)
        self.dcs = (ds_ * torch.linspace(1.4, 0.6, cout, device=gpu)).contiguous()
        self.dsh = torch.linspace(-0.2, 0.2, cout, device=gpu).contiguous()
        self.yd, self.bd = lean_real(self.xbq, self.dcodes, None, 1, st, 0, self.amb, self.dcs, self.dsh)
        self._rng = {}

    def ranges(self, fd, f1):
        if (fd, f1) not in self._rng:
            rng_d = emit_range_for(self.yd, False, fd)
            zd, _ = to_code_units(self.yd, self.bd, False, rng_d, 3)
            ydq = encode(ideal_codes(zd, False, 3), 3)
            y1, _ = lean_real(self.xq, self.codes1, self.off, 1, 1, 0, self.am, self.cs1, self.sh1, ydq, rng_d)
            self._rng[(fd, f1)] = (rng_d, emit_range_for(y1, True, f1))
        return self._rng[(fd, f1)]

    def downsample(self, fd, f1, guard=True):
        """The separate downsample launch (default LDS-DMA tile): (codes, flag)."""
        from smpq import ops
        rng_d, _ = self.ranges(fd, f1)

        def fn():
            ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
            _, yd = ops.conv2d_q(self.xbq, self.amb, self.dcodes, None, 1, 1, self.st, 0, self.dcs, self.dsh,
                                 relu=False, emit_range=rng_d, overflow=ovf, want_f32=False)
            return yd, ovf
        return run_guarded(fn) if guard else fn()

    def launch(self, fd, f1):
        from smpq import ops
        rng_d, rng1 = self.ranges(fd, f1)
        am1 = am1_for(self.gpu, self.n, rng1)

        def fn():
            ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
            p1, p2 = ops.conv_chain_q(self.xq, self.am, self.codes1, self.off, self.cs1, self.sh1, rng1, am1, ovf,
                                      ds=(self.xbq, self.amb, self.dcodes, self.dcs, self.dsh, rng_d, self.st))
            assert p2 is None
            return p1, ovf
        return run_guarded(fn)

    def separate(self, fd, f1):
        from smpq import ops
        rng_d, rng1 = self.ranges(fd, f1)
        ovf = torch.zeros(1, dtype=torch.int32, device=self.gpu)
        _, yd = ops.conv2d_q(self.xbq, self.amb, self.dcodes, None, 1, 1, self.st, 0, self.dcs, self.dsh, relu=False,
                             emit_range=rng_d, overflow=ovf, want_f32=False)
        _, y1 = ops.conv2d_q(self.xq, self.am, self.codes1, self.off, 1, 1, 1, 0, self.cs1, self.sh1, relu=True,
                             emit_range=rng1, overflow=ovf, want_f32=False, residual_q=yd, residual_range=rng_d)
        return y1, ovf

    def check(self, yd, ovf_d, p1, ovf, fd, f1, family):
        """yd: the separate downsample launch's codes (checked here too); p1, ovf: the fused launch."""
        rng_d, rng1 = self.ranges(fd, f1)
        zd, Bd = to_code_units(self.yd, self.bd, False, rng_d, 3)
        check_codes(yd, zd, Bd, False, 3, None)
        want_d = expected_overflow(zd, Bd, 3)
        assert int(ovf_d.item()) == want_d
        z1, B1 = lean_reference(self.xq, self.codes1, self.off, 1, 1, 0, self.am, self.cs1, self.sh1, yd, rng_d,
                                relu=True, emit_range=rng1)
        check_codes(p1, z1, B1, True, 3, family)
        want = max(want_d, expected_overflow(z1, B1, 3))
        assert int(ovf.item()) == want, (int(ovf.item()), want)


def _kind_cfgs(kinds, limbs, wl, cout, cin, k):
    from smpq import ops
    return [c for c in ops.tile_configs() if ops.tile_kind(c) in kinds and ops._tile_fits(c, limbs, wl, cout, cin, k)]


def nt_cases(gpu, family=None):
    """One case of each kernel family (and one of more than 256 images), guarded and checked against
    the reference: {name: [tensors on the host]}. tests/lean_nt_worker.py runs it in a process whose
    limb-plane stores are all non-temporal, the test in one with the default threshold."""
    from smpq import ops
    out = {}

    def conv(name, case, cfg):
        for f in FACTORS:
            yq, ovf = case.launch(cfg, f)
            case.check(yq, ovf, f, family)
            out["%s_f%s" % (name, f)] = [yq.cpu(), ovf.cpu()]

    lds = ConvCase(gpu, 64, 80, 3, 1, 9, 9, 3, 3, seed=101, residual=True, need_offsets=True)
    conv("lds_default", lds, -1)
    k128 = ConvCase(gpu, 128, 64, 3, 2, 17, 17, 3, 2, seed=102, relu=False)
    for kind in (ops.TILE_LDS_DMA, ops.TILE_LDS_DMA_K128):
        conv("lds_kind%d" % kind, k128, _kind_cfgs((kind,), 2, 1, 64, 128, 3)[-1])
    conv("lds_wl3", ConvCase(gpu, 256, 512, 1, 2, 9, 9, 3, 3, wl=3, seed=103, relu=False), -1)
    conv("halo", ConvCase(gpu, 64, 64, 3, 1, 13, 17, 3, 3, seed=104, residual=True),
         _kind_cfgs((ops.TILE_HALO3X3,), 3, 1, 64, 64, 3)[0])
    conv("resident_res", ConvCase(gpu, 64, 256, 1, 1, 5, 5, 3, 3, seed=105, residual=True, offsets=False, bits=(6, 4)),
         _kind_cfgs((ops.TILE_RESIDENT1X1,), 3, 1, 256, 64, 1)[0])
    big = ConvCase(gpu, 64, 256, 1, 1, 3, 3, 260, 3, wl=3, seed=106, relu=False)
    conv("resident_n260", big, _kind_cfgs((ops.TILE_RESIDENT1X1,), 3, 3, 256, 64, 1)[-1])
    pair = PairCase(gpu, 3, 9, 64, seed=107)
    for f1, f2 in ((2.0, 2.0), (2.0, 0.5)):
        p1, p2, ovf = pair.launch(f1, f2)
        pair.check(p1, p2, ovf, f1, f2, family)
        out["pair_%s_%s" % (f1, f2)] = [p1.cpu(), p2.cpu(), ovf.cpu()]
    chain = ChainDsCase(gpu, 128, 512, 256, 2, 3, 5, 9, True, seed=108)
    for fd, f1 in ((2.0, 2.0), (0.5, 2.0)):
        yd, ovd = chain.downsample(fd, f1)
        p1, ovf = chain.launch(fd, f1)
        chain.check(yd, ovd, p1, ovf, fd, f1, family)
        out["chain_%s_%s" % (fd, f1)] = [yd.cpu(), ovd.cpu(), p1.cpu(), ovf.cpu()]
    return out
