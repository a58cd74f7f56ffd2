"""The reference and the checks of tests/lean_ref.py, without a GPU: lean_reference equals a
brute-force integer convolution, check_codes accepts the ideally rounded codes and rejects every
kind of wrong kernel it is there to catch, and run_guarded reports an unwritten byte and a store
into a guard."""
import numpy as np
import pytest
import torch

import lean_ref
from lean_ref import LIMB_QMAX, check_codes, decode, encode, expected_overflow, f32, ideal_codes, lean_reference

N, H, CIN, COUT, K = 2, 3, 64, 16, 3


def _case(lw, seed):
    """Random limb planes of full-range int24 codes; image 1's range is three times image 0's."""
    g = np.random.default_rng(seed)
    qmax = int(LIMB_QMAX[3])
    xq = encode(g.integers(0, qmax + 1, (N, H, H, CIN)), 3)
    am = np.array([1.5, 4.5], np.float32)
    if lw == 1:
        wq = g.integers(-128, 128, (1, COUT, K * K * CIN)).astype(np.int8)
        off = g.integers(-90, 91, COUT).astype(np.int32)
        cs = (g.random(COUT) * 1e-3 + 5e-4).astype(np.float32)
    else:
        wq = encode(g.integers(-qmax, qmax + 1, (COUT, K * K * CIN)), 3)
        off = None
        cs = ((g.random(COUT) * 1e-3 + 5e-4) / 65536).astype(np.float32)
    sh = np.linspace(-0.3, 0.3, COUT).astype(np.float32)
    rq = encode(g.integers(-qmax, qmax + 1, (N, H, H, COUT)), 3)
    rr = 40.0
    return xq, am, wq, off, cs, sh, rq, rr


def _brute(xq, am, wq, off, cs, sh, rq, rr, relu, emit_range):
    """The same conv with exact integer sums per limb pair (einsum over the window, no im2col)."""
    L, LW = xq.shape[0], wq.shape[0]
    smin = max(0, L + LW - 4)
    w = wq.astype(np.int64).reshape(LW, COUT, K, K, CIN)
    if off is not None:
        w = w + off.astype(np.int64).reshape(1, COUT, 1, 1, 1)
    xp = np.pad(xq.astype(np.int64), ((0, 0), (0, 0), (1, 1), (1, 1), (0, 0)))
    v = np.zeros((N, H, H, COUT), np.int64)
    mag = np.zeros((N, H, H, COUT), np.float64)
    for la in range(L):
        for lw_ in range(LW):
            if la + lw_ < smin:
                continue
            t = np.zeros((N, H, H, COUT), np.int64)
            for oh in range(H):
                for ow in range(H):
                    t[:, oh, ow] = np.einsum("nrqc,orqc->no", xp[la][:, oh:oh + K, ow:ow + K], w[lw_])
            v += t * 256 ** (la + lw_)
            mag += np.abs(t).astype(np.float64) * 256.0 ** (la + lw_)
    qmax = f32(LIMB_QMAX[L])
    rs = (am * f32(f32(1.0) / qmax)).astype(np.float64).reshape(N, 1, 1, 1)
    res = decode(rq).astype(np.float64) * np.float64(f32(rr) / qmax)
    inv = np.float64(qmax / f32(emit_range))
    y = v.astype(np.float64) * rs * cs.astype(np.float64) + sh.astype(np.float64) + res
    B = (mag * rs * np.abs(cs.astype(np.float64)) + np.abs(sh.astype(np.float64)) + np.abs(res)) * inv
    z = y * inv
    return (np.maximum(z, 0) if relu else z), B


@pytest.mark.parametrize("lw,relu", [(1, True), (1, False), (3, False)])
def test_reference_equals_brute_force(lw, relu):
    xq, am, wq, off, cs, sh, rq, rr = _case(lw, 5 + lw)
    z, B = lean_reference(xq, wq, off, K, 1, 1, am, cs, sh, rq, rr, relu=relu, emit_range=123.0)
    zb, Bb = _brute(xq, am, wq, off, cs, sh, rq, rr, relu, 123.0)
    assert z.shape == (N, H, H, COUT)
    # int64 sums are exact; the float64 sum of the limb-pair terms rounds each partial sum
    np.testing.assert_allclose(z, zb, rtol=0, atol=1e-12 * B.max())
    np.testing.assert_allclose(B, Bb, rtol=1e-12)
    assert np.abs(z).max() > 1e5  # a real signal in code units


def _setup(lw=1, relu=True, factor=2.0):
    xq, am, wq, off, cs, sh, rq, rr = _case(lw, 11)
    y, bound = lean_ref.lean_real(xq, wq, off, K, 1, 1, am, cs, sh, rq, rr)
    rng = lean_ref.emit_range_for(y, relu, factor)
    z, B = lean_ref.to_code_units(y, bound, relu, rng, 3)
    return (xq, am, wq, off, cs, sh, rq, rr), rng, z, B


@pytest.mark.parametrize("lw,relu", [(1, True), (1, False), (3, False)])
@pytest.mark.parametrize("factor", [2.0, 0.5])
def test_ideal_kernel_passes(lw, relu, factor):
    _, rng, z, B = _setup(lw, relu, factor)
    yq = encode(ideal_codes(z, relu, 3), 3)
    check_codes(yq, z, B, relu, 3)
    assert expected_overflow(z, B, 3) == (1 if factor < 1 else 0)


def _rejected(yq, z, B, relu=True):
    with pytest.raises(AssertionError, match="codes off"):
        check_codes(yq, z, B, relu, 3)


def test_wrong_kernels_fail():
    (xq, am, wq, off, cs, sh, rq, rr), rng, z, B = _setup()
    good = ideal_codes(z, True, 3)
    check_codes(encode(good, 3), z, B, True, 3)
    # two channels swapped
    m = good.copy()
    m[..., [3, 4]] = m[..., [4, 3]]
    _rejected(encode(m, 3), z, B)
    # one pixel row shifted by a pixel
    m = good.copy()
    m[1, 2] = np.roll(m[1, 2], 1, axis=0)
    _rejected(encode(m, 3), z, B)
    # image 1 scaled with image 0's x_absmax
    zz, _ = lean_reference(xq, wq, off, K, 1, 1, np.array([am[0], am[0]]), cs, sh, rq, rr, relu=True, emit_range=rng)
    m = ideal_codes(zz, True, 3)
    assert (m[0] == good[0]).all()
    _rejected(encode(m, 3), z, B)
    # the lowest limb-pair product dropped (SMIN = 0: every product counts)
    x0 = xq.copy()
    x0[0] = 0
    zz, _ = lean_reference(x0, wq, off, K, 1, 1, am, cs, sh, rq, rr, relu=True, emit_range=rng)
    _rejected(encode(ideal_codes(zz, True, 3), 3), z, B)
    # the residual decoded without the 0x80 bias of its low limbs (digits read as unsigned bytes)
    r = rq.astype(np.int64)
    wrong = (r[0] & 255) + 256 * (r[1] & 255) + 65536 * r[2]
    zz = z * 0 + np.maximum((lean_ref.lean_real(xq, wq, off, K, 1, 1, am, cs, sh)[0]
                             + wrong * np.float64(f32(rr) / f32(LIMB_QMAX[3]))) * lean_ref.yq_inv(rng, 3), 0)
    _rejected(encode(ideal_codes(zz, True, 3), 3), z, B)
    # one element off by 40 codes
    m = good.copy()
    i = np.unravel_index(np.argmax(good), good.shape)
    assert 0.5 + 2e-6 * B[i] < 39  # the bound separates a 40-code error even at the largest code
    m[i] -= 40
    _rejected(encode(m, 3), z, B)
    # a negative code under ReLU, a limb plane missing
    m = good.copy()
    m[0, 0, 0, 0] = -1
    with pytest.raises(AssertionError):
        check_codes(encode(m, 3), z - 1.0, B, True, 3)
    with pytest.raises(AssertionError):
        check_codes(encode(good, 3)[:2], z, B, True, 3)


def test_overflow_flag_needs_a_clear_reference():
    _, rng, z, B = _setup(factor=2.0)
    assert expected_overflow(z, B, 3) == 0
    zz = z.copy()
    zz[0, 0, 0, 0] = LIMB_QMAX[3] + 0.4  # inside the tolerance band: no expected flag
    with pytest.raises(AssertionError, match="tolerance band"):
        expected_overflow(zz, B, 3)
    zz[1, 1, 1, 1] = -3 * LIMB_QMAX[3]  # a clear overflow decides it
    assert expected_overflow(zz, B, 3) == 1


def _fake_op(stray=None):
    """An 'op' that allocates with torch.empty, like smpq.ops, and fills its outputs; ``stray``: it
    also writes one byte at that offset from its first output's start."""
    def fn():
        out = torch.empty(3, 5, 7, dtype=torch.int8)
        out.view(-1)[:] = torch.arange(105, dtype=torch.int8)
        if stray is not None:  # (the view's storage is the whole guarded buffer)
            base = torch.zeros(0, dtype=torch.uint8).set_(out.untyped_storage())
            base[lean_ref.GUARD + stray] = 1
        f = torch.empty(4, dtype=torch.float32)
        f[:] = 2.5
        return out, f
    return fn


def test_run_guarded_reports_unwritten_bytes_and_stray_stores():
    kw = dict(device_types=("cpu",), modules=(__name__,))
    orig = torch.empty
    out, f = lean_ref.run_guarded(_fake_op(), **kw)
    assert out.flatten().tolist() == list(range(105)) and f.tolist() == [2.5] * 4
    assert torch.empty is orig  # the patch is gone

    def unwritten():
        out = torch.empty(3, 5, 7, dtype=torch.int8)
        out.view(-1)[:52] = 1
        out.view(-1)[53:] = 1  # byte 52 keeps the fill
        return out
    with pytest.raises(AssertionError, match="differ between the two fills"):
        lean_ref.run_guarded(unwritten, **kw)
    for stray in (-1, 105, -lean_ref.GUARD, 105 + lean_ref.GUARD - 1):  # just outside, and the guards' far ends
        with pytest.raises(AssertionError, match="guard (before|after)"):
            lean_ref.run_guarded(_fake_op(stray=stray), **kw)
    with pytest.raises(AssertionError, match="no guarded output"):
        lean_ref.run_guarded(lambda: torch.zeros(3), **kw)
    # tensors of other modules, dtypes and devices are left alone
    with lean_ref.guarded(0x5A, device_types=("cpu",), modules=("smpq.ops",)) as g:
        torch.empty(8, dtype=torch.int8)
    assert not g.bufs
