"""The one-row trial conv on the host (include/smpq.h "trial rows conv", csrc/trial_row_host.h): the
native twin behind ops.trial_rows_conv on CPU tensors against tests/lean_ref.py's float64 restatement
of the lean static-range epilogue, within its bound |code - z| <= 0.5 + 2e-6 B; the save / restore
round trip; the bytes it must leave alone; the argument errors of the wrapper and of the C entry
points (no GPU needed)."""
import ctypes

import numpy as np
import pytest
import torch

import lean_ref
from lean_ref import LIMB_QMAX, check_codes, encode, expected_overflow, lean_reference

FILL = 0x5A


def _case(k, L, LW, n, h, w, cin, cout, seed, residual=True):
    """Random operands of one conv: non-negative activation codes over the whole range (what a ReLU
    leaves), per-image ranges that differ, full-range weight codes, a signed residual."""
    g = np.random.default_rng(seed)
    qa, qw = int(LIMB_QMAX[L]), int(LIMB_QMAX[LW])
    xq = encode(g.integers(0, qa + 1, (n, h, w, cin)), L)
    am = (1.5 * (1.0 + np.arange(n) % 3)).astype(np.float32)
    wq = encode(g.integers(-qw, qw + 1, (cout, k * k * cin)), LW)
    cs = ((g.random(cout) * 1e-3 + 5e-4) / qw).astype(np.float32)
    sh = np.linspace(-0.3, 0.3, cout).astype(np.float32)
    rq = encode(g.integers(-qa, qa + 1, (n, h, w, cout)), L) if residual else None
    return dict(k=k, pad=k // 2, L=L, LW=LW, xq=xq, am=am, wq=wq, cs=cs, sh=sh, rq=rq, rr=2.0 if residual else None)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).clone()


def _run(c, rows, emit_range):
    """(planes after the call, baseline, save area, overflow word, the TrialRows) on CPU tensors."""
    from smpq import ops
    L, n, h, w, _ = c["xq"].shape
    cout = c["wq"].shape[1]
    g = np.random.default_rng(99)
    base = torch.from_numpy(g.integers(-128, 128, (L, n, h, w, cout)).astype(np.int8))
    yq = base.clone()
    save = torch.full((ops.trial_rows_conv_save_bytes(L, n * h * w, len(rows)),), FILL, dtype=torch.int8)
    ovf = torch.zeros(1, dtype=torch.int32)
    tr = ops.trial_rows_conv(_t(c["xq"]), _t(c["am"]), _t(c["wq"]), c["k"], c["k"], 1, c["pad"], _t(c["cs"]),
                             _t(c["sh"]), rows, yq, emit_range, ovf, save, residual_q=_t(c["rq"]),
                             residual_range=c["rr"])
    return yq, base, save, ovf, tr


CASES = [
    # k, L, LW, n, h, w, cin, cout, rows, residual
    (1, 3, 3, 3, 5, 5, 64, 32, [31, 0, 17], True),
    (1, 3, 2, 2, 3, 3, 128, 16, [5], True),      # two 64-byte K steps, SMIN = 1
    (1, 2, 2, 1, 4, 4, 64, 16, [15], True),
    (3, 3, 3, 2, 5, 5, 64, 32, [1, 30], True),    # K = 576, border and interior pixels
    (3, 3, 3, 1, 2, 2, 64, 16, [12], False),      # 2 x 2: five of nine taps fall outside, for every pixel
]


@pytest.mark.parametrize("factor", [2.0, 0.5])
@pytest.mark.parametrize("k,L,LW,n,h,w,cin,cout,rows,residual", CASES)
def test_host_twin_against_the_float64_reference(built_lib, k, L, LW, n, h, w, cin, cout, rows, residual, factor):
    from smpq import ops
    c = _case(k, L, LW, n, h, w, cin, cout, seed=11 * k + L + LW, residual=residual)
    y, bound = lean_ref.lean_real(c["xq"], c["wq"], None, k, 1, c["pad"], c["am"], c["cs"], c["sh"], c["rq"], c["rr"])
    emit_range = lean_ref.emit_range_for(y[..., rows], True, factor)
    z, B = lean_reference(c["xq"], c["wq"], None, k, 1, c["pad"], c["am"], c["cs"], c["sh"], c["rq"], c["rr"],
                          relu=True, emit_range=emit_range)
    yq, base, save, ovf, tr = _run(c, rows, emit_range)
    got = yq.numpy()
    check_codes(np.ascontiguousarray(got[..., rows]), z[..., rows], B[..., rows], True, L)
    want = expected_overflow(z[..., rows], B[..., rows], L)
    assert want == (1 if factor < 1 else 0) and int(ovf.item()) == want
    others = [ch for ch in range(cout) if ch not in rows]
    assert np.array_equal(got[..., others], base.numpy()[..., others])  # every other channel stays
    M = n * h * w
    slots = save.numpy().reshape(len(rows), L, M)
    for i, ch in enumerate(rows):  # slot i: channel rows[i]'s old bytes, limb-major
        assert np.array_equal(slots[i], base.numpy().reshape(L, M, cout)[:, :, ch])
    ops.trial_rows_conv_restore(tr, yq, save)
    assert torch.equal(yq, base)
    ops.trial_rows_conv_restore(rows, yq, save)  # (a plain list works too, and restoring twice is harmless)
    assert torch.equal(yq, base)


def test_the_twin_is_deterministic_and_reads_the_current_planes(built_lib):
    """Two calls in a row: the second saves what the first wrote and writes it again."""
    from smpq import ops
    c = _case(1, 3, 3, 2, 3, 3, 64, 16, seed=5)
    yq, base, save, ovf, tr = _run(c, [7], 50.0)
    first = yq.clone()
    save2 = torch.zeros_like(save)
    ops.trial_rows_conv(_t(c["xq"]), _t(c["am"]), _t(c["wq"]), 1, 1, 1, 0, _t(c["cs"]), _t(c["sh"]), tr, yq, 50.0, ovf,
                        save2, residual_q=_t(c["rq"]), residual_range=c["rr"])
    assert torch.equal(yq, first)
    assert np.array_equal(save2.numpy().reshape(3, -1), first.numpy().reshape(3, -1, 16)[:, :, 7])


def test_wrapper_argument_errors(built_lib):
    from smpq import ops
    c = _case(1, 3, 3, 1, 2, 2, 64, 16, seed=1)
    xq, am, wq, cs, sh, rq = (_t(c[k]) for k in ("xq", "am", "wq", "cs", "sh", "rq"))
    yq = torch.zeros(3, 1, 2, 2, 16, dtype=torch.int8)
    save = torch.zeros(ops.trial_rows_conv_save_bytes(3, 4, 2), dtype=torch.int8)
    ovf = torch.zeros(1, dtype=torch.int32)
    assert ops.trial_rows_conv_save_bytes(3, 4, 2) == 24

    def call(**kw):
        a = dict(xq=xq, am=am, wq=wq, kh=1, kw=1, stride=1, pad=0, cs=cs, sh=sh, rows=[3, 0], yq=yq, rng=1.0, ovf=ovf,
                 save=save, rq=rq, rr=2.0)
        a.update(kw)
        return ops.trial_rows_conv(a["xq"], a["am"], a["wq"], a["kh"], a["kw"], a["stride"], a["pad"], a["cs"], a["sh"],
                                   a["rows"], a["yq"], a["rng"], a["ovf"], a["save"], residual_q=a["rq"],
                                   residual_range=a["rr"])

    call()
    before = yq.clone()
    for bad in (dict(rows=[3, 3]), dict(rows=[16]), dict(rows=[-1]), dict(rows=[]), dict(kh=3, kw=3, pad=0),
                dict(stride=2), dict(kh=3, kw=3, pad=1),  # (K of the codes disagrees)
                dict(rng=0.0), dict(rng=None), dict(save=save[:23]), dict(rr=None), dict(rr=-1.0),
                dict(wq=wq[:1].contiguous()), dict(wq=wq[:, :8].contiguous()), dict(am=am[:0]),
                dict(yq=torch.zeros(3, 1, 2, 3, 16, dtype=torch.int8)), dict(yq=yq.float()),
                dict(yq=torch.zeros(1, 1, 2, 2, 16, dtype=torch.int8)), dict(cs=cs[:8].contiguous()),
                dict(ovf=torch.zeros(1)), dict(xq=xq[:2].contiguous()),
                dict(xq=xq.reshape(-1)[1:1 + 64].reshape(1, 1, 1, 1, 64))):
        with pytest.raises(ValueError):
            call(**bad)
    assert torch.equal(yq, before)
    with pytest.raises(ValueError):
        ops.trial_rows_conv_restore([16], yq, save)
    with pytest.raises(ValueError):
        ops.trial_rows_conv_restore([0, 1, 2], yq, save)  # three slots do not fit the save area


def test_c_entry_point_return_codes(built_lib):
    """Before any write: nothing behind these pointers is large enough to be read or written."""
    from smpq import _lib
    lib = built_lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) & ~15
    ch = (ctypes.c_int32 * 2)(1, 0)
    dup = (ctypes.c_int32 * 2)(1, 1)
    chp, dupp = ctypes.addressof(ch), ctypes.addressof(dup)

    def conv(xq=p16, am=p, n=1, h=1, w=1, cin=64, codes=p16, wl=3, cout=16, kh=1, kw=1, st=1, pad=0, cs=p, sh=p, L=3,
             rq=None, rr=0.0, chans=chp, nrows=2, yq=p, rng=1.0, ovf=p, save=p):
        return lib.smpq_trial_rows_conv_q_host(xq, am, n, h, w, cin, codes, wl, cout, kh, kw, st, pad, cs, sh, L, rq, rr,
                                               chans, nrows, yq, rng, ovf, save)

    E_INVALID, E_SHAPE = _lib.SMPQ_E_INVALID, _lib.SMPQ_E_SHAPE
    for kw in (dict(xq=None), dict(am=None), dict(codes=None), dict(cs=None), dict(sh=None), dict(chans=None),
               dict(yq=None), dict(ovf=None), dict(save=None), dict(L=1), dict(L=4), dict(wl=1), dict(wl=4),
               dict(L=2, wl=3), dict(rng=0.0), dict(rq=p, rr=0.0), dict(nrows=0), dict(nrows=17), dict(xq=p16 + 1),
               dict(codes=p16 + 8), dict(chans=dupp), dict(chans=(ctypes.c_int32 * 2)(1, 16)),
               dict(chans=(ctypes.c_int32 * 2)(-1, 0))):
        assert conv(**kw) == E_INVALID, kw
        assert b"smpq_trial_rows_conv_q" in lib.smpq_last_error()
    for kw in (dict(kh=3, kw=3), dict(kh=3, kw=3, pad=1, st=2), dict(kh=1, kw=3), dict(st=2), dict(pad=1), dict(cin=32),
               dict(kh=3, kw=3, pad=1, cin=576), dict(cout=24), dict(n=0), dict(h=0), dict(n=1 << 16, h=1 << 15, w=1)):
        assert conv(**kw) == E_SHAPE, kw
    restore = lib.smpq_trial_rows_conv_restore_host
    assert restore(None, 2, 3, 1, 16, p, p) == E_INVALID and restore(chp, 2, 3, 1, 16, None, p) == E_INVALID
    assert restore(chp, 2, 3, 1, 16, p, None) == E_INVALID and restore(chp, 2, 1, 1, 16, p, p) == E_INVALID
    assert restore(chp, 0, 3, 1, 16, p, p) == E_INVALID and restore(chp, 17, 3, 1, 16, p, p) == E_INVALID
    assert restore(dupp, 2, 3, 1, 16, p, p) == E_INVALID
    assert restore(chp, 2, 3, 0, 16, p, p) == E_SHAPE and restore(chp, 2, 3, 1 << 31, 16, p, p) == E_SHAPE
    assert b"smpq_trial_rows_conv_restore" in lib.smpq_last_error()
    assert bytes(buf) == b"\0" * 64
    # the device entry points check the same things before any launch
    assert lib.smpq_trial_rows_conv_q(None, p, 1, 1, 1, 64, p16, 3, 16, 1, 1, 1, 0, p, p, 3, None, 0.0, chp, 2, p, 1.0, p,
                                      p, None) == E_INVALID
    assert lib.smpq_trial_rows_conv_q(p16, p, 1, 1, 1, 64, p16, 3, 16, 3, 3, 1, 0, p, p, 3, None, 0.0, chp, 2, p, 1.0,
                                      p, p, None) == E_SHAPE
    assert lib.smpq_trial_rows_conv_restore(chp, 0, 3, 1, 16, p, p, None) == E_INVALID
