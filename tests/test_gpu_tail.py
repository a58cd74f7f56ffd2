"""The kernels behind the last feature map on the GPU, against the float64 references and bounds of
tests/tail_ref.py (tests/test_tail_ref_host.py shows on the CPU that those checkers reject wrong
kernels): avgpool + fc, softmax / cross entropy, KL rows, content fingerprints and the quantizer's
status and edges. Every output of the five entry points is written between pre-filled guard
regions in at least one test (lean_ref.run_guarded for what smpq.ops or the helpers here allocate;
stats, the fingerprint outputs and the flag inside larger pre-filled tensors whose neighbours are
checked). The bounds fix no summation order: a rewrite that reorders a sum must still pass.

Largest error / bound ratios seen on an MI355X are in DESIGN.md 1 (tail_ref.OBSERVED collects them).
"""
import numpy as np
import pytest
import torch

import tail_ref as tr
from lean_ref import GUARD, run_guarded

pytestmark = pytest.mark.gpu

HERE = (__name__,)  # run_guarded: guard the fp32 buffers this module allocates with torch.empty


def _bits(t):
    """Bitwise view for comparisons that must hold for NaN too."""
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def _framed(values, fill):
    """(whole, view): a device tensor of 3 len(values) elements pre-filled with ``fill`` whose middle
    third holds ``values``; the kernel gets the view, the test checks the rest afterwards."""
    k = len(values)
    whole = torch.full((3 * k,), fill, dtype=values.dtype, device=values.device)
    whole[k:2 * k] = values
    return whole, whole[k:2 * k]


def _frame_intact(whole, fill):
    k = whole.numel() // 3
    return bool((whole[:k] == fill).all()) and bool((whole[2 * k:] == fill).all())


# ---- 1. avgpool + fc -----------------------------------------------------------------------------
def _avgpool_fc_guarded(gpu, x, w, b):
    """(logits [n, nout], pooled [n, c]) of one call whose ``out`` is rows 2 .. 2 + n of a larger
    pre-filled logits tensor and whose pooled workspace smpq.ops allocates under guards."""
    from smpq import ops
    n, nout, c = x.shape[0], w.shape[0], x.shape[-1]

    def fn():
        g = torch.empty.__self__  # the active lean_ref.guarded
        big = torch.full(((n + 4) * nout * 4,), g.fill, dtype=torch.uint8, device=gpu)
        big = big.view(torch.float32).view(n + 4, nout)
        out = ops.avgpool_fc(x, w, b, out=big[2:2 + n])
        assert out.data_ptr() == big[2:2 + n].data_ptr()
        buf, nbytes = g.bufs[-1]
        assert len(g.bufs) == 1 and nbytes == 4 * n * c
        rest = torch.cat([big[:2], big[2 + n:]]).view(torch.uint8)
        assert bool((rest == g.fill).all()), "rows next to out= were written"
        return big[2:2 + n].clone(), buf[GUARD:GUARD + nbytes].view(torch.float32).view(n, c).clone()
    return run_guarded(fn)


@pytest.mark.parametrize("i", range(len(tr.FC_CASES)))
def test_avgpool_fc_vs_float64(gpu, i):
    from smpq import ops
    n, hw, c, nout = tr.FC_CASES[i]
    xh, wh, bh = tr.fc_inputs(i)
    x, w, b = (torch.from_numpy(a).to(gpu) for a in (xh.reshape(n, 1, hw, c), wh, bh))
    y_b, pooled = _avgpool_fc_guarded(gpu, x, w, b)
    y_0, pooled_0 = _avgpool_fc_guarded(gpu, x, w, None)
    rp, ry = tr.check_fc(pooled.cpu().numpy(), y_b.cpu().numpy(), tr.fc_reference(xh, wh, bh))
    _, ry0 = tr.check_fc(pooled_0.cpu().numpy(), y_0.cpu().numpy(), tr.fc_reference(xh, wh, None))
    print("avgpool_fc %s: error / bound pooled %.4f, logits %.4f (no bias %.4f)" % (tr.FC_CASES[i], rp, ry, ry0))
    tr.observe("fc_pooled", rp)
    tr.observe("fc_logits", max(ry, ry0))
    assert torch.equal(_bits(pooled), _bits(pooled_0))
    # the bias is added last: one rounded fp32 addition on top of the logits without it
    assert torch.equal(_bits(y_b), _bits(y_0 + b[None, :]))
    # batch invariance, bitwise: the first image, the last, and a slice across the 8-image block edge
    slices = [(0, 1), (n - 1, n)] + ([(6, min(n, 11))] if n > 8 else [])
    for lo, hi in slices:
        for bias, full in ((b, y_b), (None, y_0)):
            part = ops.avgpool_fc(x[lo:hi].contiguous(), w, bias)
            assert torch.equal(_bits(part), _bits(full[lo:hi])), (lo, hi, bias is not None)


# ---- 2. softmax / cross entropy ------------------------------------------------------------------
STATS0 = (0.5, 7.0, 11.0, 2.0)  # non-zero accumulators: the kernel must add, not store
FRAME = -123.25


def _softmax_call(x, labels, want_probs=True):
    """smpq_softmax_xent through the C ABI with row_ws and probs allocated here (guarded under
    run_guarded) and stats framed by hand: (row_ws, probs or None, stats after)."""
    from smpq import _lib
    rows, cols = x.shape
    ws = torch.empty(2 * rows, dtype=torch.float32, device=x.device)
    spare = torch.empty(rows, cols, dtype=torch.float32, device=x.device)  # probs, or a buffer no one may write
    probs = spare if want_probs else None
    whole, stats = _framed(torch.tensor(STATS0, dtype=torch.float64, device=x.device), FRAME)
    _lib.check(_lib.load().smpq_softmax_xent(_lib.ptr(x), _lib.ptr(labels), rows, cols, _lib.ptr(probs),
                                             _lib.ptr(stats), _lib.ptr(ws), _lib.stream_ptr()), "smpq_softmax_xent")
    assert _frame_intact(whole, FRAME), "stats' neighbours were written"
    if not want_probs:
        fill = torch.empty.__self__.fill  # the active lean_ref.guarded
        assert bool((spare.view(torch.uint8) == fill).all()), "probs = NULL, yet a buffer was written"
    return _bits(ws), (None if probs is None else _bits(probs)), _bits(stats.clone())


def _softmax_guarded(gpu, xh, yh, want_probs=True):
    """One guarded call on host arrays -> numpy (row_ws, probs or None, stats after)."""
    x, y = torch.from_numpy(xh).to(gpu), torch.from_numpy(yh).to(gpu)
    ws, probs, stats = run_guarded(lambda: _softmax_call(x, y, want_probs), modules=HERE)
    return (ws.view(torch.float32).cpu().numpy(), None if probs is None else probs.view(torch.float32).cpu().numpy(),
            stats.view(torch.float64).cpu().numpy())


def _check_softmax(gpu, xh, yh, family):
    ref = tr.softmax_reference(xh, yh)
    ws, probs, stats = _softmax_guarded(gpu, xh, yh)
    r = tr.check_softmax_rows(ws, probs, ref)
    tr.check_softmax_stats(np.array(STATS0), stats, ws, ref)
    print("softmax_xent %s %s: loss error / bound %.4f" % (family, xh.shape, r))
    tr.observe("softmax_loss_" + family, r)
    return ws, probs, stats, ref


@pytest.mark.parametrize("rows,cols", tr.SOFTMAX_SHAPES)
def test_softmax_xent_rows_vs_float64(gpu, rows, cols):
    xh, yh = tr.softmax_inputs(rows, cols)
    ws, probs, stats, ref = _check_softmax(gpu, xh, yh, "randn")
    assert np.array_equal(probs.argmax(axis=1), ref["pred"])
    # probs = NULL: the same stats bit for bit, and nothing but row_ws is written
    ws0, none, stats0 = _softmax_guarded(gpu, xh, yh, want_probs=False)
    assert none is None and np.array_equal(stats0.view(np.int64), stats.view(np.int64))
    assert np.array_equal(ws0.view(np.int32), ws.view(np.int32))


def test_softmax_xent_ties_take_the_first_maximal_class(gpu):
    xh, yh = tr.tie_inputs()
    ws, probs, stats, ref = _check_softmax(gpu, xh, yh, "ties")
    rows = len(yh)
    # per duplicated pair (and for the all-equal rows): label on the lowest index counts, the higher
    # duplicate and any other class do not
    assert ws[rows:].tolist() == [1.0, 0.0, 0.0] * (len(tr.TIE_PAIRS) + 1)
    for r, (lo, hi) in enumerate(tr.TIE_PAIRS):
        assert probs[3 * r, lo] == probs[3 * r, hi] == probs[3 * r].max()


def test_softmax_xent_range(gpu):
    cases = tr.range_inputs()
    for name in ("plus1000", "minus300"):
        _check_softmax(gpu, *cases[name], family=name)
    xh, yh = cases["underflow"]
    ws, probs, _, _ = _check_softmax(gpu, xh, yh, "underflow")
    top = xh.argmax(axis=1)
    other = np.ones_like(probs, bool)
    other[np.arange(len(yh)), top] = False
    assert (probs[other] == 0).all() and (probs[~other] == 1).all() and np.isfinite(ws).all()
    assert (ws[:3] == 0).all() and (ws[3:6] > 200).all()
    xh, yh = cases["neg_inf"]
    ws, probs, stats, _ = _check_softmax(gpu, xh, yh, "neg_inf")
    assert np.isinf(xh).sum() == 15 and (probs[np.isinf(xh)] == 0).all()
    assert np.isfinite(ws).all() and np.isfinite(probs).all() and np.isfinite(stats).all()


def test_softmax_xent_label_out_of_range(gpu):
    xh, yh = tr.softmax_inputs(5, 65)
    yh[1], yh[3] = -1, 65
    ws, probs, stats, ref = _check_softmax(gpu, xh, yh, "bad_label")  # NaN rows 1 and 3, the others checked
    assert np.isnan(stats[0]) and np.isnan(ws[[1, 3]]).all() and (ws[[6, 8]] == 0).all()
    assert stats[1:].tolist() == [STATS0[1] + ref["correct"].sum(), STATS0[2] + 5, STATS0[3] + 1]
    assert ref["correct"].sum() >= 1


# ---- 3. KL rows ----------------------------------------------------------------------------------
KL0 = (0.25, 3.0)


def _kl_call(a, b):
    from smpq import _lib
    rows, cols = a.shape
    ws = torch.empty(rows, dtype=torch.float32, device=a.device)
    whole, stats = _framed(torch.tensor(KL0, dtype=torch.float64, device=a.device), FRAME)
    _lib.check(_lib.load().smpq_kl_rows(_lib.ptr(a), _lib.ptr(b), rows, cols, _lib.ptr(stats), _lib.ptr(ws),
                                        _lib.stream_ptr()), "smpq_kl_rows")
    assert _frame_intact(whole, FRAME), "stats' neighbours were written"
    return _bits(ws), _bits(stats.clone())


def _kl_guarded(gpu, ah, bh):
    """One guarded call (run twice by run_guarded, which also asserts the two runs' row sums and stats
    equal bit for bit: the determinism check) -> numpy (row_ws, stats after)."""
    a, b = torch.from_numpy(ah).to(gpu), torch.from_numpy(bh).to(gpu)
    ws, stats = run_guarded(lambda: _kl_call(a, b), modules=HERE)
    return ws.view(torch.float32).cpu().numpy(), stats.view(torch.float64).cpu().numpy()


@pytest.mark.parametrize("rows,cols", tr.KL_SHAPES)
def test_kl_rows_vs_float64(gpu, rows, cols):
    for family in ("independent", "near"):
        ah, bh = tr.kl_inputs(rows, cols, family)
        ref = tr.kl_reference(ah, bh)
        ws, stats = _kl_guarded(gpu, ah, bh)
        r = tr.check_kl_rows(ws, ref)  # the absolute per-row bound, for the near family too
        tr.check_kl_stats(np.array(KL0), stats, ws, ref)
        rel = abs(ws.astype(np.float64).mean() - ref["kl"].mean()) / ref["kl"].mean()
        print("kl_rows %s %s: error / bound %.4f, mean KL %.4e, relative error of the mean %.3e" % (
            family, ah.shape, r, ref["kl"].mean(), rel))
        tr.observe("kl_" + family, r)
        tr.observe("kl_%s_mean_relative_error" % family, rel)
    ws, stats = _kl_guarded(gpu, ah, ah)  # identical inputs: exactly zero
    assert (ws == 0).all() and stats.tolist() == [KL0[0], KL0[1] + rows]


def test_kl_rows_inf_and_nan_rows(gpu):
    ah, bh = tr.kl_inputs(5, 65, "independent")
    bh[1, 7] = 0.0  # o = 0 < n: +inf
    ref = tr.kl_reference(ah, bh)
    ws, stats = _kl_guarded(gpu, ah, bh)
    tr.check_kl_rows(ws, ref)
    assert ws[1] == np.inf and stats[0] == np.inf and stats[1] == KL0[1] + 5
    ah[3, 9] = 0.0  # n = 0: NaN, the reference's 0 * log 0
    ref = tr.kl_reference(ah, bh)
    ws, stats = _kl_guarded(gpu, ah, bh)
    tr.check_kl_rows(ws, ref)
    tr.check_kl_stats(np.array(KL0), stats, ws, ref)
    assert ws[1] == np.inf and np.isnan(ws[3]) and np.isnan(stats[0]) and np.isfinite(ws[[0, 2, 4]]).all()


# ---- 4. fingerprints -----------------------------------------------------------------------------
class _Arena:
    """The tensors of tail_ref.fingerprint_layout as views of one device byte buffer, with a
    Fingerprinter over them and the reference fingerprints of the host copy."""

    def __init__(self, gpu):
        from smpq.fingerprint import Fingerprinter
        self.layout, self.host = tr.fingerprint_arena()
        self.dev = torch.from_numpy(self.host).to(gpu)
        assert self.dev.data_ptr() % 16 == 0
        self.tensors = [self.dev[off:off + nb].view(getattr(torch, dt)) for dt, off, nb in self.layout]
        for t, (_, off, nb) in zip(self.tensors, self.layout):
            assert t.is_contiguous() and t.data_ptr() % 16 == off % 16 and t.numel() * t.element_size() == nb
        self.fp = Fingerprinter(self.tensors, gpu)
        assert self.fp.n == len(self.layout)
        self.want = [tr.fingerprint_reference(self.host, off, nb) for _, off, nb in self.layout]
        self.fill = 0x5A5A5A5A5A5A5A5A

    def compute(self):
        """Fingerprints into the middle of a pre-filled int64 tensor (every slot overwritten, the
        neighbours untouched) -> list of Python ints."""
        n = self.fp.n
        whole = torch.full((3 * n,), self.fill, dtype=torch.int64, device=self.dev.device)
        self.fp.compute(whole[n:2 * n])
        assert _frame_intact(whole, self.fill), "fingerprint slots next to out were written"
        return whole[n:2 * n].cpu().numpy().view(np.uint64).tolist()

    def flip(self, offsets_and_masks):
        idx = torch.tensor([o for o, _ in offsets_and_masks], device=self.dev.device)
        mask = torch.tensor([m for _, m in offsets_and_masks], dtype=torch.uint8, device=self.dev.device)
        self.dev[idx] = self.dev[idx] ^ mask


def test_fingerprint_every_size_and_alignment(gpu):
    from smpq import _lib
    from smpq.fingerprint import host_fingerprint
    assert int(_lib.load().smpq_fingerprint_chunk_words()) == tr.CHUNK_WORDS
    a = _Arena(gpu)
    got = a.compute()
    assert got == a.want
    assert got == [host_fingerprint(t.cpu()) for t in a.tensors]
    assert a.fp.ref.cpu().numpy().view(np.uint64).tolist() == got and a.compute() == got
    assert a.fill not in got and len(set(got)) == len(got)


def test_fingerprint_sees_inside_bytes_only(gpu):
    a = _Arena(gpu)
    base = a.compute()
    assert base == a.want
    # bytes that belong to no tensor: the one before each, those completing its last word, the next
    outside = [(o, 0xFF) for o in tr.outside_bytes(a.layout)]
    a.flip(outside)
    assert a.compute() == base
    a.flip(outside)
    # bytes inside: each flip changes its own tensor's fingerprint and no other (half of the tensors
    # per compute, so that an unchanged neighbour is seen next to every changed one)
    for name, flips in tr.inside_flips(a.layout).items():
        for parity in (0, 1):
            part = [f for f in flips if f[0] % 2 == parity]
            if not part:
                continue
            a.flip([(at, mask) for _, at, mask in part])
            now = a.compute()
            hit = {t for t, _, _ in part}
            changed = {t for t in range(len(base)) if now[t] != base[t]}
            assert changed == hit, (name, parity, sorted(changed ^ hit))
            a.flip([(at, mask) for _, at, mask in part])
    assert a.compute() == base
    # order: swapping two unequal words of the 3-word tensor
    t = a.tensors[1].view(torch.int32)
    assert int(t[0]) != int(t[1])
    t[:2] = t[:2].flip(0)
    now = a.compute()
    assert now[1] != base[1] and now[:1] + now[2:] == base[:1] + base[2:]


def test_fingerprint_compare_flag(gpu):
    from smpq import _lib
    lib = _lib.load()
    n = 300  # more than the kernel's 256 threads
    a = torch.randint(-2 ** 62, 2 ** 62, (n,), generator=torch.Generator().manual_seed(8)).to(gpu)

    def compare(b, start):
        whole, flag = _framed(torch.tensor([start], dtype=torch.int32, device=gpu), 0x5A5A5A5A)
        _lib.check(lib.smpq_fingerprint_compare(_lib.ptr(a), _lib.ptr(b), n, _lib.ptr(flag), _lib.stream_ptr()),
                   "smpq_fingerprint_compare")
        assert _frame_intact(whole, 0x5A5A5A5A), "the flag's neighbours were written"
        return int(flag.item())
    same = a.clone()
    first, last = a.clone(), a.clone()
    first[0] ^= 1 << 40
    last[n - 1] ^= 1
    assert compare(same, 0) == 0 and compare(same, 2) == 2
    for b in (first, last):
        assert compare(b, 0) == 1 and compare(b, 2) == 3 and compare(b, 1) == 1


# ---- 5. quantizer status and edges ---------------------------------------------------------------
def test_quantizer_reports_the_lowest_constant_channel(gpu):
    """One call per side (no repetition to catch a race: the kernel keeps the minimum by construction)."""
    from smpq import ops
    w, bits, expect = tr.constant_channel_layer()
    wd = torch.from_numpy(w.copy()).to(gpu)
    with pytest.raises(ZeroDivisionError, match=r"constant channel 3\)"):
        ops.quantize_channels_(wd, torch.from_numpy(bits), semantics="cpu")
    # the device quantizes every non-constant channel and leaves the constant ones untouched
    assert np.array_equal(wd.cpu().numpy().view(np.uint32), expect.view(np.uint32))
    wh = torch.from_numpy(w.copy())
    with pytest.raises(ZeroDivisionError, match=r"constant channel 3\)"):
        ops.quantize_channels_(wh, torch.from_numpy(bits), semantics="cpu")
    # the host twin stops there: channels 0..2 quantized, 3 and every later one untouched
    assert np.array_equal(wh.numpy()[:3].view(np.uint32), expect[:3].view(np.uint32))
    assert np.array_equal(wh.numpy()[3:].view(np.uint32), w[3:].view(np.uint32))


@pytest.mark.parametrize("k", tr.QUANT_K)
def test_quantizer_layer_equals_host_twin(gpu, k):
    from smpq import ops
    w, bits = tr.quant_layer(k)
    for sem in ("cpu", "device"):
        wd = torch.from_numpy(w.copy()).to(gpu)
        sd = ops.quantize_channels_(wd, torch.from_numpy(bits), semantics=sem)
        wh = torch.from_numpy(w.copy())
        sh = ops.quantize_channels_(wh, torch.from_numpy(bits), semantics=sem)
        assert torch.equal(_bits(wd.cpu()), _bits(wh)), sem
        assert torch.equal(_bits(sd.cpu()), _bits(sh)), sem
        assert bool((sh[torch.from_numpy(bits) == 0] == 0).all())


def test_quantizer_subnormal_step_equals_host_twin(gpu):
    """A channel whose values are all of magnitude <= 1e-38 at 8 bits: the step (max - min) / 255 is a
    subnormal fp32. The device must equal the host twin bit for bit."""
    from smpq import ops
    g = np.random.default_rng(38)
    w = (g.uniform(-1.0, 1.0, (1, 64)) * 1e-38).astype(np.float32)
    w[0, :2] = (-1e-38, 1e-38)
    assert (np.abs(w) <= 1e-38).all() and (w != 0).all()
    wd = torch.from_numpy(w.copy()).to(gpu)
    sd = ops.quantize_channels_(wd, [8], semantics="cpu")
    wh = torch.from_numpy(w.copy())
    sh = ops.quantize_channels_(wh, [8], semantics="cpu")
    tiny = float(np.finfo(np.float32).tiny)
    assert 0 < float(sh[0]) < tiny, float(sh[0])
    print("subnormal step: host %r device %r; weights differing: %d of 64" % (
        float(sh[0]), float(sd.cpu()[0]), int((_bits(wd.cpu()) != _bits(wh)).sum())))
    assert torch.equal(_bits(sd.cpu()), _bits(sh))
    assert torch.equal(_bits(wd.cpu()), _bits(wh))
