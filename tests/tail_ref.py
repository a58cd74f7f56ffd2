"""Helpers of tests/test_gpu_tail.py and tests/test_tail_ref_host.py (not a test module): float64
references, error bounds and checkers of the kernels behind the last feature map.

  * avgpool + fc (smpq_avgpool_fc): float64 mean over the pixels and float64 matmul on the fp32
    inputs; bounds that hold for any summation order;
  * softmax / cross entropy (smpq_softmax_xent) and KL rows (smpq_kl_rows): per-row float64 values
    on the fp32 inputs (the same formulas as oracle/eval_ref.py, which reports only means);
  * fingerprints (smpq_fingerprint): a vectorised numpy restatement of H from include/smpq.h, and the
    plain-integer one test_native_host.py pins the host twin with;
  * the deterministic inputs the GPU tests and the CPU tests share, fp32 numpy emulations of correct
    kernels, and the wrong kernels the checkers must reject (test_tail_ref_host.py).

Every bound here comes from the number formats (u = 2^-24, the fp32 unit roundoff), none from what
the kernels were seen to return. Checkers return the largest error / bound ratio they saw; the GPU
tests collect those in OBSERVED (never asserted on; SMPQ_TAIL_REF_STATS=<path> writes them out).
"""
import atexit
import json
import os

import numpy as np

U = 2.0 ** -24
M32 = (1 << 32) - 1

OBSERVED = {}


def observe(family, ratio):
    OBSERVED[family] = max(OBSERVED.get(family, 0.0), float(ratio))


@atexit.register
def _dump_observed():
    path = os.environ.get("SMPQ_TAIL_REF_STATS")
    if path and OBSERVED:
        with open(path, "w") as f:
            json.dump(OBSERVED, f, indent=1, sort_keys=True)


def _ratio(err, bound):
    """max err / bound over the elements with a positive bound (the others must be exact)."""
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


# ---- avgpool + fc --------------------------------------------------------------------------------
# (n, hw, c, nout): c = 36 / 100 / 132 end in a partial or empty last K-quarter, 384 runs an odd
# number (3) of chunk steps, hw sits on both sides of the 8-wide load batches (1, 2, 8, 9, 10, 17, 49),
# n on both sides of the 8-image block, nout on both sides of the 64-output block
FC_CASES = [(3, 1, 4, 1), (9, 9, 36, 10), (8, 10, 100, 63), (7, 17, 132, 65), (5, 49, 384, 64), (17, 2, 64, 10),
            (1, 8, 512, 1000), (9, 49, 2048, 1000)]


def fc_inputs(i):
    """(x [n, hw, c], w [nout, c], b [nout]) fp32 of FC_CASES[i]. Odd cases keep the sign of randn
    (cancellation in both sums), even ones are ReLU outputs as in the network; every image has its
    own scale, so no two rows of the logits look alike."""
    n, hw, c, nout = FC_CASES[i]
    g = np.random.default_rng(1000 + i)
    x = g.standard_normal((n, hw, c)).astype(np.float32)
    if i % 2 == 0:
        x = np.maximum(x, np.float32(0))
    x *= (1.0 + np.arange(n) % 3).astype(np.float32).reshape(n, 1, 1)
    w = (g.standard_normal((nout, c)) / np.sqrt(c)).astype(np.float32)
    b = (g.standard_normal(nout) * 0.1).astype(np.float32)
    return x, w, b


def fc_reference(x, w, b=None):
    """float64 mean over the pixels, then a float64 matmul (+ bias), on the fp32 inputs, with the
    bounds of an fp32 evaluation in ANY order: a sum of hw terms and one division carry at most
    (hw + 1) u relative to the sum of magnitudes, the dot product of c such features c + 1 more
    (one product and at most c - 1 .. c additions per term, the bias one)."""
    x64, w64 = x.astype(np.float64), w.astype(np.float64)
    n, hw, c = x.shape
    pooled = x64.mean(axis=1)
    P = np.abs(x64).sum(axis=1) / hw
    y = pooled @ w64.T
    mag = P @ np.abs(w64).T
    if b is not None:
        y = y + b.astype(np.float64)
        mag = mag + np.abs(b.astype(np.float64))
    return {"pooled": pooled, "pooled_bound": (hw + 1) * U * P, "y": y, "y_bound": (hw + c + 2) * U * mag}


def check_fc(pooled, y, ref):
    """Every pooled feature and every logit against fc_reference; returns the two largest
    error / bound ratios."""
    out = []
    for name, got in (("pooled", pooled), ("y", y)):
        got = np.asarray(got)
        want, bound = ref[name], ref[name + "_bound"]
        assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
        assert np.isfinite(got).all(), name
        err = np.abs(got.astype(np.float64) - want)
        bad = err > bound
        if bad.any():
            i = np.unravel_index(np.argmax(err - bound), err.shape)
            raise AssertionError("%s: %d of %d off, worst at %s: %r, reference %r, bound %.3e" % (
                name, bad.sum(), bad.size, i, got[i], want[i], bound[i]))
        out.append(_ratio(err, bound))
    return tuple(out)


def fc_emulate(x, w, b=None, drop_k=0, drop_pixel=0, divisor_extra=0, bias_times=1):
    """fp32 numpy emulation (pixels in order, k in order, every operation rounded): (pooled, y). The
    keyword arguments make the wrong kernels: the last K element(s) or pixel(s) left out, a divisor
    of hw + 1, the bias added twice."""
    n, hw, c = x.shape
    s = np.zeros((n, c), np.float32)
    for i in range(hw - drop_pixel):
        s = s + x[:, i]
    pooled = s / np.float32(hw + divisor_extra)
    y = np.zeros((n, w.shape[0]), np.float32)
    for k in range(c - drop_k):
        y = y + pooled[:, k:k + 1] * w[:, k][None, :]
    if b is not None:
        for _ in range(bias_times):
            y = y + b[None, :]
    assert pooled.dtype == np.float32 and y.dtype == np.float32
    return pooled, y


# ---- softmax / cross entropy ---------------------------------------------------------------------
def softmax_reference(x, labels):
    """Per-row float64 values of smpq_softmax_xent on fp32 logits: probs, loss (NaN for a label
    outside [0, cols)), its bound, the first maximal class and whether it equals the label.
    Bound: the fp32 sum of the exponentials is within (cols / 64 + 12) u of s relative (64 lanes of
    cols / 64 terms, six reduction levels, the exponentials' own error), which passes through the
    log as an absolute error; log s + m - x_y is three fp32 roundings of values no larger than
    |m| + |x_y| + |log s|."""
    x = np.asarray(x, np.float32).astype(np.float64)
    labels = np.asarray(labels, np.int64)
    rows, cols = x.shape
    with np.errstate(all="ignore"):
        m = x.max(axis=1)
        e = np.exp(x - m[:, None])
        s = e.sum(axis=1)
        ok = (labels >= 0) & (labels < cols)
        xy = np.where(ok, x[np.arange(rows), np.clip(labels, 0, cols - 1)], np.nan)
        loss = np.log(s) + m - xy
        bound = (cols / 64 + 12) * U + 4 * U * (np.abs(m) + np.abs(xy) + np.abs(np.log(s)))
    pred = x.argmax(axis=1)  # numpy: the first maximal index
    return {"probs": e / s[:, None], "loss": loss, "bound": bound, "pred": pred, "correct": ok & (pred == labels),
            "valid": ok, "rows": rows, "cols": cols}


PROBS_RTOL, PROBS_ATOL = 3e-6, 1e-12  # the project's softmax tolerance (tests/test_gpu_eval.py)


def check_softmax_rows(row_ws, probs, ref):
    """row_ws fp32 [2 * rows] as the kernel leaves it and probs fp32 [rows, cols] (or None) against
    softmax_reference; returns the largest loss error / bound."""
    rows = ref["rows"]
    row_ws = np.asarray(row_ws)
    assert row_ws.dtype == np.float32 and row_ws.shape == (2 * rows,), (row_ws.dtype, row_ws.shape)
    loss, flag = row_ws[:rows].astype(np.float64), row_ws[rows:]
    v = ref["valid"]
    assert np.isnan(loss[~v]).all(), "a label outside [0, cols) must give a NaN loss"
    assert np.isfinite(loss[v]).all()
    err = np.abs(loss[v] - ref["loss"][v])
    bad = err > ref["bound"][v]
    if bad.any():
        i = int(np.argmax(err - ref["bound"][v]))
        raise AssertionError("loss: %d of %d rows off, worst (valid row %d): %r, reference %r, bound %.3e" % (
            bad.sum(), bad.size, i, loss[v][i], ref["loss"][v][i], ref["bound"][v][i]))
    want = ref["correct"].astype(np.float32)
    if not np.array_equal(flag, want):
        i = int(np.nonzero(flag != want)[0][0])
        raise AssertionError("row %d: correct flag %r, reference %r (first maximal class %d)" % (
            i, flag[i], want[i], ref["pred"][i]))
    if probs is not None:
        probs = np.asarray(probs)
        assert probs.dtype == np.float32 and probs.shape == ref["probs"].shape
        np.testing.assert_allclose(probs, ref["probs"], rtol=PROBS_RTOL, atol=PROBS_ATOL)
    return _ratio(err, ref["bound"][v])


SUM_RTOL = 2e-15  # a fixed-order double sum of <= 2^24 fp32 values and one accumulation


def check_softmax_stats(before, after, row_ws, ref):
    """stats double [4] before and after one call: [1], [2], [3] move by exactly correct / rows / 1;
    [0] by the float64 mean of the device's own per-row losses (within 2e-15 of the value) and by the
    reference mean within the mean of the per-row bounds. Any NaN row makes [0] NaN."""
    before, after = np.asarray(before, np.float64), np.asarray(after, np.float64)
    rows = ref["rows"]
    assert after[1] - before[1] == float(ref["correct"].sum()), (before, after)
    assert after[2] - before[2] == float(rows) and after[3] - before[3] == 1.0, (before, after)
    if not ref["valid"].all():
        assert np.isnan(after[0])
        return
    own = np.asarray(row_ws)[:rows].astype(np.float64).mean()
    tol = SUM_RTOL * abs(after[0])
    assert abs((after[0] - before[0]) - own) <= tol, (after[0] - before[0], own, tol)
    assert abs((after[0] - before[0]) - ref["loss"].mean()) <= ref["bound"].mean() + tol


def softmax_emulate(x, labels, last_max=False, no_max_term=False, unnormalised=False):
    """fp32 numpy emulation of a correct kernel: (row_ws, probs). The keyword arguments make the wrong
    kernels: the LAST maximal class, a loss without the max term, probabilities not divided by s."""
    x = np.asarray(x, np.float32)
    labels = np.asarray(labels, np.int64)
    rows, cols = x.shape
    with np.errstate(all="ignore"):
        m = x.max(axis=1)
        e = np.exp(x - m[:, None])
        s = e.sum(axis=1, dtype=np.float32)
        ok = (labels >= 0) & (labels < cols)
        xy = np.where(ok, x[np.arange(rows), np.clip(labels, 0, cols - 1)], np.float32(np.nan)).astype(np.float32)
        loss = ((np.log(s) + (np.float32(0) if no_max_term else m)) - xy).astype(np.float32)
    pred = cols - 1 - x[:, ::-1].argmax(axis=1) if last_max else x.argmax(axis=1)
    probs = e if unnormalised else e / s[:, None]
    assert e.dtype == np.float32 and s.dtype == np.float32 and probs.dtype == np.float32
    return np.concatenate([loss, (ok & (pred == labels)).astype(np.float32)]), probs


SOFTMAX_ROWS = (1, 3, 4, 5, 255, 256, 257)   # at cols = 65: around the 4 rows of a block and the 256-thread row sum
SOFTMAX_COLS = (1, 2, 63, 64, 65, 129, 1000)  # at rows = 5: around the 64 lanes of a row's wave
SOFTMAX_SHAPES = [(r, 65) for r in SOFTMAX_ROWS] + [(5, c) for c in SOFTMAX_COLS if c != 65]


def softmax_inputs(rows, cols, seed=0, scale=4.0, shift=0.0):
    """randn * scale + shift logits; the first third of the labels are the rows' argmax."""
    g = np.random.default_rng(7000 + 1000 * rows + cols + seed)
    x = (g.standard_normal((rows, cols)) * scale + shift).astype(np.float32)
    y = g.integers(0, cols, rows)
    y[:(rows + 2) // 3] = x[:(rows + 2) // 3].argmax(axis=1)
    return x, y.astype(np.int64)


TIE_PAIRS = ((5, 70), (63, 64), (6, 69), (0, 128))  # cols = 129; lanes (5, 6), (63, 0), (6, 5), (0, 0)
TIE_COLS = 129


def tie_inputs():
    """Rows whose maximum is duplicated at each pair of TIE_PAIRS, each three times: label on the
    lower index (correct), on the higher duplicate (not correct), elsewhere; then three all-equal
    rows (label 0: correct; label 1, label cols - 1: not)."""
    g = np.random.default_rng(71)
    xs, ys = [], []
    for lo, hi in TIE_PAIRS:
        for label in (lo, hi, (lo + 1) % TIE_COLS):
            r = g.standard_normal(TIE_COLS).astype(np.float32)
            r[lo] = r[hi] = np.float32(r.max() + 1.5)
            xs.append(r)
            ys.append(label)
    for label in (0, 1, TIE_COLS - 1):
        xs.append(np.full(TIE_COLS, 0.75, np.float32))
        ys.append(label)
    return np.stack(xs), np.array(ys, np.int64)


def range_inputs():
    """{name: (x, labels)}: logits shifted by +1000 and -300; rows whose other classes sit 200 or more
    below the maximum (their probabilities underflow to 0; label on the maximum and off it); rows with
    -inf in classes that are not the label."""
    out = {"plus1000": softmax_inputs(5, 65, seed=1, shift=1000.0),
           "minus300": softmax_inputs(5, 65, seed=2, shift=-300.0)}
    g = np.random.default_rng(72)
    x = (-200.0 - np.abs(g.standard_normal((6, 65))) * 3).astype(np.float32)
    top = np.array([0, 64, 33, 7, 63, 1])
    x[np.arange(6), top] = np.float32(1.25)
    y = top.copy()
    y[3:] = (top[3:] + 5) % 65
    out["underflow"] = (x, y.astype(np.int64))
    x, y = softmax_inputs(5, 129, seed=3)
    for r in range(5):
        cls = [c for c in (0, 3, 63, 64, 65, 128) if c != y[r]]
        x[r, cls[:r + 1]] = -np.inf
    out["neg_inf"] = (x, y)
    return out


# ---- KL rows -------------------------------------------------------------------------------------
def kl_reference(a, b):
    """Per-row float64 sum_c n_c log(n_c / o_c) on the fp32 probabilities (n = a, o = b), with the bound
    of an fp32 evaluation: the rounded quotient passes through the log as at most u per term
    (taken twice: the device log's own error near 1), the log and the product are rounded relative
    to |log|, and a 64-lane sum of the terms carries (cols / 64 + 8) u relative to sum |term|.
    IEEE throughout: o_c = 0 < n_c gives +inf, n_c = 0 gives NaN (0 * log 0), as the reference's
    own loop does."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    cols = a.shape[1]
    with np.errstate(all="ignore"):
        lg = np.log(a / b)
        t = a * lg
        kl = t.sum(axis=1)
        bound = (a * (2 * U + 4 * U * np.abs(lg))).sum(axis=1) + (cols / 64 + 8) * U * np.abs(t).sum(axis=1)
    return {"kl": kl, "bound": bound, "rows": a.shape[0]}


def check_kl_rows(row_ws, ref):
    """row_ws fp32 [rows] against kl_reference: finite rows within the bound, +inf and NaN rows as
    such; returns the largest error / bound over the finite rows."""
    row_ws = np.asarray(row_ws)
    assert row_ws.dtype == np.float32 and row_ws.shape == (ref["rows"],), (row_ws.dtype, row_ws.shape)
    got, kl = row_ws.astype(np.float64), ref["kl"]
    fin = np.isfinite(kl)
    assert np.array_equal(np.isnan(got), np.isnan(kl)), "NaN rows differ"
    assert np.array_equal(got[~fin & ~np.isnan(kl)], kl[~fin & ~np.isnan(kl)]), "infinite rows differ"
    assert np.isfinite(got[fin]).all()
    err = np.abs(got[fin] - kl[fin])
    bad = err > ref["bound"][fin]
    if bad.any():
        i = int(np.argmax(err - ref["bound"][fin]))
        raise AssertionError("KL: %d of %d rows off, worst (finite row %d): %r, reference %r, bound %.3e" % (
            bad.sum(), bad.size, i, got[fin][i], kl[fin][i], ref["bound"][fin][i]))
    return _ratio(err, ref["bound"][fin])


def check_kl_stats(before, after, row_ws, ref):
    """stats double [2]: [1] moves by exactly rows; [0] by the float64 sum of the device's own rows
    (a fixed-order double sum: within 2e-15 of the largest magnitude involved) and by the reference
    sum within the sum of the per-row bounds."""
    before, after = np.asarray(before, np.float64), np.asarray(after, np.float64)
    assert after[1] - before[1] == float(ref["rows"]), (before, after)
    rows = np.asarray(row_ws).astype(np.float64)
    if not np.isfinite(ref["kl"]).all():
        want = ref["kl"].sum()
        assert np.isnan(after[0]) if np.isnan(want) else after[0] == want, (after[0], want)
        return
    tol = SUM_RTOL * max(abs(after[0]), abs(before[0]), np.abs(rows).sum())
    assert abs((after[0] - before[0]) - rows.sum()) <= tol, (after[0] - before[0], rows.sum(), tol)
    assert abs((after[0] - before[0]) - ref["kl"].sum()) <= ref["bound"].sum() + tol


def kl_emulate(a, b):
    """fp32 numpy emulation of a correct kernel: the rows' sums."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(all="ignore"):
        t = a * np.log(a / b)
        assert t.dtype == np.float32
        return t.sum(axis=1, dtype=np.float32)


KL_SHAPES = [(r, c) for r in (1, 5, 257) for c in (7, 64, 65, 1000)]
KL_NEAR = 1e-3  # the perturbation of the near-identical family


def _softmax32(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def kl_inputs(rows, cols, family):
    """fp32 probabilities (a, b): 'independent' softmaxes, or 'near': softmax(x) against
    softmax(x + 1e-3 noise), what the search compares between two neighbouring assignments."""
    g = np.random.default_rng(9000 + 1000 * rows + cols)
    x = g.standard_normal((rows, cols)) * 2
    z = g.standard_normal((rows, cols))
    return _softmax32(x), _softmax32(z * 2 if family == "independent" else x + KL_NEAR * z)


# ---- fingerprints --------------------------------------------------------------------------------
def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def fingerprint_scalar(words):
    """sum_i H(w_i, i) mod 2^64 of a list of 32-bit words in plain Python integers (include/smpq.h)."""
    return sum(fmix32(x ^ ((i * 0x9E3779B9) & M32)) | (fmix32(x ^ ((i * 0x85EBCA6B + 0xC2B2AE35) & M32)) << 32)
               for i, x in enumerate(words)) % (1 << 64)


def _fmix32_np(h):
    h = h ^ (h >> np.uint32(16))
    h = h * np.uint32(0x85EBCA6B)
    h = h ^ (h >> np.uint32(13))
    h = h * np.uint32(0xC2B2AE35)
    return h ^ (h >> np.uint32(16))


def fingerprint_reference(buf, offset=0, nbytes=None, mask_tail=True, index_base=0):
    """The fingerprint of bytes [offset, offset + nbytes) of the uint8 array buf, vectorised in numpy
    uint32 / uint64 (wrapping arithmetic): ceil(nbytes / 4) little-endian words, the last one
    zero-padded. mask_tail=False takes the last word's missing bytes from the buffer instead and
    index_base=1 numbers the words from 1: the two wrong references test_tail_ref_host.py rejects."""
    buf = np.asarray(buf)
    assert buf.dtype == np.uint8 and buf.ndim == 1
    nbytes = buf.size - offset if nbytes is None else nbytes
    n = (nbytes + 3) // 4
    raw = np.zeros(4 * n, np.uint8)
    take = min(4 * n, buf.size - offset) if not mask_tail else nbytes
    raw[:take] = buf[offset:offset + take]
    w = raw.view("<u4").astype(np.uint32)
    i = np.arange(index_base, index_base + n, dtype=np.uint64).astype(np.uint32)
    lo = _fmix32_np(w ^ (i * np.uint32(0x9E3779B9)))
    hi = _fmix32_np(w ^ (i * np.uint32(0x85EBCA6B) + np.uint32(0xC2B2AE35)))
    h = lo.astype(np.uint64) | (hi.astype(np.uint64) << np.uint64(32))
    return int(h.sum(dtype=np.uint64))


CHUNK_WORDS = 16384  # smpq_fingerprint_chunk_words(): asserted by the GPU test
FP_GAP = 32          # bytes between two tensors of the arena (the outside-byte flips live there)


def fingerprint_layout():
    """The tensors of the fingerprint tests as slices of one byte arena: [(dtype name, offset, nbytes)]
    and the arena's size. fp32 tensors of 1, 3, 16383, 16384, 16385, 16388 and 2 * 16384 + 3 words,
    uint8 tensors of every nbytes % 4 below and above one chunk, an int16 tensor of 7 elements, and
    fp32 views whose address is 4, 8 or 12 past a 16-B boundary (below and above one chunk)."""
    spec = [("float32", 4 * w, 0) for w in (1, 3, CHUNK_WORDS - 1, CHUNK_WORDS, CHUNK_WORDS + 1, CHUNK_WORDS + 4,
                                            2 * CHUNK_WORDS + 3)]
    spec += [("uint8", nb, 0) for nb in (1, 2, 3, 5, 65537, 65539)]
    spec += [("int16", 14, 0)]
    spec += [("float32", 4 * w, mis) for w in (1000, CHUNK_WORDS + 8) for mis in (1, 2, 3)]
    out, cursor = [], 0
    for dtype, nb, mis in spec:
        off = (cursor + FP_GAP + 15) // 16 * 16 + 4 * mis
        out.append((dtype, off, nb))
        cursor = off + nb
    return out, (cursor + FP_GAP + 15) // 16 * 16


def fingerprint_arena():
    layout, size = fingerprint_layout()
    return layout, np.random.default_rng(4).integers(0, 256, size, dtype=np.uint8)


def outside_bytes(layout):
    """Arena offsets next to the tensors that belong to none of them: the byte before each tensor, the
    1-3 bytes that complete its last word, and the byte after those."""
    out = []
    for _, off, nb in layout:
        end = off + (nb + 3) // 4 * 4
        out += [off - 1] + list(range(off + nb, end + 1))
    return out


def inside_flips(layout):
    """{name: [(tensor index, arena offset, xor mask)]}: each of the last three bytes inside a tensor,
    and bit 0 of words 0, 16383 and 16384 (the last word of the first chunk, the first of the second)."""
    out = {}
    for t, (_, off, nb) in enumerate(layout):
        for back in (1, 2, 3):
            if nb >= back:
                out.setdefault("last_byte_%d" % back, []).append((t, off + nb - back, 0xFF))
        for word in (0, CHUNK_WORDS - 1, CHUNK_WORDS):
            if 4 * word < nb:
                out.setdefault("word_%d_bit0" % word, []).append((t, off + 4 * word, 0x01))
    return out


# ---- quantizer -----------------------------------------------------------------------------------
QUANT_K = (2, 63, 64, 65, 255, 256, 257, 4608, 4609)  # around one wave, one 256-thread pass, the largest R50 channel


def quant_layer(k):
    """(w fp32 [80, k], bits [80] cycling 1..8 and 0 (skip))."""
    g = np.random.default_rng(300 + k)
    w = (g.standard_normal((80, k)) * 0.05).astype(np.float32)
    bits = (np.arange(80) % 9 + 1) % 9
    return w, bits.astype(np.int8)


CONSTANT_CHANNELS = (299, 150, 3)


def constant_channel_layer():
    """(w fp32 [300, 64] with three constant channels, bits [300] (all 8), what a quantizer that skips
    the constant channels leaves: the oracle's "cpu" result for every other channel)."""
    from oracle import quant_ref
    g = np.random.default_rng(33)
    w = (g.standard_normal((300, 64)) * 0.05).astype(np.float32)
    for c in CONSTANT_CHANNELS:
        w[c] = np.float32(0.25 + c / 1024)
    expect = w.copy()
    for c in range(300):
        if c not in CONSTANT_CHANNELS:
            expect[c] = quant_ref.quantize_wgt(w[c], 8)
    return w, np.full(300, 8, np.int8), expect
