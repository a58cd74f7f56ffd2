"""The references, bounds and checkers of tests/tail_ref.py, without a GPU: each checker accepts an
fp32 numpy emulation of a correct kernel on the inputs the GPU tests use and rejects every wrong
kernel it is there to catch; the float64 references satisfy their own bounds (a bound the reference
misses, or one nothing can miss, shows here); the fingerprint reference equals the plain-integer
formula and the host twin; and the host quantizer equals the oracle bit for bit on the layers of the
GPU parity test."""
import numpy as np
import pytest
import torch

import tail_ref as tr
from oracle import eval_ref, quant_ref


def _rejects(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


# ---- avgpool + fc --------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(tr.FC_CASES)))
def test_fc_checker_accepts_fp32_and_rejects_wrong_kernels(i):
    n, hw, c, nout = tr.FC_CASES[i]
    x, w, b = tr.fc_inputs(i)
    ref = tr.fc_reference(x, w, b)
    # the reference itself, rounded to fp32 once: inside every bound, and the bounds are not vacuous
    rp, ry = tr.check_fc(ref["pooled"].astype(np.float32), ref["y"].astype(np.float32), ref)
    assert rp <= 1.0 / (hw + 1) + 1e-9 and ry <= 1.0 / (hw + c + 2) + 1e-9
    assert (ref["y_bound"] > 0).all() and (ref["y_bound"] < 0.02 * np.abs(ref["y"]).max()).all()
    pooled, y = tr.fc_emulate(x, w, b)
    rp, ry = tr.check_fc(pooled, y, ref)
    assert ry < 0.25, ry  # rounding errors do not line up: a correct kernel is far inside
    tr.check_fc(*tr.fc_emulate(x, w, None), tr.fc_reference(x, w, None))
    _rejects(tr.check_fc, *tr.fc_emulate(x, w, b, drop_k=1), ref)
    _rejects(tr.check_fc, *tr.fc_emulate(x, w, b, drop_pixel=1), ref)
    _rejects(tr.check_fc, *tr.fc_emulate(x, w, b, divisor_extra=1), ref)
    _rejects(tr.check_fc, *tr.fc_emulate(x, w, b, bias_times=2), ref)
    _rejects(tr.check_fc, pooled, tr.fc_emulate(x, w, None)[1], ref)  # the bias left out
    if n > 1:
        swapped = y.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        _rejects(tr.check_fc, pooled, swapped, ref)
    _rejects(tr.check_fc, pooled.astype(np.float64), y, ref)
    _rejects(tr.check_fc, pooled, y[:, :-1] if nout > 1 else y[:-1], ref)


def test_fc_cases_cover_the_kernel_boundaries():
    cases = tr.FC_CASES
    quarter = lambda c: ((c + 3) // 4 + 31) // 32 * 32  # noqa: E731  (fc_kernel's K-quarter width)
    assert any(quarter(c) * 3 >= c for _, _, c, _ in cases)             # an empty last quarter
    assert any(0 < c - 3 * quarter(c) < quarter(c) for _, _, c, _ in cases)  # a partial one
    steps = {quarter(c) // 32 for _, _, c, _ in cases}
    assert 1 in steps and any(s > 1 and s % 2 for s in steps) and any(s % 2 == 0 for s in steps)
    assert {1, 8, 9, 10} <= {hw for _, hw, _, _ in cases}
    assert {7, 8, 9} <= {n for n, _, _, _ in cases} and {63, 64, 65} <= {o for _, _, _, o in cases}
    signed = [bool((tr.fc_inputs(i)[0] < 0).any()) for i in range(len(cases))]
    assert sum(signed) * 2 == len(cases)


# ---- softmax / cross entropy ---------------------------------------------------------------------
def _softmax_cases():
    cases = {"%dx%d" % s: tr.softmax_inputs(*s) for s in tr.SOFTMAX_SHAPES}
    cases["ties"] = tr.tie_inputs()
    cases.update(tr.range_inputs())
    return cases


def test_softmax_reference_agrees_with_the_oracle_and_its_own_bounds():
    for name, (x, y) in _softmax_cases().items():
        ref = tr.softmax_reference(x, y)
        acc, loss, outs = eval_ref.evaluate_acc_loss_softmax([(x, y)])
        assert acc == ref["correct"].mean() and abs(loss - ref["loss"].mean()) <= 1e-12 * abs(loss), name
        assert np.array_equal(outs[0], ref["probs"]), name
        ws = np.concatenate([ref["loss"], ref["correct"]]).astype(np.float32)
        r = tr.check_softmax_rows(ws, ref["probs"].astype(np.float32), ref)
        assert r <= 0.5, (name, r)  # one rounding of the loss: u / 2 relative, far inside
        assert np.isfinite(ref["bound"]).all() and (ref["bound"] <= 3e-6 * np.maximum(np.abs(ref["loss"]), 200.0)).all()


def test_softmax_checker_accepts_fp32_and_rejects_wrong_kernels():
    for name, (x, y) in _softmax_cases().items():
        ref = tr.softmax_reference(x, y)
        ws, probs = tr.softmax_emulate(x, y)
        assert tr.check_softmax_rows(ws, probs, ref) < 1.0, name
        before = np.array([0.5, 7.0, 11.0, 2.0])
        after = before + [ws[:len(y)].astype(np.float64).mean(), ref["correct"].sum(), len(y), 1]
        tr.check_softmax_stats(before, after, ws, ref)
        _rejects(tr.check_softmax_stats, before, after + [1e-5, 0, 0, 0], ws, ref)
        _rejects(tr.check_softmax_stats, before, after + [0, 1, 0, 0], ws, ref)
        if x.shape[1] > 1 and name != "underflow":  # (there the sum of the exponentials is exactly 1)
            _rejects(tr.check_softmax_rows, ws, tr.softmax_emulate(x, y, unnormalised=True)[1], ref)
    x, y = tr.tie_inputs()
    ref = tr.softmax_reference(x, y)
    # the first maximal class: label on the lower duplicate is correct, on the higher one is not
    assert ref["correct"].tolist() == [True, False, False] * (len(tr.TIE_PAIRS) + 1)
    _rejects(tr.check_softmax_rows, tr.softmax_emulate(x, y, last_max=True)[0], None, ref)
    for name in ("plus1000", "minus300"):
        x, y = tr.range_inputs()[name]
        _rejects(tr.check_softmax_rows, tr.softmax_emulate(x, y, no_max_term=True)[0], None, tr.softmax_reference(x, y))
    x, y = tr.range_inputs()["underflow"]
    ref = tr.softmax_reference(x, y)
    assert (np.sort(ref["probs"].astype(np.float32), axis=1)[:, :-1] == 0).all() and np.isfinite(ref["loss"]).all()
    assert (ref["loss"][:3] < 1e-80).all() and (ref["loss"][3:] > 200).all()


def test_softmax_checker_label_out_of_range():
    x, y = tr.softmax_inputs(5, 65)
    y[1], y[3] = -1, 65
    ref = tr.softmax_reference(x, y)
    ws, probs = tr.softmax_emulate(x, y)
    tr.check_softmax_rows(ws, probs, ref)
    good = tr.softmax_emulate(x, np.where(ref["valid"], y, 0))[0]
    _rejects(tr.check_softmax_rows, good, None, ref)  # a finite loss for a bad label
    before = np.array([0.5, 7.0, 11.0, 2.0])
    tr.check_softmax_stats(before, before + [np.nan, ref["correct"].sum(), 5, 1], ws, ref)
    _rejects(tr.check_softmax_stats, before, before + [1.0, ref["correct"].sum(), 5, 1], ws, ref)


# ---- KL rows -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", tr.KL_SHAPES)
def test_kl_checker_accepts_fp32_and_rejects_swapped_arguments(rows, cols):
    for family in ("independent", "near"):
        a, b = tr.kl_inputs(rows, cols, family)
        ref = tr.kl_reference(a, b)
        assert abs(ref["kl"].mean() - eval_ref.kldiv([a], [b])) <= 1e-12 * abs(ref["kl"].mean())
        assert tr.check_kl_rows(ref["kl"].astype(np.float32), ref) <= 0.5  # one rounding of the result
        ws = tr.kl_emulate(a, b)
        assert tr.check_kl_rows(ws, ref) < 1.0, family
        before = np.array([0.25, 3.0])
        after = before + [ws.astype(np.float64).sum(), rows]
        tr.check_kl_stats(before, after, ws, ref)
        _rejects(tr.check_kl_stats, before, after + [0.0, 1.0], ws, ref)
        _rejects(tr.check_kl_stats, before, after + [1e-4 * rows, 0.0], ws, ref)
        if family == "independent":
            _rejects(tr.check_kl_rows, tr.kl_emulate(b, a), ref)
        else:
            # the near family is the search's noise floor: KL ~ 1e-6 / 2 * Var(noise), and the bound is
            # absolute (a few u), a visible fraction of it
            assert 1e-8 < ref["kl"].mean() < 5e-6 and (ref["bound"] < 12 * tr.U + 1e-4 * ref["kl"] + 1e-9).all()
    a, _ = tr.kl_inputs(rows, cols, "near")
    assert (tr.kl_emulate(a, a) == 0).all() and (tr.kl_reference(a, a)["kl"] == 0).all()


def test_kl_checker_inf_and_nan_rows():
    a, b = tr.kl_inputs(5, 65, "independent")
    b[1, 7] = 0.0   # o = 0 < n: +inf
    a[3, 9] = 0.0   # n = 0: NaN (0 * log 0), whatever o is
    ref = tr.kl_reference(a, b)
    assert ref["kl"][1] == np.inf and np.isnan(ref["kl"][3]) and np.isfinite(ref["kl"][[0, 2, 4]]).all()
    ws = tr.kl_emulate(a, b)
    tr.check_kl_rows(ws, ref)
    for row, v in ((1, 1.0), (3, 1.0), (1, np.nan), (3, np.inf)):
        bad = ws.copy()
        bad[row] = v
        _rejects(tr.check_kl_rows, bad, ref)


# ---- fingerprints --------------------------------------------------------------------------------
def test_fingerprint_reference_formula_and_wrong_references(built_lib):
    from smpq.fingerprint import host_fingerprint
    layout, arena = tr.fingerprint_arena()
    assert len({off % 16 for _, off, _ in layout}) == 4 and {nb % 4 for _, _, nb in layout} == {0, 1, 2, 3}
    want = [tr.fingerprint_reference(arena, off, nb) for _, off, nb in layout]
    host = [host_fingerprint(torch.from_numpy(arena[off:off + nb].copy())) for _, off, nb in layout]
    assert want == host
    for (_, off, nb), fp in list(zip(layout, want))[:2] + list(zip(layout, want))[7:11] + [(layout[13], want[13])]:
        raw = np.zeros((nb + 3) // 4 * 4, np.uint8)
        raw[:nb] = arena[off:off + nb]
        assert fp == tr.fingerprint_scalar(raw.view("<u4").tolist())
    unmasked = [tr.fingerprint_reference(arena, off, nb, mask_tail=False) for _, off, nb in layout]
    from_one = [tr.fingerprint_reference(arena, off, nb, index_base=1) for _, off, nb in layout]
    for (_, off, nb), w, u, f in zip(layout, want, unmasked, from_one):
        assert (u != w) == (nb % 4 != 0), (off, nb)  # the bytes after a partial last word must not count
        assert f != w
    with pytest.raises(AssertionError):
        assert unmasked == want
    with pytest.raises(AssertionError):
        assert from_one == want
    # the flips of the GPU test stay outside / inside the tensors they name
    inside = np.zeros(arena.size, bool)
    for _, off, nb in layout:
        assert not inside[off - tr.FP_GAP // 2:off + nb + tr.FP_GAP // 2].any()
        inside[off:off + nb] = True
    outside = tr.outside_bytes(layout)
    assert not inside[outside].any() and len(set(outside)) == len(outside)
    for flips in tr.inside_flips(layout).values():
        for t, at, mask in flips:
            assert layout[t][1] <= at < layout[t][1] + layout[t][2]


# ---- host quantizer ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", tr.QUANT_K)
def test_host_quantizer_layer_equals_oracle(built_lib, k):
    from smpq import ops
    w, bits = tr.quant_layer(k)
    got = torch.from_numpy(w.copy())
    step = ops.quantize_channels_(got, torch.from_numpy(bits), semantics="cpu")
    want = w.copy()
    for c in range(w.shape[0]):
        if bits[c]:
            want[c] = quant_ref.quantize_wgt(w[c], int(bits[c]))
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))
    assert (step.numpy()[bits == 0] == 0).all() and (step.numpy()[bits > 0] > 0).all()


def test_host_quantizer_stops_at_the_lowest_constant_channel(built_lib):
    from smpq import ops
    w, bits, expect = tr.constant_channel_layer()
    got = torch.from_numpy(w.copy())
    with pytest.raises(ZeroDivisionError, match=r"constant channel 3\)"):
        ops.quantize_channels_(got, torch.from_numpy(bits), semantics="cpu")
    # channels before it quantized, that one and every later one untouched (the reference's loop)
    assert np.array_equal(got.numpy()[:3].view(np.uint32), expect[:3].view(np.uint32))
    assert np.array_equal(got.numpy()[3:].view(np.uint32), w[3:].view(np.uint32))
