"""smpq.sensitivity on the host: the trial row patch's native twin against the quantizer's host twin
followed by a NumPy restatement of the lw >= 2 packing rule (include/smpq.h), argument validation,
the delta-loss CSV layout, and the sweep's bookkeeping on injected forwards (no GPU needed)."""
import csv
import math

import numpy as np
import pytest
import torch

WMAX = {2: 32512.0, 3: 8323072.0}


def pack_row_ref(v, s, lw, cin, taps):
    """include/smpq.h "trial row patch" steps 3-4 for one quantized row ``v`` (fp32 [cin*taps], the
    weight's own [cin][taps] order) with step ``s``: (digits int8 [lw, K] in k = tap*cin + ci order,
    wscale fp32)."""
    v = np.asarray(v, dtype=np.float32)
    s = np.float32(s)
    wmax = np.float32(WMAX[lw])
    on = bool(s > 0)
    if on:
        with np.errstate(all="ignore"):
            mf = np.rint(v / s).astype(np.float32)
            on = bool(np.all((mf * s).astype(np.float32) == v) and np.all(np.abs(mf) <= wmax))
    if on:
        m = mf.astype(np.int64)
        am, sh = int(np.abs(m).max()), 0
        while am > 0 and sh < 8 * (lw - 1) and (am << (sh + 1)) <= int(wmax):
            sh += 1
        m = m << sh
        wscale = np.float32(np.ldexp(s, -sh))
    else:
        amax = np.float32(np.abs(v).max())
        wscale = np.float32(amax / wmax) if amax > 0 else np.float32(1.0)
        m = np.clip(np.rint(v.astype(np.float64) / np.float64(wscale)), -float(wmax), float(wmax)).astype(np.int64)
    m = m.reshape(cin, taps).T.reshape(-1)  # k = tap * cin + ci
    digits = np.zeros((lw, m.size), dtype=np.int8)
    for l in range(lw):
        lo = m if l == lw - 1 else ((m + 128) & 255) - 128
        digits[l] = lo.astype(np.int8)
        m = (m - lo) >> 8
    return digits, wscale, on


def make_operand(cout, K, lw, seed):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(-128, 128, (lw, cout, K), dtype=torch.int8, generator=g)
    wscale = torch.rand(cout, generator=g) + 0.5
    a = torch.rand(cout, generator=g) + 0.5
    col_scale = (wscale * a).contiguous()
    return codes, wscale, a, col_scale


def expected_patch(built_lib, w, c, bit, sem, lw, codes, wscale, a, col_scale):
    from smpq import _lib, ops
    cout, cin, kh, kw = w.shape
    K = cin * kh * kw
    w2 = w.clone().reshape(cout, K)
    bits = torch.zeros(cout, dtype=torch.int8)
    bits[c] = bit
    step = torch.zeros(cout, dtype=torch.float32)
    rc = built_lib.smpq_quantize_channels_host_ex(_lib.ptr(w2), cout, K, _lib.ptr(bits), _lib.ptr(step), ops.QSEM[sem])
    assert rc == 0
    digits, sc, on = pack_row_ref(w2[c].numpy(), step[c].item(), lw, cin, kh * kw)
    e_codes, e_ws, e_cs = codes.clone(), wscale.clone(), col_scale.clone()
    e_codes[:, c] = torch.from_numpy(digits)
    e_ws[c] = float(sc)
    e_cs[c] = float(np.float32(sc) * np.float32(a[c].item()))
    return e_codes, e_ws, e_cs, on


@pytest.mark.parametrize("shape", [(64, 64, 1, 1), (64, 64, 3, 3)])
@pytest.mark.parametrize("lw", [2, 3])
def test_host_patch_and_restore(built_lib, shape, lw):
    from smpq import ops
    cout, cin, kh, kw = shape
    K = cin * kh * kw
    w = torch.randn(*shape, generator=torch.Generator().manual_seed(11)) * 0.05
    w0 = w.clone()
    on_grid = 0
    for bit in (8, 6, 4, 2, 16):
        for sem in ("cpu", "device"):
            for c in (0, cout - 1):
                codes, wscale, a, col_scale = make_operand(cout, K, lw, seed=bit * 7 + c)
                c0, s0, cs0 = codes.clone(), wscale.clone(), col_scale.clone()
                save = torch.full((ops.trial_save_bytes(lw, K) + 32,), 0x5A, dtype=torch.int8)
                status = torch.zeros(1, dtype=torch.int32)
                e_codes, e_ws, e_cs, on = expected_patch(built_lib, w, c, bit, sem, lw, codes, wscale, a, col_scale)
                on_grid += on
                ops.trial_row_patch(w, c, bit, a, codes, wscale, col_scale, save[:-32], status, semantics=sem)
                assert int(status) == 0
                assert torch.equal(w, w0)  # the weight is only read
                assert torch.equal(codes, e_codes), (bit, sem, c)
                assert torch.equal(wscale.view(torch.int32), e_ws.view(torch.int32)), (bit, sem, c)
                assert torch.equal(col_scale.view(torch.int32), e_cs.view(torch.int32)), (bit, sem, c)
                assert not torch.equal(codes[:, c], c0[:, c])
                assert (save[-32:] == 0x5A).all()  # nothing past the save area
                ops.trial_row_restore(c, codes, wscale, col_scale, save[:-32])
                assert torch.equal(codes, c0) and torch.equal(wscale.view(torch.int32), s0.view(torch.int32))
                assert torch.equal(col_scale.view(torch.int32), cs0.view(torch.int32))
    assert on_grid >= 12  # the exact-code branch ran (16 bits at lw 2 is the fixed-point one)


def test_host_patch_off_grid_row_falls_back_to_fixed_point(built_lib):
    # a row far from zero with a tiny range: its codes exceed WMAX, so it is coded in fixed point
    from smpq import ops
    cout, cin = 64, 64
    w = torch.randn(cout, cin, 1, 1, generator=torch.Generator().manual_seed(3)) * 0.05
    w[5] = 1000.0 + torch.rand(cin, 1, 1, generator=torch.Generator().manual_seed(4)) * 1e-3
    for lw in (2, 3):
        codes, wscale, a, col_scale = make_operand(cout, cin, lw, seed=lw)
        save = torch.zeros(ops.trial_save_bytes(lw, cin), dtype=torch.int8)
        status = torch.zeros(1, dtype=torch.int32)
        e_codes, e_ws, e_cs, on = expected_patch(built_lib, w, 5, 8, "cpu", lw, codes, wscale, a, col_scale)
        assert not on
        ops.trial_row_patch(w, 5, 8, a, codes, wscale, col_scale, save, status, semantics="cpu")
        assert torch.equal(codes, e_codes) and torch.equal(wscale, e_ws) and torch.equal(col_scale, e_cs)


def test_host_patch_constant_row(built_lib):
    from smpq import ops
    w = torch.randn(64, 64, 1, 1, generator=torch.Generator().manual_seed(5))
    w[7] = 0.25
    codes, wscale, a, col_scale = make_operand(64, 64, 2, seed=1)
    c0, s0, cs0 = codes.clone(), wscale.clone(), col_scale.clone()
    save = torch.zeros(ops.trial_save_bytes(2, 64), dtype=torch.int8)
    status = torch.zeros(1, dtype=torch.int32)
    ops.trial_row_patch(w, 7, 4, a, codes, wscale, col_scale, save, status)
    assert int(status) == 1
    assert torch.equal(codes, c0) and torch.equal(wscale, s0) and torch.equal(col_scale, cs0)
    ops.trial_row_restore(7, codes, wscale, col_scale, save)  # the save area holds the row: harmless
    assert torch.equal(codes, c0) and torch.equal(wscale, s0) and torch.equal(col_scale, cs0)


def test_argument_validation(built_lib):
    """Every check returns its code before anything is launched or written (the device entry point
    is called with bad arguments only, so it never reaches a launch)."""
    from smpq import _lib
    w = torch.randn(64, 64, 1, 1)
    codes, wscale, a, col_scale = make_operand(64, 64, 2, seed=2)
    save = torch.zeros(16 + 3 * 64, dtype=torch.int8)
    status = torch.zeros(1, dtype=torch.int32)
    c0 = codes.clone()
    P = _lib.ptr

    def host(w_=w, cout=64, cin=64, ch=0, bits=4, sem=0, lw=2, a_=a, codes_=codes, ws=wscale, cs=col_scale, sv=save,
             st=status):
        return built_lib.smpq_trial_row_patch_host(P(w_), cout, cin, 1, 1, ch, bits, sem, lw, P(a_), P(codes_), P(ws),
                                                   P(cs), P(sv), P(st))

    def dev(w_=w, cout=64, cin=64, ch=0, bits=4, sem=0, lw=2, a_=a, codes_=codes, ws=wscale, cs=col_scale, sv=save,
            st=status):
        return built_lib.smpq_trial_row_patch(P(w_), cout, cin, 1, 1, ch, bits, sem, lw, P(a_), P(codes_), None, P(ws),
                                              P(cs), P(sv), P(st), None)

    for f in (host, dev):
        for name in ("w_", "a_", "codes_", "ws", "cs", "sv", "st"):
            assert f(**{name: None}) == _lib.SMPQ_E_INVALID, name
        assert f(lw=1) == _lib.SMPQ_E_INVALID and f(lw=4) == _lib.SMPQ_E_INVALID
        assert f(ch=-1) == _lib.SMPQ_E_INVALID and f(ch=64) == _lib.SMPQ_E_INVALID
        assert f(sem=2) == _lib.SMPQ_E_INVALID
        assert f(cin=32) == _lib.SMPQ_E_SHAPE
        assert f(cin=4672) == _lib.SMPQ_E_SHAPE  # K above SMPQ_TRIAL_MAX_K
        assert f(bits=0) == _lib.SMPQ_E_BITS and f(bits=17) == _lib.SMPQ_E_BITS
        assert "smpq_trial_row_patch" in _lib.last_error()
    r = built_lib.smpq_trial_row_restore_host
    assert r(64, 64, 0, 2, None, P(wscale), P(col_scale), P(save)) == _lib.SMPQ_E_INVALID
    assert r(64, 64, 64, 2, P(codes), P(wscale), P(col_scale), P(save)) == _lib.SMPQ_E_INVALID
    assert r(64, 64, 0, 1, P(codes), P(wscale), P(col_scale), P(save)) == _lib.SMPQ_E_INVALID
    assert r(64, 32, 0, 2, P(codes), P(wscale), P(col_scale), P(save)) == _lib.SMPQ_E_SHAPE
    d = built_lib.smpq_trial_row_restore
    assert d(64, 64, 0, 2, P(codes), None, P(wscale), P(col_scale), None, None) == _lib.SMPQ_E_INVALID
    assert d(64, 32, 0, 2, P(codes), None, P(wscale), P(col_scale), P(save), None) == _lib.SMPQ_E_SHAPE
    assert torch.equal(codes, c0) and int(status) == 0
    assert host() == 0  # (and the good call passes)


def test_ops_wrappers_validate_shapes(built_lib):
    from smpq import ops
    w = torch.randn(64, 64, 1, 1)
    codes, wscale, a, col_scale = make_operand(64, 64, 2, seed=2)
    save = torch.zeros(ops.trial_save_bytes(2, 64), dtype=torch.int8)
    status = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.trial_row_patch(w, 64, 4, a, codes, wscale, col_scale, save, status)
    with pytest.raises(ValueError):
        ops.trial_row_patch(w, 0, 4, a, codes, wscale, col_scale, save[:-1], status)
    with pytest.raises(ValueError):
        ops.trial_row_patch(w, 0, 4, a, codes[:1].contiguous(), wscale, col_scale, save, status)
    with pytest.raises(ValueError):
        ops.trial_row_patch(w[:, :32].contiguous(), 0, 4, a, codes, wscale, col_scale, save, status)
    with pytest.raises(ValueError):
        ops.trial_row_restore(0, codes, wscale[:-1], col_scale, save)


# ---- CSV ----------------------------------------------------------------------------------------
def _table(bits, n=7):
    from smpq.sensitivity import DeltaLossTable
    rng = np.random.default_rng(0)
    delta = {b: rng.standard_normal(n) * 10.0 ** rng.integers(-12, 3, n) for b in bits}
    delta[bits[0]][2] = math.nan
    delta[bits[-1]][3] = -0.0
    return DeltaLossTable("resnet18" if len(bits) == 4 else "resnet50", [1, 1, 1, 2, 2, 16, 16][:n],
                          [0, 1, 63, 0, 5, 7, 511][:n], bits, delta, 1.25)


@pytest.mark.parametrize("bits", [(8, 6, 4), (8, 6, 4, 2)])
def test_csv_round_trip_and_driver_loop(built_lib, tmp_path, bits):
    from smpq.sensitivity import read_csv, write_csv
    t = _table(bits)
    path = tmp_path / "deltaloss.csv"
    write_csv(t, path)
    back = read_csv(path)
    assert back.bits == bits and np.array_equal(back.lnum, t.lnum) and np.array_equal(back.cnum, t.cnum)
    for b in bits:
        assert np.array_equal(back.delta[b].view(np.uint64), t.delta[b].view(np.uint64))
    # the drivers' own reading loop (resnet18_main.py:61-84), restated
    with open(path, encoding="utf-8-sig") as f:
        rows = list(csv.reader(f))
    assert len(rows) == 2 + len(bits) == (5 if len(bits) == 3 else 6)
    assert all(len(r) == len(t.lnum) and all(cell != "" for cell in r) for r in rows)
    for num in range(len(rows[0])):
        assert int(rows[0][num]) == t.lnum[num]
        assert int(rows[1][num]) - 1 == t.cnum[num]
        for i, b in enumerate(bits):
            v = float(rows[2 + i][num])
            assert v == t.delta[b][num] or (math.isnan(v) and math.isnan(t.delta[b][num]))
    with open(path, "rb") as f:
        assert f.read(3) == b"\xef\xbb\xbf"


def test_read_csv_drops_empty_trailing_columns(built_lib, tmp_path):
    from smpq.sensitivity import read_csv
    path = tmp_path / "ref.csv"
    path.write_text("1,1,2,,\n1,2,1,,\n0.5,-0.25,1e-3,,\n0.1,0.2,0.3,,\n-1,-2,-3,,\n9,8,7,,\n", encoding="utf-8-sig")
    t = read_csv(path)
    assert t.bits == (8, 6, 4, 2) and t.lnum.tolist() == [1, 1, 2] and t.cnum.tolist() == [0, 1, 0]
    assert t.delta[2].tolist() == [9.0, 8.0, 7.0]


# ---- the sweep's bookkeeping on injected forwards --------------------------------------------------
class FakeConv:
    def __init__(self):
        self._content_gen = 0


class FakeHooks:
    """Forwards that return the patched trial's marker as the 'loss' and the flags it was told to."""

    def __init__(self, overflow=(), raise_at=None, constant=()):
        self.overflow, self.raise_at, self.constant = set(overflow), raise_at, set(constant)
        self.log, self.cur = [], None

    def patch(self, tr, status):
        self.cur = tr
        self.log.append(("patch", tr.channel, tr.bit))
        if (tr.channel, tr.bit) in self.constant:
            status[0] = 1

    def restore(self, tr):
        self.log.append(("restore", tr.channel, tr.bit))
        self.cur = None

    def invalidate(self, tr):
        tr.conv._content_gen += 1

    def forward(self, x):
        key = (self.cur.channel, self.cur.bit)
        if key == self.raise_at:
            raise KeyboardInterrupt("stop")
        return x, torch.tensor([1 if key in self.overflow else 0, 0], dtype=torch.int32)

    def score(self, logits, y, row):
        row[0] += 100.0 * self.cur.channel + self.cur.bit
        row[3] += 1

    def slow(self, tr):
        self.log.append(("slow", tr.channel, tr.bit))
        return -1.0


def _trials(conv, channels=(0, 1, 2), bits=(8, 4)):
    from smpq.sensitivity import Trial
    return [Trial(i, 1, conv, c, b) for i, (c, b) in enumerate((c, b) for c in channels for b in bits)]


def _counts():
    return {"patched": 0, "overflowed": 0, "slow": {}, "constant": []}


def test_sweep_redoes_overflowed_trials_on_the_slow_path(built_lib):
    from smpq import sensitivity
    conv, other = FakeConv(), FakeConv()
    hooks = FakeHooks(overflow={(1, 4)}, constant={(2, 8)})
    got, counts = {}, _counts()
    batches = [(torch.zeros(1), torch.zeros(1)), (torch.zeros(1), torch.zeros(1))]
    groups = [(True, _trials(conv)), (False, _trials(other, channels=(9,), bits=(4,)))]
    sensitivity.sweep(groups, batches, hooks, "cpu", lambda tr, loss, slow, row: got.__setitem__((tr.conv, tr.channel, tr.bit), (loss, slow)), counts)
    assert counts["patched"] == 4 and counts["overflowed"] == 1
    assert counts["slow"] == {"overflow": 1, "not_patchable": 1}
    assert counts["constant"] == [(1, 2, 8)]
    assert got[(conv, 0, 8)] == (8.0, False) and got[(conv, 2, 4)] == (204.0, False)
    assert got[(conv, 1, 4)] == (-1.0, True) and got[(other, 9, 4)] == (-1.0, True)
    assert math.isnan(got[(conv, 2, 8)][0])
    # every patch is followed by its restore before the next patch; the slow trials come last
    fast = [e for e in hooks.log if e[0] != "slow"]
    assert [e[0] for e in fast] == ["patch", "restore"] * 6
    assert all(p[1:] == r[1:] for p, r in zip(fast[0::2], fast[1::2]))
    assert hooks.log[-2:] == [("slow", 1, 4), ("slow", 9, 4)] and conv._content_gen == 0


def test_sweep_restores_and_invalidates_on_an_exception(built_lib):
    from smpq import sensitivity
    conv = FakeConv()
    hooks = FakeHooks(raise_at=(1, 8))
    batches = [(torch.zeros(1), torch.zeros(1))]
    with pytest.raises(KeyboardInterrupt):
        sensitivity.sweep([(True, _trials(conv))], batches, hooks, "cpu", lambda *a: None, _counts())
    assert hooks.log[-2:] == [("patch", 1, 8), ("restore", 1, 8)]
    assert conv._content_gen == 1


def test_delta_loss_table_refuses_other_modes(built_lib):
    from smpq import engine, sensitivity
    import resnet
    net = resnet.resnet18().eval()
    with pytest.raises(ValueError):  # a model on the CPU
        sensitivity.delta_loss_table(net, [(torch.zeros(1, 3, 32, 32), torch.zeros(1, dtype=torch.long))])
    engine.set_range_mode("dynamic")
    try:
        with pytest.raises(ValueError):
            sensitivity.delta_loss_table(net, [])
    finally:
        engine.set_range_mode("static")
