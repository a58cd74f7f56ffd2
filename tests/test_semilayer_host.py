"""Semilayer trials on the host: the n-row patch's native twin against the single-row twin called once
per row (bitwise, save slots included), guard bytes, a constant row inside a list, every argument
check (through ops and through the raw C entry points, the device one included: it validates
before it launches), patchable_rows and semilayer_table's bookkeeping on injected hooks, and the
SMPQ_PATCHED_SEMILAYERS route of functions._make_semilayers on stubs (no GPU needed)."""
import math
import types

import numpy as np
import pytest
import torch

from test_sensitivity_host import make_operand

SHAPES = [(64, 64, 1, 1), (64, 64, 3, 3), (16, 512, 3, 3)]  # the last: K = 4608, the limit
GUARD = 32


def _weight(shape, seed=11):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.05


def _lists(cout, n=None):
    """Unsorted, with the first and the last channel; bits 8, 6, 4, 2 in turn."""
    ch = [cout - 1, 3, 0, cout // 2, 7, 5, cout - 2][:n]
    return ch, [(8, 6, 4, 2)[i % 4] for i in range(len(ch))]


def _guarded(nbytes, dtype=torch.int8, fill=0x5A):
    buf = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.int8)
    return buf, buf[GUARD:GUARD + nbytes].view(dtype)


def _guards_hold(buf, fill=0x5A):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())


@pytest.mark.parametrize("sem", ["cpu", "device"])
@pytest.mark.parametrize("lw", [2, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_host_rows_equal_single_rows(built_lib, shape, lw, sem):
    from smpq import ops
    cout, cin, kh, kw = shape
    K = cin * kh * kw
    w = _weight(shape)
    w0 = w.clone()
    ch, bits = _lists(cout)
    n = len(ch)
    slot = ops.trial_save_bytes(lw, K)
    assert ops.trial_rows_save_bytes(lw, K, n) == n * slot and slot % 16 == 0
    codes, wscale, a, col_scale = make_operand(cout, K, lw, seed=lw * 10 + kh)
    orig = [t.clone() for t in (codes, wscale, col_scale)]
    # the single-row twin, once per row, on a copy
    e_codes, e_ws, e_cs = [t.clone() for t in orig]
    e_slots = []
    for c, b in zip(ch, bits):
        sv = torch.zeros(slot, dtype=torch.int8)
        st = torch.zeros(1, dtype=torch.int32)
        ops.trial_row_patch(w, c, b, a, e_codes, e_ws, e_cs, sv, st, semantics=sem)
        assert int(st) == 0
        e_slots.append(sv)
    sbuf, save = _guarded(n * slot)
    tbuf, status = _guarded(4 * n, torch.int32)
    status.zero_()
    rows = ops.trial_rows_patch(w, ch, bits, a, codes, wscale, col_scale, save, status, semantics=sem)
    assert rows.n == n and rows.channels.tolist() == ch and rows.bits.tolist() == bits
    assert status.tolist() == [0] * n and torch.equal(w, w0)
    assert torch.equal(codes, e_codes)
    assert torch.equal(wscale.view(torch.int32), e_ws.view(torch.int32))
    assert torch.equal(col_scale.view(torch.int32), e_cs.view(torch.int32))
    assert not torch.equal(codes, orig[0])
    for i, sv in enumerate(e_slots):
        got = save[i * slot:(i + 1) * slot]
        # header bytes 8..15 are unused (never written): compare the two scalars and the codes
        assert torch.equal(got[:8], sv[:8]) and torch.equal(got[16:], sv[16:]), i
    assert _guards_hold(sbuf) and _guards_hold(tbuf)
    ops.trial_rows_restore(rows, codes, wscale, col_scale, save)
    for t, o in zip((codes, wscale, col_scale), orig):
        assert torch.equal(t.view(torch.int8), o.view(torch.int8))
    # ... and with the plain list again (uploaded and validated anew)
    ops.trial_rows_patch(w, ch, bits, a, codes, wscale, col_scale, save, status.zero_(), semantics=sem)
    ops.trial_rows_restore(ch, codes, wscale, col_scale, save)
    assert torch.equal(codes, orig[0]) and _guards_hold(sbuf) and _guards_hold(tbuf)


@pytest.mark.parametrize("n", [1, 64])
def test_host_rows_one_row_and_every_row(built_lib, n):
    """n = 1 and n = cout both work here: 'one channel stays free' is patchable_rows's rule."""
    from smpq import ops
    shape = (64, 64, 1, 1)
    w = _weight(shape, seed=3)
    ch = [63] if n == 1 else [int(c) for c in torch.randperm(64, generator=torch.Generator().manual_seed(1))]
    codes, wscale, a, col_scale = make_operand(64, 64, 2, seed=9)
    orig = [t.clone() for t in (codes, wscale, col_scale)]
    e = [t.clone() for t in orig]
    for c in ch:
        ops.trial_row_patch(w, c, 4, a, *e, torch.zeros(ops.trial_save_bytes(2, 64), dtype=torch.int8),
                            torch.zeros(1, dtype=torch.int32))
    sbuf, save = _guarded(ops.trial_rows_save_bytes(2, 64, n))
    status = torch.zeros(n, dtype=torch.int32)
    ops.trial_rows_patch(w, ch, 4, a, codes, wscale, col_scale, save, status)  # one bit-width for all
    for t, o in zip((codes, wscale, col_scale), e):
        assert torch.equal(t.view(torch.int8), o.view(torch.int8))
    ops.trial_rows_restore(ch, codes, wscale, col_scale, save)
    for t, o in zip((codes, wscale, col_scale), orig):
        assert torch.equal(t.view(torch.int8), o.view(torch.int8))
    assert _guards_hold(sbuf) and status.tolist() == [0] * n


def test_host_rows_constant_row_in_the_middle(built_lib):
    from smpq import ops
    w = _weight((64, 64, 1, 1), seed=5)
    w[7] = 0.25
    ch, bits = [3, 7, 60], [8, 4, 2]
    codes, wscale, a, col_scale = make_operand(64, 64, 3, seed=1)
    orig = [t.clone() for t in (codes, wscale, col_scale)]
    e = [t.clone() for t in orig]
    for c, b in ((3, 8), (60, 2)):
        ops.trial_row_patch(w, c, b, a, *e, torch.zeros(ops.trial_save_bytes(3, 64), dtype=torch.int8),
                            torch.zeros(1, dtype=torch.int32))
    save = torch.zeros(ops.trial_rows_save_bytes(3, 64, 3), dtype=torch.int8)
    status = torch.zeros(3, dtype=torch.int32)
    ops.trial_rows_patch(w, ch, bits, a, codes, wscale, col_scale, save, status)
    assert status.tolist() == [0, 1, 0]
    assert torch.equal(codes[:, 7], orig[0][:, 7]) and wscale[7] == orig[1][7] and col_scale[7] == orig[2][7]
    for t, o in zip((codes, wscale, col_scale), e):  # the other rows are patched regardless
        assert torch.equal(t.view(torch.int8), o.view(torch.int8))
    ops.trial_rows_restore(ch, codes, wscale, col_scale, save)  # the constant row's slot holds the row: harmless
    for t, o in zip((codes, wscale, col_scale), orig):
        assert torch.equal(t.view(torch.int8), o.view(torch.int8))


def test_ops_rows_argument_checks(built_lib):
    from smpq import ops
    w = _weight((64, 64, 1, 1))
    codes, wscale, a, col_scale = make_operand(64, 64, 2, seed=2)
    c0 = codes.clone()
    save = torch.zeros(ops.trial_rows_save_bytes(2, 64, 3) + 4, dtype=torch.int8)
    status = torch.zeros(3, dtype=torch.int32)

    def patch(ch=(0, 1, 2), bits=4, sv=save[:-4], st=status, w_=w, codes_=codes, ws=wscale):
        ops.trial_rows_patch(w_, ch, bits, a, codes_, ws, col_scale, sv, st)

    for bad in (dict(ch=(0, 1, 1)), dict(ch=(0, 64, 1)), dict(ch=(0, -1, 1)), dict(bits=0), dict(bits=17),
                dict(bits=(4, 4, 17)), dict(bits=(4, 4)), dict(ch=()), dict(ch=tuple(range(64)) + (0,)),
                dict(sv=save[:-5]),                      # one byte short
                dict(sv=save[1:-3]),                     # misaligned
                dict(st=status[:2]),                     # a status word short
                dict(ch=(0.5, 1, 2)),
                dict(codes_=codes[:1].contiguous()), dict(w_=w[:, :32].contiguous()), dict(ws=wscale[:-1])):
        with pytest.raises(ValueError):
            patch(**bad)
    big = torch.zeros(2, 16, 4672, dtype=torch.int8)  # K above the limit
    with pytest.raises(ValueError):
        ops.trial_rows_restore([0], big, torch.zeros(16), torch.zeros(16), torch.zeros(1 << 16, dtype=torch.int8))
    for bad in ((0, 0), (64,), ()):
        with pytest.raises(ValueError):
            ops.trial_rows_restore(bad, codes, wscale, col_scale, save[:-4])
    with pytest.raises(ValueError):
        ops.trial_rows_restore((0, 1, 2), codes, wscale, col_scale, save[:-5])
    rows = ops.trial_rows_lists([5, 1], [4, 8], 64, "cpu")
    with pytest.raises(ValueError):  # lists uploaded for another operand
        ops.trial_rows_patch(_weight((128, 64, 1, 1)), rows, None, torch.ones(128), *make_operand(128, 64, 2, 1)[:2],
                             torch.ones(128), save, status)
    assert torch.equal(codes, c0) and status.tolist() == [0, 0, 0]
    patch()  # (and the good call passes)
    assert not torch.equal(codes, c0)


def test_c_entry_points_argument_checks(built_lib):
    """Every SMPQ_E_* comes back before anything is written or launched; the device entry points are
    called with bad arguments only, so they never reach a launch (no GPU needed)."""
    from smpq import _lib
    w = _weight((64, 64, 1, 1))
    codes, wscale, a, col_scale = make_operand(64, 64, 2, seed=2)
    ch = torch.tensor([5, 63, 0], dtype=torch.int32)
    bits = torch.tensor([8, 4, 2], dtype=torch.int32)
    sbuf, save = _guarded(3 * (16 + 2 * 64))
    tbuf, status = _guarded(12, torch.int32)
    status.zero_()
    c0, s0, cs0 = codes.clone(), wscale.clone(), col_scale.clone()
    P = _lib.ptr
    INV, SHP, BITS = _lib.SMPQ_E_INVALID, _lib.SMPQ_E_SHAPE, _lib.SMPQ_E_BITS

    def host(w_=w, cout=64, cin=64, ch_=ch, b_=bits, n=3, sem=0, lw=2, a_=a, codes_=codes, ws=wscale, cs=col_scale,
             sv=save, st=status, off=0):
        return built_lib.smpq_trial_rows_patch_host(P(w_), cout, cin, 1, 1, P(ch_), P(b_), n, sem, lw, P(a_), P(codes_),
                                                    P(ws), P(cs), None if sv is None else sv.data_ptr() + off, P(st))

    def dev(w_=w, cout=64, cin=64, ch_=ch, b_=bits, n=3, sem=0, lw=2, a_=a, codes_=codes, ws=wscale, cs=col_scale,
            sv=save, st=status, off=0):
        return built_lib.smpq_trial_rows_patch(P(w_), cout, cin, 1, 1, P(ch_), P(b_), n, sem, lw, P(a_), P(codes_), None,
                                               P(ws), P(cs), None if sv is None else sv.data_ptr() + off, P(st), None)

    for f in (host, dev):
        for name in ("w_", "ch_", "b_", "a_", "codes_", "ws", "cs", "sv", "st"):
            assert f(**{name: None}) == INV, name
        assert f(n=0) == INV and f(n=-1) == INV and f(n=65) == INV
        assert "smpq_trial_rows_patch" in _lib.last_error()
        assert f(lw=1) == INV and f(lw=4) == INV and f(sem=2) == INV
        assert f(off=2) == INV  # a misaligned save area
        assert f(cin=32) == SHP
        assert f(cin=4672) == SHP  # K above SMPQ_TRIAL_MAX_K
        assert "smpq_trial_rows_patch" in _lib.last_error()
    # what only the host twin can see: the lists themselves
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)  # noqa: E731
    assert host(ch_=i32(5, 63, 5)) == INV and "twice" in _lib.last_error()
    assert host(ch_=i32(5, 64, 0)) == INV and host(ch_=i32(5, -1, 0)) == INV
    assert host(b_=i32(8, 0, 2)) == BITS and host(b_=i32(8, 4, 17)) == BITS
    assert "smpq_trial_rows_patch" in _lib.last_error()
    r = built_lib.smpq_trial_rows_restore_host
    d = built_lib.smpq_trial_rows_restore
    assert r(64, 64, None, 3, 2, P(codes), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 64, P(ch), 3, 2, None, P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 64, P(ch), 0, 2, P(codes), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 64, P(ch), 65, 2, P(codes), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 64, P(ch), 3, 1, P(codes), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 64, P(i32(1, 1, 2)), 3, 2, P(codes), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 64, P(i32(1, 64, 2)), 3, 2, P(codes), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 32, P(ch), 3, 2, P(codes), P(wscale), P(col_scale), P(save)) == SHP
    assert r(64, 4672, P(ch), 3, 2, P(codes), P(wscale), P(col_scale), P(save)) == SHP
    assert "smpq_trial_rows_restore" in _lib.last_error()
    assert d(64, 64, None, 3, 2, P(codes), None, P(wscale), P(col_scale), P(save), None) == INV
    assert d(64, 64, P(ch), 3, 2, P(codes), None, P(wscale), P(col_scale), None, None) == INV
    assert d(64, 64, P(ch), 65, 2, P(codes), None, P(wscale), P(col_scale), P(save), None) == INV
    assert d(64, 32, P(ch), 3, 2, P(codes), None, P(wscale), P(col_scale), P(save), None) == SHP
    # nothing was written
    assert torch.equal(codes, c0) and torch.equal(wscale, s0) and torch.equal(col_scale, cs0)
    assert status.tolist() == [0, 0, 0] and _guards_hold(sbuf) and _guards_hold(tbuf)
    assert bool((save == 0x5A).all())
    assert host() == 0  # (and the good call passes)
    assert not torch.equal(codes, c0) and _guards_hold(sbuf) and _guards_hold(tbuf)


# ---- patchable_rows ---------------------------------------------------------------------------------
def test_patchable_rows_wants_a_free_channel_outside_the_semilayer(built_lib, monkeypatch):
    from smpq import engine, ops, sensitivity
    from smpq.qconv import QConv2d
    conv = QConv2d(64, 8, kernel_size=1, bias=False)
    codes = torch.zeros(2, 8, 64, dtype=torch.int8)
    if ops.KMAJOR[0]:
        codes._smpq_km = torch.zeros(2, 1, 8, 64, dtype=torch.int8)
    plan = types.SimpleNamespace(codes=codes, offset=None)
    monkeypatch.setattr(engine, "conv_plan", lambda c, bn: plan)
    assert sensitivity.patchable_rows(conv, None, [0, 1, 2])
    assert sensitivity.patchable_rows(conv, None, range(7))
    assert not sensitivity.patchable_rows(conv, None, range(8))  # it would complete the conv
    conv._bits_host[[6, 7]] = 8
    assert sensitivity.patchable_rows(conv, None, [0, 1, 2, 3, 4])
    assert not sensitivity.patchable_rows(conv, None, range(6))  # every free channel
    assert sensitivity.patchable_rows(conv, None, [6, 7])  # re-quantizing quantized channels frees none
    assert sensitivity.patchable(conv, None, 0)  # (the single-row rule is as it was)
    plan.offset = torch.zeros(8, dtype=torch.int32)
    assert not sensitivity.patchable_rows(conv, None, [0])
    plan.offset, plan.codes = None, torch.zeros(1, 8, 64, dtype=torch.int8)
    assert not sensitivity.patchable_rows(conv, None, [0])
    assert not sensitivity.patchable_rows(torch.nn.Conv2d(64, 8, 1), None, [0])


# ---- semilayer_table's bookkeeping on injected hooks ----------------------------------------------------
class FakeConv:
    def __init__(self):
        self._content_gen = 0


class FakeHooks:
    """Forwards whose 'loss' is the patched semilayer's marker; flags and status as told."""

    def __init__(self, overflow=(), raise_at=None, constant=()):
        self.overflow, self.raise_at, self.constant = set(overflow), raise_at, dict(constant)
        self.log, self.cur = [], None

    def patch(self, sem, status):
        self.cur = sem
        self.log.append(("patch", sem.index))
        assert status.numel() == len(sem.channels)
        if sem.index in self.constant:
            status[sem.channels.index(self.constant[sem.index])] = 1

    def restore(self, sem):
        self.log.append(("restore", sem.index))
        self.cur = None

    def invalidate(self, sem):
        sem.conv._content_gen += 1

    def forward(self, x):
        if self.cur.index == self.raise_at:
            raise KeyboardInterrupt("stop")
        return x, torch.tensor([1 if self.cur.index in self.overflow else 0, 0], dtype=torch.int32)

    def score_kl(self, logits, y, ref, row, kl_row):
        row += torch.tensor([10.0 + self.cur.index, 3.0, 4.0, 1.0], dtype=torch.float64)
        kl_row += torch.tensor([float(ref) * (1 + self.cur.index), 4.0], dtype=torch.float64)

    def slow(self, sem):
        self.log.append(("slow", sem.index))
        return 0.5, -1.0, -2.0


def _sems(conv, other):
    from smpq.sensitivity import Semilayer
    return [Semilayer(0, 3, conv, [4, 1], [8, 8], 576), Semilayer(1, 3, conv, [0, 2, 5], [4, 6, 2], 576),
            Semilayer(2, 3, conv, [7], [4], 576), Semilayer(3, 3, conv, [6, 3], [4, 4], 576),
            Semilayer(4, 9, other, [0], [8], 64)]


def _row_counts():
    return {"patched": 0, "overflowed": 0, "slow": {}, "constant": [], "rows_patched": 0, "max_rows": 0}


def test_semilayer_param_is_the_references_sum(built_lib):
    conv = FakeConv()
    sems = _sems(conv, conv)
    assert sems[0].param == 576 * (24 / 32) + 576 * (24 / 32)
    want = 0.0
    for b in (4, 6, 2):
        want += 576 * ((32 - b) / 32)
    assert sems[1].param == want and sems[4].param == 64 * 0.75


def test_sweep_rows_order_overflow_constant(built_lib):
    from smpq import sensitivity
    conv, other = FakeConv(), FakeConv()
    sems = _sems(conv, other)
    hooks = FakeHooks(overflow={2}, constant={1: 2})
    got, counts = {}, _row_counts()
    batches = [(torch.zeros(1), torch.zeros(1)), (torch.zeros(1), torch.zeros(1))]
    refs = [1.0, 2.0]
    order = []

    def out(sem, loss, acc, kl, slow, row, kl_row):
        order.append(sem.index)
        got[sem.index] = (loss, acc, kl, slow, row, kl_row)

    sensitivity.sweep_rows([(True, sems[:4]), (False, sems[4:])], batches, refs, hooks, "cpu", out, counts)
    assert order == [0, 1, 3, 2, 4]  # the conv's patched results in order, then the slow ones
    assert counts["patched"] == 2 and counts["overflowed"] == 1 and counts["rows_patched"] == 4 and counts["max_rows"] == 2
    assert counts["slow"] == {"overflow": 1, "not_patchable": 1}
    assert counts["constant"] == [(3, 2, 6)]  # (lnum, channel, its bit-width)
    assert got[0] == (10.0, 0.75, 3.0 / 8.0, False, [20.0, 6.0, 8.0, 2.0], [3.0, 8.0])
    assert got[3][:4] == (13.0, 0.75, 12.0 / 8.0, False)
    assert all(math.isnan(v) for v in got[1][:3]) and got[1][3:] == (False, None, None)
    assert got[2] == (-1.0, 0.5, -2.0, True, None, None) and got[4] == (-1.0, 0.5, -2.0, True, None, None)
    fast = [e for e in hooks.log if e[0] != "slow"]
    assert fast == [(k, i) for i in range(4) for k in ("patch", "restore")]
    assert hooks.log[-2:] == [("slow", 2), ("slow", 4)] and conv._content_gen == 0


def test_sweep_rows_restores_and_invalidates_on_an_exception(built_lib):
    from smpq import sensitivity
    conv = FakeConv()
    hooks = FakeHooks(raise_at=1)
    with pytest.raises(KeyboardInterrupt):
        sensitivity.sweep_rows([(True, _sems(conv, conv)[:4])], [(torch.zeros(1), torch.zeros(1))], [1.0], hooks, "cpu",
                               lambda *a: None, _row_counts())
    assert hooks.log[-2:] == [("patch", 1), ("restore", 1)]
    assert conv._content_gen == 1


def test_semilayer_table_refuses_other_modes_and_bad_lists(built_lib):
    from smpq import engine, sensitivity
    import resnet
    net = resnet.resnet18().eval()
    with pytest.raises(ValueError):  # a model on the CPU
        sensitivity.semilayer_table(net, [(torch.zeros(1, 3, 32, 32), torch.zeros(1, dtype=torch.long))], [(1, [0], 8)])
    engine.set_range_mode("dynamic")
    try:
        with pytest.raises(ValueError):
            sensitivity.semilayer_table(net, [], [(1, [0], 8)])
    finally:
        engine.set_range_mode("static")
    for bad in ([(0, [0], 8)], [(17, [0], 8)], [(1, [], 8)], [(1, [0, 0], 8)], [(1, [64], 8)], [(1, [0], 17)],
                [(1, [0, 1], [8])]):
        with pytest.raises(ValueError):
            sensitivity._semilayers(net, bad)
    sems = sensitivity._semilayers(net, [(16, range(0, 512, 2), 4), (1, [3, 1], (8, 2))])
    assert sems[0].lnum == 16 and sems[0].conv is net.layer4[1].conv2 and len(sems[0].channels) == 256
    assert sems[0].param == 256 * 4608 * (28 / 32) and sems[1].bits == [8, 2]


# ---- the drop-in switch on stubs --------------------------------------------------------------------------
def _lists_for_dropin():
    # rows: [layer_index, block_index, lnum, cnum, w_bit, flag, x, y] (functions.make_divide_minusplusmodels)
    minus = [[0, 0, 1, 5, 8, 0, 0, 0], [0, 0, 1, 9, 8, 0, 0, 0], [0, 0, 2, 3, 6, -1, 0, 0]]
    plus = [[0, 0, 1, 7, 4, 1, 0, 0], [0, 1, 3, 0, 4, 2, 0, 0], [0, 1, 3, 63, 2, 2, 0, 0]]
    return minus, plus


def test_dropin_bookkeeping_on_stubs(built_lib, monkeypatch, capsys):
    monkeypatch.setenv("SMPQ_SYNTHETIC", "1")
    import functions
    import imagenet
    import resnet
    from smpq import sensitivity
    from smpq.batches import ResidentSet
    net = resnet.resnet18().eval()
    loader = ResidentSet([])
    loader.dev = torch.device("cuda", 0)  # bound, as far as the route's test goes; never iterated
    monkeypatch.setattr(imagenet, "val_loader", loader)
    built, tables, evals = [], [], []

    def constructor(num_classes=1000, pretrained=None):
        assert num_classes == 1000 and pretrained == "imagenet"
        built.append(types.SimpleNamespace(to=lambda d: None, eval=lambda: None))
        return built[-1]

    def table_stub(net, batches, semilayers, reference_outputs=None, progress=None):
        tables.append((net, batches, [(ln, list(c), list(b)) for ln, c, b in semilayers], reference_outputs))
        n = len(semilayers)
        return types.SimpleNamespace(kl=np.arange(1, n + 1, dtype=np.float64) * 0.5,
                                     param=np.arange(1, n + 1, dtype=np.float64) * 7.0,
                                     report=lambda: {"constant": []})

    def eval_stub(net, device, data_loader):
        evals.append(net)
        return 0.5, 1.0, ["after"]

    monkeypatch.setattr(resnet, "resnet18", constructor)
    monkeypatch.setattr(sensitivity, "semilayer_table", table_stub)
    monkeypatch.setattr(functions, "evaluate_acc_loss_softmax", eval_stub)
    monkeypatch.setattr(functions, "KLdiv", lambda a, b: 36.0)
    monkeypatch.setattr(functions, "channel_wise_quantizationperchan", lambda t, bit, i: t)
    monkeypatch.setattr(functions.engine, "get_range_mode", lambda: "static")
    monkeypatch.setattr(functions, "PATCHED_SEMILAYERS", [True])
    monkeypatch.setattr(functions, "_PATCHED", dict(functions._PATCHED, announced=False))
    minus, plus = _lists_for_dropin()
    orig = "ORIGINAL"
    semilayers, orders = functions.make_semilayers_resnet18(net, "cuda:0", orig, minus, plus)
    rows = _lists_for_dropin()
    assert semilayers == [rows[0][:2], rows[0][2:], rows[1][:1], rows[1][1:]]
    assert minus[-1] == [0, 0, 100, 0, 0, 0, 0, 0] and plus[-1] == minus[-1] and len(minus) == 4 and len(plus) == 4
    # the first semilayer through the ordinary path, on the caller's net: KL 36 / param
    param0 = 0.0
    for _ in range(2):
        param0 += 576 * ((32 - 8) / 32)
    assert evals == [net] and len(built) == 1
    assert len(tables) == 1 and tables[0][0] is built[0] and tables[0][1] is loader and tables[0][3] is orig
    assert tables[0][2] == [(2, [3], [6]), (1, [7], [4]), (3, [0, 63], [4, 2])]
    assert orders == [[0, 36.0 / param0], [1, 0.5 / 7.0], [2, 1.0 / 14.0], [3, 1.5 / 21.0]]
    out, err = capsys.readouterr()
    lines = [l for l in out.splitlines() if "semilayer-No." in l]
    assert [l.split("semilayer-No.")[1].split()[0] for l in lines] == ["0", "1", "2", "3"]
    assert lines[3].startswith("2 bit") and "layernumber= 3 channels= 2" in lines[3]
    assert err.count("SMPQ_PATCHED_SEMILAYERS=1") == 1
    assert functions.patched_semilayers_report() == {"calls": 1, "semilayers": 3, "fallbacks": 0}
    # a second call announces nothing more
    functions.make_semilayers_resnet18(net, "cuda:0", orig, *_lists_for_dropin())
    assert "SMPQ_PATCHED_SEMILAYERS=1" not in capsys.readouterr().err and len(built) == 2


def test_dropin_falls_back_with_a_line_and_a_counter(built_lib, monkeypatch, capsys):
    monkeypatch.setenv("SMPQ_SYNTHETIC", "1")
    import functions
    import imagenet
    from smpq.batches import ResidentSet
    calls = []
    monkeypatch.setattr(functions, "_make_semilayers_ordinary", lambda *a: calls.append(a) or ("S", "O"))
    monkeypatch.setattr(functions, "_make_semilayers_patched", lambda *a: pytest.fail("the patched route ran"))
    monkeypatch.setattr(functions, "_PATCHED", dict(functions._PATCHED, announced=True, fallbacks=0))
    monkeypatch.setattr(functions, "PATCHED_SEMILAYERS", [True])
    monkeypatch.setattr(imagenet, "val_loader", [(torch.zeros(1), torch.zeros(1))])  # not a ResidentSet
    assert functions.make_semilayers_resnet18(None, "cuda:0", None, [], []) == ("S", "O")
    assert "not a ResidentSet" in capsys.readouterr().err
    monkeypatch.setattr(imagenet, "val_loader", ResidentSet([]))  # a ResidentSet, but bound to nothing
    functions.make_semilayers_resnet18(None, "cuda:0", None, [], [])
    assert "not a ResidentSet bound" in capsys.readouterr().err
    bound = ResidentSet([])
    bound.dev = torch.device("cuda", 0)
    monkeypatch.setattr(imagenet, "val_loader", bound)
    monkeypatch.setattr(functions.engine, "get_range_mode", lambda: "dynamic")
    functions.make_semilayers_resnet18(None, "cuda:0", None, [], [])
    assert "range mode is not static" in capsys.readouterr().err
    assert functions.patched_semilayers_report()["fallbacks"] == 3 and len(calls) == 3
    # off (the default): the ordinary route, silently
    monkeypatch.setattr(functions, "PATCHED_SEMILAYERS", [False])
    functions.make_semilayers_resnet18(None, "cuda:0", None, [], [])
    assert capsys.readouterr().err == "" and len(calls) == 4
    assert functions.patched_semilayers_report()["fallbacks"] == 3
