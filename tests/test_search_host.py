"""smpq.search on the host: the exact8 rows patch's native twin against the quantizer's host twin
followed by a NumPy restatement of the lw == 1 packing rule (include/smpq.h), its status words and
argument checks, patchable_rows_x8 on stub plans, and a Session's bookkeeping on injected hooks (no
GPU needed)."""
import math
import types

import numpy as np
import pytest
import torch

from test_sensitivity_host import pack_row_ref  # noqa: F401  (the lw >= 2 rule this one sits beside)

GUARD = 64


def pack_row_x8_ref(v, s, cin, taps):
    """include/smpq.h "trial rows patch, exact8 operands" steps 3-5 for one quantized row ``v`` (fp32
    [cin*taps], the weight's own [cin][taps] order) with step ``s``: (codes int8 [K] in
    k = tap*cin + ci order, offset, status 0 / 3); the caller decides status 4."""
    v = np.asarray(v, dtype=np.float32)
    s = np.float32(s)
    if not s > 0:
        return None, 0, 3
    with np.errstate(all="ignore"):
        mf = np.rint(v / s).astype(np.float32)
        on = bool(np.all((mf * s).astype(np.float32) == v) and np.all(np.abs(mf) <= np.float32(32512.0)))
    if not on:
        return None, 0, 3
    m = mf.astype(np.int64)
    mmin, mmax = int(m.min()), int(m.max())
    if mmax - mmin > 255:
        return None, 0, 3
    o = mmin + 128 if (mmin < -128 or mmax > 127) else 0
    codes = (m - o).reshape(cin, taps).T.reshape(-1)
    assert codes.min() >= -128 and codes.max() <= 127
    return codes.astype(np.int8), o, 0


def _quantize(built_lib, w2d, rows, bits, sem):
    """The quantizer's host twin on ``rows`` of ``w2d`` (in place): the fp32 steps [cout] (0 elsewhere)."""
    from smpq import _lib, ops
    cout, K = w2d.shape
    b = torch.zeros(cout, dtype=torch.int8)
    b[list(rows)] = torch.tensor(list(bits), dtype=torch.int8)
    step = torch.zeros(cout, dtype=torch.float32)
    assert built_lib.smpq_quantize_channels_host_ex(_lib.ptr(w2d), cout, K, _lib.ptr(b), _lib.ptr(step), ops.QSEM[sem]) == 0
    return step


def make_x8_operand(built_lib, shape, seed, sem="cpu", offsets=True):
    """A weight with every row quantized at 8 bits and its exact8 operand by the NumPy rule:
    (w, codes [1, cout, K], offset or None, wscale, bn_a, col_scale)."""
    cout, cin, kh, kw = shape
    K = cin * kh * kw
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(*shape, generator=g) * 0.05).contiguous()
    step = _quantize(built_lib, w.view(cout, K), range(cout), [8] * cout, sem)
    codes = torch.zeros(1, cout, K, dtype=torch.int8)
    offset = torch.zeros(cout, dtype=torch.int32)
    for c in range(cout):
        row, o, st = pack_row_x8_ref(w[c].reshape(-1).numpy(), step[c].item(), cin, kh * kw)
        assert st == 0
        codes[0, c] = torch.from_numpy(row)
        offset[c] = o
    a = torch.rand(cout, generator=g) + 0.5
    col_scale = (step * a).contiguous()
    return w, codes, (offset if offsets else None), step.clone(), a, col_scale


def expected_x8(built_lib, w, chans, bits, sem, codes, offset, wscale, a, col_scale):
    cout, cin, kh, kw = w.shape
    w2 = w.clone()
    step = _quantize(built_lib, w2.view(cout, -1), chans, bits, sem)
    e = [codes.clone(), None if offset is None else offset.clone(), wscale.clone(), col_scale.clone()]
    status = []
    for c in chans:
        row, o, st = pack_row_x8_ref(w2[c].reshape(-1).numpy(), step[c].item(), cin, kh * kw)
        if st == 0 and o != 0 and offset is None:
            st = 4
        status.append(st)
        if st:
            continue
        e[0][0, c] = torch.from_numpy(row)
        if offset is not None:
            e[1][c] = o
        e[2][c] = float(step[c])
        e[3][c] = float(np.float32(step[c].item()) * np.float32(a[c].item()))
    return e, status


def _same(ts, es):
    for t, e in zip(ts, es):
        if t is None or e is None:
            assert t is None and e is None
        else:
            assert t.dtype == e.dtype and torch.equal(t.contiguous().view(torch.uint8), e.contiguous().view(torch.uint8))


def _guarded(size, fill, dtype):
    buf = torch.full((size + 2 * GUARD,), fill, dtype=dtype)
    return buf, buf[GUARD:GUARD + size]


def _holds(buf, size, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + size:] == fill).all())


@pytest.mark.parametrize("shape", [(64, 64, 1, 1), (64, 64, 3, 3)])
def test_host_x8_patch_and_restore(built_lib, shape):
    from smpq import ops
    cout, cin, kh, kw = shape
    K = cin * kh * kw
    patched = 0
    for sem in ("cpu", "device"):
        w, codes, offset, wscale, a, col_scale = make_x8_operand(built_lib, shape, 11, sem)
        assert bool((offset != 0).any())  # (8-bit rows whose codes leave [-128, 127]: offsets matter)
        w0 = w.clone()
        orig = [t.clone() for t in (codes, offset, wscale, col_scale)]
        for chans in ([0], [cout - 1, 0, 5], list(range(cout))):
            n = len(chans)
            bits = [(8, 6, 4, 2)[i % 4] for i in range(n)]
            size = ops.trial_rows_save_bytes(1, K, n)
            buf, save = _guarded(size, 0x5A, torch.int8)
            sbuf, status = _guarded(n, 0x5A5A5A5A, torch.int32)
            status.zero_()
            e, want = expected_x8(built_lib, w, chans, bits, sem, codes, offset, wscale, a, col_scale)
            assert want == [0] * n
            rows = ops.trial_rows_patch_x8(w, chans, bits, a, codes, offset, wscale, col_scale, save, status, semantics=sem)
            assert status.tolist() == want and torch.equal(w, w0)
            _same((codes, offset, wscale, col_scale), e)
            assert n == 1 or not torch.equal(codes, orig[0])  # (8 bits over an 8-bit row changes nothing)
            patched += n
            # the slot: the row's two scalars, its offset at byte 8, its code bytes
            slot = save[:16 + K]
            c = chans[0]
            assert slot[:8].view(torch.float32).tolist() == [orig[2][c].item(), orig[3][c].item()]
            assert slot[8:12].view(torch.int32).item() == orig[1][c].item() and torch.equal(slot[16:], orig[0][0, c])
            ops.trial_rows_restore_x8(rows, codes, offset, wscale, col_scale, save)
            _same((codes, offset, wscale, col_scale), orig)
            assert _holds(buf, size, 0x5A) and _holds(sbuf, n, 0x5A5A5A5A)
    assert patched == 2 * (1 + 3 + cout)


def test_host_x8_constant_row_in_the_middle(built_lib):
    from smpq import ops
    w, codes, offset, wscale, a, col_scale = make_x8_operand(built_lib, (64, 64, 1, 1), 5)
    w[9] = 0.25
    orig = [t.clone() for t in (codes, offset, wscale, col_scale)]
    e, want = expected_x8(built_lib, w, [3, 60], [6, 2], "cpu", codes, offset, wscale, a, col_scale)
    save = torch.zeros(ops.trial_rows_save_bytes(1, 64, 3), dtype=torch.int8)
    status = torch.zeros(3, dtype=torch.int32)
    ops.trial_rows_patch_x8(w, [3, 9, 60], [6, 4, 2], a, codes, offset, wscale, col_scale, save, status, semantics="cpu")
    assert status.tolist() == [0, 1, 0] and want == [0, 0]
    _same((codes, offset, wscale, col_scale), e)  # row 9 as it was, its neighbours patched
    assert torch.equal(codes[0, 9], orig[0][0, 9]) and not torch.equal(codes[0, 3], orig[0][0, 3])
    ops.trial_rows_restore_x8([3, 9, 60], codes, offset, wscale, col_scale, save)
    _same((codes, offset, wscale, col_scale), orig)


def test_host_x8_row_that_needs_an_offset_the_operand_lacks(built_lib):
    """Every value in [1.0, 1.1] at 4 bits: the codes would be 150..165, so o != 0; with offset=NULL
    that is status 4 and the row stays; with an offset tensor it is patched."""
    from smpq import ops
    w, codes, offset, wscale, a, col_scale = make_x8_operand(built_lib, (64, 64, 1, 1), 7)
    w[5] = torch.linspace(1.0, 1.1, 64).reshape(64, 1, 1)
    orig = [t.clone() for t in (codes, wscale, col_scale)]
    save = torch.zeros(ops.trial_rows_save_bytes(1, 64, 2), dtype=torch.int8)
    status = torch.zeros(2, dtype=torch.int32)
    ops.trial_rows_patch_x8(w, [5, 6], [4, 4], a, codes, None, wscale, col_scale, save, status, semantics="cpu")
    assert status[0].item() == 4
    assert torch.equal(codes[0, 5], orig[0][0, 5]) and wscale[5] == orig[1][5] and col_scale[5] == orig[2][5]
    assert save[8:12].view(torch.int32).item() == 0  # the slot's offset word without an offset tensor
    ops.trial_rows_restore_x8([5, 6], codes, None, wscale, col_scale, save)
    _same((codes, wscale, col_scale), orig)
    status.zero_()
    e, want = expected_x8(built_lib, w, [5], [4], "cpu", codes, offset, wscale, a, col_scale)
    ops.trial_rows_patch_x8(w, [5], [4], a, codes, offset, wscale, col_scale, save, status, semantics="cpu")
    assert want == [0] and status[0].item() == 0 and offset[5].item() == 150 + 128
    _same((codes, offset, wscale, col_scale), e)
    assert int(codes[0, 5].min()) == -128 and int(codes[0, 5].max()) == 165 - 278


def test_host_x8_off_grid_row(built_lib):
    # test_host_patch_off_grid_row_falls_back_to_fixed_point's row: far from zero with a tiny range, its
    # codes exceed 32512; the normal path would not pack this conv exact8
    from smpq import ops
    w, codes, offset, wscale, a, col_scale = make_x8_operand(built_lib, (64, 64, 1, 1), 3)
    w[5] = 1000.0 + torch.rand(64, 1, 1, generator=torch.Generator().manual_seed(4)) * 1e-3
    orig = [t.clone() for t in (codes, offset, wscale, col_scale)]
    e, want = expected_x8(built_lib, w, [5], [8], "cpu", codes, offset, wscale, a, col_scale)
    assert want == [3]
    save = torch.zeros(ops.trial_rows_save_bytes(1, 64, 1), dtype=torch.int8)
    status = torch.zeros(1, dtype=torch.int32)
    ops.trial_rows_patch_x8(w, [5], [8], a, codes, offset, wscale, col_scale, save, status, semantics="cpu")
    assert status.tolist() == [3]
    _same((codes, offset, wscale, col_scale), orig)
    ops.trial_rows_restore_x8([5], codes, offset, wscale, col_scale, save)
    _same((codes, offset, wscale, col_scale), orig)


def test_x8_argument_validation(built_lib):
    """Every check returns its code before anything is launched or written (the device entry points
    are called with bad arguments only)."""
    from smpq import _lib
    w, codes, offset, wscale, a, col_scale = make_x8_operand(built_lib, (64, 64, 1, 1), 2)
    c0 = codes.clone()
    save = torch.full((3 * (16 + 64),), 0x5A, dtype=torch.int8)
    status = torch.zeros(3, dtype=torch.int32)
    P = _lib.ptr
    INV, SHP, BITS = _lib.SMPQ_E_INVALID, _lib.SMPQ_E_SHAPE, _lib.SMPQ_E_BITS

    def i32(*v):
        return torch.tensor(v, dtype=torch.int32)

    ch, bits = i32(3, 0, 63), i32(8, 4, 2)
    keep = [ch, bits]

    def host(w_=w, cout=64, cin=64, ch_=ch, b_=bits, n=3, sem=0, a_=a, codes_=codes, off=offset, ws=wscale, cs=col_scale,
             sv=save, st=status):
        return built_lib.smpq_trial_rows_patch_x8_host(P(w_), cout, cin, 1, 1, P(ch_), P(b_), n, sem, P(a_), P(codes_),
                                                       P(off), P(ws), P(cs), P(sv), P(st))

    def dev(w_=w, cout=64, cin=64, ch_=ch, b_=bits, n=3, sem=0, a_=a, codes_=codes, off=offset, ws=wscale, cs=col_scale,
            sv=save, st=status):
        return built_lib.smpq_trial_rows_patch_x8(P(w_), cout, cin, 1, 1, P(ch_), P(b_), n, sem, P(a_), P(codes_), None,
                                                  P(off), P(ws), P(cs), P(sv), P(st), None)

    for f in (host, dev):
        for name in ("w_", "ch_", "b_", "a_", "codes_", "ws", "cs", "sv", "st"):
            assert f(**{name: None}) == INV, name
        assert f(n=0) == INV and f(n=65) == INV and f(sem=2) == INV and f(cout=0) == INV
        assert f(cin=32) == SHP and f(cin=4672) == SHP
        assert "smpq_trial_rows_patch_x8" in _lib.last_error()
    # the lists are the host twin's to check
    assert host(ch_=i32(3, 64, 0)) == INV and host(ch_=i32(3, -1, 0)) == INV and host(ch_=i32(3, 0, 3)) == INV
    assert host(b_=i32(8, 0, 2)) == BITS and host(b_=i32(8, 9, 2)) == BITS and host(b_=i32(16, 4, 2)) == BITS
    assert "1..8" in _lib.last_error()
    r = built_lib.smpq_trial_rows_restore_x8_host
    d = built_lib.smpq_trial_rows_restore_x8
    assert r(64, 64, None, 3, P(codes), P(offset), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 64, P(ch), 3, None, P(offset), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 64, P(ch), 0, P(codes), P(offset), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 64, P(i32(1, 64, 2)), 3, P(codes), P(offset), P(wscale), P(col_scale), P(save)) == INV
    assert r(64, 32, P(ch), 3, P(codes), P(offset), P(wscale), P(col_scale), P(save)) == SHP
    assert d(64, 64, P(ch), 3, P(codes), None, P(offset), P(wscale), P(col_scale), None, None) == INV
    assert d(64, 64, P(ch), 65, P(codes), None, P(offset), P(wscale), P(col_scale), P(save), None) == INV
    assert d(64, 4672, P(ch), 3, P(codes), None, P(offset), P(wscale), P(col_scale), P(save), None) == SHP
    assert torch.equal(codes, c0) and status.tolist() == [0, 0, 0] and bool((save == 0x5A).all())
    assert host() == 0 and host(off=None) in (0,)  # (the good calls pass; offset may be NULL)
    assert keep


def test_x8_ops_wrappers_validate(built_lib):
    from smpq import ops
    w, codes, offset, wscale, a, col_scale = make_x8_operand(built_lib, (64, 64, 1, 1), 2)
    save = torch.zeros(ops.trial_rows_save_bytes(1, 64, 2), dtype=torch.int8)
    status = torch.zeros(2, dtype=torch.int32)
    good = dict(w=w, channels=[1, 2], bits=[4, 4], bn_a=a, codes=codes, offset=offset, wscale=wscale,
                col_scale=col_scale, save=save, status=status)
    for bad in (dict(channels=[1, 64]), dict(channels=[1, 1]), dict(channels=[]), dict(bits=[4, 9]), dict(bits=[4]),
                dict(codes=torch.zeros(2, 64, 64, dtype=torch.int8)), dict(codes=codes[0]),
                dict(offset=offset.to(torch.int64)), dict(offset=offset[:-1]), dict(offset=torch.zeros(128, dtype=torch.int32)[::2]),
                dict(save=save[:-1]), dict(status=status[:1]), dict(wscale=wscale[:-1]), dict(bn_a=a.double()),
                dict(w=w[:, :32].contiguous())):
        with pytest.raises(ValueError):
            ops.trial_rows_patch_x8(**dict(good, **bad))
    with pytest.raises(ValueError):
        ops.trial_rows_restore_x8([1, 2], codes, offset[:-1], wscale, col_scale, save)
    with pytest.raises(ValueError):
        ops.trial_rows_restore_x8([1, 2], codes, offset, wscale, col_scale, save[:-1])
    with pytest.raises(ValueError):
        ops.trial_rows_lists([0], 9, 64, "cpu", max_bits=8)
    assert status.tolist() == [0, 0]
    ops.trial_rows_patch_x8(**good)


# ---- patchable_rows_x8 ------------------------------------------------------------------------------
def test_patchable_rows_x8_on_stub_plans(built_lib, monkeypatch):
    from smpq import engine, ops, sensitivity
    from smpq.qconv import QConv2d
    conv = QConv2d(64, 8, kernel_size=1, bias=False)
    codes = torch.zeros(1, 8, 64, dtype=torch.int8)
    if ops.KMAJOR[0]:
        codes._smpq_km = torch.zeros(1, 1, 8, 64, dtype=torch.int8)
    plan = types.SimpleNamespace(codes=codes, offset=None, kind="exact8")
    monkeypatch.setattr(engine, "conv_plan", lambda c, bn: plan)
    assert not sensitivity.patchable_rows_x8(conv, None, [0], 4)  # a free channel: not an exact8 conv
    conv._bits_host[:] = 8
    assert sensitivity.patchable_rows_x8(conv, None, [0], 4)
    assert sensitivity.patchable_rows_x8(conv, None, range(8), [8, 6, 4, 2, 8, 6, 4, 2])  # all of its channels
    assert not sensitivity.patchable_rows_x8(conv, None, [0, 1], [4, 9])  # a wider row cannot be exact8
    assert not sensitivity.patchable_rows(conv, None, [0])  # (and the lw >= 2 rule refuses it, as before)
    plan.offset = torch.zeros(8, dtype=torch.int32)
    assert sensitivity.patchable_rows_x8(conv, None, [0], 4)
    plan.kind = "exact16"
    assert not sensitivity.patchable_rows_x8(conv, None, [0], 4)
    plan.kind, plan.codes = "exact8", torch.zeros(2, 8, 64, dtype=torch.int8)
    assert not sensitivity.patchable_rows_x8(conv, None, [0], 4)
    plan.codes = torch.zeros(1, 8, 64, dtype=torch.int8)  # no K-major copy
    assert sensitivity.patchable_rows_x8(conv, None, [0], 4) == (not ops.KMAJOR[0])
    plan.codes = torch.zeros(1, 8, 32, dtype=torch.int8)
    assert not sensitivity.patchable_rows_x8(conv, None, [0], 4)
    assert not sensitivity.patchable_rows_x8(torch.nn.Conv2d(64, 8, 1), None, [0], 4)


# ---- a Session on injected hooks ----------------------------------------------------------------------
class FakeConv:
    def __init__(self, block):
        self.block, self._content_gen = block, 0


class FakeStore:
    pass


class FakeHooks:
    """Eight blocks, one conv each (lnum = block + 1). A forward's 'statistics' are the patched
    semilayer's marker; flags, status words, routes and batch sizes as told."""
    plan = None
    _state = None
    reference = None
    device = "cpu"

    def __init__(self, nbatches=2, overflow=(), raise_at=None, status=None, routes=None, unresumable=(), nbytes=None):
        self.convs = [FakeConv(j) for j in range(8)]
        self.batches = [(torch.full((1,), float(i)), torch.zeros(1)) for i in range(nbatches)]
        self.overflow, self.raise_at, self.status = set(overflow), raise_at, dict(status or {})
        self.routes, self.unresumable, self.nbytes = dict(routes or {}), set(unresumable), nbytes or {}
        self.log, self.cur, self.sig, self.cal_sig, self.evals, self.fills, self.resumes = [], None, 0, 0, 0, [], []

    def semilayer(self, lnum, channels, bit):
        from smpq.sensitivity import Semilayer
        if not 1 <= lnum <= 8:
            raise ValueError("lnum")
        channels = list(channels)
        bits = [bit] * len(channels) if isinstance(bit, int) else list(bit)
        return Semilayer(0, lnum, self.convs[lnum - 1], channels, bits, 64)

    def rebind(self):
        self.cal_sig = self.sig
        self._state = None

    def held(self):
        return self.cal_sig == self.sig

    def signature(self):
        return self.sig

    def counters(self):
        return (self.evals, 0, 0)

    def ordinary_eval(self):
        self.evals += 1
        self.log.append(("eval",))
        return 0.5 + self.sig, 2.0, [torch.ones(1) for _ in self.batches]

    def kl_of(self, reference, outs):
        return 0.25 * self.sig

    def unpatched_pass(self):
        st = torch.zeros(4, dtype=torch.float64)
        for x, y in self.batches:
            self.score_kl(None, y, None, st, torch.zeros(2, dtype=torch.float64))
        return st.tolist(), [0, 0], [torch.ones(1) for _ in self.batches]

    def kl_stats(self, refs, probs):
        return [0.0, 4.0 * len(self.batches)]

    def constant_rows(self, conv):
        return [c == 7 for c in range(8)]

    def route(self, sem):
        return self.routes.get(sem.lnum, "patched")

    def zeros(self, n, dtype):
        return torch.zeros(n, dtype=dtype)

    def block_index(self, name):
        return int(name[1:])

    def boundary_conv(self, j):
        return self.convs[j]

    def block_of(self, conv):
        return conv.block

    def block_name(self, j):
        return "b%d" % j

    def kept_bytes(self, x, j):
        return self.nbytes.get(j, 100)

    def fill(self, x, j):
        from smpq.suffix import Kept
        self.fills.append((j, int(x[0])))
        if j in self.unresumable:
            return None
        k = Kept([(0, 1, torch.zeros(self.kept_bytes(x, j), dtype=torch.int8), 1.0)], 1)
        return k

    def sync(self):
        pass

    def prepare_one(self, sem, route):
        self.log.append(("prepare", sem.lnum, route))

    def patch(self, sem, status):
        self.cur = sem
        self.log.append(("patch", sem.lnum))
        for i, word in self.status.get(sem.lnum, {}).items():
            status[i] = word

    def restore(self, sem):
        self.log.append(("restore", sem.lnum))
        self.cur = None

    def invalidate(self, sem):
        sem.conv._content_gen += 1

    def _flags(self):
        ln = self.cur.lnum if self.cur is not None else None
        if ln is not None and ln == self.raise_at:
            raise KeyboardInterrupt("stop")
        return torch.tensor([1 if ln in self.overflow else 0, 0], dtype=torch.int32)

    def forward(self, x):
        return x, self._flags()

    def resume(self, kept, j):
        self.resumes.append(j)
        if self.plan is not None:
            self.plan.resumed += 1
            self.plan.launches += 8 - j
        return None, self._flags()

    def score_kl(self, logits, y, ref, row, kl_row):
        mark = 0.0 if self.cur is None else float(self.cur.lnum)
        row += torch.tensor([10.0 + mark, 3.0, 4.0, 1.0], dtype=torch.float64)
        kl_row += torch.tensor([mark, 4.0], dtype=torch.float64)

    def slow(self, sem):
        self.log.append(("slow", sem.lnum))
        self._state = "snapshot"
        self.sig += 1  # (a restore moves the signature)
        return 0.125, 3.0, 0.75

    def commit(self, sem):
        self.log.append(("commit", sem.lnum, tuple(sem.channels), tuple(sem.bits)))
        self.sig += 1


def _session(hooks, **kw):
    from smpq import search
    kw.setdefault("boundaries", ("b3", "b6"))
    return search.Session(None, hooks.batches, hooks=hooks, **kw)


def test_session_routes_and_boundary_pick(built_lib):
    hooks = FakeHooks(routes={2: "patched_x8", 8: None})
    s = _session(hooks)
    assert s.base.acc == 0.5 and s.base.loss == 2.0 and s.base.kl == 0.0 and s.base.route == "base"
    assert sorted(s.stores()) == [3, 6] and all(st.kept == 2 for st in s.stores().values())
    assert hooks.fills == [(6, 0), (6, 1), (3, 0), (3, 1)]  # deepest first, one fill per batch
    assert hooks.resumes == [6, 6, 3, 3]  # the self-checks
    del hooks.resumes[:]
    want = {1: None, 2: None, 3: None, 4: "b3", 6: "b3", 7: "b6"}  # the deepest kept boundary j <= b; none before the first
    for lnum, name in want.items():
        r = s.trial(lnum, [0, 1, 2], 4)
        assert r.route == ("patched_x8" if lnum == 2 else "patched") and r.resumed_from == name, lnum
        assert r.stats == [2 * (10.0 + lnum), 6.0, 8.0, 2.0] and r.kl_stats == [2.0 * lnum, 8.0]
        assert (r.loss, r.acc, r.kl) == (10.0 + lnum, 0.75, lnum / 4.0)
        assert r.param == 3 * 64 * (28 / 32) and r.channels == [0, 1, 2] and r.bits == [4, 4, 4]
    assert hooks.resumes == [3, 3, 3, 3, 6, 6]
    assert s.trial(2, [5], (6,)).route == "patched_x8"
    r = s.trial(8, [0], 4)
    assert r.route == "slow:not_patchable" and (r.acc, r.loss, r.kl) == (0.125, 3.0, 0.75) and r.stats is None
    assert not s.stores()  # a slow trial rewrote the model: everything kept is released ...
    assert s.trial(1, [0], 8).route == "patched"  # ... and the next trial follows one more rebase
    r = s.trial(1, [0, 7], 8)
    assert r.route == "constant" and math.isnan(r.acc) and math.isnan(r.kl)
    rep = s.report()
    assert rep["trials"] == {"patched": 6, "patched_x8": 2, "slow:not_patchable": 1, "constant": 1}
    assert rep["rebases"] == {"construction": 1, "slow": 1} and rep["rows_patched"] == 6 * 3 + 1 + 1
    assert rep["constant"] == [(1, 7, 8)]
    assert rep["rebase"]["calibrations"] == 2 and rep["patched_trials"] == dict.fromkeys(rep["patched_trials"], 0)
    rows = {row["block"]: row for row in rep["boundaries"]}
    assert rows[3]["kept"] == 2 and rows[6]["self_check"] is True and rows[6]["self_check_conv_launches"] == 2 * 2
    s.close()
    assert not s.stores()
    with pytest.raises(RuntimeError):
        s.trial(1, [0], 4)


def test_session_counts_the_trials_resumes_per_boundary(built_lib):
    hooks = FakeHooks()
    with _session(hooks) as s:
        s.trial(4, [0], 4)
        s.trial(8, [0], 4)
        rows = {row["block"]: row for row in s.report()["boundaries"]}
        assert (rows[3]["resumed_forwards"], rows[3]["resumed_conv_launches"]) == (2, 2 * 5)
        assert (rows[6]["resumed_forwards"], rows[6]["resumed_conv_launches"]) == (2, 2 * 2)
    assert not s.stores()
    rows = {row["block"]: row for row in s.report()["boundaries"]}  # the counts outlive the release
    assert (rows[3]["resumed_forwards"], rows[6]["resumed_conv_launches"]) == (2, 2 * 2)


def test_session_budget_admits_deepest_first(built_lib):
    sizes = {6: 100, 3: 200}
    s = _session(FakeHooks(nbytes=sizes), boundary_bytes=200)  # both batches of b6, nothing of b3
    assert sorted(s.stores()) == [6] and s.stores()[6].bytes == 200
    assert s.trial(5, [0], 4).resumed_from is None and s.trial(7, [0], 4).resumed_from == "b6"
    rows = {row["block"]: row for row in s.report()["boundaries"]}
    assert rows[3]["kept"] == 0 and rows[3]["full"] == 2
    hooks = FakeHooks(nbytes=sizes)
    s = _session(hooks, boundary_bytes=100)  # one batch of b6: the second batch replays
    assert s.stores()[6].kept == 1 and [e is not None for e in s.stores()[6].entries] == [True, False]
    del hooks.resumes[:]
    r = s.trial(7, [0], 4)
    assert r.resumed_from == "b6" and hooks.resumes == [6] and r.stats[3] == 2.0
    s = _session(FakeHooks(nbytes=sizes), boundary_bytes=500)  # b6 whole, then b3's first batch
    assert s.stores()[6].kept == 2 and s.stores()[3].kept == 1
    s = _session(FakeHooks(), boundaries=())
    assert not s.stores() and s.trial(8, [0], 4).resumed_from is None and s.report()["boundaries"] == []
    with pytest.raises(ValueError):
        _session(FakeHooks(), boundary_bytes=-1)


def test_session_unresumable_boundary_is_reported_and_not_used(built_lib):
    hooks = FakeHooks(unresumable={3})
    s = _session(hooks)
    assert sorted(s.stores()) == [6]
    rows = {row["block"]: row for row in s.report()["boundaries"]}
    assert rows[3]["resumable"] is False and rows[3]["kept"] == 0 and rows[6]["resumable"] is True
    assert s.trial(5, [0], 4).resumed_from is None


def test_session_self_check_failure_releases_the_stores(built_lib):
    hooks = FakeHooks()
    real = hooks.resume
    hooks.resume = lambda kept, j: (None, torch.tensor([1 if j == 3 else 0, 0], dtype=torch.int32)) if j == 3 else real(kept, j)
    from smpq import search
    with pytest.raises(RuntimeError):
        search.Session(None, hooks.batches, hooks=hooks, boundaries=("b3", "b6"))


def test_session_restores_and_invalidates_on_an_exception(built_lib):
    hooks = FakeHooks(raise_at=5)
    s = _session(hooks)
    with pytest.raises(KeyboardInterrupt):
        s.trial(5, [0, 1], 4)
    assert hooks.log[-2:] == [("patch", 5), ("restore", 5)] and hooks.convs[4]._content_gen == 1
    assert not s.stores()  # nothing is kept after an exception inside a trial
    with pytest.raises(RuntimeError):
        s.accept()
    assert s.trial(4, [0], 4).route == "patched" and s.report()["rebases"] == {"construction": 1, "exception": 1}


def test_session_overflow_and_unpackable_go_slow_and_flag_a_rebase(built_lib):
    hooks = FakeHooks(overflow={4}, status={5: {1: 3}, 6: {0: 4}, 2: {0: 1}})
    s = _session(hooks)
    r = s.trial(4, [0, 1], 4)
    assert r.route == "slow:overflow" and (r.acc, r.loss, r.kl) == (0.125, 3.0, 0.75) and r.resumed_from is None
    assert [e[0] for e in hooks.log[-4:]] == ["prepare", "patch", "restore", "slow"]
    assert s.trial(5, [0, 1], 4).route == "slow:unpackable" and s.trial(6, [0], 4).route == "slow:unpackable"
    assert s.trial(2, [3], 4).route == "constant"  # the kernel's own word for a constant row
    rep = s.report()
    assert rep["trials"] == {"slow:overflow": 1, "slow:unpackable": 2, "constant": 1}
    assert rep["rebases"] == {"construction": 1, "slow": 3} and rep["rows_patched"] == 0
    assert rep["constant"] == [(2, 3, 4)]


def test_session_accept(built_lib):
    hooks = FakeHooks()
    s = _session(hooks)
    with pytest.raises(RuntimeError):
        s.accept()  # no trial yet
    s.trial(1, [0, 7], 4)
    with pytest.raises(RuntimeError):
        s.accept()  # a constant one
    s.trial(3, [0, 1], 4)
    s.trial(5, [2, 4], (6, 4))
    base = s.accept()
    assert ("commit", 5, (2, 4), (6, 4)) in hooks.log and hooks.log[-1] == ("eval",)
    assert base is s.base and base.acc == 1.5 and base.kl == 0.25 and sorted(s.stores()) == [3, 6]
    assert s.report()["rebases"] == {"construction": 1, "accept": 1}
    with pytest.raises(RuntimeError):
        s.accept()  # the trial is spent
    s.trial(5, [0], 4)
    hooks.sig += 1  # the caller changed the model
    with pytest.raises(RuntimeError):
        s.accept()
    with pytest.raises(RuntimeError):
        s.trial(5, [0], 4)  # ... and said nothing
    s.rebase()
    assert not s.stores() and s.trial(5, [0], 4).route == "patched"
    assert s.report()["rebases"] == {"construction": 1, "accept": 1, "explicit": 1}
    s.trial(8, [0], 4)
    hooks.routes[8] = None
    assert s.trial(8, [1], 4).route == "slow:not_patchable"
    s.accept()  # a slow trial can be accepted too: the model is the state it was tried on
    assert hooks.log[-2][:2] == ("commit", 8)


def test_session_refuses_other_modes(built_lib):
    from smpq import engine, search
    import resnet
    net = resnet.resnet18().eval()
    with pytest.raises(ValueError):  # a model on the CPU
        search.Session(net, [(torch.zeros(1, 3, 32, 32), torch.zeros(1, dtype=torch.long))])
    engine.set_range_mode("dynamic")
    try:
        with pytest.raises(ValueError):
            search.Session(net, [])
    finally:
        engine.set_range_mode("static")
