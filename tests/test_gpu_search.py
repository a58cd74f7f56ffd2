"""smpq.search on the GPU: the exact8 rows patch kernel against the normal quantize + pack + fold path
(bitwise), a session's trials against a really quantized model under the session's ranges (bitwise,
both patches), what trials leave behind, accept() against the public API, and the kept boundaries
against the replay route (bitwise)."""
import types

import numpy as np
import pytest
import torch

from test_gpu import build_model
from test_gpu_semilayer import _reference_stats
from test_gpu_sensitivity import _batches, knobs  # noqa: F401  (knobs: a fixture)

pytestmark = pytest.mark.gpu

GUARD = 64
ZERO = {"calibrations": 0, "graph_captures": 0, "repack": 0}


def _set(graph, limbs):
    from smpq import engine, ops
    engine.USE_GRAPH[0] = graph
    ops.set_act_limbs(limbs)


def _mixed_bits(n):
    return [(8, 6, 4, 2)[i % 4] for i in range(n)]


def _bytes_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- the kernel against the normal path -----------------------------------------------------------
@pytest.mark.parametrize("shape", [(64, 64, 1, 1), (64, 64, 3, 3), (128, 256, 1, 1), (64, 512, 3, 3)])
def test_x8_kernel_matches_quantize_pack_fold(gpu, shape):
    """Every row at 8 bits, packed with one weight limb (offsets in most rows). One row, three unsorted
    rows with the first and the last channel, and all rows (K = 4608 is the row limit), at mixed
    8 / 6 / 4 / 2 bits: after the patch the whole operand (codes, K-major copy, offset, wscale,
    col_scale) equals quantize_channels_ of those rows on a clone + pack_weights_ex(..., 1) with the
    merged steps + _fold; after the restore it equals the original; the guards hold."""
    from smpq import engine, ops
    cout, cin, kh, kw = shape
    K = cin * kh * kw
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(*shape, generator=g) * 0.05).to(gpu)
    bn = torch.nn.BatchNorm2d(cout)
    bn.running_var.copy_(torch.rand(cout, generator=g) + 0.5)
    bn.weight.data.copy_(torch.rand(cout, generator=g) + 0.5)
    bn = bn.to(gpu).eval()
    conv = types.SimpleNamespace(bias=None)
    a = engine._bn_fold(bn)[0].contiguous()
    step = ops.quantize_channels_(w.view(cout, -1), np.full(cout, 8))
    codes, offset, wscale, st = ops.pack_weights_ex(w, step, 1)
    assert st.tolist()[:2] == [0, 0] and bool((offset != 0).any())
    km = codes._smpq_km
    col_scale, _ = engine._fold(conv, bn, wscale)
    orig = [t.clone() for t in (codes, km, offset, wscale, col_scale)]
    for chans in ([0], [cout - 1, 0, 5], list(reversed(range(cout)))):
        n = len(chans)
        rbits = _mixed_bits(n)
        size = ops.trial_rows_save_bytes(1, K, n)
        buf = torch.full((size + 2 * GUARD,), 0x5A, dtype=torch.int8, device=gpu)
        save = buf[GUARD:GUARD + size]
        sbuf = torch.full((n + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        status = sbuf[GUARD:GUARD + n]
        for sem in ("cpu", "device"):
            what = (n, sem)
            w2 = w.clone()
            bits = np.zeros(cout, dtype=np.int64)
            bits[chans] = rbits
            step2 = ops.quantize_channels_(w2.view(cout, -1), bits, semantics=sem)
            merged = torch.where(torch.from_numpy(bits > 0).to(gpu), step2, step)
            e_codes, e_off, e_ws, e_st = ops.pack_weights_ex(w2, merged, 1)
            assert e_st.tolist()[:2] == [0, 0], what  # (the normal path packs it exact8)
            e_cs, _ = engine._fold(conv, bn, e_ws)
            status.zero_()
            rows = ops.trial_rows_patch_x8(w, chans, rbits, a, codes, offset, wscale, col_scale, save, status, km=km,
                                           semantics=sem)
            assert status.tolist() == [0] * n, what
            for name, t, e in (("codes", codes, e_codes), ("km", km, e_codes._smpq_km), ("offset", offset, e_off),
                               ("wscale", wscale, e_ws), ("col_scale", col_scale, e_cs)):
                assert _bytes_equal(t, e), (name,) + what
            ops.trial_rows_restore_x8(rows, codes, offset, wscale, col_scale, save, km=km)
            for t, o in zip((codes, km, offset, wscale, col_scale), orig):
                assert _bytes_equal(t, o), what
            assert bool((buf[:GUARD] == 0x5A).all()) and bool((buf[GUARD + size:] == 0x5A).all()), what
            assert bool((sbuf[:GUARD] == 0x5A5A5A5A).all()) and bool((sbuf[GUARD + n:] == 0x5A5A5A5A).all()), what


def test_x8_kernel_status_words(gpu):
    """A constant row (1), a row off the grid (3) and a row that needs an offset the operand does not
    have (4), between two rows that are patched: the three stay as they are, bit for bit."""
    from smpq import ops
    cout, K = 64, 64
    w = (torch.randn(cout, K, 1, 1, generator=torch.Generator().manual_seed(6)) * 0.05).to(gpu)
    step = ops.quantize_channels_(w.view(cout, -1), np.full(cout, 8))
    codes, offset, wscale, _ = ops.pack_weights_ex(w, step, 1)
    km = codes._smpq_km
    w[9] = -0.5
    w[20] = (1000.0 + torch.rand(K, 1, 1, generator=torch.Generator().manual_seed(4)) * 1e-3).to(gpu)
    w[30] = torch.linspace(1.0, 1.1, K).reshape(K, 1, 1).to(gpu)
    a = torch.ones(cout, device=gpu)
    col_scale = (wscale * a).contiguous()
    orig = [t.clone() for t in (codes, km, wscale, col_scale)]
    chans, bits = [3, 9, 20, 30, 60], [6, 4, 8, 4, 2]
    save = torch.zeros(ops.trial_rows_save_bytes(1, K, 5), dtype=torch.int8, device=gpu)
    status = torch.zeros(5, dtype=torch.int32, device=gpu)
    ops.trial_rows_patch_x8(w, chans, bits, a, codes, None, wscale, col_scale, save, status, km=km)
    got = status.tolist()
    assert got[1:4] == [1, 3, 4] and all(v in (0, 4) for v in (got[0], got[4])), got
    kmr = km.view(1, K // 64, cout, 64)
    for c, word in zip(chans, got):
        same = torch.equal(codes[0, c], orig[0][0, c]) and torch.equal(kmr[0, :, c], orig[1][0, :, c]) \
            and wscale[c] == orig[2][c] and col_scale[c] == orig[3][c]
        assert same == (word != 0 or bits[chans.index(c)] == 8), (c, word)
    ops.trial_rows_restore_x8(chans, codes, None, wscale, col_scale, save, km=km)
    for t, o in zip((codes, km, wscale, col_scale), orig):
        assert _bytes_equal(t, o)
    status.zero_()
    off0 = offset.clone()
    ops.trial_rows_patch_x8(w, [30], [4], a, codes, offset, wscale, col_scale, save, status, km=km)
    assert status.tolist()[0] == 0 and int(offset[30]) == 150 + 128  # with an offset tensor the row is coded
    ops.trial_rows_restore_x8([30], codes, offset, wscale, col_scale, save, km=km)
    for t, o in zip((codes, km, offset, wscale, col_scale), orig[:2] + [off0] + orig[2:]):
        assert _bytes_equal(t, o)


# ---- trials against a really quantized model ------------------------------------------------------
def _operands(net):
    """test_gpu_sensitivity._operands plus the exact8 operands' offsets."""
    from smpq.qconv import QConv2d
    out = {}
    for name, m in net.named_modules():
        if isinstance(m, QConv2d) and m._pack is not None and m._pack[1] is not None:
            codes, _, offset, wscale, _ = m._pack[1]
            ts = [codes, wscale]
            for t in (getattr(codes, "_smpq_km", None), offset):
                if t is not None:
                    ts.append(t)
            if getattr(m, "_fold_cache", None) is not None:
                ts += [m._fold_cache[1].col_scale, m._fold_cache[1].col_shift]
            out[name] = ts
    return out


def _check_session_trials(gpu, arch, assign, cal_case, batches, semilayers, route, graph, limbs):
    import functions
    from smpq import engine, search
    _set(graph, limbs)
    net = build_model(gpu, arch, assign, cal_case)
    ref = build_model(gpu, arch, assign, cal_case)
    standing = {k: v.detach().clone() for k, v in net.state_dict().items()}
    acc0, loss0, outs0 = functions.evaluate_acc_loss_softmax(net, gpu, batches)
    refs = [p.clone() for p in outs0]
    with search.Session(net, batches, reference_outputs=refs, boundaries=()) as s:
        cal = engine.model_state(net).ranges
        ops_before = _operands(net)
        copies = {k: [t.clone() for t in ts] for k, ts in ops_before.items()}
        entries = dict(engine.model_state(net).graphs.entries)
        assert (s.base.acc, s.base.loss, s.base.kl) == (acc0, loss0, 0.0)
        rows = 0
        for i, (lnum, channels, bit) in enumerate(semilayers):
            channels = list(channels)
            r = s.trial(lnum, channels, bit)
            assert r.route == route and r.resumed_from is None, (i, lnum, r)
            want_st, want_kl = _reference_stats(ref, standing, net, cal, lnum, channels, [bit] * len(channels), batches, refs)
            assert r.stats == want_st, (i, lnum, r.stats, want_st)
            assert r.kl_stats == want_kl, (i, lnum, r.kl_stats, want_kl)
            assert r.loss == want_st[0] / want_st[3] and r.acc == want_st[1] / want_st[2]
            assert r.kl == want_kl[0] / want_kl[1] and r.kl > 0
            assert r.param == len(channels) * net_row_elems(net, lnum) * ((32 - bit) / 32)
            rows += len(channels)
        rep = s.report()
        assert rep["trials"] == {route: len(semilayers)} and rep["rows_patched"] == rows, rep
        assert rep["rebases"] == {"construction": 1} and not rep["constant"], rep
        assert rep["patched_trials"] == ZERO and rep["boundaries"] == [], rep
        # what the trials left behind: the model, the operands (the same tensors, equal bytes), ranges, graphs
        for k, v in net.state_dict().items():
            assert torch.equal(v, standing[k]), k
        now = _operands(net)
        assert now.keys() == ops_before.keys() and len(now) >= 17
        for k, ts in now.items():
            assert len(ts) == len(copies[k])
            for t, t0, c in zip(ts, ops_before[k], copies[k]):
                assert t is t0 and _bytes_equal(t, c), k
        st = engine.model_state(net)
        assert st.ranges is cal
        assert st.graphs.entries.keys() == entries.keys() and all(st.graphs.entries[k] is v for k, v in entries.items())


def net_row_elems(net, lnum):
    from smpq import assignments
    return assignments.conv_for_lnum(net, lnum).weight[0].numel()


GRAPH_LIMBS = [(True, 3), (True, 2), (False, 3), (False, 2)]


@pytest.mark.parametrize("graph,limbs", GRAPH_LIMBS)
def test_trials_equal_a_quantized_model_resnet18_pristine(gpu, knobs, graph, limbs):  # noqa: F811
    _, dev = _batches(gpu)
    semilayers = [(1, range(0, 64, 2), 8), (8, [5, 127, 64], 4), (16, range(0, 511), 2), (16, [511], 4)]
    _check_session_trials(gpu, "resnet18", None, "r18_u8_cal", dev, semilayers, "patched", graph, limbs)


@pytest.mark.parametrize("graph,limbs", GRAPH_LIMBS)
def test_trials_equal_a_quantized_model_resnet18_exact8(gpu, knobs, graph, limbs):  # noqa: F811
    # every searched conv fully quantized at 8 bits: one weight limb, offsets
    _, dev = _batches(gpu)
    semilayers = [(8, [5, 127, 64], 4), (16, range(0, 512, 2), 6), (1, range(64), 4)]
    _check_session_trials(gpu, "resnet18", "r18_u8", "r18_u8_cal", dev, semilayers, "patched_x8", graph, limbs)


@pytest.mark.parametrize("graph,limbs", GRAPH_LIMBS)
def test_trials_equal_a_quantized_model_resnet50_exact8(gpu, knobs, graph, limbs):  # noqa: F811
    # lnum 5, 6: layer 1, whose chained conv3 + conv1 launches read these operands; 47, 48: the last block
    _, dev = _batches(gpu, n=4)
    cout = {5: 64, 6: 256, 47: 512, 48: 2048}
    semilayers = [(ln, range(ln % 2, c, 2), 4) for ln, c in cout.items()]
    _check_session_trials(gpu, "resnet50", "r50_mixed", "r50_mixed_cal", dev, semilayers, "patched_x8", graph, limbs)


# ---- accept -----------------------------------------------------------------------------------------
def test_accept_commits_and_rebases(gpu, knobs):  # noqa: F811
    import functions
    from smpq import assignments, search
    _set(True, 3)
    host, dev = _batches(gpu)
    net = build_model(gpu, "resnet18", None, "r18_u8_cal")
    net2 = build_model(gpu, "resnet18", None, "r18_u8_cal")
    original = [p.clone() for p in functions.evaluate_acc_loss_softmax(net2, gpu, host)[2]]
    conv, conv2 = assignments.conv_for_lnum(net, 3), assignments.conv_for_lnum(net2, 3)
    most = list(range(63))
    with search.Session(net, dev, reference_outputs=original) as s:
        with pytest.raises(RuntimeError):
            s.accept()
        assert s.trial(3, most, 8).route == "patched"
        official = s.accept()
        assert official is s.base and conv._bits_host.tolist() == [8] * 63 + [0]
        for c in most:
            conv2.weight.data = functions.channel_wise_quantizationperchan(conv2.weight.data, 8, c)
        acc, loss, outs = functions.evaluate_acc_loss_softmax(net2, gpu, host)
        sd2 = net2.state_dict()
        accepted = {k: v.detach().clone() for k, v in net.state_dict().items()}
        assert accepted.keys() == sd2.keys() and all(torch.equal(v, sd2[k]) for k, v in accepted.items())
        assert (official.acc, official.loss, official.kl) == (acc, loss, functions.KLdiv(original, outs))
        with pytest.raises(RuntimeError):
            s.accept()  # that trial is spent
        # the trial that completes the accepted conv cannot be patched: the public route, the model restored
        r = s.trial(3, [63], 8)
        assert r.route == "slow:not_patchable" and r.stats is None and r.resumed_from is None
        conv2.weight.data = functions.channel_wise_quantizationperchan(conv2.weight.data, 8, 63)
        acc, loss, outs = functions.evaluate_acc_loss_softmax(net2, gpu, host)
        assert (r.acc, r.loss, r.kl) == (acc, loss, functions.KLdiv(original, outs))
        for k, v in net.state_dict().items():
            assert torch.equal(v, accepted[k]), k
        assert conv._bits_host.tolist() == [8] * 63 + [0] and not s.stores()
        assert s.report()["rebases"] == {"construction": 1, "accept": 1}
        r = s.trial(4, [1, 2], 4)
        assert r.route == "patched" and r.resumed_from is None and np.isfinite(r.stats).all()
        rep = s.report()
        assert rep["rebases"] == {"construction": 1, "accept": 1, "slow": 1}  # exactly one more
        assert rep["trials"] == {"patched": 2, "slow:not_patchable": 1} and rep["patched_trials"] == ZERO
        assert (s.base.acc, s.base.loss, s.base.kl) == (official.acc, official.loss, official.kl)
        # accepting the slow trial's conv turns it exact8: its next trial takes the new patch
        assert s.trial(3, [63], 8).route == "slow:not_patchable"
        s.accept()
        assert conv.fully_quantized() and s.trial(3, [0, 63], 4).route == "patched_x8"


# ---- boundaries ---------------------------------------------------------------------------------------
# a trial in the block before, at and after each default boundary (layer3.0, layer4.0), and the last block
BOUNDARY_TRIALS = {"resnet18": [(8, None), (9, "layer3.0"), (12, "layer3.0"), (13, "layer4.0"), (16, "layer4.0")],
                   "resnet50": [(21, None), (22, "layer3.0"), (39, "layer3.0"), (40, "layer4.0"), (48, "layer4.0")]}
_REPLAYED = {}


def _boundary_net(gpu, arch):
    return build_model(gpu, arch, None, {"resnet18": "r18_u8_cal", "resnet50": "r50_mixed_cal"}[arch])


def _replayed(gpu, arch, dev):
    """The same trials of a session without boundaries, computed once and shared (never written to)."""
    from smpq import search
    if arch not in _REPLAYED:
        with search.Session(_boundary_net(gpu, arch), dev, boundaries=()) as s:
            _REPLAYED[arch] = [(r.stats, r.kl_stats) for r in (s.trial(ln, [0, 3], 4) for ln, _ in BOUNDARY_TRIALS[arch])]
            assert s.report()["trials"] == {"patched": 5}
    return _REPLAYED[arch]


def _launches_per_forward(net, j, n):
    from smpq import assignments, suffix
    from smpq.qconv import QConv2d
    blocks = assignments.blocks_of(net)
    return sum(isinstance(m, QConv2d) for b in blocks[j:] for m in b.modules()) * len(suffix.slices(n))


@pytest.mark.parametrize("arch,n", [("resnet18", 8), ("resnet50", 4)])
def test_default_boundaries_equal_the_replay_route(gpu, knobs, arch, n):  # noqa: F811
    from smpq import prefix, search, suffix
    _set(True, 3)
    _, dev = _batches(gpu, n=n)
    want = _replayed(gpu, arch, dev)
    net = _boundary_net(gpu, arch)
    s = search.Session(net, dev)
    j3, j4 = prefix.block_index(net, "layer3.0"), prefix.block_index(net, "layer4.0")
    stores = s.stores()
    assert sorted(stores) == [j3, j4] and all(st.kept == 2 and st.complete for st in stores.values())
    rows = {row["name"]: row for row in s.report()["boundaries"]}
    assert list(rows) == ["layer4.0", "layer3.0"]  # deepest first
    for name, j in (("layer3.0", j3), ("layer4.0", j4)):
        row = rows[name]
        assert row["resumable"] and row["self_check"] is True and (row["kept"], row["full"]) == (2, 0), row
        assert row["bytes"] == 2 * suffix.kept_bytes(net, dev[0][0], j)
        assert row["self_check_conv_launches"] == 2 * _launches_per_forward(net, j, n)
    resumed = {"layer3.0": 0, "layer4.0": 0}
    for (lnum, name), (st, kl) in zip(BOUNDARY_TRIALS[arch], want):
        r = s.trial(lnum, [0, 3], 4)
        assert r.route == "patched" and r.resumed_from == name, (lnum, r)
        assert r.stats == st and r.kl_stats == kl, (lnum, r.stats, st, r.kl_stats, kl)
        if name:
            resumed[name] += 2
    rep = s.report()
    assert rep["patched_trials"] == ZERO and rep["rebases"] == {"construction": 1}
    for row in rep["boundaries"]:
        j = prefix.block_index(net, row["name"])
        assert row["resumed_forwards"] == resumed[row["name"]] == 4
        assert row["resumed_conv_launches"] == 4 * _launches_per_forward(net, j, n)
    s.close()
    assert not s.stores() and all(st.entries == [] and st.bytes == 0 for st in stores.values())


def test_boundary_budget(gpu, knobs):  # noqa: F811
    from smpq import prefix, search, suffix
    _set(True, 3)
    _, dev = _batches(gpu)
    want = _replayed(gpu, "resnet18", dev)
    net = _boundary_net(gpu, "resnet18")
    j4 = prefix.block_index(net, "layer4.0")
    one = suffix.kept_bytes(net, dev[0][0], j4)  # layer3.0's batch is twice that
    with search.Session(net, dev, boundary_bytes=2 * one) as s:  # admits only layer4.0
        assert sorted(s.stores()) == [j4] and s.stores()[j4].kept == 2 and s.stores()[j4].bytes == 2 * one
        rows = {row["name"]: row for row in s.report()["boundaries"]}
        assert (rows["layer3.0"]["kept"], rows["layer3.0"]["full"], rows["layer3.0"]["self_check"]) == (0, 2, None)
        for (lnum, name), (st, kl) in zip(BOUNDARY_TRIALS["resnet18"], want):
            r = s.trial(lnum, [0, 3], 4)
            assert r.resumed_from == (name if name == "layer4.0" else None) and r.stats == st and r.kl_stats == kl, lnum
    net = _boundary_net(gpu, "resnet18")
    with search.Session(net, dev, boundary_bytes=one) as s:  # one batch: the second batch replays
        st4 = s.stores()[j4]
        assert sorted(s.stores()) == [j4] and [e is not None for e in st4.entries] == [True, False]
        lnum, _ = BOUNDARY_TRIALS["resnet18"][-1]
        r = s.trial(lnum, [0, 3], 4)
        assert r.resumed_from == "layer4.0" and (r.stats, r.kl_stats) == want[-1]
        (row,) = [row for row in s.report()["boundaries"] if row["name"] == "layer4.0"]
        assert (row["kept"], row["full"], row["resumed_forwards"]) == (1, 1, 1)


def test_an_exception_inside_a_trial_empties_the_stores(gpu, knobs, monkeypatch):  # noqa: F811
    from smpq import assignments, search, suffix
    _set(True, 3)
    _, dev = _batches(gpu)
    want = _replayed(gpu, "resnet18", dev)
    net = _boundary_net(gpu, "resnet18")
    s = search.Session(net, dev)
    stores = list(s.stores().values())
    conv = assignments.conv_for_lnum(net, 16)
    before = {k: [t.clone() for t in ts] for k, ts in _operands(net).items()}
    gen = conv._content_gen
    real, calls = suffix.resume, []

    def resume(*a, **kw):
        calls.append(1)
        if len(calls) == 2:  # the trial's second batch
            raise RuntimeError("injected")
        return real(*a, **kw)

    monkeypatch.setattr(suffix, "resume", resume)
    with pytest.raises(RuntimeError, match="injected"):
        s.trial(16, [0, 3], 4)
    torch.cuda.synchronize()
    assert not s.stores() and all(st.entries == [] and st.bytes == 0 for st in stores)
    now = _operands(net)
    for k, ts in now.items():  # the rows' restore ran
        for t, c in zip(ts, before[k]):
            assert _bytes_equal(t, c), k
    assert conv._content_gen == gen + 1  # and the conv is marked for repacking
    monkeypatch.setattr(suffix, "resume", real)
    r = s.trial(16, [0, 3], 4)  # after one more rebase the session goes on
    assert r.resumed_from == "layer4.0" and (r.stats, r.kl_stats) == want[-1]
    assert s.report()["rebases"] == {"construction": 1, "exception": 1}
    s.close()
