"""smpq.sensitivity on the GPU: the trial row patch kernel against the normal quantize + pack + fold
path (bitwise), a sweep's trials against a really quantized model under the same ranges (bitwise),
what a sweep leaves behind, the slow path, and the deltas against the CPU oracle."""
import types

import numpy as np
import pytest
import torch

from test_gpu import build_model

pytestmark = pytest.mark.gpu

IMG_SEED = 77
LABEL_SEED = 182  # chosen on the CPU with ORACLE_CHANNELS (test_deltas_against_the_oracle)


def _batches(gpu, n=8, count=2, hw=224, seed=IMG_SEED, label_seed=LABEL_SEED):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(n, 3, hw, hw, generator=g) for _ in range(count)]
    ys = torch.randint(0, 1000, (n * count,), generator=torch.Generator().manual_seed(label_seed))
    host = [(x, ys[i * n:(i + 1) * n].clone()) for i, x in enumerate(xs)]
    return host, [(x.to(gpu), y.to(gpu)) for x, y in host]


@pytest.fixture
def knobs():
    """Range mode, graph switch and limb count as they were, whatever a test sets."""
    from smpq import engine, ops
    saved = engine.get_range_mode(), engine.USE_GRAPH[0], ops.get_act_limbs()
    engine.set_range_mode("static")
    yield
    engine.set_range_mode(saved[0])
    engine.USE_GRAPH[0] = saved[1]
    ops.set_act_limbs(saved[2])


# ---- the kernel against the normal path -----------------------------------------------------------
@pytest.mark.parametrize("lw", [2, 3])
@pytest.mark.parametrize("shape", [(64, 64, 1, 1), (64, 64, 3, 3), (128, 256, 1, 1)])
def test_patch_kernel_matches_quantize_pack_fold(gpu, shape, lw):
    """K = 64 (one K-major group), K = 576 (tap-major order), 128 x 256 (more rows than a group):
    after the patch the whole operand equals quantize_channels_ on a clone + pack_weights_ex with
    that step + _fold; after the restore it equals the original; the save area's guards hold."""
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
    codes, _, wscale, _ = ops.pack_weights_ex(w, torch.zeros(cout, device=gpu), lw)
    km = codes._smpq_km
    col_scale, _ = engine._fold(conv, bn, wscale)
    orig = [t.clone() for t in (codes, km, wscale, col_scale)]
    size = ops.trial_save_bytes(lw, K)
    buf = torch.full((size + 64,), 0x5A, dtype=torch.int8, device=gpu)
    save = buf[32:32 + size]
    for bit in (8, 6, 4, 2):
        for sem in ("cpu", "device"):
            for c in (0, cout - 1):
                w2 = w.clone()
                bits = np.zeros(cout, dtype=np.int64)
                bits[c] = bit
                step = ops.quantize_channels_(w2.view(cout, -1), bits, semantics=sem)
                e_codes, _, e_ws, _ = ops.pack_weights_ex(w2, step, lw)
                e_cs, _ = engine._fold(conv, bn, e_ws)
                status = torch.zeros(1, dtype=torch.int32, device=gpu)
                ops.trial_row_patch(w, c, bit, a, codes, wscale, col_scale, save, status, km=km, semantics=sem)
                what = (bit, sem, c)
                assert int(status) == 0
                assert torch.equal(codes, e_codes), what
                assert torch.equal(km, e_codes._smpq_km), what
                assert torch.equal(wscale.view(torch.int32), e_ws.view(torch.int32)), what
                assert torch.equal(col_scale.view(torch.int32), e_cs.view(torch.int32)), what
                ops.trial_row_restore(c, codes, wscale, col_scale, save, km=km)
                for t, o in zip((codes, km, wscale, col_scale), orig):
                    assert torch.equal(t.view(torch.int8), o.view(torch.int8)), what
                assert bool((buf[:32] == 0x5A).all()) and bool((buf[32 + size:] == 0x5A).all()), what


def test_patch_kernel_constant_row(gpu):
    from smpq import ops
    w = torch.randn(64, 64, 1, 1, generator=torch.Generator().manual_seed(6)).to(gpu)
    w[9] = -0.5
    codes, _, wscale, _ = ops.pack_weights_ex(w, torch.zeros(64, device=gpu), 2)
    km = codes._smpq_km
    a = torch.ones(64, device=gpu)
    col_scale = (wscale * a).contiguous()
    orig = [t.clone() for t in (codes, km, wscale, col_scale)]
    save = torch.zeros(ops.trial_save_bytes(2, 64), dtype=torch.int8, device=gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    ops.trial_row_patch(w, 9, 4, a, codes, wscale, col_scale, save, status, km=km)
    assert int(status) == 1
    ops.trial_row_restore(9, codes, wscale, col_scale, save, km=km)
    for t, o in zip((codes, km, wscale, col_scale), orig):
        assert torch.equal(t, o)


# ---- a trial against a really quantized model ------------------------------------------------------
def _reference_stats(ref, pristine, base, cal, lnum, c, bit, batches):
    """The statistics of ``ref`` (a second model holding ``pristine``) with channel ``c`` of conv
    ``lnum`` really quantized, forwarded eagerly under the ranges of ``base``'s calibration."""
    import functions
    from smpq import assignments, engine, ops, quant
    ref.load_state_dict(pristine)
    conv = assignments.conv_for_lnum(ref, lnum)
    functions.channel_wise_quantizationperchan(conv.weight.data, bit, c)
    quant.check_pending()
    assert int(conv.qbits[c]) == bit
    with torch.no_grad():
        cm = engine.calibration_maxima(ref, batches[0][0])
        maxima = [cal.by_conv[id(m)] / engine.HEADROOM for m in base.modules() if id(m) in cal.by_conv]
        assert len(maxima) == len(cm.keys)
        cm.maxima = torch.tensor(maxima, dtype=torch.float32, device=cm.maxima.device)
        engine.set_calibration(ref, cm, widen=False)
        rr = engine.model_state(ref).ranges
        assert list(rr.by_conv.values()) == [cal.by_conv[id(m)] for m in base.modules() if id(m) in cal.by_conv]
        st = torch.zeros(4, dtype=torch.float64, device=batches[0][0].device)
        for x, y in batches:
            logits, ovf = engine._static_eager(ref, x, rr)
            assert ovf.tolist() == [0, 0]
            ops.softmax_xent(logits, y, st, want_probs=False)
    return st.tolist()


def _check_trials(gpu, arch, cal_case, batches, channels, picks, bits, graph, limbs):
    from smpq import engine, ops, sensitivity
    engine.USE_GRAPH[0] = graph
    ops.set_act_limbs(limbs)
    net = build_model(gpu, arch, None, cal_case)
    ref = build_model(gpu, arch, None, cal_case)
    pristine = {k: v.detach().clone() for k, v in net.state_dict().items()}
    table = sensitivity.delta_loss_table(net, batches, bits=bits, lnums=sorted(channels), channels=channels)
    rep = table.report()
    assert rep["patched"] == rep["trials"] and not rep["slow"] and not rep["constant"], rep
    assert rep["during_trials"] == {"calibrations": 0, "graph_captures": 0, "repack": 0}, rep
    cal = engine.model_state(net).ranges
    cols = {(int(l), int(c)): i for i, (l, c) in enumerate(zip(table.lnum, table.cnum))}
    for lnum, c, bit in picks:
        want = _reference_stats(ref, pristine, net, cal, lnum, c, bit, batches)
        got = table.stats[bit][cols[(lnum, c)]].tolist()
        assert got == want, (lnum, c, bit, got, want)
        assert table.delta[bit][cols[(lnum, c)]] == got[0] / got[3] - table.base_loss
    for k, v in net.state_dict().items():
        assert torch.equal(v, pristine[k]), k


@pytest.mark.parametrize("graph,limbs", [(True, 3), (True, 2), (False, 3), (False, 2)])
def test_trials_equal_a_quantized_model_resnet18(gpu, knobs, graph, limbs):
    _, dev = _batches(gpu)
    channels = {1: [0, 63], 8: [5, 127], 16: [0, 511]}
    picks = [(1, 0, 8), (1, 63, 2), (8, 5, 4), (8, 127, 8), (16, 0, 2), (16, 511, 4)]
    _check_trials(gpu, "resnet18", "r18_u8_cal", dev, channels, picks, (8, 4, 2), graph, limbs)


@pytest.mark.parametrize("graph,limbs", [(True, 3), (True, 2), (False, 3), (False, 2)])
def test_trials_equal_a_quantized_model_resnet50(gpu, knobs, graph, limbs):
    # a conv1, a conv2 and a conv3 of layer 1 (block 1: lnum 4..6) and of layer 4 (block 15: 46..48)
    _, dev = _batches(gpu, n=4)
    channels = {4: [0], 5: [63], 6: [255], 46: [511], 47: [0], 48: [2047]}
    picks = [(ln, cs[0], 4) for ln, cs in channels.items()]
    _check_trials(gpu, "resnet50", "r50_mixed_cal", dev, channels, picks, (4,), graph, limbs)


# ---- what a sweep leaves behind -----------------------------------------------------------------------
def _operands(net):
    from smpq.qconv import QConv2d
    out = {}
    for name, m in net.named_modules():
        if isinstance(m, QConv2d) and m._pack is not None and m._pack[1] is not None:
            codes, _, _, wscale, _ = m._pack[1]
            ts = [codes, wscale]
            if getattr(codes, "_smpq_km", None) is not None:
                ts.append(codes._smpq_km)
            if getattr(m, "_fold_cache", None) is not None:
                ts += [m._fold_cache[1].col_scale, m._fold_cache[1].col_shift]
            out[name] = ts
    return out


def test_sweep_moves_nothing_else(gpu, knobs):
    import functions
    from smpq import engine, sensitivity, stats
    host, dev = _batches(gpu)
    net = build_model(gpu, "resnet18", None, "r18_u8_cal")
    loss_before = functions.evaluate_loss(net, gpu, host)
    sensitivity.delta_loss_table(net, dev, bits=(4,), lnums=[1], channels=[0])  # graphs for dev's addresses
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ops_before = _operands(net)
    assert len(ops_before) >= 17
    copies = {k: [t.clone() for t in ts] for k, ts in ops_before.items()}
    st = engine.model_state(net)
    ranges, entries = st.ranges, dict(st.graphs.entries)
    assert ranges is not None and entries
    counters = {k: stats[k] for k in ("calibrations", "graph_captures", "repack")}
    table = sensitivity.delta_loss_table(net, dev, bits=(8, 2), lnums=[2, 15], channels=[3, 60])
    rep = table.report()
    assert rep["trials"] == 8 and rep["patched"] == 8 and not rep["slow"], rep
    assert rep["during_trials"] == {"calibrations": 0, "graph_captures": 0, "repack": 0}, rep
    # the baseline's share: its one calibration; the graphs and operands were there already
    assert {k: stats[k] - counters[k] for k in counters} == {"calibrations": 1, "graph_captures": 0, "repack": 0}
    assert rep["baseline"] == {"calibrations": 1, "graph_captures": 0, "repack": 0}, rep
    assert np.isfinite(table.delta[8]).all() and np.isfinite(table.delta[2]).all()
    assert (table.delta[2] != 0).any()
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    now = _operands(net)
    assert now.keys() == ops_before.keys()
    for k, ts in now.items():
        for t, t0, c in zip(ts, ops_before[k], copies[k]):
            assert t is t0 and torch.equal(t, c), k
    st = engine.model_state(net)
    assert st.ranges is ranges
    assert st.graphs.entries.keys() == entries.keys() and all(st.graphs.entries[k] is v for k, v in entries.items())
    assert functions.evaluate_loss(net, gpu, host) == loss_before


# ---- the slow path -----------------------------------------------------------------------------------
def test_slow_path_for_a_fully_quantized_conv(gpu, knobs):
    import functions
    from smpq import assignments, quant, sensitivity
    host, dev = _batches(gpu)
    net = build_model(gpu, "resnet18", None, "r18_u8_cal")
    conv = assignments.conv_for_lnum(net, 3)
    quant.quantize_layer_(conv, np.full(conv.out_channels, 8))
    assert not sensitivity.patchable(conv, sensitivity.bn_for(net, conv))
    assert sensitivity.patchable(assignments.conv_for_lnum(net, 4), net.layer1[1].bn2)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    table = sensitivity.delta_loss_table(net, dev, bits=(4,), lnums=[3], channels=[0, 5])
    rep = table.report()
    assert rep["trials"] == 2 and rep["patched"] == 0 and rep["slow"] == {"not_patchable": 2}, rep
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert (conv._bits_host == 8).all()
    # the same trial by hand through the public API
    base = functions.evaluate_loss(net, gpu, host)
    assert base == table.eval_loss
    functions.channel_wise_quantizationperchan(conv.weight.data, 4, 5)
    loss = functions.evaluate_loss(net, gpu, host)
    net.load_state_dict(sd)
    assert table.delta[4][1] == loss - base


# ---- against the CPU oracle ---------------------------------------------------------------------------
# 2-bit trials of 12 fixed channels of lnum 15 / 16 (layer4.1 conv1 / conv2), chosen on the CPU
# together with LABEL_SEED so that several oracle deltas clear ten times the bound below.
ORACLE_CHANNELS = {15: [12, 53, 94, 232, 302, 325, 331], 16: [109, 158, 213, 291, 510]}


def test_deltas_against_the_oracle(gpu, knobs):
    """|delta_gpu - delta_oracle| <= 8e-4 * max|logit|: the project's parity bound is a logit error of
    at most 2e-4 * max|logit| on a forward, which moves a batch-mean cross entropy by at most twice
    that (|d lse| <= max|d logit| and |d logit_label| <= max|d logit|), and a delta is the difference
    of two such losses. Only trials whose oracle |delta| is at least ten times the bound are
    compared (at least 3 must be), and their signs must agree."""
    import torch.nn.functional as F
    from oracle import torch_ref
    from smpq import engine, ops, sensitivity
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)  # the parity mode the bound is stated for
    host, dev = _batches(gpu)
    net = build_model(gpu, "resnet18", None, "r18_u8_cal")
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    x = torch.cat([x for x, _ in host])

    def loss_of(logits):
        l = logits.double()
        return float(sum(F.cross_entropy(l[i * 8:(i + 1) * 8], y) for i, (_, y) in enumerate(host)) / len(host))

    base_logits = torch_ref.resnet_forward("resnet18", sd, x)
    bound = 8e-4 * float(base_logits.abs().max())
    base = loss_of(base_logits)
    want = {}
    for ln, name in ((15, "layer4.1.conv1.weight"), (16, "layer4.1.conv2.weight")):
        for c in ORACLE_CHANNELS[ln]:
            w = sd[name].clone()
            ops.quantize_channels_(w[c].reshape(1, -1), [2], semantics="device")  # what the GPU quantizer rounds to
            want[(ln, c)] = loss_of(torch_ref.resnet_forward("resnet18", dict(sd, **{name: w}), x)) - base
    assert len(want) == 12
    table = sensitivity.delta_loss_table(net, dev, bits=(2,), lnums=[15, 16], channels=ORACLE_CHANNELS)
    assert table.report()["patched"] == 12
    compared = 0
    for i, (ln, c) in enumerate(zip(table.lnum.tolist(), table.cnum.tolist())):
        got, ref = float(table.delta[2][i]), want[(ln, c)]
        print("lnum %d channel %d: gpu %.6e oracle %.6e diff %.2e (bound %.2e)" % (ln, c, got, ref, abs(got - ref), bound))
        if abs(ref) >= 10 * bound:
            compared += 1
            assert abs(got - ref) <= bound, (ln, c, got, ref, bound)
            assert (got > 0) == (ref > 0), (ln, c, got, ref)
    assert compared >= 3, "only %d of the 12 oracle deltas reach ten times the bound" % compared


# ---- one trial, three callers ----------------------------------------------------------------------------
@pytest.mark.parametrize("resumed", [False, True])
def test_the_three_callers_run_the_same_trial(gpu, knobs, resumed):
    """The tables and the session share one trial loop (trials.guarded_trial, suffix.score_pass), so
    the same channel at the same bit-width gives the same four statistics, as float64 bits, whether
    it is a delta_loss_table column, a one-channel semilayer of semilayer_table or a Session trial:
    a first conv, a mid conv and the last conv of a block at suffix.first_block, by replay
    (``resumed`` off) and resumed (the delta-loss side with the rows route, which that last conv
    takes). The model and its packed operands are left bitwise as they were."""
    from smpq import engine, ops, search, sensitivity, suffix
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)
    _, dev = _batches(gpu, n=4)
    net = build_model(gpu, "resnet18", None, "r18_u8_cal")
    last = 2 * (suffix.first_block(net) + 1)  # conv2 of the first resumed BasicBlock
    picks = [(1, 7), (8, 100), (last, 33)]
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    sensitivity.ordinary_loss(net, dev)  # packs every operand
    ops_before = _operands(net)
    copies = {k: [t.clone() for t in ts] for k, ts in ops_before.items()}
    assert len(ops_before) >= 17

    delta = sensitivity.delta_loss_table(net, dev, bits=(4,), lnums=[ln for ln, _ in picks],
                                         channels={ln: [c] for ln, c in picks}, suffix=resumed, rows=resumed)
    semi = sensitivity.semilayer_table(net, dev, [(ln, [c], 4) for ln, c in picks], suffix=resumed)
    with search.Session(net, dev, boundaries=None if resumed else ()) as s:
        results = [s.trial(ln, [c], 4) for ln, c in picks]
    assert delta.report()["patched"] == 3 and semi.report()["patched"] == 3
    assert [r.route for r in results] == ["patched"] * 3
    if resumed:
        blocks = {b["block"]: b for b in delta.report()["suffix"]["blocks"]}
        assert blocks[last // 2 - 1]["rows"] == "used" and blocks[last // 2 - 1]["rows_trials"] == 1
        assert semi.report()["suffix"]["resumed_forwards"] > 0 and results[2].resumed_from is not None
    for i, (ln, c) in enumerate(picks):
        assert (int(delta.lnum[i]), int(delta.cnum[i]), int(semi.lnum[i])) == (ln, c, ln)
        a = np.asarray(delta.stats[4][i], dtype=np.float64).tobytes()
        b = np.asarray(semi.stats[i], dtype=np.float64).tobytes()
        d = np.asarray(results[i].stats, dtype=np.float64).tobytes()
        print("lnum %d channel %d: %r %r %r" % (ln, c, delta.stats[4][i].tolist(), semi.stats[i].tolist(), results[i].stats))
        assert a == b == d, (ln, c)
        assert not np.isnan(delta.stats[4][i]).any()
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    now = _operands(net)
    assert now.keys() == ops_before.keys()
    for k, ts in now.items():
        for t, t0, cp in zip(ts, ops_before[k], copies[k]):
            assert t is t0 and torch.equal(t, cp), k
