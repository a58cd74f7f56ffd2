"""Semilayer trials on the GPU (smpq.sensitivity.semilayer_table): the n-row patch kernel against the
normal quantize + pack + fold path (bitwise), trials against a really quantized model under the same
ranges (bitwise), what a table leaves behind, the slow path, the CPU oracle, and the
SMPQ_PATCHED_SEMILAYERS route of functions.make_semilayers_resnet18."""
import types

import numpy as np
import pytest
import torch

from test_gpu import build_model
from test_gpu_sensitivity import _batches, _operands, knobs  # noqa: F401  (knobs: a fixture)

pytestmark = pytest.mark.gpu

GUARD = 64


def _mixed_bits(n):
    return [(8, 6, 4, 2)[i % 4] for i in range(n)]


# ---- the kernel against the normal path -----------------------------------------------------------
@pytest.mark.parametrize("lw", [2, 3])
@pytest.mark.parametrize("shape", [(64, 64, 1, 1), (64, 64, 3, 3), (128, 256, 1, 1), (64, 512, 3, 3)])
def test_rows_kernel_matches_quantize_pack_fold(gpu, shape, lw):
    """One row, three unsorted rows with the first and the last channel, and all rows but one (more
    workgroups than a K-major group has rows; K = 4608 is the row limit): after the patch the whole
    operand equals quantize_channels_ on a clone + pack_weights_ex with that step + _fold; after the
    restore it equals the original; the guards around the save area and the status words hold."""
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
    for chans in ([0], [cout - 1, 0, 5], [c for c in reversed(range(cout)) if c != 3]):
        n = len(chans)
        rbits = _mixed_bits(n)
        size = ops.trial_rows_save_bytes(lw, K, n)
        buf = torch.full((size + 2 * GUARD,), 0x5A, dtype=torch.int8, device=gpu)
        save = buf[GUARD:GUARD + size]
        sbuf = torch.full((n + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        status = sbuf[GUARD:GUARD + n]
        for sem in ("cpu", "device"):
            what = (n, sem)
            w2 = w.clone()
            bits = np.zeros(cout, dtype=np.int64)
            bits[chans] = rbits
            step = ops.quantize_channels_(w2.view(cout, -1), bits, semantics=sem)
            e_codes, _, e_ws, _ = ops.pack_weights_ex(w2, step, lw)
            e_cs, _ = engine._fold(conv, bn, e_ws)
            status.zero_()
            rows = ops.trial_rows_patch(w, chans, rbits, a, codes, wscale, col_scale, save, status, km=km, semantics=sem)
            assert status.tolist() == [0] * n, what
            assert torch.equal(codes, e_codes), what
            assert torch.equal(km, e_codes._smpq_km), what
            assert torch.equal(wscale.view(torch.int32), e_ws.view(torch.int32)), what
            assert torch.equal(col_scale.view(torch.int32), e_cs.view(torch.int32)), what
            ops.trial_rows_restore(rows, codes, wscale, col_scale, save, km=km)
            for t, o in zip((codes, km, wscale, col_scale), orig):
                assert torch.equal(t.view(torch.int8), o.view(torch.int8)), what
            assert bool((buf[:GUARD] == 0x5A).all()) and bool((buf[GUARD + size:] == 0x5A).all()), what
            assert bool((sbuf[:GUARD] == 0x5A5A5A5A).all()) and bool((sbuf[GUARD + n:] == 0x5A5A5A5A).all()), what


def test_rows_kernel_constant_row_in_the_middle(gpu):
    from smpq import ops
    w = torch.randn(64, 64, 1, 1, generator=torch.Generator().manual_seed(6)).to(gpu)
    w[9] = -0.5
    codes, _, wscale, _ = ops.pack_weights_ex(w, torch.zeros(64, device=gpu), 2)
    km = codes._smpq_km
    a = torch.ones(64, device=gpu)
    col_scale = (wscale * a).contiguous()
    orig = [t.clone() for t in (codes, km, wscale, col_scale)]
    # the other two rows, by the single-row kernel on a copy
    e = [t.clone() for t in orig]
    for c, b in ((3, 8), (60, 2)):
        ops.trial_row_patch(w, c, b, a, e[0], e[2], e[3], torch.zeros(ops.trial_save_bytes(2, 64), dtype=torch.int8, device=gpu),
                            torch.zeros(1, dtype=torch.int32, device=gpu), km=e[1])
    save = torch.zeros(ops.trial_rows_save_bytes(2, 64, 3), dtype=torch.int8, device=gpu)
    status = torch.zeros(3, dtype=torch.int32, device=gpu)
    ops.trial_rows_patch(w, [3, 9, 60], [8, 4, 2], a, codes, wscale, col_scale, save, status, km=km)
    assert status.tolist() == [0, 1, 0]
    for t, o in zip((codes, km, wscale, col_scale), e):  # row 9 as it was, the others patched
        assert torch.equal(t.view(torch.int8), o.view(torch.int8))
    assert not torch.equal(codes, orig[0])
    ops.trial_rows_restore([3, 9, 60], codes, wscale, col_scale, save, km=km)
    for t, o in zip((codes, km, wscale, col_scale), orig):
        assert torch.equal(t.view(torch.int8), o.view(torch.int8))


# ---- a trial against a really quantized model ------------------------------------------------------
def _reference_stats(ref, pristine, base, cal, lnum, channels, bits, batches, refs):
    """(stats, kl_stats) of ``ref`` (a second model holding ``pristine``) with ``channels`` of conv
    ``lnum`` really quantized one by one, forwarded eagerly under the ranges of ``base``'s
    calibration and scored with the trial's two ops against ``refs``."""
    import functions
    from smpq import assignments, engine, ops, quant
    ref.load_state_dict(pristine)
    conv = assignments.conv_for_lnum(ref, lnum)
    for c, b in zip(channels, bits):
        conv.weight.data = functions.channel_wise_quantizationperchan(conv.weight.data, b, c)
    quant.check_pending()
    assert [int(conv._bits_host[c]) for c in channels] == list(bits)
    with torch.no_grad():
        cm = engine.calibration_maxima(ref, batches[0][0])
        maxima = [cal.by_conv[id(m)] / engine.HEADROOM for m in base.modules() if id(m) in cal.by_conv]
        assert len(maxima) == len(cm.keys)
        cm.maxima = torch.tensor(maxima, dtype=torch.float32, device=cm.maxima.device)
        engine.set_calibration(ref, cm, widen=False)
        rr = engine.model_state(ref).ranges
        assert list(rr.by_conv.values()) == [cal.by_conv[id(m)] for m in base.modules() if id(m) in cal.by_conv]
        st = torch.zeros(4, dtype=torch.float64, device=batches[0][0].device)
        kl = torch.zeros(2, dtype=torch.float64, device=batches[0][0].device)
        for (x, y), r in zip(batches, refs):
            logits, ovf = engine._static_eager(ref, x, rr)
            assert ovf.tolist() == [0, 0]
            ops.kl_rows(r, ops.softmax_xent(logits.float().contiguous(), y, st, want_probs=True), kl)
    return st.tolist(), kl.tolist()


def _check_semilayers(gpu, arch, cal_case, batches, semilayers, graph, limbs):
    import functions
    from smpq import engine, ops, sensitivity
    engine.USE_GRAPH[0] = graph
    ops.set_act_limbs(limbs)
    net = build_model(gpu, arch, None, cal_case)
    ref = build_model(gpu, arch, None, cal_case)
    pristine = {k: v.detach().clone() for k, v in net.state_dict().items()}
    refs = [p.clone() for p in functions.evaluate_acc_loss_softmax(net, gpu, batches)[2]]
    table = sensitivity.semilayer_table(net, batches, semilayers, reference_outputs=refs)
    rep = table.report()
    assert rep["trials"] == rep["patched"] == len(semilayers) and not rep["slow"] and not rep["constant"], rep
    assert rep["during_trials"] == {"calibrations": 0, "graph_captures": 0, "repack": 0}, rep
    assert rep["rows_patched"] == sum(len(list(c)) for _, c, _ in semilayers)
    assert rep["max_rows"] == max(len(list(c)) for _, c, _ in semilayers)
    cal = engine.model_state(net).ranges
    for i, (lnum, channels, bit) in enumerate(semilayers):
        channels = list(channels)
        want_st, want_kl = _reference_stats(ref, pristine, net, cal, lnum, channels, [bit] * len(channels), batches, refs)
        assert table.stats[i].tolist() == want_st, (i, lnum, table.stats[i].tolist(), want_st)
        assert table.kl_stats[i].tolist() == want_kl, (i, lnum, table.kl_stats[i].tolist(), want_kl)
        assert table.loss[i] == want_st[0] / want_st[3] and table.acc[i] == want_st[1] / want_st[2]
        assert table.kl[i] == want_kl[0] / want_kl[1] and table.kl[i] > 0
        assert table.param[i] == len(channels) * _row_elems(net, lnum) * ((32 - bit) / 32)
    for k, v in net.state_dict().items():
        assert torch.equal(v, pristine[k]), k


def _row_elems(net, lnum):
    from smpq import assignments
    return assignments.conv_for_lnum(net, lnum).weight[0].numel()


@pytest.mark.parametrize("graph,limbs", [(True, 3), (True, 2), (False, 3), (False, 2)])
def test_semilayers_equal_a_quantized_model_resnet18(gpu, knobs, graph, limbs):  # noqa: F811
    _, dev = _batches(gpu)
    semilayers = [(1, range(0, 64, 2), 8), (8, [5, 127, 64], 4), (16, range(0, 511), 2), (16, [511], 4)]
    _check_semilayers(gpu, "resnet18", "r18_u8_cal", dev, semilayers, graph, limbs)


@pytest.mark.parametrize("graph,limbs", [(True, 3), (True, 2), (False, 3), (False, 2)])
def test_semilayers_equal_a_quantized_model_resnet50(gpu, knobs, graph, limbs):  # noqa: F811
    # a conv1, a conv2 and a conv3 of layer 1 (block 1: lnum 4..6) and of layer 4 (block 15: 46..48)
    _, dev = _batches(gpu, n=4)
    cout = {4: 64, 5: 64, 6: 256, 46: 512, 47: 512, 48: 2048}
    semilayers = [(ln, range(ln % 2, c, 2), 4) for ln, c in cout.items()]
    _check_semilayers(gpu, "resnet50", "r50_mixed_cal", dev, semilayers, graph, limbs)


# ---- what a table leaves behind -------------------------------------------------------------------------
def test_table_moves_nothing_else(gpu, knobs):  # noqa: F811
    import functions
    from smpq import engine, sensitivity, stats
    host, dev = _batches(gpu)
    net = build_model(gpu, "resnet18", None, "r18_u8_cal")
    loss_before = functions.evaluate_loss(net, gpu, host)
    sensitivity.semilayer_table(net, dev, [(1, [0], 4)])  # graphs for dev's addresses
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    ops_before = _operands(net)
    assert len(ops_before) >= 17
    copies = {k: [t.clone() for t in ts] for k, ts in ops_before.items()}
    st = engine.model_state(net)
    ranges, entries = st.ranges, dict(st.graphs.entries)
    assert ranges is not None and entries
    counters = {k: stats[k] for k in ("calibrations", "graph_captures", "repack")}
    table = sensitivity.semilayer_table(net, dev, [(2, range(0, 64, 2), 8), (15, range(1, 512, 2), 2),
                                                   (15, [3, 60], (8, 2)), (2, range(63), 4)])
    rep = table.report()
    assert rep["trials"] == 4 and rep["patched"] == 4 and not rep["slow"], rep
    assert rep["rows_patched"] == 32 + 256 + 2 + 63 and rep["max_rows"] == 256
    assert rep["during_trials"] == {"calibrations": 0, "graph_captures": 0, "repack": 0}, rep
    # the baseline's share: its one calibration; the graphs and operands were there already
    assert {k: stats[k] - counters[k] for k in counters} == {"calibrations": 1, "graph_captures": 0, "repack": 0}
    assert rep["baseline"] == {"calibrations": 1, "graph_captures": 0, "repack": 0}, rep
    assert np.isfinite(table.loss).all() and np.isfinite(table.kl).all() and (table.kl > 0).all()
    assert table.lnum.tolist() == [2, 15, 15, 2] and table.bits[2] == [8, 2]  # results in the order given
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


# ---- the definition of 'no change' ------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False])
def test_base_loss_is_the_unpatched_pass_and_self_kl_is_zero(gpu, knobs, graph):  # noqa: F811
    from smpq import engine, ops, sensitivity
    engine.USE_GRAPH[0] = graph
    _, dev = _batches(gpu)
    net = build_model(gpu, "resnet18", None, "r18_u8_cal")
    table = sensitivity.semilayer_table(net, dev, [(4, [1, 2], 8)])  # reference_outputs=None
    cal = engine.model_state(net).ranges
    st = torch.zeros(4, dtype=torch.float64, device=gpu)
    kl = torch.zeros(2, dtype=torch.float64, device=gpu)
    with torch.no_grad():
        for x, y in dev:
            logits, ovf = engine._graph_forward(net, x, cal) if graph else engine._static_eager(net, x, cal)
            assert ovf.tolist() == [0, 0]
            p = ops.softmax_xent(logits.float().contiguous(), y, st, want_probs=True)
            ops.kl_rows(p, p.clone(), kl)
    st, kl = st.tolist(), kl.tolist()
    assert table.base_loss == st[0] / st[3]
    assert kl == [0.0, 16.0]  # the reference against itself through the trial's ops: exactly 0
    assert table.kl[0] > 0 and table.kl[0] == table.kl_stats[0][0] / 16.0


# ---- the slow path -----------------------------------------------------------------------------------
def test_slow_path_for_a_semilayer_that_completes_a_conv(gpu, knobs):  # noqa: F811
    import functions
    from smpq import assignments, quant, sensitivity
    host, dev = _batches(gpu)
    net = build_model(gpu, "resnet18", None, "r18_u8_cal")
    conv = assignments.conv_for_lnum(net, 3)
    bits = np.full(conv.out_channels, 8)
    bits[[0, 5, 9, 63]] = 0  # four free channels
    quant.quantize_layer_(conv, bits)
    bn = sensitivity.bn_for(net, conv)
    assert sensitivity.patchable_rows(conv, bn, [0, 5, 9]) and not sensitivity.patchable_rows(conv, bn, [63, 0, 5, 9])
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    table = sensitivity.semilayer_table(net, dev, [(3, [63, 0, 5, 9], 4), (3, [0, 5, 9], 4)])
    rep = table.report()
    assert rep["trials"] == 2 and rep["patched"] == 1 and rep["slow"] == {"not_patchable": 1}, rep
    assert table.slow.tolist() == [True, False] and np.isnan(table.stats[0]).all() and np.isfinite(table.stats[1]).all()
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert conv._bits_host.tolist() == bits.tolist()
    # the same steps by hand through the public API
    _, base_loss, base_outs = functions.evaluate_acc_loss_softmax(net, gpu, host)
    assert base_loss == table.eval_loss
    for c in (63, 0, 5, 9):
        conv.weight.data = functions.channel_wise_quantizationperchan(conv.weight.data, 4, c)
    acc, loss, outs = functions.evaluate_acc_loss_softmax(net, gpu, host)
    kl = functions.KLdiv(base_outs, outs)
    net.load_state_dict(sd)
    assert (table.acc[0], table.loss[0], table.kl[0]) == (acc, loss, kl)
    assert table.param[0] == 4 * 576 * (28 / 32)


# ---- against the CPU oracle ---------------------------------------------------------------------------
def test_semilayer_against_the_oracle(gpu, knobs, monkeypatch):  # noqa: F811
    """tests/test_gpu_driver.py's case (ResNet-18, 32 synthetic images in 2 batches, labels the network
    gets mostly right) and its bounds for a semilayer step: top-1 accuracy equal, loss within 1e-3
    relative, KL within 1 % relative of the oracle's, for the first half of layer3.1.conv2 (lnum 12)
    at 4 bits against the pristine evaluation's softmax."""
    monkeypatch.setenv("SMPQ_SYNTHETIC", "1")
    import functions
    import imagenet
    from oracle import eval_ref, torch_ref
    from smpq import assignments, engine, ops, sensitivity
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)
    arch = "resnet18"
    net = build_model(gpu, arch, None, "r18_u8_cal")
    loader = list(imagenet.SyntheticImageNet(n_images=32, batch_size=16, seed=5))
    sd0 = {k: v.detach().cpu() for k, v in net.state_dict().items() if not k.endswith(("qbits", "qstep"))}
    base_logits = [torch_ref.resnet_forward(arch, sd0, x) for x, _ in loader]
    loader = [(x, torch.where(torch.arange(len(y)) % 4 == 0, y, l.argmax(1))) for (x, y), l in zip(loader, base_logits)]
    _, _, originaloutputs = functions.evaluate_acc_loss_softmax(net, gpu, loader)
    originaloutputs = [o.clone() for o in originaloutputs]
    _, _, r_orig = eval_ref.evaluate_acc_loss_softmax([(l.numpy(), y.numpy()) for l, (_, y) in zip(base_logits, loader)])
    conv = assignments.conv_for_lnum(net, 12)
    assert conv is net.layer3[1].conv2
    half = list(range(conv.out_channels // 2))
    # the oracle's weights: what the GPU quantizer rounds those channels to
    w = sd0["layer3.1.conv2.weight"].clone()
    bits = [4] * len(half) + [0] * (conv.out_channels - len(half))
    ops.quantize_channels_(w.view(conv.out_channels, -1), bits, semantics="device")
    sd1 = dict(sd0, **{"layer3.1.conv2.weight": w})
    r_acc, r_loss, r_after = eval_ref.evaluate_acc_loss_softmax(
        [(torch_ref.resnet_forward(arch, sd1, x).numpy(), y.numpy()) for x, y in loader])
    r_kl = eval_ref.kldiv(r_orig, r_after)
    dev = [(x.to(gpu), y.to(gpu)) for x, y in loader]
    table = sensitivity.semilayer_table(net, dev, [(12, half, 4)], reference_outputs=originaloutputs)
    assert table.report()["patched"] == 1
    acc, loss, kl = float(table.acc[0]), float(table.loss[0]), float(table.kl[0])
    print("semilayer lnum 12, 128 channels at 4 bits: acc %.4f (oracle %.4f) loss %.6f (oracle %.6f, rel %.2e) "
          "KL %.4e (oracle %.4e, rel %.2e)" % (acc, r_acc, loss, r_loss, abs(loss - r_loss) / abs(r_loss), kl, r_kl,
                                               abs(kl - r_kl) / r_kl))
    assert acc == r_acc
    assert abs(loss - r_loss) <= 1e-3 * abs(r_loss)
    assert abs(kl - r_kl) <= 0.01 * r_kl


# ---- the drop-in switch ---------------------------------------------------------------------------------
def test_dropin_switch_on_the_gpu(gpu, knobs, monkeypatch):  # noqa: F811
    monkeypatch.setenv("SMPQ_SYNTHETIC", "1")
    import functions
    import imagenet
    import resnet
    from smpq import sensitivity
    from smpq.batches import ResidentSet
    host, _ = _batches(gpu)
    pristine_net = build_model(gpu, "resnet18", None, "r18_u8_cal")
    pristine = {k: v.detach().clone() for k, v in pristine_net.state_dict().items()}
    real = resnet.resnet18
    built = []

    def constructor(num_classes=1000, pretrained=None):
        net = real()
        net.load_state_dict(pristine)
        built.append(net)
        return net.to(gpu).eval()

    loader = ResidentSet(host, device=gpu)
    monkeypatch.setattr(imagenet, "val_loader", loader)
    monkeypatch.setattr(resnet, "resnet18", constructor)
    _, _, originaloutputs = functions.evaluate_acc_loss_softmax(pristine_net, gpu, loader)
    originaloutputs = [o.clone() for o in originaloutputs]

    def lists():
        # [layer_index, block_index, lnum, cnum, w_bit, flag, ., .]
        minus = [[0, 0, 2, c, 4, 0, 0, 0] for c in (5, 9, 33)] + [[1, 1, 8, c, 2, -1, 0, 0] for c in (127, 0)]
        plus = [[3, 1, 16, c, 4, 1, 0, 0] for c in range(0, 512, 8)]
        return minus, plus

    monkeypatch.setattr(functions, "PATCHED_SEMILAYERS", [False])
    minus, plus = lists()
    semis_off, orders_off = functions.make_semilayers_resnet18(constructor(), gpu, originaloutputs, minus, plus)
    assert len(orders_off) == 3 and len(built) == 4

    monkeypatch.setattr(functions, "PATCHED_SEMILAYERS", [True])
    del built[:]
    minus, plus = lists()
    caller = constructor()
    before = functions.patched_semilayers_report()
    semis_on, orders_on = functions.make_semilayers_resnet18(caller, gpu, originaloutputs, minus, plus)
    after = functions.patched_semilayers_report()
    assert after["calls"] == before["calls"] + 1 and after["semilayers"] == before["semilayers"] + 2
    assert after["fallbacks"] == before["fallbacks"]
    assert len(built) == 2  # the caller's and ONE more
    assert semis_on == semis_off
    assert minus[-1] == [0, 0, 100, 0, 0, 0, 0, 0] and plus[-1] == minus[-1] and len(minus) == 6 and len(plus) == 65
    assert [o[0] for o in orders_on] == [0, 1, 2]
    assert orders_on[0] == orders_off[0]  # the same code path, bit for bit
    assert int(caller.layer1[0].conv2._bits_host[5]) == 4  # the caller's model stays quantized with it
    fresh = constructor()
    table = sensitivity.semilayer_table(fresh, loader, [(8, [127, 0], 2), (16, list(range(0, 512, 8)), 4)],
                                        reference_outputs=originaloutputs)
    assert table.report()["patched"] == 2
    for i in (0, 1):
        assert orders_on[i + 1][1] == float(table.kl[i]) / float(table.param[i])
        # and the ordinary route's value is what it approximates (fresh calibration per semilayer there)
        print("semilayer %d: patched %.6e ordinary %.6e" % (i + 1, orders_on[i + 1][1], orders_off[i + 1][1]))
        assert orders_on[i + 1][1] > 0
