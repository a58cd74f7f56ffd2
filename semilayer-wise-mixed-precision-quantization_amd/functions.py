"""Drop-in for the reference's ``functions`` module (functions.py:1-612).

Same names, signatures and return values:
  quantize_wgt, channel_wise_quantizationperchan      -> smpq.quant (libsmpq, bit-exact)
  evaluate_loss, evaluate_acc_loss_softmax             -> GPU eval loop over net(x) + the fused
                                                          softmax / CE / top-1 kernel, one host
                                                          sync per call instead of per batch
  KLdiv                                                -> smpq_kl_rows on device (same formula)
  make_divide_minusplusmodels, make_quantizedlists,
  make_semilayers_resnet18/34/50                       -> the search bookkeeping, restated
The reference's quirks that change results are kept on purpose (they are what a drop-in must
reproduce): the dummy sentinel rows appended to the caller's lists, the semilayer split on
``dlists[i][index] <= 0`` indexed by list position (functions.py:171-173), and the sensitivity
pass quantizing the caller's net for its first semilayer before switching to fresh models.

SMPQ_PATCHED_SEMILAYERS=1 (read at import, off by default): the sensitivity pass evaluates every
semilayer after its first as one smpq.sensitivity.semilayer_table on ONE fresh model, patching the
semilayer's packed weight rows in place instead of quantizing and loading a model per semilayer
(DESIGN.md 5g). Same lists, indices and print lines; the KL values come from evaluations under the
fresh model's own static ranges, not from a calibration per semilayer.
"""
import os
import sys

import torch

from smpq import engine, memo, ops, sensitivity
from smpq.batches import DeviceBatches, ResidentSet
from smpq.models import ResNet
from smpq.quant import channel_wise_quantizationperchan, quantize_wgt  # noqa: F401

_SENTINEL = [0, 0, 100, 0, 0, 0, 0, 0]
PATCHED_SEMILAYERS = [os.environ.get("SMPQ_PATCHED_SEMILAYERS", "0") == "1"]
_PATCHED = {"announced": False, "calls": 0, "semilayers": 0, "fallbacks": 0}


def patched_semilayers_report():
    """Counters of the SMPQ_PATCHED_SEMILAYERS route: calls that took it, semilayers it evaluated
    through semilayer_table, and calls that fell back to the ordinary route."""
    return {k: v for k, v in _PATCHED.items() if k != "announced"}


def _run_eval(net, device, data_loader, want_probs):
    """Forward every batch, then the fused softmax / cross-entropy / top-1 kernel
    (smpq_softmax_xent) accumulates [loss_sum, correct, seen, batches] on the device: one host
    sync per evaluation. Host batches reach the device through DeviceBatches (the copy of the
    next batch overlaps this batch's forward); a smpq.batches.ResidentSet is iterated as it is (it
    reads its loader once and serves later evaluations from the device). Returns (stats float64
    [4] on the device, list of softmax outputs). With smpq.memo on, an evaluation of a ResidentSet
    that repeats a recorded one returns that record (stats on the host, clones of its softmax
    outputs) without iterating the set; every other case runs the loop below unchanged."""
    net.to(device)
    net.eval()
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    token = None
    if memo.ENABLED[0]:  # SMPQ_EVAL_MEMO (off by default): a repeated evaluation launches nothing
        token = memo.begin(net, dev, data_loader, want_probs)
        if token is not None and token.entry is not None:
            return memo.hit_result(token)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    outputs = []
    if isinstance(net, ResNet):
        engine.new_evaluation(net)  # ranges from this pass's own first batch: history-independent
    if isinstance(data_loader, ResidentSet):
        batches = data_loader.bind(dev)  # (a CPU device is a ValueError: there is no CPU form)
    else:
        batches = DeviceBatches(data_loader, dev) if dev.type == "cuda" else data_loader
    with torch.no_grad():
        for x, y in batches:
            x = x.to(device, non_blocking=True)
            out = net(x).float().contiguous()
            p = ops.softmax_xent(out, y, stats, want_probs=want_probs)
            if want_probs:
                outputs.append(p)
    if token is not None:  # a miss that ran to its end: recorded if the set now vouches for a replay
        stats = memo.finish(token, stats, outputs)
    return stats, outputs


def _finish(stats):
    loss_sum, correct, seen, count = stats.tolist()  # the one host sync
    return correct / seen, loss_sum / count


def evaluate_loss(net, device, data_loader):
    """functions.py:45-82: mean over batches of the batch CE loss (the reference's second,
    redundant forward per batch at :71 only recomputed the prediction, so it is not repeated)."""
    stats, _ = _run_eval(net, device, data_loader, want_probs=False)
    return _finish(stats)[1]


def evaluate_acc_loss_softmax(net, device, data_loader):
    """functions.py:84-129: (top-1 accuracy, mean batch loss, list of per-batch softmax)."""
    stats, outs = _run_eval(net, device, data_loader, want_probs=True)
    acc, loss = _finish(stats)
    return acc, loss, outs


def KLdiv(n_out, out):
    """functions.py:131-149: mean over images of sum_c p_c * log(p_c / q_c) (smpq_kl_rows per
    batch pair, accumulated on the device, one host sync)."""
    stats = None
    for p, q in zip(n_out, out):
        if stats is None:
            stats = torch.zeros(2, dtype=torch.float64, device=q.device)
        ops.kl_rows(p.to(q.device), q, stats)
    s, n = stats.tolist()
    return s / n


def make_divide_minusplusmodels(paramlists, dlists, index):
    """functions.py:151-184: split rows into (delta <= 0, delta > 0) semilayer lists; flag
    counters move by one whenever the layer number changes between consecutive rows."""
    minus, plus = [], []
    mflag, pflag = 0, 1
    last = len(paramlists) - 1
    for i, row in enumerate(paramlists):
        base = [row[0], row[1], row[2], row[3], row[4]]
        tail = [row[6], row[7]]
        if dlists[i][index] <= 0:
            minus.append(base + [mflag] + tail)
        else:
            plus.append(base + [pflag] + tail)
        if i == last:
            print('function debug:number of total channels=', len(minus) + len(plus),
                  'No.1:', len(minus), 'No.2:', len(plus))
            break
        if row[2] != paramlists[i + 1][2]:
            mflag -= 1
            pflag += 1
    return minus, plus


def _target_conv(layers, arch, layer_index, block_index, lnum):
    blk = layers[layer_index][block_index]
    if arch == "resnet50":
        return (blk.conv3, blk.conv1, blk.conv2)[lnum % 3]
    return blk.conv1 if lnum % 2 != 0 else blk.conv2


def _make_semilayers(net, device, originaloutputs, listminus, listplus, arch):
    import imagenet
    why = _patched_route_refused(imagenet.val_loader) if PATCHED_SEMILAYERS[0] else "off"
    if PATCHED_SEMILAYERS[0] and not _PATCHED["announced"]:
        _PATCHED["announced"] = True
        print("smpq: SMPQ_PATCHED_SEMILAYERS=1 -> the sensitivity pass patches each semilayer's packed weight "
              "rows on one fresh model (smpq.sensitivity.semilayer_table) instead of quantizing a model per "
              "semilayer", file=sys.stderr)
    if why is None:
        got = _make_semilayers_patched(net, device, originaloutputs, listminus, listplus, arch)
        if got is not None:
            return got
    elif why != "off":
        _PATCHED["fallbacks"] += 1
        print("smpq: SMPQ_PATCHED_SEMILAYERS falls back to the ordinary sensitivity pass: %s" % why, file=sys.stderr)
    return _make_semilayers_ordinary(net, device, originaloutputs, listminus, listplus, arch)


def _patched_route_refused(loader):
    """Why this call cannot take the patched route (None when it can)."""
    if not (isinstance(loader, ResidentSet) and loader.dev is not None and loader.dev.type == "cuda"):
        return "imagenet.val_loader is not a ResidentSet bound to a CUDA device"
    if engine.get_range_mode() != "static":
        return "the range mode is not static"
    return None


def _walk_semilayers(listminus, listplus):
    """The reference's walk over the two lists (sentinel rows appended by the caller): the groups of
    rows that end where the layer number changes, in order."""
    groups = []
    for lst in (listminus, listplus):
        group = []
        for i, row in enumerate(lst):
            if row[2] == 100:
                break
            group.append(list(row))
            if row[2] != lst[i + 1][2]:
                groups.append(group)
                group = []
    return groups


def _make_semilayers_patched(net, device, originaloutputs, listminus, listplus, arch):
    """The switch-on route; None (nothing touched yet) when a semilayer cannot be expressed as one
    semilayer_table trial, so the caller runs the ordinary route."""
    import imagenet
    import resnet
    for lst in (listminus, listplus):
        lst.append(list(_SENTINEL))
    groups = _walk_semilayers(listminus, listplus)
    if any(len({r[3] for r in g}) != len(g) for g in groups[1:]):
        for lst in (listminus, listplus):  # the ordinary route appends its own
            lst.pop()
        _PATCHED["fallbacks"] += 1
        print("smpq: SMPQ_PATCHED_SEMILAYERS falls back to the ordinary sensitivity pass: a semilayer lists a "
              "channel twice", file=sys.stderr)
        return None
    _PATCHED["calls"] += 1
    semilayers, orders = [], []
    if not groups:
        return semilayers, orders

    def line(group, index, kldiv):
        print(group[-1][4], 'bit', 'semilayer-No.', index, 'layernumber=', group[-1][2], 'channels=', len(group),
              'total KL divergence=', kldiv)

    # the first semilayer as ever, on the caller's net (which stays quantized with it)
    first = groups[0]
    layers = [net.layer1, net.layer2, net.layer3, net.layer4]
    param = 0.0
    for row in first:
        conv = _target_conv(layers, arch, row[0], row[1], row[2])
        conv.weight.data = channel_wise_quantizationperchan(conv.weight.data, row[4], row[3])
        param += conv.weight[row[3]].data.numel() * ((32 - row[4]) / 32)
    semilayers.append(first)
    _, _, afteroutputs = evaluate_acc_loss_softmax(net, device, imagenet.val_loader)
    kldiv = KLdiv(originaloutputs, afteroutputs) / param
    line(first, 0, kldiv)
    orders.append([0, kldiv])
    if len(groups) > 1:
        fresh = getattr(resnet, arch)(num_classes=1000, pretrained='imagenet')  # ONE model for all the rest
        fresh.to(device)
        fresh.eval()
        table = sensitivity.semilayer_table(
            fresh, imagenet.val_loader, [(g[0][2], [r[3] for r in g], [r[4] for r in g]) for g in groups[1:]],
            reference_outputs=originaloutputs)
        const = table.report()["constant"]
        if const:  # the reference raises at the first constant channel it quantizes (functions.py:40)
            raise ZeroDivisionError("float division by zero (constant channel %s of lnum %s)" % (const[0][1], const[0][0]))
        _PATCHED["semilayers"] += len(groups) - 1
        for index, group in enumerate(groups[1:], start=1):
            semilayers.append(group)
            kldiv = float(table.kl[index - 1]) / float(table.param[index - 1])
            line(group, index, kldiv)
            orders.append([index, kldiv])
    return semilayers, orders


def _make_semilayers_ordinary(net, device, originaloutputs, listminus, listplus, arch):
    import imagenet
    import resnet
    semilayers, orders = [], []
    index = 0
    for lst in (listminus, listplus):
        lst.append(list(_SENTINEL))
    layers = [net.layer1, net.layer2, net.layer3, net.layer4]
    for lst in (listminus, listplus):
        group, param, counta = [], 0.0, 0
        for i, row in enumerate(lst):
            layer_index, block_index, lnum, cnum, w_bit = row[0], row[1], row[2], row[3], row[4]
            if lnum == 100:
                break
            group.append(list(row))
            conv = _target_conv(layers, arch, layer_index, block_index, lnum)
            conv.weight.data = channel_wise_quantizationperchan(conv.weight.data, w_bit, cnum)
            param += conv.weight[cnum].data.numel() * ((32 - w_bit) / 32)
            counta += 1
            if lnum != lst[i + 1][2]:
                semilayers.append(group)
                _, _, afteroutputs = evaluate_acc_loss_softmax(net, device, imagenet.val_loader)
                kldiv = KLdiv(originaloutputs, afteroutputs) / param
                print(w_bit, 'bit', 'semilayer-No.', index, 'layernumber=', lnum, 'channels=', counta,
                      'total KL divergence=', kldiv)
                orders.append([index, kldiv])
                net = getattr(resnet, arch)(num_classes=1000, pretrained='imagenet')
                layers = [net.layer1, net.layer2, net.layer3, net.layer4]
                group, param, counta = [], 0.0, 0
                index += 1
    return semilayers, orders


def make_semilayers_resnet18(net, device, originaloutputs, listminus, listplus):
    """functions.py:186-319."""
    return _make_semilayers(net, device, originaloutputs, listminus, listplus, "resnet18")


def make_semilayers_resnet34(net, device, originaloutputs, listminus, listplus):
    """functions.py:321-454."""
    return _make_semilayers(net, device, originaloutputs, listminus, listplus, "resnet34")


def make_semilayers_resnet50(net, device, originaloutputs, listminus, listplus):
    """functions.py:456-588."""
    return _make_semilayers(net, device, originaloutputs, listminus, listplus, "resnet50")


def make_quantizedlists(semilayers, orders):
    """functions.py:590-612: concatenate semilayers in ascending sensitivity + sentinel row."""
    orders.sort(key=lambda x: x[1])
    flat = []
    for inum, _ in orders:
        flat.extend(list(r) for r in semilayers[inum])
        print('debug layernum=', semilayers[inum][-1][2], 'number of channels=', len(semilayers[inum]))
    print('number of valuationfirsts list=', len(flat))
    flat.append(list(_SENTINEL))
    return flat
