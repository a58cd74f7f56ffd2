"""What a sensitivity trial is, whoever runs it: smpq.sensitivity's two tables and smpq.search's Session.

A trial patches rows of ONE conv's packed operand in place, forwards and scores every batch, and puts
the bytes back. This module holds the one guarded trial (``guarded_trial``:
patch, suffix.score_pass, restore, invalidate on failure), the trial objects (``Trial``: one row;
``Semilayer``: n rows), what decides whether an operand can be patched (``patchable*``), the callers'
common preconditions (``setup``) and the hooks on the real engine (``EngineHooks``). The loop over the
batches itself is suffix.score_pass, next to the store it walks.
"""
import numpy as np
import torch

from . import assignments, checkpoint, engine, ops, prefix
from . import suffix as _suffix
from .batches import ResidentSet
from .qconv import QConv2d, stats
from .quant import channel_wise_quantizationperchan, check_pending

COUNTERS = ("calibrations", "graph_captures", "repack")


def counters():
    """The engine's calibrations, graph captures and repacks so far (COUNTERS' order)."""
    return tuple(stats.get(k, 0) for k in COUNTERS)


class Trial:
    """One trial of delta_loss_table: channel ``channel`` of conv ``lnum`` at ``bit`` bits, for column
    ``col``. A semilayer of one channel (``channels``, ``bits``) patched as a single row."""
    __slots__ = ("col", "lnum", "conv", "channel", "bit", "channels", "bits")
    kind = "row"  # ops.trial_row_patch

    def __init__(self, col, lnum, conv, channel, bit):
        self.col, self.lnum, self.conv, self.channel, self.bit = col, lnum, conv, channel, bit
        self.channels, self.bits = [channel], [bit]


class Semilayer:
    """One trial of semilayer_table: ``channels`` (distinct) of conv ``lnum`` at ``bits`` (one
    bit-width per channel). ``param`` is what functions._make_semilayers accumulates: the sum over
    the channels of K * (32 - bit) / 32. ``rows``: the hooks' uploaded lists (ops.TrialRows);
    ``kind``: "rows" (ops.trial_rows_patch) or "rows_x8" (ops.trial_rows_patch_x8)."""
    __slots__ = ("index", "lnum", "conv", "channels", "bits", "param", "rows", "kind")

    def __init__(self, index, lnum, conv, channels, bits, k_elems):
        self.index, self.lnum, self.conv = index, lnum, conv
        self.channels = [int(c) for c in channels]
        self.bits = [int(b) for b in bits]
        self.param = 0.0
        for b in self.bits:  # in the reference's order of accumulation
            self.param += k_elems * ((32 - b) / 32)
        self.rows, self.kind = None, "rows"


# ---- which operands can be patched ----------------------------------------------------------------
def bn_for(net, conv):
    """The BatchNorm the engine folds onto ``conv`` (convN -> bnN of its block), or None."""
    for b in assignments.blocks_of(net):
        for i in (1, 2, 3):
            if getattr(b, "conv%d" % i, None) is conv:
                return getattr(b, "bn%d" % i, None)
    return None


def _operand(conv, bn):
    """What the three patchable predicates ask of the operand alone: the ConvPlan of a QConv2d whose
    codes are [LW, cout, K] with the K-major copy there exactly when ops.KMAJOR is on and K a multiple
    of 64 within the patch kernels' row limit; None otherwise."""
    if not isinstance(conv, QConv2d):
        return None
    plan = engine.conv_plan(conv, bn)
    if plan is None or plan.codes.dim() != 3:
        return None
    if (getattr(plan.codes, "_smpq_km", None) is not None) != bool(ops.KMAJOR[0]):
        return None
    if plan.codes.shape[2] % 64 != 0 or plan.codes.shape[2] > ops.TRIAL_MAX_K:
        return None
    return plan


def _free(conv, bn):
    """The free (unquantized) channel mask of a conv whose 'fixed' / 'exact16' operand (LW >= 2, no
    offsets) can be patched in place, or None."""
    plan = _operand(conv, bn)
    if plan is None or plan.codes.shape[0] < 2 or plan.offset is not None:
        return None
    return np.asarray(conv._bits_host <= 0)


def patchable(conv, bn, channel=None):
    """Can a trial of ``conv`` (folded with ``bn``) patch its packed operand in place? True when
      * the conv has a ConvPlan whose codes are [LW, cout, K] with LW >= 2 and no offsets (kinds
        'fixed' and 'exact16': every row coded independently of the others);
      * another channel stays unquantized whichever channel is tried (``channel``: besides that
        one), so the normal path would pack the quantized model with the same LW: a trial that
        completes a conv would turn it 'exact8' there;
      * the K-major copy on the codes is there exactly when ops.KMAJOR is on;
      * K is within the patch kernel's row limit."""
    free = _free(conv, bn)
    if free is None:
        return False
    others = int(free.sum()) - (1 if channel is None or free[int(channel)] else 0)
    return others >= 1


def patchable_rows(conv, bn, channels):
    """patchable for a semilayer trial: patchable's conditions on the operand, and at least one
    channel OUTSIDE ``channels`` is unquantized (a semilayer that completes a conv would be packed
    'exact8' on the normal path, with another LW)."""
    free = _free(conv, bn)
    if free is None:
        return False
    free = free.copy()
    free[[int(c) for c in channels]] = False
    return bool(free.any())


def patchable_rows_x8(conv, bn, channels, bits):
    """Can a trial that RE-quantizes ``channels`` of a fully quantized ``conv`` at ``bits`` (one
    int or one per channel) patch its 'exact8' operand in place (ops.trial_rows_patch_x8)? True when
      * the conv has a ConvPlan whose codes are [1, cout, K] of kind 'exact8';
      * the K-major copy on the codes is there exactly when ops.KMAJOR is on;
      * K is a multiple of 64 within the patch kernel's row limit;
      * every channel of the conv is quantized, so that it stays fully quantized whatever the
        channels and the normal path would again pack one int8 plane;
      * every bit-width is at most 8 (a wider row cannot be exact8).
    Whether a ROW can then be coded (on the grid, within 256 levels, with an offset only where the
    operand has offsets) is the kernel's answer, in its status words. codes, their K-major copy,
    offset, wscale and the folded col_scale are all an exact8 operand is: the resident 1x1 tiles, the
    halo 3x3 tiles and the chained conv3 / conv1 launches read these same tensors."""
    plan = _operand(conv, bn)
    if plan is None or getattr(plan, "kind", None) != "exact8" or plan.codes.shape[0] != 1:
        return False
    if not conv.fully_quantized():
        return False
    bits = [bits] if isinstance(bits, (int, np.integer)) else list(bits)
    return len([int(c) for c in channels]) > 0 and all(1 <= int(b) <= 8 for b in bits)


def constant_rows(conv):
    """Per output channel of ``conv``: is its weight row constant? (The reference raises on such a
    channel, functions.py:40; a host list, one host read.)"""
    with torch.no_grad():
        w2d = conv.weight.detach().reshape(conv.out_channels, -1)
        return (w2d.amax(1) == w2d.amin(1)).tolist()


# ---- evaluations and statistics ---------------------------------------------------------------------
def ordinary_eval(net, batches, want_probs=True):
    """functions.evaluate_acc_loss_softmax on device batches: (top-1 accuracy, mean batch loss, the
    per-batch softmax outputs or with ``want_probs`` off Nones), a fresh calibration on the first
    batch, float64 statistics, one host sync."""
    acc, outs = None, []
    engine.new_evaluation(net)
    with torch.no_grad():
        for x, y in batches:
            out = net(x).float().contiguous()
            if acc is None:
                acc = torch.zeros(4, dtype=torch.float64, device=out.device)
            outs.append(ops.softmax_xent(out, y, acc, want_probs=want_probs))
    loss_sum, correct, seen, count = acc.tolist()
    return correct / seen, loss_sum / count, outs


def ordinary_loss(net, batches):
    """functions.evaluate_loss on device batches: the mean over batches of the batch-mean cross entropy."""
    return ordinary_eval(net, batches, want_probs=False)[1]


def kl_stats(reference, outs):
    """ops.kl_rows accumulated over the (reference, output) softmax pairs: [sum over images of
    sum_c p * log(p / q), images] on the host (one host read)."""
    st = torch.zeros(2, dtype=torch.float64, device=outs[0].device)
    for p, q in zip(reference, outs):
        ops.kl_rows(p.to(q.device), q, st)
    return st.tolist()


def kl_of(reference, outs):
    """functions.KLdiv(reference, outs): sum over images of sum_c p * log(p / q), over the images."""
    s, n = kl_stats(reference, outs)
    return s / n


def unpatched_pass(hooks, batches, device, want_probs=False):
    """Every batch through the trials' own forward with no patch: (statistics, flags, each batch's
    softmax or None) with the first two on the host. (A function of its own: a replay hands out its
    graph's flag tensor, which lives in the graph pool; nothing here but the softmax tensors, which
    are fresh, outlives the call, so a later release of the graphs frees the pool whole.)"""
    base = torch.zeros(4, dtype=torch.float64, device=device)
    flags = torch.zeros(2, dtype=torch.int32, device=device)
    probs = [] if want_probs else None
    with torch.no_grad():
        _suffix.score_pass(hooks, batches, None, None, base, None, flags, probs=probs)
    return base.tolist(), flags.tolist(), probs


# ---- the callers' common ground ----------------------------------------------------------------------
def setup(who, net, batches):
    """The preconditions of ``who`` (delta_loss_table, semilayer_table, search.Session): static range
    mode, no data-parallel group, an eval-mode fused net on the GPU; ValueError otherwise. Returns
    (a parameter of the net, ``batches`` as a list of device pairs or the ResidentSet bound to the
    net's device)."""
    if engine.get_range_mode() != "static":
        raise ValueError("smpq: %s needs the static range mode (engine.set_range_mode)" % who)
    if engine.get_dp_group() is not None:
        raise ValueError("smpq: %s runs on one GPU (no data-parallel group)" % who)
    p = next(net.parameters())
    if not p.is_cuda or net.training or not getattr(net, "fused", True):
        raise ValueError("smpq: %s needs an eval-mode smpq ResNet on the GPU" % who)
    if isinstance(batches, ResidentSet):
        batches.bind(p.device)
    else:
        batches = list(batches)
        if not batches or any(not (torch.is_tensor(x) and x.device == p.device) for x, _ in batches):
            raise ValueError("smpq: batches must be (x, y) pairs with x on the model's device, or a ResidentSet")
        batches = [(x, torch.as_tensor(y).to(p.device)) for x, y in batches]
    return p, batches


def guarded_trial(hooks, tr, status, batches, store, refs, row, kl_row, flags):
    """THE trial, without a host sync: patch ``tr``'s rows (``status``: its int32 constant-channel
    words, one per row), forward and score every batch (suffix.score_pass: into ``row`` float64 [4]
    and, with ``refs``, ``kl_row`` float64 [2]; the forwards' flags ORed into ``flags`` int32 [2]:
    overflow, stale content), restore. Hooks: patch(tr, status), restore(tr), invalidate(tr) and
    score_pass's. The restore runs whatever happens; after an exception the conv's operand is also
    marked for repacking (invalidate), then the exception goes on. ``store`` (suffix.Store or None): as
    in score_pass; a single-row trial (``Trial``) of the store's ``rows`` conv takes the rows route
     and is counted in the block's report row."""
    rows = store is not None and store.rows is not None and store.rows is tr.conv and tr.kind == "row"
    if rows:
        store.row["rows_trials"] += 1
    failed = False
    try:
        hooks.patch(tr, status)
        _suffix.score_pass(hooks, batches, store, refs, row, kl_row, flags, rows_channel=tr.channel if rows else None)
    except BaseException:
        failed = True
        raise
    finally:
        hooks.restore(tr)
        if failed:
            hooks.invalidate(tr)


class EngineHooks:
    """The trials' hooks on the real engine, for every caller: the three patches, the forwards, the
    scores, the slow trial, and what suffix.enter calls. ``cal``: the StaticRanges an ordinary
    evaluation installed (``rebind``); ``reference``: what slow semilayer trials are compared with;
    ``plan``: the suffix.Plan whose resumed forwards are being counted, or None."""
    plan = None
    reference = None
    _check = True
    _row_list = None

    def __init__(self, net, batches):
        self.net, self.batches, self.cal = net, batches, None
        self._conv = self._state = self._save = None

    def rebind(self):
        """After an ordinary evaluation: bind the ranges it installed, forget the last conv and the
        state's snapshot. Returns the ranges object."""
        self.cal = engine.model_state(self.net).ranges
        self._conv = self._state = None
        return self.cal

    # ---- the patches: one row, n rows, n rows of an exact8 operand ----
    def _bind(self, conv):
        if self._conv is not conv:
            bn = bn_for(self.net, conv)
            plan = engine.conv_plan(conv, bn)
            with torch.no_grad():
                a = engine._bn_fold(bn)[0].contiguous() if bn is not None else torch.ones_like(plan.col_scale)
                wscale = conv.packed()[3]
            self._conv, self._plan, self._a, self._wscale = conv, plan, a, wscale
            self._km = getattr(plan.codes, "_smpq_km", None)
            self._reserve(1)

    def _reserve(self, n):
        """The one save area holds at least ``n`` rows of the bound conv."""
        lw, _, K = self._plan.codes.shape
        need, dev = ops.trial_rows_save_bytes(lw, K, n), self._plan.codes.device
        if self._save is None or self._save.numel() < need or self._save.device != dev:
            self._save = torch.empty(need, dtype=torch.int8, device=dev)

    def prepare(self, sems, kind="rows"):
        """Upload the lists of every semilayer of one conv up front and size the save area."""
        self._bind(sems[0].conv)
        cout = self._plan.codes.shape[1]
        for sem in sems:
            sem.kind = kind
            sem.rows = ops.trial_rows_lists(sem.channels, sem.bits, cout, self._plan.codes.device,
                                            max_bits=8 if kind == "rows_x8" else 16)
        self._reserve(max(len(s.channels) for s in sems))

    def patch(self, tr, status):
        self._bind(tr.conv)
        self.new_trial()
        p, w = self._plan, tr.conv.weight.detach()
        if tr.kind == "row":
            ops.trial_row_patch(w, tr.channel, tr.bit, self._a, p.codes, self._wscale, p.col_scale, self._save, status,
                                km=self._km)
        elif tr.kind == "rows":
            ops.trial_rows_patch(w, tr.rows, None, self._a, p.codes, self._wscale, p.col_scale, self._save, status,
                                 km=self._km)
        else:
            ops.trial_rows_patch_x8(w, tr.rows, None, self._a, p.codes, p.offset, self._wscale, p.col_scale, self._save,
                                    status, km=self._km)

    def restore(self, tr):
        p = self._plan
        if tr.kind == "row":
            ops.trial_row_restore(tr.channel, p.codes, self._wscale, p.col_scale, self._save, km=self._km)
        elif tr.kind == "rows":
            ops.trial_rows_restore(tr.rows, p.codes, self._wscale, p.col_scale, self._save, km=self._km)
        else:
            ops.trial_rows_restore_x8(tr.rows, p.codes, p.offset, self._wscale, p.col_scale, self._save, km=self._km)

    def invalidate(self, tr):
        tr.conv._content_gen += 1

    # ---- forwards and scores ----
    def forward(self, x):
        if engine.USE_GRAPH[0]:
            return engine._graph_forward(self.net, x, self.cal)
        return engine._static_eager(self.net, x, self.cal)

    def score(self, logits, y, row, want_probs=False):
        return ops.softmax_xent(logits.float().contiguous(), y, row, want_probs=want_probs)

    def score_kl(self, logits, y, ref, row, kl_row):
        probs = ops.softmax_xent(logits.float().contiguous(), y, row, want_probs=True)
        ops.kl_rows(ref, probs, kl_row)

    def slow(self, tr):
        """One trial through the public API on the model itself: quantize its channels one by one,
        evaluate, put weights and metadata back bitwise. A Trial: the loss, as functions.evaluate_loss
        does; a Semilayer: (acc, loss, kl), as functions.evaluate_acc_loss_softmax and KLdiv against
        the reference do."""
        if self._state is None:
            self._state = checkpoint.snapshot(self.net)
        try:
            for c, bit in zip(tr.channels, tr.bits):
                channel_wise_quantizationperchan(tr.conv.weight.data, bit, c)
            check_pending()
            if tr.kind == "row":
                return ordinary_loss(self.net, self.batches)
            acc, loss, outs = ordinary_eval(self.net, self.batches)
            return acc, loss, kl_of(self.reference, outs)
        finally:
            try:
                check_pending()
            except ZeroDivisionError:
                pass
            checkpoint.restore_(self.net, self._state)

    # ---- what suffix.enter calls ----
    def block_of(self, conv):
        return _suffix.block_of(self.net, conv)

    def block_name(self, j):
        return prefix.block_names(self.net)[j]

    def kept_bytes(self, x, j):
        return _suffix.kept_bytes(self.net, x, j)

    def fill(self, x, j):
        return _suffix.fill(self.net, x, self.cal, j)

    def new_trial(self):
        self._check = True

    def resume(self, kept, j):
        """suffix.resume (looked up at call time), counted in ``plan``; the content check is enqueued
        for the first resumed batch after every ``new_trial``."""
        before = stats["hip_conv"]
        out = _suffix.resume(self.net, kept, self.cal, j, check=self._check)
        self._check = False
        if self.plan is not None:
            self.plan.resumed += 1
            self.plan.launches += stats["hip_conv"] - before
        return out

    def sync(self):
        torch.cuda.synchronize()

    # ---- the rows route ----
    def last_conv(self, j):
        return _suffix.last_conv(self.net, j)[0]

    def rows_block(self, j):
        """None when block ``j``'s last conv may go the rows route, else why not."""
        if j >= len(engine._blocks(self.net)) - 1:
            return "last_block"  # its output is fp32 for the average pool
        conv, bn = _suffix.last_conv(self.net, j)
        if not _suffix.rows_geometry(conv):
            return "geometry"
        return None if patchable(conv, bn) else "not_patchable"

    def rows_bytes(self, x, j):
        return _suffix.rows_bytes(self.net, x, j)

    def fill_rows(self, x, j):
        return _suffix.fill_rows(self.net, x, self.cal, j)

    def _one_row(self, j, channel, device):
        """The uploaded one-entry list of a trial's channel (made once per trial, not per batch)."""
        key = (j, int(channel), device)
        if self._row_list is None or self._row_list[0] != key:
            self._row_list = (key, ops.trial_rows_lists([int(channel)], 8, _suffix.last_conv(self.net, j)[0].out_channels,
                                                        device, "trial_rows_conv"))
        return self._row_list[1]

    def rows_check(self, st, j):
        """The one-row conv of channel 0 from the UNPATCHED operand into every kept input of block
        j + 1: the bytes it replaced must be the bytes it wrote (compared on the device, one host
        read), and it must not flag an overflow."""
        dev = next(e for e in st.entries if e is not None).parts[0][2].device
        rows = self._one_row(j, 0, dev)
        bad = torch.zeros(2, dtype=torch.int32, device=dev)
        for e in st.entries:
            if e is None or e.rows is None:
                continue
            done = []
            try:
                _suffix.rows_conv(self.net, e, j, rows, bad[:1], done)
                for save, (_, _, q, _) in zip(e.rows.saves, e.rows.next.parts):
                    old = save[:q.shape[0] * q[0, ..., 0].numel()].view(q.shape[0], -1)
                    bad[1:] |= (old != q.reshape(q.shape[0], -1, q.shape[-1])[:, :, 0]).any().to(torch.int32)
            finally:
                _suffix.rows_restore(e, rows, done)
        return not any(bad.tolist())

    def resume_rows(self, kept, j, channel):
        """A trial's forward of one batch on the rows route: channel ``channel`` of block ``j``'s last
        conv from its patched operand into the kept input of block j + 1, the resumed forward from
        there, the old bytes back (whatever happens): (logits, flags with the one-row conv's overflow
        in word 0)."""
        flag = torch.zeros(2, dtype=torch.int32, device=kept.parts[0][2].device)
        rows = self._one_row(j, channel, flag.device)
        done = []
        try:
            _suffix.rows_conv(self.net, kept, j, rows, flag[:1], done)
            logits, ovf = self.resume(kept.rows.next, j + 1)
            torch.bitwise_or(flag, ovf, out=flag)
        finally:
            _suffix.rows_restore(kept, rows, done)
        return logits, flag
