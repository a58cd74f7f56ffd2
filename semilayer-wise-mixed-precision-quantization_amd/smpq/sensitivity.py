"""Per-channel delta-loss table: what the search drivers read from dataset/resnetNN_deltaloss.csv.

For every output channel of every searched conv and every bit-width, the change of the loss when
that ONE channel is quantized (its sign decides the channel's semilayer,
functions.make_divide_minusplusmodels). The reference ships the three files for the torchvision
weights and no way to make them; ``delta_loss_table`` + ``write_csv`` make one for any model.

A trial never touches a model tensor. The channel's row of the conv's packed operand (codes, their
K-major copy, wscale, the folded col_scale) is overwritten in place with what the normal path would
have packed for the quantized channel (ops.trial_row_patch), the captured static-range graphs are
replayed over every batch, and the saved bytes are put back (ops.trial_row_restore). Signature,
content fingerprint, installed ranges and graphs stay valid, so a trial costs two small launches
plus its forwards: no fingerprint, no repack, no calibration, no capture.

What cannot be patched runs through the public API on the model itself ("slow" trials): a conv
that is not ``patchable``, and a trial whose replay overflowed a static range.

``semilayer_table`` is the same for the reference's semilayer sensitivity pass
(functions.make_semilayers_resnetNN): a trial patches ALL rows of one semilayer (a subset of one
conv's output channels) in one launch (ops.trial_rows_patch), and every batch is scored for loss,
top-1 and the KL divergence against reference outputs.

With ``suffix=True`` (SMPQ_TRIAL_SUFFIX=1; off by default) both tables visit their convs in block
order and a trial of a deep enough block forwards only the blocks from that one on, eagerly, from
block inputs kept by one prefix pass per block (smpq.suffix); the statistics are the
replayed trial's bit for bit.
"""
import csv
import math
import time

import numpy as np
import torch

from . import assignments, engine
from . import suffix as _suffix  # (the tables have a ``suffix`` argument)
from .trials import (COUNTERS, EngineHooks, Semilayer, Trial, bn_for, constant_rows, counters, guarded_trial, kl_stats,
                     ordinary_eval, ordinary_loss, patchable, patchable_rows, setup, unpatched_pass)
from .trials import kl_of, patchable_rows_x8  # noqa: F401 (part of this module's face, with the names above)


def arch_of(net):
    blocks = assignments.blocks_of(net)
    if hasattr(blocks[0], "conv3"):
        return {16: "resnet50"}.get(len(blocks), "resnet-bottleneck-%d" % len(blocks))
    return {8: "resnet18", 16: "resnet34"}.get(len(blocks), "resnet-basic-%d" % len(blocks))


class DeltaLossTable:
    """One column per (lnum, channel): ``lnum`` and ``cnum`` (0-based) int64 arrays, ``delta[bit]``
    float64 arrays (trial loss - base loss; nan for a constant channel), ``bits`` in the order of the
    file's rows (descending). ``base_loss``: the unquantized model's loss through the sweep's own
    replays (what patched trials are compared with); ``eval_loss``: the same model's loss from an
    ordinary evaluation (what slow trials are compared with; it equals functions.evaluate_loss).
    ``owned``: None, or on the table of a sharded call (``shard=(rank, world)``) a bool array per
    column: the columns this rank computed; every other column is nan (so is a constant channel:
    ``owned`` alone tells them apart). merge_delta_loss makes the complete table of the parts."""

    def __init__(self, arch, lnum, cnum, bits, delta, base_loss, eval_loss=None, report=None):
        self.arch = arch
        self.lnum = np.asarray(lnum, dtype=np.int64)
        self.cnum = np.asarray(cnum, dtype=np.int64)
        self.bits = tuple(int(b) for b in bits)
        self.delta = {int(b): np.asarray(delta[b], dtype=np.float64) for b in self.bits}
        self.base_loss = base_loss
        self.eval_loss = base_loss if eval_loss is None else eval_loss
        # per bit [columns, 4]: a patched trial's softmax_xent statistics (loss sum, correct, rows,
        # batches); nan rows for slow trials and constant channels
        self.stats = {}
        self.owned = None
        self._report = dict(report or {})

    def report(self):
        """Counters of the sweep: trials, patched, slow by reason, constant channels (listed),
        and the calibrations, graph captures and repacks seen by the baseline and by the trials;
        ``suffix``: what the store kept per block (suffix.Plan.report(); {} with the switch off).
        A sharded call counts its own trials only and adds ``shard``: [rank, world]; a merged table
        has the sums, ``world`` and ``ranks``: the parts' reports in rank order."""
        return dict(self._report)


def write_csv(table, path):
    """The reference's layout (resnet18_main.py:61-84): row 0 lnum, row 1 the 1-based channel, then
    one row per bit-width, descending; utf-8-sig, repr-exact floats, no empty trailing column.
    ValueError for the partial table of a sharded call (merge_delta_loss the parts first)."""
    owned = getattr(table, "owned", None)
    if owned is not None and not np.all(owned):
        raise ValueError("smpq: write_csv of a partial table (%d of %d columns owned): merge the shards first"
                         % (int(np.sum(owned)), len(owned)))
    with open(path, "w", encoding="utf-8-sig", newline="") as f:
        wr = csv.writer(f)
        wr.writerow([int(v) for v in table.lnum])
        wr.writerow([int(v) + 1 for v in table.cnum])
        for b in table.bits:
            wr.writerow([repr(float(v)) for v in table.delta[b]])


def read_csv(path, bits=None, arch=None):
    """write_csv's inverse (also reads the reference's files; empty trailing cells are dropped).
    ``bits``: the bit-width of each value row, default 8, 6, 4(, 2) by the number of rows."""
    with open(path, encoding="utf-8-sig", newline="") as f:
        rows = [r for r in csv.reader(f) if r]
    n = len(rows[0])
    while n and rows[0][n - 1].strip() == "":
        n -= 1
    if bits is None:
        bits = (8, 6, 4, 2)[:len(rows) - 2]
    if len(bits) != len(rows) - 2:
        raise ValueError("smpq: %s has %d value rows, %d bit-widths given" % (path, len(rows) - 2, len(bits)))
    lnum = [int(v) for v in rows[0][:n]]
    cnum = [int(v) - 1 for v in rows[1][:n]]
    delta = {int(b): [float(v) for v in rows[2 + i][:n]] for i, b in enumerate(bits)}
    return DeltaLossTable(arch, lnum, cnum, bits, delta, None)


# ---- sharding a table's trials over ranks -------------------------------------------
def check_shard(shard):
    """``shard`` as (rank, world) ints, or None; ValueError unless world >= 1 and 0 <= rank < world."""
    if shard is None:
        return None
    try:
        rank, world = (int(v) for v in shard)
    except (TypeError, ValueError):
        raise ValueError("smpq: shard must be (rank, world), not %r" % (shard,)) from None
    if world < 1 or not 0 <= rank < world:
        raise ValueError("smpq: shard %r is not (rank, world) with world >= 1 and 0 <= rank < world" % (shard,))
    return rank, world


def shard_owner(world, lnum=None, count=None):
    """The rank that owns each column of a sharded table, as an int64 array: the one assignment
    both tables and their merges use. It depends on the selection alone, never on the model's
    values, the data or a measured cost.

    delta_loss_table: give ``lnum``, the lnum of every column in the table's order (what _select
    gives; ``table.lnum``). The column at position i among the columns of ITS conv belongs to rank
    i % world, with all its bit-widths: every rank visits every conv (and block) that has at least
    ``world`` selected channels, and owns ceil or floor of each conv's share.
    semilayer_table: give ``count``, the number of semilayers; semilayer i belongs to rank i % world."""
    world = int(world)
    if world < 1:
        raise ValueError("smpq: world must be >= 1, not %d" % world)
    if (lnum is None) == (count is None):
        raise ValueError("smpq: shard_owner takes lnum (delta_loss_table) or count (semilayer_table)")
    if lnum is None:
        return np.arange(int(count), dtype=np.int64) % world
    seen = {}
    owner = np.empty(len(lnum), dtype=np.int64)
    for col, ln in enumerate(lnum):
        ln = int(ln)
        owner[col] = seen.get(ln, 0) % world
        seen[ln] = seen.get(ln, 0) + 1
    return owner


# ---- the sweep ---------------------------------------------------------------------------------
def run_patched(trials, batches, hooks, table, flags, status, store=None, refs=None, kl=None):
    """The patched trials of ONE conv, without a host sync: trials.guarded_trial for trial i with
    ``table[i]``, ``flags[i]``, its status words ``status[i]`` and, with ``refs``, ``kl[i]``."""
    for i, tr in enumerate(trials):
        guarded_trial(hooks, tr, status[i], batches, store, refs, table[i], None if kl is None else kl[i], flags[i])


def _figures(row, kl_row=None):
    """What a table reports of a patched trial's raw statistics: (loss,), with a KL row (loss, top-1, KL)."""
    if kl_row is None:
        return (row[0] / row[3],)
    return row[0] / row[3], row[1] / row[2], kl_row[0] / kl_row[1]


def sweep(groups, batches, hooks, device, out, counts, progress=None, plan=None, refs=None):
    """Every trial of ``groups`` ([(patchable?, [Trial or Semilayer, ...]), ...], one group per conv):
    the patched ones conv by conv (one host sync per conv), then the slow ones (convs that are not
    patchable, overflowed trials) through ``hooks.slow(trial)``. ``refs``: None for the delta-loss
    table (a trial's figures are (loss,), hooks.slow gives the loss), the reference softmax per batch
    for the semilayer table (figures (loss, top-1, KL), every batch scored against its reference,
    hooks.slow gives (acc, loss, kl)). ``out(trial, *figures, slow, row)``, with ``refs``
    ``out(trial, *figures, slow, row, kl_row)``, receives every result (``row`` / ``kl_row``: a patched
    trial's raw statistics, else None); a constant channel makes its
    trial's figures nan and is listed in ``counts``, the bookkeeping (``rows_patched`` and ``max_rows``
    are kept when it has them). ``plan`` (suffix.Plan or None): the groups are visited in block order
    and the patched trials of a block run from its kept inputs (suffix.enter, whose self-check also
    compares the KL statistics with ``refs``); the store is released when the block changes, after
    the last patched trial and on any exception."""
    what = "delta-loss" if refs is None else "semilayer"
    blank = (math.nan,) * (1 if refs is None else 3)
    none = (None,) if refs is None else (None, None)  # a trial without raw statistics
    slow = []
    done = 0
    if plan is not None:  # block order (stable), so that the store is filled once per block
        groups = sorted(groups, key=lambda g: hooks.block_of(g[1][0].conv))
    try:
        for fast, trials in groups:
            if not fast:
                slow += [(tr, "not_patchable") for tr in trials]
                continue
            store = None if plan is None else _suffix.enter(plan, hooks, trials[0].conv, batches, device, refs)
            widths = [len(tr.channels) for tr in trials]
            table = torch.zeros(len(trials), 4, dtype=torch.float64, device=device)
            kl = None if refs is None else torch.zeros(len(trials), 2, dtype=torch.float64, device=device)
            flags = torch.zeros(len(trials), 2, dtype=torch.int32, device=device)
            words = torch.zeros(sum(widths), dtype=torch.int32, device=device)
            run_patched(trials, batches, hooks, table, flags, torch.split(words, widths), store, refs, kl)
            rows, kls = table.tolist(), [None] * len(trials) if kl is None else kl.tolist()
            fl, st = flags.tolist(), words.tolist()  # the conv's one host sync
            at = 0
            for tr, n, row, klrow, (ovf, stale) in zip(trials, widths, rows, kls, fl):
                const = [(tr.lnum, c, b) for c, b, word in zip(tr.channels, tr.bits, st[at:at + n]) if word]
                at += n
                if stale:
                    raise RuntimeError("smpq: the model's weights changed while the %s sweep ran" % what)
                if const:  # the whole trial nan, its constant channels listed
                    counts["constant"] += const
                    out(tr, *blank, False, *none)
                elif ovf:
                    counts["overflowed"] += 1
                    slow.append((tr, "overflow"))
                else:
                    counts["patched"] += 1
                    if "rows_patched" in counts:
                        counts["rows_patched"] += n
                        counts["max_rows"] = max(counts["max_rows"], n)
                    out(tr, *_figures(row, klrow), False, *((row,) if kl is None else (row, klrow)))
            done += len(trials)
            if progress is not None:
                progress(done, counts)
    finally:
        if plan is not None:
            plan.store.release()
    for tr, why in slow:
        counts["slow"][why] = counts["slow"].get(why, 0) + 1
        try:
            got = hooks.slow(tr)
            figures = (got,) if refs is None else (got[1], got[0], got[2])
        except ZeroDivisionError:  # the reference raises on a constant channel (functions.py:40)
            counts["constant"] += [(tr.lnum, c, b) for c, b in zip(tr.channels, tr.bits)]
            figures = blank
        out(tr, *figures, True, *none)
        done += 1
        if progress is not None:
            progress(done, counts)


def sweep_rows(groups, batches, refs, hooks, device, out, counts, progress=None, plan=None):
    """sweep with ``refs`` (the semilayer table's call, in its earlier argument order)."""
    sweep(groups, batches, hooks, device, out, counts, progress, plan, refs)


def _select(net, lnums, channels):
    convs = assignments.addressable_convs(net)
    lnums = list(range(1, len(convs) + 1)) if lnums is None else [int(v) for v in lnums]
    cols = []
    for ln in lnums:
        if not 1 <= ln <= len(convs):
            raise ValueError("smpq: lnum %d outside 1..%d" % (ln, len(convs)))
        conv = assignments.conv_for_lnum(net, ln)
        if channels is None:
            chans = range(conv.out_channels)
        elif isinstance(channels, dict):
            chans = channels.get(ln, range(conv.out_channels))
        else:
            chans = channels
        for c in chans:
            if not 0 <= int(c) < conv.out_channels:
                raise ValueError("smpq: channel %d outside lnum %d's %d channels" % (c, ln, conv.out_channels))
            cols.append((ln, conv, int(c)))
    return cols


class _Run:
    """What both tables do around their sweep: the baseline before it, the report after it."""

    def __init__(self, what, net, batches, want_probs):
        """The baseline of the ``what`` sweep: one ordinary evaluation installs the static ranges
        (``eval_loss``; with ``want_probs`` its softmax outputs ``eval_outs``), the hooks are bound to
        them, one unpatched pass of the trials' own forward captures every graph (``base``: its
        statistics, ``base_loss``; ``base_probs``) and must hold."""
        self.what, self.net = what, net
        self.before, self.t0 = counters(), time.perf_counter()
        if want_probs:
            _, self.eval_loss, self.eval_outs = ordinary_eval(net, batches)
        else:
            self.eval_loss, self.eval_outs = ordinary_loss(net, batches), None
        self.hooks = EngineHooks(net, batches)
        self.cal = self.hooks.rebind()
        device = next(net.parameters()).device
        self.base, flags, self.base_probs = unpatched_pass(self.hooks, batches, device, want_probs)
        if any(flags) or engine._signature(net) != self.cal.sig:
            raise RuntimeError("smpq: the baseline of the %s sweep did not hold (overflow or changed weights)" % what)
        self.base_loss = self.base[0] / self.base[3]
        self.plan = None

    def suffix_plan(self, budget, base_kl=None, rows=False):
        """Visit the convs in block order through a suffix.Plan bound to the hooks."""
        self.plan = _suffix.Plan(budget, self.base, base_kl, first=_suffix.first_block(self.net), rows=rows)
        self.hooks.plan = self.plan

    def start(self):
        """The baseline ends here (the unpatched pass ended in a host read), the trials begin."""
        self.mid, self.t1 = counters(), time.perf_counter()
        return {"patched": 0, "overflowed": 0, "slow": {}, "constant": []}

    def report(self, trials, counts, shard):
        """The trials ended (the last conv's in a host read): the model must be what the baseline left
        unless a slow trial ran; the table's report()."""
        after, t2 = counters(), time.perf_counter()
        if not counts["slow"] and (engine._signature(self.net) != self.cal.sig
                                   or engine.model_state(self.net).ranges is not self.cal):
            raise RuntimeError("smpq: the model changed while the %s sweep ran" % self.what)
        rep = dict(counts, slow=dict(counts["slow"]), constant=list(counts["constant"]))
        rep.update(trials=trials, baseline=dict(zip(COUNTERS, (m - b for m, b in zip(self.mid, self.before)))),
                   during_trials=dict(zip(COUNTERS, (a - m for a, m in zip(after, self.mid)))),
                   baseline_s=self.t1 - self.t0, trials_s=t2 - self.t1,
                   suffix=self.plan.report() if self.plan is not None else {})
        for k, a, b in zip(("calibrations", "captures", "repacks"), after, self.before):  # totals of the whole call
            rep[k] = a - b
        if shard is not None:
            rep["shard"] = list(shard)
        return rep


def delta_loss_table(net, batches, bits=(8, 6, 4), lnums=None, channels=None, progress=None, suffix=None,
                     suffix_bytes=None, rows=None, shard=None):
    """The delta-loss table of ``net`` on ``batches`` (a list of (x, y) device tensors, or a
    ResidentSet): for every selected conv (``lnums``, default all searched convs in
    assignments.conv_for_lnum's numbering), channel (``channels``: None = all, a sequence for every
    conv, or {lnum: sequence}) and bit-width, loss(with that one channel quantized) - loss(as it is),
    the loss being functions.evaluate_loss's: the mean over batches of the batch-mean cross entropy.
    Static range mode on the GPU without a data-parallel group; ValueError otherwise.

    One ordinary evaluation installs the static ranges (the sweep's only calibration); one pass of
    the sweep's own replays over the unpatched model captures the graphs and gives ``base_loss``.
    Patched trials reuse those ranges: their logits differ from a freshly calibrated evaluation of
    the quantized model below the activation code step. The model, its operands, ranges and graphs
    are left bitwise as the baseline made them, unless a slow trial ran (those rewrite and restore
    the model's tensors, after every patched trial is done). ``progress(done, counts)``: called
    after every conv.

    ``suffix`` (None: SMPQ_TRIAL_SUFFIX, off by default): the convs are visited in block order and
    the trials of a deep enough block (smpq.suffix.MIN_SKIPPED) forward only the blocks from that one
    on, eagerly, from block inputs kept by one prefix pass per block under ``suffix_bytes`` (None:
    SMPQ_TRIAL_SUFFIX_GB, else unbounded); same statistics bit for bit, ``report()["suffix"]`` says
    what was kept.

    ``rows`` (None: SMPQ_TRIAL_ROWS, off by default; honoured only with the suffix on): a trial of a
    resumed block's LAST conv (conv3 of a Bottleneck, conv2 of a BasicBlock; not the net's last block)
    computes only the patched output channel (ops.trial_rows_conv), in place into the kept input of
    the next block, and resumes from that block; same statistics bit for bit, ``report()["suffix"]``
    says per block whether the route was used or why not.

    ``shard=(rank, world)`` (None: every trial): this call runs only the trials of the columns
    shard_owner gives ``rank`` and pays the whole baseline (and, per block it visits, the prefix pass
    and self-checks); a conv of which it owns nothing is skipped. The table has every column, nan
    outside ``table.owned``; merge_delta_loss of the ``world`` tables is the unsharded table bit for
    bit. dp.sharded_delta_loss_table runs one rank of it and gathers."""
    shard = check_shard(shard)
    use_suffix, budget = _suffix.switch(suffix, suffix_bytes)
    use_rows = _suffix.rows_switch(rows, use_suffix)
    bits = tuple(sorted({int(b) for b in bits}, reverse=True))
    if not bits or bits[-1] < 1 or bits[0] > 16:
        raise ValueError("smpq: bit-widths must be within 1..16")
    p, batches = setup("delta_loss_table", net, batches)
    cols = _select(net, lnums, channels)
    owned = None if shard is None else shard_owner(shard[1], lnum=[ln for ln, _, _ in cols]) == shard[0]

    run = _Run("delta-loss", net, batches, False)
    eval_loss, base_loss = run.eval_loss, run.base_loss
    if use_suffix:
        run.suffix_plan(budget, rows=use_rows)
    counts = run.start()

    groups = []
    by_conv = {}
    for col, (ln, conv, c) in enumerate(cols):
        by_conv.setdefault(ln, (conv, []))[1].append((col, c))
    const_rows = {ln: constant_rows(conv) for ln, (conv, _) in by_conv.items()}
    delta = {bit: np.full(len(cols), np.nan, dtype=np.float64) for bit in bits}
    for ln, (conv, chans) in by_conv.items():
        bn = bn_for(net, conv)
        trials = []
        for col, c in chans:
            if owned is not None and not owned[col]:
                continue
            for bit in bits:
                if const_rows[ln][c]:  # the reference raises there (functions.py:40): nan, listed
                    counts["constant"].append((ln, c, bit))
                else:
                    trials.append(Trial(col, ln, conv, c, bit))
        ok = {c: patchable(conv, bn, c) for _, c in chans}
        fast = [tr for tr in trials if ok[tr.channel]]
        rest = [tr for tr in trials if not ok[tr.channel]]
        if fast:
            groups.append((True, fast))
        if rest:
            groups.append((False, rest))

    trial_stats = {bit: np.full((len(cols), 4), np.nan, dtype=np.float64) for bit in bits}

    def out(tr, loss, slow, row):
        delta[tr.bit][tr.col] = loss - (eval_loss if slow else base_loss)
        if row is not None:
            trial_stats[tr.bit][tr.col] = row

    with torch.no_grad():
        sweep(groups, batches, run.hooks, p.device, out, counts, progress, run.plan)
    mine = len(cols) if owned is None else int(owned.sum())
    table = DeltaLossTable(arch_of(net), [ln for ln, _, _ in cols], [c for _, _, c in cols], bits, delta, base_loss,
                           eval_loss, run.report(mine * len(bits), counts, shard))
    table.stats = trial_stats
    table.owned = owned
    return table


# ---- semilayer trials: many rows of one conv per trial -------------------------------
class SemilayerTable:
    """One entry per semilayer, in the order given: ``lnum``, ``channels``, ``bits``, ``param``;
    ``loss`` (mean over batches of the batch-mean cross entropy), ``acc`` (top-1), ``kl``
    (functions.KLdiv's sum / images against the reference outputs) as float64 arrays, nan for a
    semilayer with a constant channel; ``stats`` [., 4] and ``kl_stats`` [., 2] the raw statistics
    of a patched trial (nan rows for slow ones); ``slow`` marks the trials that ran through the
    public API. ``base_loss`` / ``eval_loss`` as in DeltaLossTable; ``owned``: None, or the bool
    array of the semilayers a sharded call ran (the others are nan; merge_semilayers)."""

    def __init__(self, arch, sems, base_loss, eval_loss, report=None, arrays=None):
        """``sems``: the Semilayers; or None with ``arrays``: their (lnum, channels, bits, param)."""
        lnum, channels, bits, param = arrays or ([s.lnum for s in sems], [s.channels for s in sems],
                                                 [s.bits for s in sems], [s.param for s in sems])
        n = len(lnum)
        self.arch = arch
        self.lnum = np.asarray(lnum, dtype=np.int64)
        self.channels = [list(c) for c in channels]
        self.bits = [list(b) for b in bits]
        self.param = np.asarray(param, dtype=np.float64)
        self.loss = np.full(n, np.nan, dtype=np.float64)
        self.acc = np.full(n, np.nan, dtype=np.float64)
        self.kl = np.full(n, np.nan, dtype=np.float64)
        self.stats = np.full((n, 4), np.nan, dtype=np.float64)
        self.kl_stats = np.full((n, 2), np.nan, dtype=np.float64)
        self.slow = np.zeros(n, dtype=bool)
        self.owned = None
        self.base_loss, self.eval_loss = base_loss, eval_loss
        self._report = dict(report or {})

    def report(self):
        """delta_loss_table's counters, plus ``rows_patched`` (rows over all patched trials) and
        ``max_rows`` (the largest n of one patch)."""
        return dict(self._report)


def _semilayers(net, semilayers):
    convs = assignments.addressable_convs(net)
    sems = []
    for index, (ln, channels, bit) in enumerate(semilayers):
        ln = int(ln)
        if not 1 <= ln <= len(convs):
            raise ValueError("smpq: lnum %d outside 1..%d" % (ln, len(convs)))
        conv = assignments.conv_for_lnum(net, ln)
        channels = [int(c) for c in channels]
        bits = [int(bit)] * len(channels) if isinstance(bit, (int, np.integer)) else [int(b) for b in bit]
        if not channels or len(bits) != len(channels):
            raise ValueError("smpq: semilayer %d needs channels and one bit-width, or one per channel" % index)
        if len(set(channels)) != len(channels):
            raise ValueError("smpq: semilayer %d lists a channel twice" % index)
        if min(channels) < 0 or max(channels) >= conv.out_channels:
            raise ValueError("smpq: semilayer %d has a channel outside lnum %d's %d channels" % (index, ln, conv.out_channels))
        if min(bits) < 1 or max(bits) > 16:
            raise ValueError("smpq: bit-widths must be within 1..16")
        sems.append(Semilayer(index, ln, conv, channels, bits, conv.weight[0].numel()))
    return sems


def semilayer_table(net, batches, semilayers, reference_outputs=None, progress=None, suffix=None, suffix_bytes=None,
                    shard=None):
    """The reference's semilayer sensitivity pass (functions._make_semilayers) on ``net`` as it is:
    for every ``(lnum, channels, bit)`` of ``semilayers`` (``bit``: one int or one per channel), the
    loss, top-1 accuracy and KL divergence against ``reference_outputs`` of the model with THOSE
    channels of that conv quantized, every semilayer starting from the same model. Returns a
    SemilayerTable. Preconditions and ValueErrors are delta_loss_table's.

    ``reference_outputs``: the per-batch softmax list functions.KLdiv takes; None = the softmax of
    the unpatched pass (of the ordinary evaluation for slow trials), so no change gives KL exactly 0.
    A trial patches the semilayer's rows of the conv's packed operand in one launch
    (ops.trial_rows_patch), replays the captured graphs, scores every batch eagerly and restores;
    it runs under the baseline's ranges, as delta_loss_table's trials do. Semilayers that are not
    patchable_rows and overflowed trials run afterwards through the public API on the model itself,
    which is restored bitwise after each. ``suffix`` / ``suffix_bytes``: as in delta_loss_table.
    ``shard=(rank, world)``: only the semilayers shard_owner gives ``rank`` (position i of
    ``semilayers`` -> rank i % world) are run, after the whole baseline; ``table.owned`` marks them and
    merge_semilayers joins the parts."""
    shard = check_shard(shard)
    use_suffix, budget = _suffix.switch(suffix, suffix_bytes)
    p, batches = setup("semilayer_table", net, batches)
    sems = _semilayers(net, semilayers)
    owned = None if shard is None else shard_owner(shard[1], count=len(sems)) == shard[0]
    if reference_outputs is not None:
        reference_outputs = [r.to(p.device) for r in reference_outputs]

    run = _Run("semilayer", net, batches, True)
    hooks = run.hooks
    if reference_outputs is not None and len(reference_outputs) != len(run.base_probs):  # (a ResidentSet has no len)
        raise ValueError("smpq: reference_outputs must hold one softmax tensor per batch")
    # what slow trials are compared with, and the patched ones
    hooks.reference = run.eval_outs if reference_outputs is None else reference_outputs
    refs = run.base_probs if reference_outputs is None else reference_outputs
    if reference_outputs is not None:
        run.eval_outs = None
    if use_suffix:  # what a block's self-check must reproduce: the unpatched pass's KL statistics too
        run.suffix_plan(budget, kl_stats(refs, run.base_probs))
    counts = dict(run.start(), rows_patched=0, max_rows=0)

    table = SemilayerTable(arch_of(net), sems, run.base_loss, run.eval_loss)
    table.owned = owned
    by_conv = {}
    for sem in sems:
        if owned is None or owned[sem.index]:
            by_conv.setdefault(sem.lnum, []).append(sem)
    groups = []
    with torch.no_grad():
        for ln, group in by_conv.items():
            conv = group[0].conv
            bn = bn_for(net, conv)
            const_rows = constant_rows(conv)
            fast, rest = [], []
            for sem in group:
                const = [(ln, c, b) for c, b in zip(sem.channels, sem.bits) if const_rows[c]]
                if const:  # the reference raises there (functions.py:40): the whole semilayer nan, listed
                    counts["constant"] += const
                elif patchable_rows(conv, bn, sem.channels):
                    fast.append(sem)
                else:
                    rest.append(sem)
            if fast:
                hooks.prepare(fast)
                groups.append((True, fast))
            if rest:
                groups.append((False, rest))

    def out(sem, loss, acc, klv, slow, row, kl_row):
        i = sem.index
        table.loss[i], table.acc[i], table.kl[i], table.slow[i] = loss, acc, klv, slow
        if row is not None:
            table.stats[i], table.kl_stats[i] = row, kl_row

    with torch.no_grad():
        sweep(groups, batches, hooks, p.device, out, counts, progress, run.plan, refs)
    table._report = run.report(len(sems) if owned is None else int(owned.sum()), counts, shard)
    return table


# ---- merging the tables of a sharded call (host only) -------------------------------
def _same_bits(a, b):
    """Two losses equal as bits (float64), None only with None. No tolerance on purpose: every rank
    computed the baseline from the same model and data, so a difference is a fault to be reported."""
    if a is None or b is None:
        return a is None and b is None
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _parts(tables):
    tables = list(tables)
    if not tables:
        raise ValueError("smpq: nothing to merge")
    return tables


def _merge_owned(tables, n, what):
    """The part that owns each of ``n`` columns (int array), after checking the parts' baselines and
    that their ``owned`` masks are disjoint and cover every column (None counts as all true)."""
    first = tables[0]
    for i, t in enumerate(tables):
        if t.arch != first.arch:
            raise ValueError("smpq: part %d is a table of %s, part 0 of %s" % (i, t.arch, first.arch))
        shard = t.report().get("shard")
        if shard is not None and list(shard) != [i, len(tables)]:
            raise ValueError("smpq: part %d is shard %r of its call, not (%d, %d): the parts go in rank order, all of them"
                             % (i, tuple(shard), i, len(tables)))
        for name in ("base_loss", "eval_loss"):
            if not _same_bits(getattr(t, name), getattr(first, name)):
                raise ValueError("smpq: part %d has %s %r, part 0 has %r: the ranks did not see the same model and data"
                                 % (i, name, getattr(t, name), getattr(first, name)))
    part = np.full(n, -1, dtype=np.int64)
    for i, t in enumerate(tables):
        owned = np.ones(n, dtype=bool) if t.owned is None else np.asarray(t.owned, dtype=bool)
        if owned.shape != (n,):
            raise ValueError("smpq: part %d's owned mask has shape %r for %d %ss" % (i, owned.shape, n, what))
        twice = np.flatnonzero(owned & (part >= 0))
        if twice.size:
            raise ValueError("smpq: %s %d is owned by part %d and part %d" % (what, twice[0], part[twice[0]], i))
        part[owned] = i
    missing = np.flatnonzero(part < 0)
    if missing.size:
        raise ValueError("smpq: %s %d is owned by no part" % (what, missing[0]))
    return part


def _merge_report(tables, extra=()):
    reps = [t.report() for t in tables]
    slow = {}
    for r in reps:
        for why, k in r.get("slow", {}).items():
            slow[why] = slow.get(why, 0) + k
    out = {k: sum(r.get(k, 0) for r in reps) for k in ("trials", "patched", "overflowed") + tuple(extra)}
    out["slow"] = slow
    out["constant"] = sorted(tuple(c) for r in reps for c in r.get("constant", ()))
    out["world"] = len(tables)
    out["baseline_s"] = max(r.get("baseline_s", 0.0) for r in reps)
    out["trials_s"] = max(r.get("trials_s", 0.0) for r in reps)
    out["ranks"] = reps
    return out


def merge_delta_loss(tables):
    """The complete DeltaLossTable (``owned`` None) of the tables that the ranks of one sharded
    delta_loss_table call returned, in rank order. Every column's deltas and trial statistics are
    copied, as they are, from the part that owns it; nothing is averaged or recomputed, so the
    result is the unsharded table bit for bit. ValueError, naming the first offending part or
    column, unless arch, columns and bit-widths are the same, ``base_loss`` and ``eval_loss`` are
    equal as bits in every part, and the ``owned`` masks are disjoint and cover every column.
    report(): trials, patched, overflowed and slow summed, constant concatenated and sorted,
    ``world``, ``ranks`` (the parts' reports in rank order), baseline_s / trials_s the maximum."""
    tables = _parts(tables)
    first = tables[0]
    for i, t in enumerate(tables):
        if t.bits != first.bits:
            raise ValueError("smpq: part %d has bit-widths %r, part 0 has %r" % (i, t.bits, first.bits))
        if t.lnum.shape != first.lnum.shape:
            raise ValueError("smpq: part %d has %d columns, part 0 has %d" % (i, len(t.lnum), len(first.lnum)))
        differ = np.flatnonzero((t.lnum != first.lnum) | (t.cnum != first.cnum))
        if differ.size:
            raise ValueError("smpq: column %d is (lnum %d, channel %d) in part %d and (lnum %d, channel %d) in part 0"
                             % (differ[0], t.lnum[differ[0]], t.cnum[differ[0]], i, first.lnum[differ[0]],
                                first.cnum[differ[0]]))
    n = len(first.lnum)
    part = _merge_owned(tables, n, "column")
    delta = {b: np.full(n, np.nan, dtype=np.float64) for b in first.bits}
    stats_ = {b: np.full((n, 4), np.nan, dtype=np.float64) for b in first.bits}
    for i, t in enumerate(tables):
        mine = part == i
        for b in first.bits:
            delta[b][mine] = t.delta[b][mine]
            if b in t.stats:
                stats_[b][mine] = t.stats[b][mine]
    out = DeltaLossTable(first.arch, first.lnum, first.cnum, first.bits, delta, first.base_loss, first.eval_loss,
                         _merge_report(tables))
    out.stats = stats_
    return out


def merge_semilayers(tables):
    """merge_delta_loss for the SemilayerTables of one sharded semilayer_table call: ``loss``,
    ``acc``, ``kl``, ``stats``, ``kl_stats`` and ``slow`` of every semilayer come from the part that
    owns it. The parts must list the same semilayers (lnum, channels, bits). report() also sums
    ``rows_patched`` and takes the maximum of ``max_rows``."""
    tables = _parts(tables)
    first = tables[0]
    for i, t in enumerate(tables):
        if len(t.channels) != len(first.channels):
            raise ValueError("smpq: part %d has %d semilayers, part 0 has %d" % (i, len(t.channels), len(first.channels)))
        for j in range(len(first.channels)):
            if int(t.lnum[j]) != int(first.lnum[j]) or t.channels[j] != first.channels[j] or t.bits[j] != first.bits[j]:
                raise ValueError("smpq: semilayer %d of part %d is not part 0's" % (j, i))
    n = len(first.channels)
    part = _merge_owned(tables, n, "semilayer")
    out = SemilayerTable(first.arch, None, first.base_loss, first.eval_loss,
                         arrays=(first.lnum, first.channels, first.bits, first.param))
    for i, t in enumerate(tables):
        mine = part == i
        for name in ("loss", "acc", "kl", "stats", "kl_stats", "slow"):
            getattr(out, name)[mine] = getattr(t, name)[mine]
    rep = _merge_report(tables, extra=("rows_patched",))
    rep["max_rows"] = max(r.get("max_rows", 0) for r in rep["ranks"])
    out._report = rep
    return out
