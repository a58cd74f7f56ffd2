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
import types

import numpy as np
import torch

from . import assignments, checkpoint, engine, ops
from . import suffix as _suffix  # (the tables have a ``suffix`` argument)
from .batches import ResidentSet
from .qconv import QConv2d, stats
from .quant import channel_wise_quantizationperchan, check_pending


def bn_for(net, conv):
    """The BatchNorm the engine folds onto ``conv`` (convN -> bnN of its block), or None."""
    for b in assignments.blocks_of(net):
        for i in (1, 2, 3):
            if getattr(b, "conv%d" % i, None) is conv:
                return getattr(b, "bn%d" % i, None)
    return None


def patchable(conv, bn, channel=None):
    """Can a trial of ``conv`` (folded with ``bn``) patch its packed operand in place? True when
      * the conv has a ConvPlan whose codes are [LW, cout, K] with LW >= 2 and no offsets (kinds
        'fixed' and 'exact16': every row coded independently of the others);
      * another channel stays unquantized whichever channel is tried (``channel``: besides that
        one), so the normal path would pack the quantized model with the same LW: a trial that
        completes a conv would turn it 'exact8' there;
      * the K-major copy on the codes is there exactly when ops.KMAJOR is on;
      * K is within the patch kernel's row limit."""
    free = _patchable_operand(conv, bn)
    if free is None:
        return False
    others = int(free.sum()) - (1 if channel is None or free[int(channel)] else 0)
    return others >= 1


def _patchable_operand(conv, bn):
    """patchable's conditions on the operand alone: the conv's free (unquantized) channel mask, or
    None when its packed operand cannot be patched in place whatever the channels."""
    if not isinstance(conv, QConv2d):
        return None
    plan = engine.conv_plan(conv, bn)
    if plan is None or plan.codes.dim() != 3 or plan.codes.shape[0] < 2 or plan.offset is not None:
        return None
    if (getattr(plan.codes, "_smpq_km", None) is not None) != bool(ops.KMAJOR[0]):
        return None
    if plan.codes.shape[2] % 64 != 0 or plan.codes.shape[2] > ops.TRIAL_MAX_K:
        return None
    return np.asarray(conv._bits_host <= 0)


def patchable_rows(conv, bn, channels):
    """patchable for a semilayer trial: patchable's conditions on the operand, and at least one
    channel OUTSIDE ``channels`` is unquantized (a semilayer that completes a conv would be packed
    'exact8' on the normal path, with another LW)."""
    free = _patchable_operand(conv, bn)
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
    if not isinstance(conv, QConv2d):
        return False
    plan = engine.conv_plan(conv, bn)
    if plan is None or getattr(plan, "kind", None) != "exact8" or plan.codes.dim() != 3 or plan.codes.shape[0] != 1:
        return False
    if (getattr(plan.codes, "_smpq_km", None) is not None) != bool(ops.KMAJOR[0]):
        return False
    if plan.codes.shape[2] % 64 != 0 or plan.codes.shape[2] > ops.TRIAL_MAX_K:
        return False
    if not conv.fully_quantized():
        return False
    bits = [bits] if isinstance(bits, (int, np.integer)) else list(bits)
    return len([int(c) for c in channels]) > 0 and all(1 <= int(b) <= 8 for b in bits)


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
class Trial:
    __slots__ = ("col", "lnum", "conv", "channel", "bit")

    def __init__(self, col, lnum, conv, channel, bit):
        self.col, self.lnum, self.conv, self.channel, self.bit = col, lnum, conv, channel, bit


def _or_flags(dst, ovf):
    torch.bitwise_or(dst, ovf, out=dst)


def _walk(batches, store):
    """(kept input or None, x, y) per batch: the store's walk, or every batch in full without one."""
    return ((None, x, y) for x, y in batches) if store is None else store.walk(batches)


def run_patched(trials, batches, hooks, table, flags, status, store=None):
    """The patched trials of ONE conv, without a host sync: for trial i patch, forward every batch
    into ``table[i]`` (float64 [4] softmax_xent statistics), OR the replays' flags into ``flags[i]``
    (int32 [2]: overflow, stale content), restore. ``status[i]`` is the patch's constant-channel
    word. ``hooks``: patch(trial, status_word), restore(trial), forward(x) -> (logits, flag tensor),
    score(logits, y, row), invalidate(trial). The restore runs whatever happens; after an exception
    the conv's operand is also marked for repacking (invalidate), then the exception goes on.
    ``store`` (suffix.Store of the conv's block, or None): a batch it keeps runs through
    hooks.resume(kept, block) instead, from the kept block input on; when the conv is
    the block's last and the store holds the rows route's tensors (``store.rows``),
    through hooks.resume_rows(kept, block, channel): the patched channel alone is recomputed into
    the kept input of the next block, which is put back before the operand is."""
    for i, tr in enumerate(trials):
        failed = False
        rows = store is not None and store.rows is not None and store.rows is tr.conv
        if rows:
            store.row["rows_trials"] += 1
        try:
            hooks.patch(tr, status[i:i + 1])
            for kept, x, y in _walk(batches, store):
                if kept is None:
                    logits, ovf = hooks.forward(x)
                elif rows and kept.rows is not None:
                    logits, ovf = hooks.resume_rows(kept, store.block, tr.channel)
                else:
                    logits, ovf = hooks.resume(kept, store.block)
                _or_flags(flags[i], ovf)
                hooks.score(logits, y, table[i])
        except BaseException:
            failed = True
            raise
        finally:
            hooks.restore(tr)
            if failed:
                hooks.invalidate(tr)


def _by_block(groups, hooks):
    """``groups`` in block order (stable), so that a table fills the store once per block."""
    return sorted(groups, key=lambda g: hooks.block_of(g[1][0].conv))


def sweep(groups, batches, hooks, device, out, counts, progress=None, plan=None):
    """Every trial of ``groups`` ([(patchable?, [Trial, ...]), ...], one group per conv): the
    patched ones conv by conv (one host sync per conv), then the slow ones (convs that are not
    patchable, overflowed trials) through ``hooks.slow(trial) -> loss``. ``out(trial, loss, slow, row)``
    receives every result (``row``: a patched trial's four statistics, else None); ``counts`` the bookkeeping.
    ``plan`` (suffix.Plan or None): the groups are visited in block order and the patched trials of
    a block run from its kept inputs (suffix.enter); the store is released when the block changes,
    after the last patched trial and on any exception."""
    slow = []
    done = 0
    if plan is not None:
        groups = _by_block(groups, hooks)
    try:
        for fast, trials in groups:
            if not fast:
                slow += [(tr, "not_patchable") for tr in trials]
                continue
            store = None if plan is None else _suffix.enter(plan, hooks, trials[0].conv, batches, device)
            table = torch.zeros(len(trials), 4, dtype=torch.float64, device=device)
            flags = torch.zeros(len(trials), 2, dtype=torch.int32, device=device)
            status = torch.zeros(len(trials), dtype=torch.int32, device=device)
            run_patched(trials, batches, hooks, table, flags, status, store)
            rows, fl, st = table.tolist(), flags.tolist(), status.tolist()  # the conv's one host sync
            for tr, row, (ovf, stale), const in zip(trials, rows, fl, st):
                if stale:
                    raise RuntimeError("smpq: the model's weights changed while the delta-loss sweep ran")
                if const:
                    counts["constant"].append((tr.lnum, tr.channel, tr.bit))
                    out(tr, math.nan, False, None)
                elif ovf:
                    counts["overflowed"] += 1
                    slow.append((tr, "overflow"))
                else:
                    counts["patched"] += 1
                    out(tr, row[0] / row[3], False, row)
            done += len(trials)
            if progress is not None:
                progress(done, counts)
    finally:
        if plan is not None:
            plan.store.release()
    for tr, why in slow:
        counts["slow"][why] = counts["slow"].get(why, 0) + 1
        try:
            loss = hooks.slow(tr)
        except ZeroDivisionError:  # the reference raises on a constant channel (functions.py:40)
            counts["constant"].append((tr.lnum, tr.channel, tr.bit))
            loss = math.nan
        out(tr, loss, True, None)
        done += 1
        if progress is not None:
            progress(done, counts)


class _EngineHooks(_suffix.EngineHooks):
    """The sweep's hooks on the real engine: ``cal`` the StaticRanges installed by the baseline.
    (suffix.EngineHooks adds what a table with a suffix.Plan calls: block_of, fill, resume.)"""

    def __init__(self, net, cal, batches):
        self.net, self.cal, self.batches = net, cal, batches
        self._conv = None
        self._state = None

    def _bind(self, conv):
        if self._conv is not conv:
            bn = bn_for(self.net, conv)
            plan = engine.conv_plan(conv, bn)
            with torch.no_grad():
                a = engine._bn_fold(bn)[0].contiguous() if bn is not None else torch.ones_like(plan.col_scale)
                wscale = conv.packed()[3]
                lw, _, K = plan.codes.shape
                self._save = torch.empty(ops.trial_save_bytes(lw, K), dtype=torch.int8, device=plan.codes.device)
            self._conv, self._plan, self._a, self._wscale = conv, plan, a, wscale
            self._km = getattr(plan.codes, "_smpq_km", None)

    def patch(self, tr, status):
        self._bind(tr.conv)
        self.new_trial()
        ops.trial_row_patch(tr.conv.weight.detach(), tr.channel, tr.bit, self._a, self._plan.codes, self._wscale,
                            self._plan.col_scale, self._save, status, km=self._km)

    def restore(self, tr):
        ops.trial_row_restore(tr.channel, self._plan.codes, self._wscale, self._plan.col_scale, self._save, km=self._km)

    def invalidate(self, tr):
        tr.conv._content_gen += 1

    def forward(self, x):
        if engine.USE_GRAPH[0]:
            return engine._graph_forward(self.net, x, self.cal)
        return engine._static_eager(self.net, x, self.cal)

    def score(self, logits, y, row):
        ops.softmax_xent(logits.float().contiguous(), y, row, want_probs=False)

    def slow(self, tr):
        """One trial through the public API on the model itself: quantize the channel, evaluate as
        functions.evaluate_loss does, put weight and metadata back bitwise."""
        if self._state is None:
            self._state = checkpoint.snapshot(self.net)
        try:
            channel_wise_quantizationperchan(tr.conv.weight.data, tr.bit, tr.channel)
            check_pending()
            return ordinary_loss(self.net, self.batches)
        finally:
            try:
                check_pending()
            except ZeroDivisionError:
                pass
            checkpoint.restore_(self.net, self._state)


def ordinary_loss(net, batches):
    """functions.evaluate_loss on device batches: a fresh calibration on the first batch, the mean
    over batches of the batch-mean cross entropy from float64 statistics (one host sync)."""
    acc = None
    engine.new_evaluation(net)
    with torch.no_grad():
        for x, y in batches:
            out = net(x).float().contiguous()
            if acc is None:
                acc = torch.zeros(4, dtype=torch.float64, device=out.device)
            ops.softmax_xent(out, y, acc, want_probs=False)
    loss_sum, _, _, count = acc.tolist()
    return loss_sum / count


def _unpatched_pass(hooks, batches, device):
    """Every batch through the trials' own forward with no patch: (statistics, flags) on the host.
    (A function of its own: a replay hands out its graph's flag tensor, which lives in the graph
    pool; nothing here outlives the call, so a later release of the graphs frees the pool whole.)"""
    base = torch.zeros(4, dtype=torch.float64, device=device)
    flags = torch.zeros(2, dtype=torch.int32, device=device)
    with torch.no_grad():
        for x, y in batches:
            logits, ovf = hooks.forward(x)
            _or_flags(flags, ovf)
            hooks.score(logits, y, base)
    return base.tolist(), flags.tolist()


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


def _suffix_plan(net, hooks, on, budget, base, base_kl=None, rows=False):
    """The table's suffix.Plan (bound to ``hooks``), or None with the switch off."""
    if not on:
        return None
    hooks.plan = _suffix.Plan(budget, base, base_kl, first=_suffix.first_block(net), rows=rows)
    return hooks.plan


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
    if engine.get_range_mode() != "static":
        raise ValueError("smpq: delta_loss_table needs the static range mode (engine.set_range_mode)")
    if engine.get_dp_group() is not None:
        raise ValueError("smpq: delta_loss_table runs on one GPU (no data-parallel group)")
    p = next(net.parameters())
    if not p.is_cuda or net.training or not getattr(net, "fused", True):
        raise ValueError("smpq: delta_loss_table needs an eval-mode smpq ResNet on the GPU")
    if isinstance(batches, ResidentSet):
        batches.bind(p.device)
    else:
        batches = list(batches)
        if not batches or any(not (torch.is_tensor(x) and x.device == p.device) for x, _ in batches):
            raise ValueError("smpq: batches must be (x, y) pairs with x on the model's device, or a ResidentSet")
        batches = [(x, torch.as_tensor(y).to(p.device)) for x, y in batches]
    cols = _select(net, lnums, channels)
    owned = None if shard is None else shard_owner(shard[1], lnum=[ln for ln, _, _ in cols]) == shard[0]

    before = {k: stats.get(k, 0) for k in ("calibrations", "graph_captures", "repack")}
    t0 = time.perf_counter()
    eval_loss = ordinary_loss(net, batches)
    cal = engine.model_state(net).ranges
    hooks = _EngineHooks(net, cal, batches)
    b, bflags = _unpatched_pass(hooks, batches, p.device)  # captures every graph
    if any(bflags) or engine._signature(net) != cal.sig:
        raise RuntimeError("smpq: the baseline of the delta-loss sweep did not hold (overflow or changed weights)")
    base_loss = b[0] / b[3]
    plan = _suffix_plan(net, hooks, use_suffix, budget, b, rows=use_rows)
    mid = {k: stats.get(k, 0) for k in before}
    t1 = time.perf_counter()  # (the pass above ended in a host read)

    groups = []
    by_conv = {}
    for col, (ln, conv, c) in enumerate(cols):
        by_conv.setdefault(ln, (conv, []))[1].append((col, c))
    with torch.no_grad():
        const_rows = {}
        for ln, (conv, chans) in by_conv.items():
            w2d = conv.weight.detach().reshape(conv.out_channels, -1)
            const_rows[ln] = (w2d.amax(1) == w2d.amin(1)).tolist()
    counts = {"patched": 0, "overflowed": 0, "slow": {}, "constant": []}
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
        sweep(groups, batches, hooks, p.device, out, counts, progress, plan)
    after = {k: stats.get(k, 0) for k in before}
    t2 = time.perf_counter()  # (so did the last conv's trials)
    if not counts["slow"] and (engine._signature(net) != cal.sig or engine.model_state(net).ranges is not cal):
        raise RuntimeError("smpq: the model changed while the delta-loss sweep ran")
    mine = len(cols) if owned is None else int(owned.sum())
    report = {"trials": mine * len(bits), "patched": counts["patched"], "overflowed": counts["overflowed"],
              "slow": dict(counts["slow"]), "constant": list(counts["constant"]),
              "baseline": {k: mid[k] - before[k] for k in before},
              "during_trials": {k: after[k] - mid[k] for k in before},
              "baseline_s": t1 - t0, "trials_s": t2 - t1, "suffix": plan.report() if plan is not None else {}}
    for k in before:  # totals seen during the whole call
        report[{"graph_captures": "captures", "repack": "repacks"}.get(k, k)] = after[k] - before[k]
    if shard is not None:
        report["shard"] = list(shard)
    table = DeltaLossTable(arch_of(net), [ln for ln, _, _ in cols], [c for _, _, c in cols], bits, delta, base_loss,
                           eval_loss, report)
    table.stats = trial_stats
    table.owned = owned
    return table


# ---- semilayer trials: many rows of one conv per trial -------------------------------
class Semilayer:
    """One trial of semilayer_table: ``channels`` (distinct) of conv ``lnum`` at ``bits`` (one
    bit-width per channel). ``param`` is what functions._make_semilayers accumulates: the sum over
    the channels of K * (32 - bit) / 32. ``rows``: the hooks' uploaded lists (ops.TrialRows)."""
    __slots__ = ("index", "lnum", "conv", "channels", "bits", "param", "rows")

    def __init__(self, index, lnum, conv, channels, bits, k_elems):
        self.index, self.lnum, self.conv = index, lnum, conv
        self.channels = [int(c) for c in channels]
        self.bits = [int(b) for b in bits]
        self.param = 0.0
        for b in self.bits:  # in the reference's order of accumulation
            self.param += k_elems * ((32 - b) / 32)
        self.rows = None


class SemilayerTable:
    """One entry per semilayer, in the order given: ``lnum``, ``channels``, ``bits``, ``param``;
    ``loss`` (mean over batches of the batch-mean cross entropy), ``acc`` (top-1), ``kl``
    (functions.KLdiv's sum / images against the reference outputs) as float64 arrays, nan for a
    semilayer with a constant channel; ``stats`` [., 4] and ``kl_stats`` [., 2] the raw statistics
    of a patched trial (nan rows for slow ones); ``slow`` marks the trials that ran through the
    public API. ``base_loss`` / ``eval_loss`` as in DeltaLossTable; ``owned``: None, or the bool
    array of the semilayers a sharded call ran (the others are nan; merge_semilayers)."""

    def __init__(self, arch, sems, base_loss, eval_loss, report=None):
        n = len(sems)
        self.arch = arch
        self.lnum = np.asarray([s.lnum for s in sems], dtype=np.int64)
        self.channels = [list(s.channels) for s in sems]
        self.bits = [list(s.bits) for s in sems]
        self.param = np.asarray([s.param for s in sems], dtype=np.float64)
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


def run_patched_rows(sems, batches, refs, hooks, table, kl, flags, status, store=None):
    """The patched semilayer trials of ONE conv, without a host sync; run_patched with n rows per
    trial. For trial i: patch its rows, forward every batch b and score it against ``refs[b]`` into
    ``table[i]`` (float64 [4]) and ``kl[i]`` (float64 [2]), OR the replays' flags into ``flags[i]``,
    restore. ``status[i]`` is the trial's int32 [n] constant-channel words. Hooks: patch(sem, status),
    restore(sem), forward(x), score_kl(logits, y, ref, row, kl_row), invalidate(sem). ``store``: as
    in run_patched."""
    for i, sem in enumerate(sems):
        failed = False
        try:
            hooks.patch(sem, status[i])
            for (kept, x, y), ref in zip(_walk(batches, store), refs):
                logits, ovf = hooks.forward(x) if kept is None else hooks.resume(kept, store.block)
                _or_flags(flags[i], ovf)
                hooks.score_kl(logits, y, ref, table[i], kl[i])
        except BaseException:
            failed = True
            raise
        finally:
            hooks.restore(sem)
            if failed:
                hooks.invalidate(sem)


def sweep_rows(groups, batches, refs, hooks, device, out, counts, progress=None, plan=None):
    """sweep for semilayer trials. ``groups``: [(patchable?, [Semilayer, ...]), ...], one group per
    conv (one host sync per group); ``refs``: the reference softmax per batch. Results go to
    ``out(sem, loss, acc, kl, slow, row, kl_row)``. A constant channel makes its whole semilayer nan
    and is listed; an overflowed trial is redone by ``hooks.slow(sem) -> (acc, loss, kl)`` after all
    patched trials, with the semilayers that are not patchable. ``plan``: as in sweep (its
    self-check also compares the KL statistics)."""
    nan = math.nan
    slow = []
    done = 0
    if plan is not None:
        groups = _by_block(groups, hooks)
    try:
        for fast, sems in groups:
            if not fast:
                slow += [(sem, "not_patchable") for sem in sems]
                continue
            store = None if plan is None else _suffix.enter(plan, hooks, sems[0].conv, batches, device, refs)
            table = torch.zeros(len(sems), 4, dtype=torch.float64, device=device)
            kl = torch.zeros(len(sems), 2, dtype=torch.float64, device=device)
            flags = torch.zeros(len(sems), 2, dtype=torch.int32, device=device)
            words = torch.zeros(sum(len(s.channels) for s in sems), dtype=torch.int32, device=device)
            status = list(torch.split(words, [len(s.channels) for s in sems]))
            run_patched_rows(sems, batches, refs, hooks, table, kl, flags, status, store)
            rows, kls, fl, st = table.tolist(), kl.tolist(), flags.tolist(), words.tolist()  # the conv's one host sync
            at = 0
            for sem, row, klrow, (ovf, stale) in zip(sems, rows, kls, fl):
                const = [c for c, word in zip(sem.channels, st[at:at + len(sem.channels)]) if word]
                at += len(sem.channels)
                if stale:
                    raise RuntimeError("smpq: the model's weights changed while the semilayer sweep ran")
                if const:
                    counts["constant"] += [(sem.lnum, c, sem.bits[sem.channels.index(c)]) for c in const]
                    out(sem, nan, nan, nan, False, None, None)
                elif ovf:
                    counts["overflowed"] += 1
                    slow.append((sem, "overflow"))
                else:
                    counts["patched"] += 1
                    counts["rows_patched"] += len(sem.channels)
                    counts["max_rows"] = max(counts["max_rows"], len(sem.channels))
                    out(sem, row[0] / row[3], row[1] / row[2], klrow[0] / klrow[1], False, row, klrow)
            done += len(sems)
            if progress is not None:
                progress(done, counts)
    finally:
        if plan is not None:
            plan.store.release()
    for sem, why in slow:
        counts["slow"][why] = counts["slow"].get(why, 0) + 1
        acc, loss, klv = hooks.slow(sem)  # (constant channels never get here: semilayer_table lists them first)
        out(sem, loss, acc, klv, True, None, None)
        done += 1
        if progress is not None:
            progress(done, counts)


class _RowsHooks(_EngineHooks):
    """sweep_rows's hooks on the real engine. ``reference``: what slow trials are compared with."""

    def __init__(self, net, cal, batches, reference):
        super().__init__(net, cal, batches)
        self.reference = reference
        self._rows_save = None

    def prepare(self, sems):
        """Upload the lists of every semilayer of one conv up front and size the save area."""
        conv = sems[0].conv
        self._bind(conv)
        lw, cout, K = self._plan.codes.shape
        for sem in sems:
            sem.rows = ops.trial_rows_lists(sem.channels, sem.bits, cout, self._plan.codes.device)
        need = ops.trial_rows_save_bytes(lw, K, max(len(s.channels) for s in sems))
        if self._rows_save is None or self._rows_save.numel() < need or self._rows_save.device != self._plan.codes.device:
            self._rows_save = torch.empty(need, dtype=torch.int8, device=self._plan.codes.device)

    def patch(self, sem, status):
        self._bind(sem.conv)
        self.new_trial()
        ops.trial_rows_patch(sem.conv.weight.detach(), sem.rows, None, self._a, self._plan.codes, self._wscale,
                             self._plan.col_scale, self._rows_save, status, km=self._km)

    def restore(self, sem):
        ops.trial_rows_restore(sem.rows, self._plan.codes, self._wscale, self._plan.col_scale, self._rows_save, km=self._km)

    def invalidate(self, sem):
        sem.conv._content_gen += 1

    def score_kl(self, logits, y, ref, row, kl_row):
        probs = ops.softmax_xent(logits.float().contiguous(), y, row, want_probs=True)
        ops.kl_rows(ref, probs, kl_row)

    def slow(self, sem):
        """One semilayer through the public API on the model itself: quantize its channels one by
        one, evaluate as functions.evaluate_acc_loss_softmax does, KL against the reference, put
        weights and metadata back bitwise. Returns (acc, loss, kl)."""
        if self._state is None:
            self._state = checkpoint.snapshot(self.net)
        try:
            for c, bit in zip(sem.channels, sem.bits):
                channel_wise_quantizationperchan(sem.conv.weight.data, bit, c)
            check_pending()
            acc, loss, outs = ordinary_eval(self.net, self.batches)
            return acc, loss, kl_of(self.reference, outs)
        finally:
            try:
                check_pending()
            except ZeroDivisionError:
                pass
            checkpoint.restore_(self.net, self._state)


def ordinary_eval(net, batches):
    """functions.evaluate_acc_loss_softmax on device batches: (top-1 accuracy, mean batch loss, the
    per-batch softmax outputs), a fresh calibration on the first batch, one host sync."""
    acc, outs = None, []
    engine.new_evaluation(net)
    with torch.no_grad():
        for x, y in batches:
            out = net(x).float().contiguous()
            if acc is None:
                acc = torch.zeros(4, dtype=torch.float64, device=out.device)
            outs.append(ops.softmax_xent(out, y, acc, want_probs=True))
    loss_sum, correct, seen, count = acc.tolist()
    return correct / seen, loss_sum / count, outs


def kl_of(reference, outs):
    """functions.KLdiv(reference, outs): sum over images of sum_c p * log(p / q), over the images."""
    st = torch.zeros(2, dtype=torch.float64, device=outs[0].device)
    for p, q in zip(reference, outs):
        ops.kl_rows(p.to(q.device), q, st)
    s, n = st.tolist()
    return s / n


def _unpatched_pass_probs(hooks, batches, device):
    """_unpatched_pass that also returns each batch's softmax (fresh tensors, outside any graph pool)."""
    base = torch.zeros(4, dtype=torch.float64, device=device)
    flags = torch.zeros(2, dtype=torch.int32, device=device)
    probs = []
    with torch.no_grad():
        for x, y in batches:
            logits, ovf = hooks.forward(x)
            _or_flags(flags, ovf)
            probs.append(ops.softmax_xent(logits.float().contiguous(), y, base, want_probs=True))
    return base.tolist(), flags.tolist(), probs


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
    if engine.get_range_mode() != "static":
        raise ValueError("smpq: semilayer_table needs the static range mode (engine.set_range_mode)")
    if engine.get_dp_group() is not None:
        raise ValueError("smpq: semilayer_table runs on one GPU (no data-parallel group)")
    p = next(net.parameters())
    if not p.is_cuda or net.training or not getattr(net, "fused", True):
        raise ValueError("smpq: semilayer_table needs an eval-mode smpq ResNet on the GPU")
    if isinstance(batches, ResidentSet):
        batches.bind(p.device)
    else:
        batches = list(batches)
        if not batches or any(not (torch.is_tensor(x) and x.device == p.device) for x, _ in batches):
            raise ValueError("smpq: batches must be (x, y) pairs with x on the model's device, or a ResidentSet")
        batches = [(x, torch.as_tensor(y).to(p.device)) for x, y in batches]
    sems = _semilayers(net, semilayers)
    owned = None if shard is None else shard_owner(shard[1], count=len(sems)) == shard[0]
    if reference_outputs is not None:
        reference_outputs = [r.to(p.device) for r in reference_outputs]

    before = {k: stats.get(k, 0) for k in ("calibrations", "graph_captures", "repack")}
    t0 = time.perf_counter()
    _, eval_loss, eval_outs = ordinary_eval(net, batches)
    cal = engine.model_state(net).ranges
    hooks = _RowsHooks(net, cal, batches, eval_outs if reference_outputs is None else reference_outputs)
    b, bflags, base_probs = _unpatched_pass_probs(hooks, batches, p.device)  # captures every graph
    if any(bflags) or engine._signature(net) != cal.sig:
        raise RuntimeError("smpq: the baseline of the semilayer sweep did not hold (overflow or changed weights)")
    base_loss = b[0] / b[3]
    if reference_outputs is not None and len(reference_outputs) != len(base_probs):  # (a ResidentSet has no len)
        raise ValueError("smpq: reference_outputs must hold one softmax tensor per batch")
    refs = base_probs if reference_outputs is None else reference_outputs
    if reference_outputs is not None:
        del eval_outs
    plan = None
    if use_suffix:  # what a block's self-check must reproduce: the unpatched pass's KL statistics too
        base_kl = torch.zeros(2, dtype=torch.float64, device=p.device)
        for ref, probs in zip(refs, base_probs):
            ops.kl_rows(ref, probs, base_kl)
        plan = _suffix_plan(net, hooks, True, budget, b, base_kl.tolist())
    mid = {k: stats.get(k, 0) for k in before}
    t1 = time.perf_counter()

    counts = {"patched": 0, "overflowed": 0, "slow": {}, "constant": [], "rows_patched": 0, "max_rows": 0}
    table = SemilayerTable(arch_of(net), sems, base_loss, eval_loss)
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
            w2d = conv.weight.detach().reshape(conv.out_channels, -1)
            const_rows = (w2d.amax(1) == w2d.amin(1)).tolist()
            fast, rest = [], []
            for sem in group:
                const = [c for c in sem.channels if const_rows[c]]
                if const:  # the reference raises there (functions.py:40): the whole semilayer nan, listed
                    counts["constant"] += [(ln, c, sem.bits[sem.channels.index(c)]) for c in const]
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
        sweep_rows(groups, batches, refs, hooks, p.device, out, counts, progress, plan)
    after = {k: stats.get(k, 0) for k in before}
    t2 = time.perf_counter()
    if not counts["slow"] and (engine._signature(net) != cal.sig or engine.model_state(net).ranges is not cal):
        raise RuntimeError("smpq: the model changed while the semilayer sweep ran")
    report = {"trials": len(sems) if owned is None else int(owned.sum()), "patched": counts["patched"],
              "overflowed": counts["overflowed"], "slow": dict(counts["slow"]), "constant": list(counts["constant"]),
              "rows_patched": counts["rows_patched"], "max_rows": counts["max_rows"],
              "baseline": {k: mid[k] - before[k] for k in before},
              "during_trials": {k: after[k] - mid[k] for k in before},
              "baseline_s": t1 - t0, "trials_s": t2 - t1, "suffix": plan.report() if plan is not None else {}}
    for k in before:
        report[{"graph_captures": "captures", "repack": "repacks"}.get(k, k)] = after[k] - before[k]
    if shard is not None:
        report["shard"] = list(shard)
    table._report = report
    return table


# ---- merging the tables of a sharded call (host only) -------------------------------
def _same_bits(a, b):
    """Two losses equal as bits (float64), None only with None. No tolerance on purpose: every rank
    computed the baseline from the same model and data, so a difference is a fault to be reported."""
    if a is None or b is None:
        return a is None and b is None
    return np.float64(a).tobytes() == np.float64(b).tobytes()


def _merge_owned(tables, n, what):
    """The part that owns each of ``n`` columns (int array), after checking the parts' baselines and
    that their ``owned`` masks are disjoint and cover every column (None counts as all true)."""
    if not tables:
        raise ValueError("smpq: nothing to merge")
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
    tables = list(tables)
    if not tables:
        raise ValueError("smpq: nothing to merge")
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
    tables = list(tables)
    if not tables:
        raise ValueError("smpq: nothing to merge")
    first = tables[0]
    for i, t in enumerate(tables):
        if len(t.channels) != len(first.channels):
            raise ValueError("smpq: part %d has %d semilayers, part 0 has %d" % (i, len(t.channels), len(first.channels)))
        for j in range(len(first.channels)):
            if int(t.lnum[j]) != int(first.lnum[j]) or t.channels[j] != first.channels[j] or t.bits[j] != first.bits[j]:
                raise ValueError("smpq: semilayer %d of part %d is not part 0's" % (j, i))
    n = len(first.channels)
    part = _merge_owned(tables, n, "semilayer")
    # (SemilayerTable reads lnum, channels, bits and param of each entry, nothing else)
    sems = [types.SimpleNamespace(lnum=int(first.lnum[j]), channels=first.channels[j], bits=first.bits[j],
                                  param=float(first.param[j])) for j in range(n)]
    out = SemilayerTable(first.arch, sems, first.base_loss, first.eval_loss)
    for i, t in enumerate(tables):
        mine = part == i
        for name in ("loss", "acc", "kl", "stats", "kl_stats", "slow"):
            getattr(out, name)[mine] = getattr(t, name)[mine]
    rep = _merge_report(tables, extra=("rows_patched",))
    rep["max_rows"] = max(r.get("max_rows", 0) for r in rep["ranks"])
    out._report = rep
    return out
