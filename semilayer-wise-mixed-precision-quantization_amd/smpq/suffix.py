"""A sensitivity trial's forward from the patched conv's block on.

A trial of smpq.sensitivity patches rows of ONE conv. Every block before that conv's block computes
bit for bit what the unpatched pass computed, so the table keeps the limb-plane input of that block
for its batches (one eager prefix pass per block, ``fill``) and a trial forwards only the blocks from
there to the logits (``resume``).

Everything here is eager, static range mode, one GPU, and local to one table: no graph is captured,
extended or replayed, nothing is allocated in a graph pool, and the engine is only called, through
``stem_forward``, ``block_forward``, ``_head``, ``_blocks`` and ``Ctx``. The ordinary evaluation
path never comes here.

A kept input is the eager forward's own output tensors (``Act.q`` per batch slice, fresh from ops)
and the producing conv's static range; ``amax`` is the shared range tensor of that conv and is looked
up again at resume. The batch is cut into the slices ``engine._forward`` would give it, so every
conv runs at a shape the replay route runs too, and the slices go one after another on the current
stream. Block 0 (the stem's output) is supported like any other; the default cut never selects it.

The rows route (``rows=True`` on delta_loss_table, SMPQ_TRIAL_ROWS=1): a trial of a
block's LAST conv changes one channel of the next block's input, so the block's prefix pass
(``fill_rows``) also keeps that input and what the last conv read (``RowsKept``), and the trial
computes the patched channel alone into it (``rows_conv``, ops.trial_rows_conv), resumes from the
next block and puts the bytes back (``rows_restore``). The one edit outside this module is
engine.block_forward's optional ``keep`` tap.

``score_pass`` is the one loop over a table's or a session's batches: it walks the store (or the
plain batches) and picks each batch's forward. The hooks it calls on the real engine are
smpq.trials.EngineHooks; this module imports neither smpq.trials nor smpq.sensitivity.
"""
import itertools
import os
import sys
import time

import torch

from . import assignments, engine, ops, prefix

# SMPQ_TRIAL_SUFFIX=1: delta_loss_table / semilayer_table run their trials through this module
# (read at import, off by default, announced once on stderr at first use)
TRIAL_SUFFIX = [os.environ.get("SMPQ_TRIAL_SUFFIX", "0") == "1"]
_ANNOUNCED = [False]
# the resumed forward is used for a block only when at least this share of the net's blocks lies
# before it (j / blocks); shallower blocks keep the replay route. 7 / 16 is ResNet-50's layer3.0, the
# shallowest measured block whose resumed trial beat the replay (tools/suffix_bench.py,
# profiles/trial_suffix.json: 0.59 of the replay's time there, 1.05 at block 0); the same share is
# layer3.0 in ResNet-18 and ResNet-34 too.
MIN_SKIPPED = [7 / 16]


def _gb(text):
    """SMPQ_TRIAL_SUFFIX_GB's value in bytes, None (unbounded) when unset or empty."""
    if text is None or not text.strip():
        return None
    v = float(text)
    if not v >= 0:
        raise ValueError("smpq: SMPQ_TRIAL_SUFFIX_GB must be a number >= 0, not %r" % (text,))
    return int(v * (1 << 30))


TRIAL_SUFFIX_BYTES = [_gb(os.environ.get("SMPQ_TRIAL_SUFFIX_GB"))]


def switch(suffix=None, suffix_bytes=None):
    """(on?, byte budget or None) from a table's arguments, the environment's values for the ones
    left at None."""
    on = TRIAL_SUFFIX[0] if suffix is None else bool(suffix)
    if on and not _ANNOUNCED[0]:
        _ANNOUNCED[0] = True
        print("smpq: SMPQ_TRIAL_SUFFIX=1 -> sensitivity trials of the deep blocks forward only the blocks from "
              "the patched conv on, eagerly, from block inputs kept by one prefix pass per block "
              "(smpq.suffix)", file=sys.stderr)
    budget = TRIAL_SUFFIX_BYTES[0] if suffix_bytes is None else int(suffix_bytes)
    if budget is not None and budget < 0:
        raise ValueError("smpq: suffix_bytes must be >= 0")
    return on, budget


# SMPQ_TRIAL_ROWS=1: delta_loss_table's trials of a block's LAST conv recompute only the patched
# output channel into the kept input of the next block and resume from there. Read at
# import, off by default, honoured only with the suffix on, announced once on stderr at first use.
TRIAL_ROWS = [os.environ.get("SMPQ_TRIAL_ROWS", "0") == "1"]
_ROWS_ANNOUNCED = [False]


def rows_switch(rows=None, suffix_on=True):
    """Is the rows route on for a table? ``rows``: the table's argument (None: SMPQ_TRIAL_ROWS)."""
    on = bool(suffix_on) and (TRIAL_ROWS[0] if rows is None else bool(rows))
    if on and not _ROWS_ANNOUNCED[0]:
        _ROWS_ANNOUNCED[0] = True
        print("smpq: SMPQ_TRIAL_ROWS=1 -> delta-loss trials of a block's last conv recompute only the patched "
              "output channel into the kept input of the next block and resume from there (smpq.suffix)",
              file=sys.stderr)
    return on


def block_of(net, conv):
    """Forward-order index (prefix.block_names' numbering) of the block that owns the searched
    conv ``conv``; ValueError for a conv no block owns (the stem, a downsample)."""
    names = prefix.block_names(net)
    for j, b in enumerate(assignments.blocks_of(net)):
        if any(getattr(b, "conv%d" % i, None) is conv for i in (1, 2, 3)):
            assert j < len(names)
            return j
    raise ValueError("smpq suffix: not a searched conv of this net")


def first_block(net):
    """The shallowest block the resumed forward is used for (MIN_SKIPPED)."""
    n = len(prefix.block_names(net))
    return next((j for j in range(n) if j >= MIN_SKIPPED[0] * n), n)


def slices(n, ranges=True):
    """The (start, end) parts engine._forward runs a static-range batch of ``n`` images as."""
    c = engine.CHUNK[0]
    parts = [(s, min(n, s + c)) for s in range(0, n, c)]
    nst = engine.STREAMS[0] if ranges else 1
    if nst > 1 and n >= 2 * nst and len(parts) == 1:
        step = (n + nst - 1) // nst
        parts = [(s, min(n, s + step)) for s in range(0, n, step)]
    return parts


def _producer(net, blocks, j):
    """The conv whose epilogue writes block ``j``'s input."""
    if j == 0:
        return net.conv1
    b = blocks[j - 1]
    return b.conv3 if hasattr(b, "conv3") else b.conv2


class Kept:
    """One batch's kept block input: per slice (start, end, limb planes, range), the batch's
    labels, its image count and the bytes of its planes."""
    __slots__ = ("parts", "y", "n", "nbytes", "rows")

    def __init__(self, parts, n, y=None):
        self.parts, self.n, self.y = parts, n, y
        self.nbytes = sum(q.numel() * q.element_size() for _, _, q, _ in parts)
        self.rows = None  # the rows route's extra tensors of this batch (RowsKept), or None


def _nbytes(t):
    return t.numel() * t.element_size()


class RowsKept:
    """What the rows route keeps of one batch of block j besides the block's input:
    per slice the Acts fed to the block's last conv and added as its identity (engine.block_forward's
    tap) and a save area for the digit bytes a trial replaces; ``next``: the Kept input of block
    j + 1, the planes a trial writes one channel of. ``nbytes``: what this adds to the store (the
    identity of a block without a downsample is the block input already kept)."""
    __slots__ = ("taps", "saves", "next", "nbytes")

    def __init__(self, taps, nxt, block_input):
        self.taps, self.next = taps, nxt
        self.saves = [torch.empty(ops.trial_rows_conv_save_bytes(q.shape[0], q[0, ..., 0].numel(), 1),
                                  dtype=torch.int8, device=q.device) for _, _, q, _ in nxt.parts]
        held = {p[2].data_ptr() for p in block_input.parts}
        self.nbytes = nxt.nbytes + sum(_nbytes(s) for s in self.saves) + sum(
            _nbytes(x.q) + (0 if ident.q.data_ptr() in held else _nbytes(ident.q)) for x, ident in taps)


def rows_bytes(net, x, j):
    """RowsKept.nbytes of batch ``x`` ([n, c, h, w]) at block ``j``, from the shapes alone (computed
    before the fill): the last conv's input planes, the downsample's output planes where the block
    has one, block j + 1's input planes and one channel's save area."""
    blk = engine._blocks(net)[j]
    last = blk.conv3 if hasattr(blk, "conv3") else blk.conv2
    limbs, n, h, w, c = prefix.boundary_shape(net, j + 1, x.shape[0], x.shape[2], x.shape[3], ops.get_act_limbs())
    nxt = prefix.boundary_bytes(limbs, c, h, w, n)
    return (nxt + prefix.boundary_bytes(limbs, last.in_channels, h, w, n) + (nxt if blk.downsample is not None else 0)
            + ops.trial_rows_conv_save_bytes(limbs, n * h * w, 1))


def _prefix_pass(net, x, cal, j, tap):
    """The one prefix pass behind fill and fill_rows: stem + blocks 0..j-1 of batch ``x`` under the
    installed StaticRanges ``cal``, slice by slice on the current stream, and with ``tap`` on through
    block ``j`` with engine.block_forward's tap. (Kept or None, why): fill_rows' return values."""
    assert not torch.cuda.is_current_stream_capturing()
    blocks = engine._blocks(net)
    n = x.shape[0]
    ctx = engine.Ctx(n, x.device, ranges=cal.by_conv, cache=cal.tensors)
    parts, taps, nparts, why = [], [], [], None
    try:
        for lane, (s0, s1) in enumerate(slices(n)):
            ctx.n, ctx.lane = s1 - s0, lane
            act, t1 = engine.stem_forward(net, x[s0:s1], ctx), None
            for i in range(j):
                act, t1 = engine.block_forward(blocks[i], act, ctx, last=False, t1=t1, nxt=blocks[i + 1])
            if t1 is not None or act.q is None or act.rng is None or act.f32 is not None:
                return None, None
            parts.append((s0, s1, act.q, act.rng))
            if tap and why is None:
                keep = {}
                out, t1 = engine.block_forward(blocks[j], act, ctx, last=False, t1=None, nxt=blocks[j + 1], keep=keep)
                if "x" not in keep:
                    why = "no_tap"
                elif t1 is not None or out.q is None or out.rng is None or out.f32 is not None:
                    why = "next_not_resumable"
                else:
                    taps.append((keep["x"], keep["identity"]))
                    nparts.append((s0, s1, out.q, out.rng))
    finally:
        ctx.n, ctx.lane = n, None
    kept = Kept(parts, n)
    if tap and why is None:
        kept.rows = RowsKept(taps, Kept(nparts, n), kept)
    return kept, why


def fill(net, x, cal, j):
    """Stem + blocks 0..j-1 of batch ``x`` under the installed StaticRanges ``cal``, slice by slice
    on the current stream: the Kept input of block ``j``, or None when it cannot be resumed from
    (block j-1 handed on a chained conv1 output, or the input is not limb planes with a static
    range and nothing else). An overflow in the prefix is not looked at: the table's unpatched
    pass ran the same launches on the same data and held."""
    if not 0 <= j < len(engine._blocks(net)):
        raise ValueError("smpq suffix: block %d outside 0..%d" % (j, len(engine._blocks(net)) - 1))
    return _prefix_pass(net, x, cal, j, False)[0]


def fill_rows(net, x, cal, j):
    """fill(net, x, cal, j) whose one pass goes on through block ``j`` with engine.block_forward's tap:
    (Kept or None, why). ``why`` is None when ``kept.rows`` holds the rows route's tensors, else the
    reason it does not: "no_tap" (the last conv ran in a chain or fused-downsample launch, or not
    from and to static limb planes) or "next_not_resumable" (block j + 1's input fails fill's rule).
    The Kept itself is fill's, whatever ``why``."""
    if not 0 <= j < len(engine._blocks(net)) - 1:
        raise ValueError("smpq suffix: block %d has no next block to write into" % j)
    return _prefix_pass(net, x, cal, j, True)


def last_conv(net, j):
    """(conv, bn) of block ``j``'s last conv: conv3 of a Bottleneck, conv2 of a BasicBlock."""
    blk = engine._blocks(net)[j]
    return (blk.conv3, blk.bn3) if hasattr(blk, "conv3") else (blk.conv2, blk.bn2)


def rows_conv(net, kept, j, rows, flag, done):
    """The rows route's write: the channel(s) ``rows`` (ops.TrialRows) of block ``j``'s last conv, from
    its operand as it is now (patched or not), into every slice of ``kept.rows.next``
    (ops.trial_rows_conv; the old bytes go to the slices' save areas, an overflow to ``flag`` int32
    [1]). ``done`` (a list) grows by one per slice written, for rows_restore."""
    conv, bn = last_conv(net, j)
    plan = engine.conv_plan(conv, bn)
    for (x, ident), save, (_, _, q, rng) in zip(kept.rows.taps, kept.rows.saves, kept.rows.next.parts):
        ops.trial_rows_conv(x.q, x.amax, plan.codes, conv.kernel_size[0], conv.kernel_size[1], conv.stride[0],
                            conv.padding[0], plan.col_scale, plan.col_shift, rows, q, rng, flag, save,
                            residual_q=ident.q, residual_range=ident.rng)
        done.append(1)


def rows_restore(kept, rows, done):
    """Put back what rows_conv replaced in the first ``len(done)`` slices of ``kept.rows.next``."""
    for _, save, (_, _, q, _) in zip(done, kept.rows.saves, kept.rows.next.parts):
        ops.trial_rows_conv_restore(rows, q, save)


def rows_geometry(conv):
    """Is ``conv`` one of the two geometries ops.trial_rows_conv computes?"""
    geo = (conv.kernel_size, conv.stride, conv.padding, conv.dilation, conv.groups)
    return geo in (((1, 1), (1, 1), (0, 0), (1, 1), 1), ((3, 3), (1, 1), (1, 1), (1, 1), 1)) \
        and conv.in_channels % 64 == 0 and conv.out_channels % 16 == 0 and ops.get_act_limbs() in (2, 3)


def resume(net, kept, cal, j, check=True):
    """Blocks j..end and the head from ``kept`` (fill's, same ``cal`` and ``j``), slice by slice on
    the current stream: (logits [n, classes], the Ctx.overflow int32 pair). ``check``: enqueue the
    weights' content check into word 1 (a trial needs it once, not once per batch)."""
    assert not torch.cuda.is_current_stream_capturing()
    blocks = engine._blocks(net)
    dev = kept.parts[0][2].device
    ctx = engine.Ctx(kept.n, dev, ranges=cal.by_conv, cache=cal.tensors)
    src = _producer(net, blocks, j)
    y = torch.empty(kept.n, net.fc.out_features, dtype=torch.float32, device=dev) \
        if isinstance(net.fc, torch.nn.Linear) else None
    outs = []
    try:
        for lane, (s0, s1, q, rng) in enumerate(kept.parts):
            ctx.n, ctx.lane = s1 - s0, lane
            act, t1 = engine.Act(q=q, amax=ctx.range_tensor(src), rng=rng), None
            for i in range(j, len(blocks)):
                nxt = blocks[i + 1] if i + 1 < len(blocks) else None
                act, t1 = engine.block_forward(blocks[i], act, ctx, last=nxt is None, t1=t1, nxt=nxt)
            outs.append(engine._head(net, act.f32, out=None if y is None else y[s0:s1]))
    finally:
        ctx.n, ctx.lane = kept.n, None
    if y is None:
        y = torch.cat(outs) if len(outs) > 1 else outs[0]
    if check:
        cal.fp.check(ctx.overflow[1:])
    return y, ctx.overflow


def kept_bytes(net, x, j):
    """prefix.boundary_bytes of batch ``x`` ([n, c, h, w]) at block ``j`` with the current limb count."""
    limbs, n, h, w, c = prefix.boundary_shape(net, j, x.shape[0], x.shape[2], x.shape[3], ops.get_act_limbs())
    return prefix.boundary_bytes(limbs, c, h, w, n)


class Store:
    """The kept inputs of ONE block for the batches of a table, under a byte budget (None:
    unbounded). Batches are offered in order; each is admitted if it still fits, otherwise it is
    marked "full forward" (a later, smaller batch may still fit). An admitted batch's labels are
    kept with it, so when every batch is kept a trial does not iterate the set."""

    def __init__(self, budget=None):
        self.budget = None if budget is None else int(budget)
        self.block, self.entries, self.bytes = None, [], 0
        # the rows route: the block's last conv while its trials may use the entries'
        # RowsKept, else None; ``row``: the block's report row (rows trials are counted there)
        self.rows, self.row = None, None

    def fits(self, nbytes):
        return self.budget is None or self.bytes + int(nbytes) <= self.budget

    def begin(self, block):
        if self.entries:
            self.release()
        self.block = block

    def add(self, kept, nbytes=0):
        """The next batch's entry: a kept input (``nbytes`` counted), or None = full forward."""
        self.entries.append(kept)
        if kept is not None:
            self.bytes += int(nbytes)

    def drop_kept(self):
        """Every batch becomes a full forward (the block turned out not to be resumable)."""
        self.entries = [None] * len(self.entries)
        self.bytes = 0

    def drop_rows(self):
        """Every kept batch goes back to the block's own input alone (no rows route for this block)."""
        for e in self.entries:
            if e is not None and e.rows is not None:
                self.bytes -= e.rows.nbytes
                e.rows = None
        self.rows = None

    @property
    def rows_kept(self):
        return sum(e is not None and e.rows is not None for e in self.entries)

    @property
    def rows_bytes(self):
        return sum(e.rows.nbytes for e in self.entries if e is not None and e.rows is not None)

    @property
    def kept(self):
        return sum(e is not None for e in self.entries)

    @property
    def complete(self):
        return bool(self.entries) and self.kept == len(self.entries)

    def walk(self, batches):
        """(kept or None, x, y) per batch; ``x`` is None for a kept batch. ``batches`` is iterated
        only when some batch is not kept."""
        if self.complete:
            for e in self.entries:
                yield e, None, e.y
            return
        at = -1
        for at, (x, y) in enumerate(batches):
            e = self.entries[at] if at < len(self.entries) else None
            yield (e, None, e.y) if e is not None else (None, x, y)
        if self.entries and at + 1 != len(self.entries):
            raise RuntimeError("smpq suffix: the set gave %d batches, the prefix pass saw %d" % (at + 1, len(self.entries)))

    def release(self):
        self.block, self.entries, self.bytes = None, [], 0
        self.rows, self.row = None, None


class Plan:
    """A table's use of the store. ``base`` / ``base_kl``: the host statistics of the table's
    unpatched replay pass, which every block's self-check must reproduce bitwise; ``first``: the
    shallowest block that is resumed (shallower ones keep the replay); ``blocks``: the report rows,
    one per block visited; ``launches`` / ``resumed``: conv launches issued by, and number of,
    resumed forwards (self-checks included)."""

    def __init__(self, budget, base, base_kl=None, first=0, rows=False):
        self.store = Store(budget)
        self.base, self.base_kl, self.first = list(base), None if base_kl is None else list(base_kl), first
        self.blocks, self.launches, self.resumed = [], 0, 0
        self.visited = None
        self.rows = bool(rows)  # the rows route for the last convs of eligible blocks

    def report(self):
        return {"first_block": self.first, "blocks": [dict(b) for b in self.blocks],
                "resumed_forwards": self.resumed, "resumed_conv_launches": self.launches}


def enter(plan, hooks, conv, batches, device, refs=None):
    """Called ahead of the patched trials of ``conv``: the store to walk for them, or None (this
    block keeps the replay route). On a change of block the store is released and, for a block at or
    beyond ``plan.first``, refilled by one eager prefix pass over ``batches``; then one unpatched
    pass through the suffix must reproduce ``plan.base`` (and ``plan.base_kl`` with ``refs``)
    bitwise, else RuntimeError. Hooks: block_of(conv), block_name(j), kept_bytes(x, j), fill(x, j)
    -> Kept or None, resume(kept, j), forward(x), score / score_kl, sync().

    With ``plan.rows`` the same pass also keeps, for every batch that fits with them,
    what the rows route needs (``kept.rows``), ``store.rows`` becomes the block's last conv, and two
    more checks run before any trial: the one-row kernel on the unpatched operand must leave the kept
    planes as they are, and an unpatched resume from block j + 1 must reproduce the statistics too.
    The block's report row says ``rows``: "used", or why not ("off", "below_cut", "last_block",
    "geometry", "not_patchable", "no_tap", "next_not_resumable", "not_resumable", "budget"). More
    hooks then: rows_block(j) -> None or why not, last_conv(j), rows_bytes(x, j), fill_rows(x, j) ->
    (Kept or None, why), rows_check(store, j) -> bool."""
    j = hooks.block_of(conv)
    st = plan.store
    if plan.visited == j:
        return st if st.kept else None
    st.release()  # the block changes
    plan.visited = j
    row = {"block": j, "name": hooks.block_name(j), "used": j >= plan.first, "resumable": None, "kept": 0,
           "full": None, "bytes": 0, "prefix_pass_s": 0.0, "self_check": None, "self_check_s": 0.0,
           "rows": "off", "rows_kept": 0, "rows_trials": 0, "rows_bytes": 0, "rows_self_check": None,
           "rows_self_check_s": 0.0}
    plan.blocks.append(row)
    if not row["used"]:
        if plan.rows:
            row["rows"] = "below_cut"
        return None
    why = hooks.rows_block(j) if plan.rows else "off"  # None: the rows route is still possible
    hooks.sync()
    t0 = time.perf_counter()
    st.begin(j)
    resumable = True
    for x, y in batches:
        nb = hooks.kept_bytes(x, j)
        extra = hooks.rows_bytes(x, j) if why is None else 0  # (all sizes before the fill)
        kept = None
        if resumable and why is None and st.fits(nb + extra):
            kept, why = hooks.fill_rows(x, j)
            if why is not None:
                st.drop_rows()
        elif resumable and st.fits(nb):  # without the extra tensors: this batch is kept 5h's way
            kept = hooks.fill(x, j)
        else:
            nb = None  # not tried
        if nb is not None and kept is None:
            resumable = False
            st.drop_kept()
        more = 0
        if kept is not None:
            if kept.nbytes != nb:
                raise RuntimeError("smpq suffix: block %d keeps %d bytes of a batch, %d expected" % (j, kept.nbytes, nb))
            if kept.rows is not None:
                more = kept.rows.nbytes
                if more != extra:
                    raise RuntimeError("smpq suffix: block %d keeps %d more bytes of a batch for the rows route, %d "
                                       "expected" % (j, more, extra))
            kept.y = y
        st.add(kept, (nb or 0) + more)
    hooks.sync()
    row.update(resumable=resumable, kept=st.kept, full=len(st.entries) - st.kept, bytes=st.bytes,
               prefix_pass_s=time.perf_counter() - t0)
    if plan.rows:
        if why is None and not resumable:
            why = "not_resumable"
        elif why is None and not st.rows_kept:
            why = "budget"
        row.update(rows=why or "used", rows_kept=st.rows_kept, rows_bytes=st.rows_bytes)
    if not st.kept:
        return None
    # the self-check: no patch, through the suffix, against the table's unpatched replay pass
    same, got = _unpatched(plan, st, hooks, batches, device, refs, False)
    row["self_check"], row["self_check_s"] = same, time.perf_counter() - t0 - row["prefix_pass_s"]
    if not same:
        st.release()
        raise RuntimeError("smpq suffix: block %s resumed without a patch does not reproduce the unpatched pass "
                           "(statistics %r against %r)" % (row["name"], got, plan.base))
    if st.rows_kept:
        # the rows route's: the one-row kernel on the unpatched operand changes nothing, and the kept
        # inputs of block j + 1 resume to the same statistics
        t1 = time.perf_counter()
        planes = hooks.rows_check(st, j)
        same, got = _unpatched(plan, st, hooks, batches, device, refs, True)
        row["rows_self_check"], row["rows_self_check_s"] = bool(planes and same), time.perf_counter() - t1
        if not (planes and same):
            st.release()
            raise RuntimeError("smpq suffix: block %s fails the rows route's self-check (%s)" % (
                row["name"], "the one-row conv of the unpatched operand changed the kept planes" if not planes else
                "statistics %r against %r resumed from the next block" % (got, plan.base)))
        st.rows, st.row = hooks.last_conv(j), row
    return st


def score_pass(hooks, batches, store, refs, row, kl_row, flags, rows_channel=None, rows_from_next=False, probs=None):
    """THE loop over the batches: forward every batch and score it into ``row``
    (float64 [4]), ORing the forwards' flag pairs into ``flags`` (int32 [2]). Every trial, self-check
    and unpatched pass of the tables and the session comes here. ``store`` (a Store or None): a batch
    it keeps runs through hooks.resume(kept, store.block) from its kept block input instead of
    hooks.forward(x); with ``rows_channel`` a batch that has ``kept.rows`` runs through
    hooks.resume_rows(kept, store.block, rows_channel), with ``rows_from_next`` through
    hooks.resume(kept.rows.next, store.block + 1) (the rows route's self-check). ``refs`` (one
    reference softmax per batch, or None): with them a batch is scored by hooks.score_kl(logits, y,
    ref, row, kl_row), without by hooks.score(logits, y, row). ``probs`` (a list or None): grows by
    each batch's softmax, hooks.score(logits, y, row, True)'s, for the baseline that needs them."""
    walk = ((None, x, y) for x, y in batches) if store is None else store.walk(batches)
    for (kept, x, y), ref in zip(walk, itertools.repeat(None) if refs is None else refs):
        if kept is None:
            logits, ovf = hooks.forward(x)
        elif rows_channel is not None and kept.rows is not None:
            logits, ovf = hooks.resume_rows(kept, store.block, rows_channel)
        elif rows_from_next and kept.rows is not None:
            logits, ovf = hooks.resume(kept.rows.next, store.block + 1)
        else:
            logits, ovf = hooks.resume(kept, store.block)
        torch.bitwise_or(flags, ovf, out=flags)
        if probs is not None:
            probs.append(hooks.score(logits, y, row, True))
        elif refs is None:
            hooks.score(logits, y, row)
        else:
            hooks.score_kl(logits, y, ref, row, kl_row)
    for _ in walk:  # (run the generator to its end: Store.walk's batch-count check)
        pass


def _unpatched(plan, st, hooks, batches, device, refs, rows):
    """One unpatched pass over the store's batches: (does it reproduce the plan's base statistics
    bitwise with zero flags?, the statistics). ``rows``: a batch with a RowsKept resumes from its
    kept input of the next block instead of the store's."""
    got = torch.zeros(4, dtype=torch.float64, device=device)
    kl = torch.zeros(2, dtype=torch.float64, device=device)
    flags = torch.zeros(2, dtype=torch.int32, device=device)
    score_pass(hooks, batches, st, refs, got, kl, flags, rows_from_next=rows)
    same = got.tolist() == plan.base and (refs is None or kl.tolist() == plan.base_kl) and not any(flags.tolist())
    return same, got.tolist()
