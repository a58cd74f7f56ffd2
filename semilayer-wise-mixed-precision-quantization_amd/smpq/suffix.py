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
"""
import os
import sys
import time

import torch

from . import assignments, engine, ops, prefix
from .qconv import stats

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
    __slots__ = ("parts", "y", "n", "nbytes")

    def __init__(self, parts, n, y=None):
        self.parts, self.n, self.y = parts, n, y
        self.nbytes = sum(q.numel() * q.element_size() for _, _, q, _ in parts)


def fill(net, x, cal, j):
    """Stem + blocks 0..j-1 of batch ``x`` under the installed StaticRanges ``cal``, slice by slice
    on the current stream: the Kept input of block ``j``, or None when it cannot be resumed from
    (block j-1 handed on a chained conv1 output, or the input is not limb planes with a static
    range and nothing else). An overflow in the prefix is not looked at: the table's unpatched
    pass ran the same launches on the same data and held."""
    assert not torch.cuda.is_current_stream_capturing()
    blocks = engine._blocks(net)
    if not 0 <= j < len(blocks):
        raise ValueError("smpq suffix: block %d outside 0..%d" % (j, len(blocks) - 1))
    n = x.shape[0]
    ctx = engine.Ctx(n, x.device, ranges=cal.by_conv, cache=cal.tensors)
    parts = []
    try:
        for lane, (s0, s1) in enumerate(slices(n)):
            ctx.n, ctx.lane = s1 - s0, lane
            act, t1 = engine.stem_forward(net, x[s0:s1], ctx), None
            for i in range(j):
                act, t1 = engine.block_forward(blocks[i], act, ctx, last=False, t1=t1, nxt=blocks[i + 1])
            if t1 is not None or act.q is None or act.rng is None or act.f32 is not None:
                return None
            parts.append((s0, s1, act.q, act.rng))
    finally:
        ctx.n, ctx.lane = n, None
    return Kept(parts, n)


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


class Plan:
    """A table's use of the store. ``base`` / ``base_kl``: the host statistics of the table's
    unpatched replay pass, which every block's self-check must reproduce bitwise; ``first``: the
    shallowest block that is resumed (shallower ones keep the replay); ``blocks``: the report rows,
    one per block visited; ``launches`` / ``resumed``: conv launches issued by, and number of,
    resumed forwards (self-checks included)."""

    def __init__(self, budget, base, base_kl=None, first=0):
        self.store = Store(budget)
        self.base, self.base_kl, self.first = list(base), None if base_kl is None else list(base_kl), first
        self.blocks, self.launches, self.resumed = [], 0, 0
        self.visited = None

    def report(self):
        return {"first_block": self.first, "blocks": [dict(b) for b in self.blocks],
                "resumed_forwards": self.resumed, "resumed_conv_launches": self.launches}


def enter(plan, hooks, conv, batches, device, refs=None):
    """Called ahead of the patched trials of ``conv``: the store to walk for them, or None (this
    block keeps the replay route). On a change of block the store is released and, for a block at or
    beyond ``plan.first``, refilled by one eager prefix pass over ``batches``; then one unpatched
    pass through the suffix must reproduce ``plan.base`` (and ``plan.base_kl`` with ``refs``)
    bitwise, else RuntimeError. Hooks: block_of(conv), block_name(j), kept_bytes(x, j), fill(x, j)
    -> Kept or None, resume(kept, j), forward(x), score / score_kl, sync()."""
    j = hooks.block_of(conv)
    st = plan.store
    if plan.visited == j:
        return st if st.kept else None
    st.release()  # the block changes
    plan.visited = j
    row = {"block": j, "name": hooks.block_name(j), "used": j >= plan.first, "resumable": None, "kept": 0,
           "full": None, "bytes": 0, "prefix_pass_s": 0.0, "self_check": None, "self_check_s": 0.0}
    plan.blocks.append(row)
    if not row["used"]:
        return None
    hooks.sync()
    t0 = time.perf_counter()
    st.begin(j)
    resumable = True
    for x, y in batches:
        nb = hooks.kept_bytes(x, j)
        kept = None
        if resumable and st.fits(nb):
            kept = hooks.fill(x, j)
            if kept is None:
                resumable = False
                st.drop_kept()
        if kept is not None:
            if kept.nbytes != nb:
                raise RuntimeError("smpq suffix: block %d keeps %d bytes of a batch, %d expected" % (j, kept.nbytes, nb))
            kept.y = y
        st.add(kept, nb)
    hooks.sync()
    row.update(resumable=resumable, kept=st.kept, full=len(st.entries) - st.kept, bytes=st.bytes,
               prefix_pass_s=time.perf_counter() - t0)
    if not st.kept:
        return None
    # the self-check: no patch, through the suffix, against the table's unpatched replay pass
    got = torch.zeros(4, dtype=torch.float64, device=device)
    kl = torch.zeros(2, dtype=torch.float64, device=device)
    flags = torch.zeros(2, dtype=torch.int32, device=device)
    walk = st.walk(batches)
    for (kept, x, y), ref in zip(walk, refs if refs is not None else _nones()):
        logits, ovf = hooks.forward(x) if kept is None else hooks.resume(kept, j)
        torch.bitwise_or(flags, ovf, out=flags)
        if refs is None:
            hooks.score(logits, y, got)
        else:
            hooks.score_kl(logits, y, ref, got, kl)
    for _ in walk:  # (run the generator to its end: its batch-count check)
        pass
    same = got.tolist() == plan.base and (refs is None or kl.tolist() == plan.base_kl) and not any(flags.tolist())
    row["self_check"], row["self_check_s"] = same, time.perf_counter() - t0 - row["prefix_pass_s"]
    if not same:
        st.release()
        raise RuntimeError("smpq suffix: block %s resumed without a patch does not reproduce the unpatched pass "
                           "(statistics %r against %r)" % (row["name"], got.tolist(), plan.base))
    return st


def _nones():
    while True:
        yield None


class EngineHooks:
    """enter's and the trials' hooks on the real engine (mixed into sensitivity's hooks, which give
    ``net`` and ``cal``). ``resume`` looks ``suffix.resume`` up at call time and enqueues the content
    check for the first resumed batch after every ``new_trial``."""
    plan = None
    _check = True

    def block_of(self, conv):
        return block_of(self.net, conv)

    def block_name(self, j):
        return prefix.block_names(self.net)[j]

    def kept_bytes(self, x, j):
        return kept_bytes(self.net, x, j)

    def fill(self, x, j):
        return fill(self.net, x, self.cal, j)

    def new_trial(self):
        self._check = True

    def resume(self, kept, j):
        before = stats["hip_conv"]
        out = resume(self.net, kept, self.cal, j, check=self._check)
        self._check = False
        if self.plan is not None:
            self.plan.resumed += 1
            self.plan.launches += stats["hip_conv"] - before
        return out

    def sync(self):
        torch.cuda.synchronize()
