"""A search session: the drivers' main-loop semilayer trials by patch, accepted by commit.

The drivers' main loop (resnet50_main.py:186-243) takes the last accepted state, quantizes ONE
semilayer, evaluates it, keeps it if the accuracy held and otherwise restores the state and
evaluates that again. About nine trials in ten are thrown away, and each pays a calibration forward,
the graph captures, every conv's repack after the restore and a second evaluation. A ``Session``
runs such a trial the way smpq.sensitivity's tables run theirs: the semilayer's rows of the conv's
packed operand are patched in place, every batch is forwarded and scored, the bytes are put back.
No model tensor is written before ``accept()``.

    with search.Session(net, batches, reference_outputs=originaloutputs) as s:   # net: the standing state
        r = s.trial(lnum, channels, bit)          # bit: one int or one per channel; the model is not written
        if r.acc >= preacc:
            official = s.accept()                 # commits the LAST trial to the model, rebases, returns the new base

What a patched trial's ``acc`` / ``loss`` / ``kl`` are: the figures of the model with those channels
quantized UNDER THE STANDING STATE'S STATIC RANGES, with no calibration forward on the first batch
(the two differences DESIGN.md 5f names: the reference's route calibrates every evaluated model
afresh on its first batch). The accepted state's official figures, bit for bit what
functions.evaluate_acc_loss_softmax + functions.KLdiv return for it, come from ``accept()``
(``s.base``). A driver that wants the reference's decision bit for bit compares ``official.acc``; if
that disagrees with the trial's decision it rolls back with checkpoint.restore_ + ``s.rebase()``.

Two patches: a conv with a free channel left outside the semilayer has a 'fixed' / 'exact16'
operand (sensitivity.patchable_rows, ops.trial_rows_patch, route "patched"); a conv whose every
channel is quantized already has an 'exact8' one (sensitivity.patchable_rows_x8,
ops.trial_rows_patch_x8, route "patched_x8": the 6- and 4-bit passes re-quantize exactly such
convs). What neither covers (a trial that completes a conv, an overflowed static range, a row the
exact8 coder cannot take) runs through the public API on the model itself and restores it ("slow:*");
the session then rebuilds its baseline at the next trial.

Kept boundaries: at every rebase the session keeps the limb-plane input of a few blocks
(``boundaries``, default prefix.DEFAULT_BLOCKS) for its batches (smpq.suffix: eager, nothing
captured or replayed by new code), and a patched trial of a conv in block b forwards only the blocks
from the deepest kept boundary j <= b on. Static range mode, one GPU, eval-mode smpq ResNet.
"""
import math
import time

import torch

from . import assignments, engine, prefix, sensitivity, trials
from . import suffix as _suffix
from .quant import channel_wise_quantizationperchan, check_pending

_COUNTERS = trials.COUNTERS


class Result:
    """One trial (or, as ``Session.base``, one standing state: acc, loss, kl and route "base").
    ``param``: the reference's sum (sensitivity.Semilayer); ``stats`` [4] / ``kl_stats`` [2]: a patched
    trial's raw float64 statistics (None otherwise); ``route``: "patched", "patched_x8", "constant",
    "slow:not_patchable", "slow:overflow", "slow:unpackable"; ``resumed_from``: the block a patched
    trial's forwards were resumed from, or None (the replay)."""
    __slots__ = ("lnum", "channels", "bits", "param", "acc", "loss", "kl", "stats", "kl_stats", "route",
                 "resumed_from")

    def __init__(self, lnum=None, channels=None, bits=None, param=None, acc=math.nan, loss=math.nan, kl=math.nan,
                 stats=None, kl_stats=None, route=None, resumed_from=None):
        self.lnum, self.channels, self.bits, self.param = lnum, channels, bits, param
        self.acc, self.loss, self.kl, self.stats, self.kl_stats = acc, loss, kl, stats, kl_stats
        self.route, self.resumed_from = route, resumed_from

    def __repr__(self):
        return "Result(lnum=%r, rows=%r, acc=%r, loss=%r, kl=%r, route=%r, resumed_from=%r)" % (
            self.lnum, None if self.channels is None else len(self.channels), self.acc, self.loss, self.kl,
            self.route, self.resumed_from)


class EngineHooks(trials.EngineHooks):
    """What a Session asks of the engine (tests inject a fake): the trials' hooks, plus the route, the
    commit and the session's views of the model."""

    def __init__(self, net, batches):
        super().__init__(net, batches)
        self.device = next(net.parameters()).device

    # -- the state -----------------------------------------------------------------------------
    def semilayer(self, lnum, channels, bit):
        return sensitivity._semilayers(self.net, [(lnum, channels, bit)])[0]

    def held(self):
        """Is the model what the ranges were installed for?"""
        return engine._signature(self.net) == self.cal.sig and engine.model_state(self.net).ranges is self.cal

    def signature(self):
        return engine._signature(self.net)

    def counters(self):
        return trials.counters()

    def ordinary_eval(self):
        return trials.ordinary_eval(self.net, self.batches)

    def kl_of(self, reference, outs):
        return trials.kl_of(reference, outs)

    def unpatched_pass(self):
        return trials.unpatched_pass(self, self.batches, self.device, True)

    def kl_stats(self, refs, probs):
        return trials.kl_stats(refs, probs)

    def constant_rows(self, conv):
        return trials.constant_rows(conv)

    def route(self, sem):
        bn = trials.bn_for(self.net, sem.conv)
        if trials.patchable_rows(sem.conv, bn, sem.channels):
            return "patched"
        if trials.patchable_rows_x8(sem.conv, bn, sem.channels, sem.bits):
            return "patched_x8"
        return None

    def zeros(self, n, dtype):
        return torch.zeros(n, dtype=dtype, device=self.device)

    def prepare_one(self, sem, route):
        self.prepare([sem], "rows_x8" if route == "patched_x8" else "rows")

    # -- boundaries ----------------------------------------------------------------------------
    def block_index(self, name):
        return prefix.block_index(self.net, name)

    def boundary_conv(self, j):
        return assignments.blocks_of(self.net)[j].conv1

    # -- the commit -----------------------------------------------------------------------------
    def commit(self, sem):
        for c, bit in zip(sem.channels, sem.bits):
            channel_wise_quantizationperchan(sem.conv.weight.data, bit, c)
        check_pending()


class Session:
    """See the module's docstring. ``batches``: a list of device (x, y) pairs or a ResidentSet;
    ``reference_outputs``: the per-batch softmax list functions.KLdiv takes (the drivers'
    ``originaloutputs``), None = the softmax of the constructing state's ordinary evaluation, kept for
    the session's whole life. ``boundaries``: block names kept at every rebase (None:
    prefix.DEFAULT_BLOCKS, () none) under ``boundary_bytes`` (None: unbounded), deepest first.
    Preconditions and ValueErrors are sensitivity.semilayer_table's.

    A rebase (at construction, after accept(), after a slow trial, after rebase(); lazy except
    after accept()) is one ordinary evaluation (the state's official ``base``: acc, loss, kl, bit for
    bit functions.evaluate_acc_loss_softmax + functions.KLdiv), one unpatched pass through the
    trials' own forward (graph captures, base statistics) and the boundary fill with its self-check.
    ``hooks``: the engine's side (tests)."""

    def __init__(self, net, batches, reference_outputs=None, boundaries=None, boundary_bytes=None, hooks=None):
        if hooks is None:
            p, batches = trials.setup("search.Session", net, batches)
            if reference_outputs is not None:
                reference_outputs = [r.to(p.device) for r in reference_outputs]
            hooks = EngineHooks(net, batches)
        if boundary_bytes is not None and int(boundary_bytes) < 0:
            raise ValueError("smpq: boundary_bytes must be >= 0")
        self.net, self.batches, self.hooks = net, batches, hooks
        self.reference = reference_outputs
        names = prefix.DEFAULT_BLOCKS if boundaries is None else tuple(boundaries)
        # deepest first (prefix.admit's order): each boundary is offered what the deeper ones left of the budget
        self._wanted = sorted({int(hooks.block_index(n)) for n in names}, reverse=True)
        self._budget = None if boundary_bytes is None else int(boundary_bytes)
        self.base = None
        self._plans = {}       # block index -> suffix.Plan holding that boundary's Store
        self._last = None      # (Semilayer, Result, signature) of the last trial
        self._pending = "construction"
        self._closed = False
        self._rep = {"trials": {}, "rebases": {}, "rows_patched": 0, "constant": [],
                     "rebase": dict.fromkeys(_COUNTERS, 0), "patched_trials": dict.fromkeys(_COUNTERS, 0),
                     "rebase_s": 0.0, "boundaries": []}
        self._rebase_now()

    # -- life cycle ---------------------------------------------------------------------------
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        """Release every kept boundary and the state's snapshot."""
        self._release()
        self.hooks._state = None
        self._last = None
        self._closed = True

    def _release(self):
        for j, plan in self._plans.items():
            for row in self._rep["boundaries"]:  # (the report keeps what the trials resumed from it)
                if row["block"] == j:
                    row["resumed_forwards"], row["resumed_conv_launches"] = plan.resumed, plan.launches
            plan.store.release()
        self._plans = {}

    def stores(self):
        """{block index: suffix.Store} of the kept boundaries (empty after close())."""
        return {j: plan.store for j, plan in self._plans.items()}

    def rebase(self):
        """The caller changed the model (e.g. checkpoint.restore_): rebuild the baseline at the next trial."""
        self._release()
        self._last = None
        self._pending = self._pending or "explicit"

    def _rebase_now(self):
        hooks, cause = self.hooks, self._pending
        self._release()
        hooks.sync()
        t0 = time.perf_counter()
        before = hooks.counters()
        acc, loss, outs = hooks.ordinary_eval()
        if self.reference is None:
            self.reference = outs
        if len(self.reference) != len(outs):
            raise ValueError("smpq: reference_outputs must hold one softmax tensor per batch")
        hooks.reference = self.reference
        self.base = Result(acc=acc, loss=loss, kl=hooks.kl_of(self.reference, outs), route="base")
        del outs
        hooks.rebind()
        b, flags, probs = hooks.unpatched_pass()  # captures every graph
        if any(flags) or not hooks.held():
            raise RuntimeError("smpq: the baseline of the search session did not hold (overflow or changed weights)")
        self._base_stats, self._base_kl = list(b), hooks.kl_stats(self.reference, probs)
        del probs
        rows = []
        left = self._budget
        try:
            for j in self._wanted:  # deepest first
                plan = _suffix.Plan(left, self._base_stats, self._base_kl, first=0)
                hooks.plan = plan
                store = _suffix.enter(plan, hooks, hooks.boundary_conv(j), self.batches, hooks.device, self.reference)
                row = dict(plan.blocks[-1], resumed_forwards=0, resumed_conv_launches=0)
                row["self_check_conv_launches"] = plan.launches
                rows.append(row)
                if store is not None:
                    self._plans[j] = plan
                    plan.launches = plan.resumed = 0  # from here on: the trials' resumes
                    if left is not None:
                        left -= store.bytes
        except BaseException:
            self._release()
            raise
        finally:
            hooks.plan = None
        hooks.sync()
        after = hooks.counters()
        for k, a, c in zip(_COUNTERS, before, after):
            self._rep["rebase"][k] += c - a
        self._rep["rebases"][cause] = self._rep["rebases"].get(cause, 0) + 1
        self._rep["rebase_s"] += time.perf_counter() - t0
        self._rep["boundaries"] = rows
        self._constant = {}
        self._pending = None

    # -- trials ------------------------------------------------------------------------------
    def pick(self, block):
        """The deepest kept boundary j <= ``block`` (a block index), or None."""
        at = [j for j, plan in self._plans.items() if j <= block and plan.store.kept]
        return max(at) if at else None

    def trial(self, lnum, channels, bit):
        """The standing state with ``channels`` of conv ``lnum`` quantized at ``bit`` (one int, or one
        per channel): a Result. The model is not written (a slow trial writes and restores it)."""
        if self._closed:
            raise RuntimeError("smpq: the search session is closed")
        hooks = self.hooks
        sem = hooks.semilayer(lnum, channels, bit)
        if self._pending:
            self._rebase_now()
        if not hooks.held():
            raise RuntimeError("smpq: the model changed since the session's last rebase (call rebase())")
        res = Result(lnum=sem.lnum, channels=list(sem.channels), bits=list(sem.bits), param=sem.param)
        const = self._constant.get(sem.lnum)
        if const is None:
            const = self._constant[sem.lnum] = hooks.constant_rows(sem.conv)
        bad = [c for c in sem.channels if const[c]]
        if bad:  # the reference raises there (functions.py:40)
            return self._done(sem, res, "constant", bad)
        route = hooks.route(sem)
        if route is None:
            return self._slow(sem, res, "not_patchable")
        n = len(sem.channels)
        hooks.prepare_one(sem, route)
        j = self.pick(hooks.block_of(sem.conv))
        plan = self._plans.get(j)
        table, kl = hooks.zeros(4, torch.float64), hooks.zeros(2, torch.float64)
        flags, status = hooks.zeros(2, torch.int32), hooks.zeros(n, torch.int32)
        before = hooks.counters()
        hooks.plan = plan
        try:
            with torch.no_grad():
                trials.guarded_trial(hooks, sem, status, self.batches, None if plan is None else plan.store,
                                     self.reference, table, kl, flags)
        except BaseException:
            self._release()
            self._last = None
            self._pending = self._pending or "exception"
            raise
        finally:
            hooks.plan = None
        got = torch.cat([table, kl, flags.to(torch.float64), status.to(torch.float64)]).tolist()  # the one host read
        after = hooks.counters()
        for k, a, c in zip(_COUNTERS, before, after):
            self._rep["patched_trials"][k] += c - a
        row, klrow, (ovf, stale), words = got[:4], got[4:6], got[6:8], [int(v) for v in got[8:]]
        if stale or not hooks.held():
            raise RuntimeError("smpq: the model's weights changed while the search session's trial ran")
        if any(wd == 1 for wd in words):
            return self._done(sem, res, "constant", [c for c, wd in zip(sem.channels, words) if wd == 1])
        if any(wd == 2 for wd in words):
            raise RuntimeError("smpq: the patch kernel refused a list entry (status 2)")
        if any(words):  # 3: off the grid or more than 256 levels; 4: an offset the operand does not have
            return self._slow(sem, res, "unpackable")
        if ovf:
            return self._slow(sem, res, "overflow")
        res.stats, res.kl_stats = row, klrow
        res.loss, res.acc, res.kl = row[0] / row[3], row[1] / row[2], klrow[0] / klrow[1]
        res.resumed_from = None if j is None else hooks.block_name(j)
        self._rep["rows_patched"] += n
        return self._done(sem, res, route)

    def _done(self, sem, res, route, constant=None):
        res.route = route
        self._rep["trials"][route] = self._rep["trials"].get(route, 0) + 1
        if constant is not None:
            self._rep["constant"] += [(sem.lnum, c, sem.bits[sem.channels.index(c)]) for c in constant]
            self._last = None
        else:
            self._last = (sem, res, self.hooks.signature())
        return res

    def _slow(self, sem, res, why):
        """The trial through the public API on the model itself, which is restored bitwise; the
        restore moves the model's signature, so the baseline is rebuilt at the next trial."""
        self._release()
        self._pending = self._pending or "slow"
        res.acc, res.loss, res.kl = self.hooks.slow(sem)
        return self._done(sem, res, "slow:" + why)

    def accept(self):
        """Commit the LAST trial's channels to the model (channel_wise_quantizationperchan +
        check_pending), drop the state's snapshot, rebase at once: the new ``base``, the accepted
        state's official figures. RuntimeError without a preceding trial, after a constant one, or
        when the model changed since that trial."""
        if self._closed or self._last is None:
            raise RuntimeError("smpq: accept() needs a preceding trial of this state (not a constant one)")
        sem, _, sig = self._last
        if self.hooks.signature() != sig:
            raise RuntimeError("smpq: the model changed since the trial accept() would commit")
        self._last = None
        self._release()
        self.hooks.commit(sem)
        self._pending = "accept"
        self._rebase_now()
        return self.base

    def report(self):
        """``trials`` by route; ``rebases`` by cause (construction, accept, slow, explicit, exception);
        ``rows_patched``; ``constant`` [(lnum, channel, bit)]; ``rebase`` / ``patched_trials``: the
        calibrations, graph captures and repacks seen by rebases and by patched trials (the latter
        0 / 0 / 0); ``rebase_s``; ``boundaries``: suffix.enter's row per boundary of the last rebase
        (block, name, resumable, kept, full, bytes, self_check, ...), plus ``resumed_forwards`` and
        ``resumed_conv_launches`` of the trials since (kept when the boundary is released)."""
        rep = {k: (dict(v) if isinstance(v, dict) else list(v) if isinstance(v, list) else v)
               for k, v in self._rep.items()}
        rows = []
        for row in self._rep["boundaries"]:
            row = dict(row)
            plan = self._plans.get(row["block"])
            if plan is not None:
                row["resumed_forwards"], row["resumed_conv_launches"] = plan.resumed, plan.launches
            rows.append(row)
        rep["boundaries"] = rows
        return rep
