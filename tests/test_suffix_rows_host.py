"""The rows route of smpq.suffix on the host, on injected forwards as in
tests/test_suffix_host.py: which blocks are eligible and each "why not", the budget's fallback to the
block input alone, which trials take the route, the order of the two restores when a resumed forward
fails, the report keys and the switch (no GPU needed)."""
import importlib

import pytest
import torch

from test_suffix_host import BATCHES, FakeConv, FakeHooks, _kept, _run, _trials


class FakeRows:
    def __init__(self, nbytes):
        self.nbytes, self.next = nbytes, _kept(4)


class RowsHooks(FakeHooks):
    """FakeHooks + what suffix.enter and sensitivity.run_patched call for the rows route. ``why``:
    {block: reason} of rows_block; ``fill_why``: {block: reason} that fill_rows finds at the batch
    index ``fill_at``; ``last``: {block: its last conv}."""

    def __init__(self, last, why=None, fill_why=None, fill_at=0, extra=6, planes_ok=True, wrong_next=(), **kw):
        super().__init__(**kw)
        self.last, self.why, self.fill_why, self.fill_at = last, dict(why or {}), dict(fill_why or {}), fill_at
        self.extra, self.planes_ok, self.wrong_next, self.filled = extra, planes_ok, set(wrong_next), 0

    def rows_block(self, j):
        return self.why.get(j)

    def last_conv(self, j):
        return self.last[j]

    def rows_bytes(self, x, j):
        return self.extra

    def fill_rows(self, x, j):
        self.log.append(("fill_rows", j, x))
        if j in self.not_resumable:
            return None, None
        kept = _kept(self.nbytes)
        at, self.filled = self.filled, self.filled + 1
        if j in self.fill_why and at >= self.fill_at:
            return kept, self.fill_why[j]
        kept.rows = FakeRows(self.extra)
        return kept, None

    def rows_check(self, st, j):
        self.log.append(("rows_check", j))
        return self.planes_ok

    def resume(self, kept, j):
        out, flags = super().resume(kept, j)
        return out + (0.25 if j in self.wrong_next else 0.0), flags

    def resume_rows(self, kept, j, channel):
        self.log.append(("resume_rows", j, channel))
        assert kept.rows is not None
        return self._value(), torch.zeros(2, dtype=torch.int32)


def _plan(budget=None, first=0, rows=True, batches=2):
    from smpq import suffix
    return suffix.Plan(budget, [float(batches), 0.0, 0.0, float(batches)], first=first, rows=rows)


ROW_KEYS = {"rows", "rows_kept", "rows_trials", "rows_bytes", "rows_self_check", "rows_self_check_s"}


def test_last_conv_trials_take_the_route_and_the_others_resume(built_lib):
    c1, c2 = FakeConv(6), FakeConv(6)  # the block's first and last conv
    hooks = RowsHooks({6: c2})
    plan = _plan()
    got, counts = _run([(True, _trials(c1)), (True, _trials(c2))], hooks, plan)
    assert counts["patched"] == 4 and got[(6, 1, 8)] == (6108.0, False)
    assert [e[0] for e in hooks.log if e[0] in ("fill", "fill_rows")] == ["fill_rows"] * 2  # ONE pass, with the tap
    # the self-check from block 6, the planes check, the self-check from block 7; then c1's trials
    # resume from block 6 and c2's take the rows route with the trial's channel
    seq = [e[:2] if e[0] != "resume_rows" else e for e in hooks.log if e[0] in ("resume", "rows_check", "resume_rows")]
    assert seq == [("resume", 6)] * 2 + [("rows_check", 6)] + [("resume", 7)] * 2 + [("resume", 6)] * 4 + \
        [("resume_rows", 6, 0)] * 2 + [("resume_rows", 6, 1)] * 2
    (b,) = plan.report()["blocks"]
    assert ROW_KEYS <= set(b)
    assert (b["rows"], b["rows_kept"], b["rows_trials"], b["rows_bytes"], b["rows_self_check"]) == ("used", 2, 2, 12, True)
    assert (b["kept"], b["full"], b["bytes"], b["self_check"]) == (2, 0, 2 * 10 + 12, True)
    assert plan.store.rows is None and plan.store.row is None and plan.store.entries == []  # released at the end


@pytest.mark.parametrize("why", ["last_block", "geometry", "not_patchable"])
def test_a_block_that_is_not_eligible_keeps_the_suffix_route(built_lib, why):
    c2 = FakeConv(6)
    hooks = RowsHooks({6: c2}, why={6: why})
    plan = _plan()
    got, _ = _run([(True, _trials(c2))], hooks, plan)
    assert got[(6, 0, 8)] == (6008.0, False)
    assert [e[0] for e in hooks.log if e[0] in ("fill", "fill_rows")] == ["fill"] * 2
    assert not [e for e in hooks.log if e[0] in ("rows_check", "resume_rows")]
    assert [e[1] for e in hooks.log if e[0] == "resume"] == [6] * 6
    (b,) = plan.report()["blocks"]
    assert (b["rows"], b["rows_kept"], b["rows_trials"], b["rows_bytes"], b["rows_self_check"]) == (why, 0, 0, 0, None)
    assert (b["kept"], b["bytes"]) == (2, 20)


@pytest.mark.parametrize("why,at", [("no_tap", 0), ("next_not_resumable", 0), ("no_tap", 1)])
def test_a_tap_that_stays_empty_drops_the_route_for_the_whole_block(built_lib, why, at):
    c2 = FakeConv(6)
    hooks = RowsHooks({6: c2}, fill_why={6: why}, fill_at=at)
    plan = _plan()
    got, _ = _run([(True, _trials(c2))], hooks, plan)
    assert got[(6, 1, 8)] == (6108.0, False)
    # the batch that found it is still kept (its block input is fill's); later batches are filled plainly
    assert [e[0] for e in hooks.log if e[0] in ("fill", "fill_rows")] == ["fill_rows"] * (at + 1) + ["fill"] * (1 - at)
    assert not [e for e in hooks.log if e[0] in ("rows_check", "resume_rows")]
    (b,) = plan.report()["blocks"]
    assert (b["rows"], b["rows_kept"], b["rows_trials"], b["rows_bytes"]) == (why, 0, 0, 0)
    assert (b["kept"], b["bytes"], b["resumable"]) == (2, 20, True)  # an earlier batch's extra bytes are given back


def test_the_other_reasons(built_lib):
    c2, c9 = FakeConv(2), FakeConv(9)
    hooks = RowsHooks({2: c2, 9: c9}, not_resumable={9})
    plan = _plan(first=3)
    _run([(True, _trials(c2)), (True, _trials(c9))], hooks, plan)
    b2, b9 = plan.report()["blocks"]
    assert (b2["used"], b2["rows"]) == (False, "below_cut")
    assert (b9["resumable"], b9["rows"], b9["kept"]) == (False, "not_resumable", 0)
    off = _plan(rows=False)
    hooks = RowsHooks({6: c2})
    _run([(True, _trials(FakeConv(6)))], hooks, off)
    (b,) = off.report()["blocks"]
    assert ROW_KEYS <= set(b) and (b["rows"], b["rows_trials"], b["rows_self_check"]) == ("off", 0, None)
    assert not [e for e in hooks.log if e[0] in ("fill_rows", "rows_check", "resume_rows")]


def test_budget_falls_back_to_the_block_input_batch_by_batch(built_lib):
    c2 = FakeConv(6)
    # 10 bytes per block input, 6 more for the rows route: 27 holds the first batch with them (16) and
    # the second without (10); the third fits neither way and is forwarded in full
    hooks = RowsHooks({6: c2})
    plan = _plan(budget=27, batches=3)
    batches = BATCHES + [("x2", "y2")]
    from smpq import sensitivity
    got = {}
    sensitivity.sweep([(True, _trials(c2, channels=(0,)))], batches, hooks, "cpu",
                      lambda tr, loss, slow, row: got.__setitem__(hooks._key(tr), loss),
                      {"patched": 0, "overflowed": 0, "slow": {}, "constant": []}, plan=plan)
    assert got == {(6, 0, 8): 6008.0}
    assert [e[0] for e in hooks.log if e[0] in ("fill", "fill_rows")] == ["fill_rows", "fill"]
    (b,) = plan.report()["blocks"]
    assert (b["kept"], b["full"], b["bytes"], b["rows"], b["rows_kept"], b["rows_bytes"]) == (2, 1, 26, "used", 1, 6)
    trial = [e[0] if e[0] != "forward" else e for e in hooks.log if e[0] in ("resume_rows", "resume", "forward")][-3:]
    assert trial == ["resume_rows", "resume", ("forward", "x2")]
    # no batch fits with the extra tensors: the block is kept 5h's way, and the report says why
    hooks = RowsHooks({6: c2})
    plan = _plan(budget=15)
    _run([(True, _trials(c2, channels=(0,)))], hooks, plan)
    (b,) = plan.report()["blocks"]
    assert (b["kept"], b["bytes"], b["rows"], b["rows_kept"], b["rows_self_check"]) == (1, 10, "budget", 0, None)
    assert [e[0] for e in hooks.log if e[0] in ("fill", "fill_rows")] == ["fill"]
    assert not [e for e in hooks.log if e[0] in ("rows_check", "resume_rows")]


@pytest.mark.parametrize("planes_ok,wrong_next", [(False, ()), (True, (7,))])
def test_a_failed_rows_self_check_raises_and_releases(built_lib, planes_ok, wrong_next):
    c2 = FakeConv(6)
    hooks = RowsHooks({6: c2}, planes_ok=planes_ok, wrong_next=wrong_next)
    plan = _plan()
    with pytest.raises(RuntimeError, match="rows route's self-check"):
        _run([(True, _trials(c2))], hooks, plan)
    assert not [e for e in hooks.log if e[0] == "patch"]  # no trial ran on it
    (b,) = plan.report()["blocks"]
    assert b["self_check"] is True and b["rows_self_check"] is False
    assert plan.store.entries == [] and plan.store.block is None and plan.store.rows is None


def test_restore_order_when_the_resumed_forward_fails(built_lib, monkeypatch):
    """The real EngineHooks.resume_rows around injected launches: the kept planes are put back first
    (only the slices that were written), then the operand, then the conv is invalidated, and the
    sweep releases the store."""
    from smpq import suffix, trials

    log = []

    class Hooks(RowsHooks, trials.EngineHooks):
        net = None
        resume_rows = trials.EngineHooks.resume_rows

        def _one_row(self, j, channel, device):
            return ("rows", j, channel)

        def patch(self, tr, status):
            log.append("patch")
            super().patch(tr, status)

        def restore(self, tr):
            log.append("operand_restore")
            super().restore(tr)

        def invalidate(self, tr):
            log.append("invalidate")
            super().invalidate(tr)

        def resume(self, kept, j):
            if self.cur is not None:
                log.append("resume %d" % j)
                raise KeyboardInterrupt("stop")
            return RowsHooks.resume(self, kept, j)

    def rows_conv(net, kept, j, rows, flag, done):
        log.append("rows_conv %r" % (rows,))
        done.append(1)  # one slice written

    def rows_restore(kept, rows, done):
        log.append("rows_restore %r %d" % (rows, len(done)))

    monkeypatch.setattr(suffix, "rows_conv", rows_conv)
    monkeypatch.setattr(suffix, "rows_restore", rows_restore)
    c2 = FakeConv(6)
    hooks = Hooks({6: c2})
    plan = _plan()
    released = []
    real = plan.store.release
    plan.store.release = lambda: (released.append(list(log)), real())[1]
    with pytest.raises(KeyboardInterrupt):
        _run([(True, _trials(c2, channels=(3,)))], hooks, plan)
    assert log == ["patch", "rows_conv ('rows', 6, 3)", "resume 7", "rows_restore ('rows', 6, 3) 1", "operand_restore",
                   "invalidate"]
    assert released[-1] == log and c2._content_gen == 1  # the store went after both restores
    assert plan.store.entries == [] and plan.store.rows is None


def test_semilayer_trials_of_the_rows_conv_resume_from_the_block(built_lib):
    """The one loop serves both tables, so this pins who takes the rows route: a semilayer sweep
    (with refs) over a block's last conv, through a plan with rows=True whose store holds the route's
    tensors, still resumes every batch from block j (a semilayer of one channel too): the route is
    for the single-row trials (Trial) of the store's ``rows`` conv. Both self-checks run, and compare
    the KL statistics as well."""
    from smpq import sensitivity, suffix
    c2 = FakeConv(6)
    refs = [0.25, 0.5]
    sems = [sensitivity.Semilayer(0, 1, c2, [0, 1], [8, 8], 64), sensitivity.Semilayer(1, 1, c2, [3], [4], 64)]
    counts = {"patched": 0, "overflowed": 0, "slow": {}, "constant": [], "rows_patched": 0, "max_rows": 0}
    hooks = RowsHooks({6: c2})
    plan = suffix.Plan(None, [2.0, 0.0, 2.0, 2.0], [0.75, 2.0], first=0, rows=True)
    got = {}
    sensitivity.sweep([(True, sems)], BATCHES, hooks, "cpu",
                      lambda sem, loss, acc, kl, slow, row, kl_row: got.__setitem__(sem.index, (loss, kl, slow)),
                      counts, plan=plan, refs=refs)
    assert got == {0: (6000.0, 0.375, False), 1: (6001.0, 0.375, False)}
    assert counts["patched"] == 2 and counts["rows_patched"] == 3 and counts["max_rows"] == 2
    assert not [e for e in hooks.log if e[0] == "resume_rows"]
    seq = [e[:2] for e in hooks.log if e[0] in ("resume", "rows_check")]
    assert seq == [("resume", 6)] * 2 + [("rows_check", 6)] + [("resume", 7)] * 2 + [("resume", 6)] * 4
    assert [e[0] for e in hooks.log if e[0] in ("patch", "restore")] == ["patch", "restore"] * 2
    (b,) = plan.report()["blocks"]
    assert (b["rows"], b["rows_kept"], b["rows_trials"], b["self_check"], b["rows_self_check"]) == ("used", 2, 0, True, True)
    assert plan.store.entries == [] and plan.store.rows is None
    # the KL statistics are part of the self-check: another base_kl fails it before any trial
    hooks = RowsHooks({6: c2})
    plan = suffix.Plan(None, [2.0, 0.0, 2.0, 2.0], [0.5, 2.0], first=0, rows=True)
    with pytest.raises(RuntimeError, match="does not reproduce"):
        sensitivity.sweep([(True, sems)], BATCHES, hooks, "cpu", lambda *a: None, dict(counts), plan=plan, refs=refs)
    assert not [e for e in hooks.log if e[0] == "patch"] and plan.store.entries == []


def test_env_switch(built_lib, monkeypatch, capsys):
    from smpq import suffix
    try:
        monkeypatch.delenv("SMPQ_TRIAL_ROWS", raising=False)
        importlib.reload(suffix)
        assert suffix.TRIAL_ROWS == [False]  # off by default
        assert suffix.rows_switch() is False and suffix.rows_switch(None, True) is False
        assert suffix.rows_switch(True, False) is False  # honoured only with the suffix on
        assert capsys.readouterr().err == ""
        assert suffix.rows_switch(True, True) is True
        assert "SMPQ_TRIAL_ROWS=1" in capsys.readouterr().err
        assert suffix.rows_switch(True) is True and capsys.readouterr().err == ""  # announced once
        monkeypatch.setenv("SMPQ_TRIAL_ROWS", "1")
        importlib.reload(suffix)
        assert suffix.TRIAL_ROWS == [True] and suffix.rows_switch() is True and suffix.rows_switch(False) is False
        assert suffix.rows_switch(None, False) is False
    finally:
        monkeypatch.undo()
        importlib.reload(suffix)


def test_rows_bytes_are_the_design_documents(built_lib):
    """Per image at 3 limbs: the last conv's input, the next block's input, a
    downsample's output where the block has one, and one channel's save area."""
    import resnet
    from smpq import ops, prefix, suffix
    with torch.device("meta"):
        r50, r18 = resnet.resnet50().eval(), resnet.resnet18().eval()
    assert ops.get_act_limbs() == 3
    x = torch.empty(1, 3, 224, 224, device="meta")
    for name in ("layer3.1", "layer3.5"):
        j = prefix.block_index(r50, name)
        assert suffix.kept_bytes(r50, x, j) == 602112
        assert suffix.rows_bytes(r50, x, j) == 150528 + 602112 + 3 * 14 * 14
    j = prefix.block_index(r50, "layer4.1")
    assert suffix.rows_bytes(r50, x, j) == 75264 + 301056 + 3 * 49
    j = prefix.block_index(r50, "layer3.0")  # a block with a downsample keeps its output too
    assert suffix.rows_bytes(r50, x, j) == 150528 + 2 * 602112 + 3 * 196
    j = prefix.block_index(r18, "layer4.0")
    assert suffix.rows_bytes(r18, x, j) == 3 * 49 * 512 * 3 + 3 * 49
    assert ops.trial_rows_conv_save_bytes(3, 196, 1) == 588


def test_the_table_takes_the_argument(built_lib):
    import resnet
    from smpq import sensitivity
    net = resnet.resnet18().eval()
    x = [(torch.zeros(1, 3, 32, 32), torch.zeros(1, dtype=torch.long))]
    with pytest.raises(ValueError):  # a model on the CPU, whatever the switch
        sensitivity.delta_loss_table(net, x, suffix=True, rows=True)
