"""smpq.suffix on the host: which block owns a searched conv, the store's admission arithmetic, the
order of groups and the store's fill / release sequence through sensitivity.sweep / sweep_rows on
injected forwards, and the environment switches (no GPU needed)."""
import importlib

import pytest
import torch


def _meta(arch):
    import resnet
    torch.manual_seed(0)
    with torch.device("meta"):
        return getattr(resnet, arch)().eval()


# ---- block_of ------------------------------------------------------------------------------------
@pytest.mark.parametrize("arch,convs", [("resnet18", 16), ("resnet34", 32), ("resnet50", 48)])
def test_block_of_every_lnum(built_lib, arch, convs):
    from smpq import assignments, prefix, suffix
    net = _meta(arch)
    names = prefix.block_names(net)
    module_name = {id(m): n for n, m in net.named_modules()}
    assert len(assignments.addressable_convs(net)) == convs
    seen = []
    for ln in range(1, convs + 1):
        conv = assignments.conv_for_lnum(net, ln)
        j = suffix.block_of(net, conv)
        assert module_name[id(conv)].rsplit(".", 1)[0] == names[j], (ln, names[j])
        assert prefix.block_index(net, names[j]) == j
        seen.append(j)
    assert seen == sorted(seen) and set(seen) == set(range(len(names)))  # lnum order is block order
    with pytest.raises(ValueError):
        suffix.block_of(net, net.conv1)
    with pytest.raises(ValueError):
        suffix.block_of(net, net.layer2[0].downsample[0])


def test_first_block_follows_the_share_of_blocks_skipped(built_lib, monkeypatch):
    from smpq import suffix
    from smpq import prefix
    r50, r18 = _meta("resnet50"), _meta("resnet18")
    for net in (r50, r18, _meta("resnet34")):  # the shipped cut: layer3.0 in every family
        assert prefix.block_names(net)[suffix.first_block(net)] == "layer3.0"
    monkeypatch.setattr(suffix, "MIN_SKIPPED", [0.0])
    assert suffix.first_block(r50) == 0
    monkeypatch.setattr(suffix, "MIN_SKIPPED", [0.5])
    assert suffix.first_block(r50) == 8 and suffix.first_block(r18) == 4
    monkeypatch.setattr(suffix, "MIN_SKIPPED", [0.8])
    assert suffix.first_block(r50) == 13 and suffix.first_block(r18) == 7  # 13/16 = 0.8125, 7/8 = 0.875
    monkeypatch.setattr(suffix, "MIN_SKIPPED", [1.0])
    assert suffix.first_block(r50) == 16  # no block


def test_slices_are_the_forwards_own(built_lib, monkeypatch):
    from smpq import engine, suffix
    monkeypatch.setattr(engine, "STREAMS", [2])
    monkeypatch.setattr(engine, "CHUNK", [256])
    assert suffix.slices(8) == [(0, 4), (4, 8)]
    assert suffix.slices(5) == [(0, 3), (3, 5)]
    assert suffix.slices(4) == [(0, 2), (2, 4)]
    assert suffix.slices(3) == [(0, 3)]
    assert suffix.slices(256) == [(0, 128), (128, 256)]
    assert suffix.slices(300) == [(0, 256), (256, 300)]  # chunks are not cut again
    monkeypatch.setattr(engine, "STREAMS", [1])
    assert suffix.slices(8) == [(0, 8)]


# ---- the store -----------------------------------------------------------------------------------
def _kept(nbytes, y=None):
    from smpq import suffix
    return suffix.Kept([(0, 1, torch.zeros(nbytes, dtype=torch.int8), 1.0)], 1, y)


def test_store_admission_against_boundary_bytes(built_lib):
    from smpq import prefix, suffix
    net = _meta("resnet50")
    j = prefix.block_index(net, "layer3.0")
    limbs, n, h, w, c = prefix.boundary_shape(net, j, 256, 224, 224, 3)
    assert (limbs, n, h, w, c) == (3, 256, 28, 28, 512)
    per_batch = prefix.boundary_bytes(limbs, c, h, w, n)
    assert per_batch == 1204224 * 256  # DESIGN.md 5e's bytes per image at layer3.0
    x = torch.empty(256, 3, 224, 224, device="meta")
    assert suffix.kept_bytes(net, x, j) == per_batch
    assert suffix.kept_bytes(net, x, prefix.block_index(net, "layer4.0")) == 602112 * 256
    small = suffix.kept_bytes(net, torch.empty(100, 3, 224, 224, device="meta"), j)

    st = suffix.Store(budget=2 * per_batch + small)
    st.begin(j)
    order = []
    for nb in (per_batch, per_batch, per_batch, small, small):  # in order; what fits is admitted
        ok = st.fits(nb)
        order.append(ok)
        st.add(_kept(8) if ok else None, nb)
    assert order == [True, True, False, True, False]
    assert st.bytes == 2 * per_batch + small and st.kept == 3 and not st.complete and st.block == j
    st.release()
    assert st.entries == [] and st.bytes == 0 and st.block is None and st.kept == 0

    assert not suffix.Store(budget=0).fits(1) and suffix.Store(budget=0).fits(0)
    assert suffix.Store(budget=None).fits(1 << 60)
    exact = suffix.Store(budget=per_batch)
    assert exact.fits(per_batch)
    exact.add(_kept(8), per_batch)
    assert not exact.fits(per_batch)


def test_store_walk_iterates_the_set_only_when_it_must(built_lib):
    from smpq import suffix

    class Set:
        def __init__(self, n):
            self.n, self.iterated = n, 0

        def __iter__(self):
            self.iterated += 1
            return iter([("x%d" % i, "y%d" % i) for i in range(self.n)])

    st = suffix.Store()
    st.begin(3)
    a, b = _kept(4, "ya"), _kept(4, "yb")
    st.add(a, 4)
    st.add(b, 4)
    s = Set(2)
    assert list(st.walk(s)) == [(a, None, "ya"), (b, None, "yb")] and s.iterated == 0
    st.begin(4)
    st.add(a, 4)
    st.add(None, 4)
    assert list(st.walk(s)) == [(a, None, "ya"), (None, "x1", "y1")] and s.iterated == 1
    with pytest.raises(RuntimeError):
        list(st.walk(Set(3)))  # the set changed its length under the table
    st.release()
    assert list(st.walk(Set(2))) == [(None, "x0", "y0"), (None, "x1", "y1")]


# ---- the sweeps on injected forwards ---------------------------------------------------------------
class FakeConv:
    def __init__(self, block):
        self.block, self._content_gen = block, 0


class FakeHooks:
    """Forwards and resumed forwards that score the patched trial's marker (1.0 without a patch)."""

    def __init__(self, not_resumable=(), raise_at=None, nbytes=10, wrong=()):
        self.not_resumable, self.raise_at, self.nbytes, self.wrong = set(not_resumable), raise_at, nbytes, set(wrong)
        self.log, self.cur = [], None

    # the trials' hooks
    def patch(self, tr, status):
        self.cur = tr
        self.log.append(("patch", self._key(tr)))

    def restore(self, tr):
        self.log.append(("restore", self._key(tr)))
        self.cur = None

    def invalidate(self, tr):
        tr.conv._content_gen += 1

    @staticmethod
    def _key(tr):
        return (tr.conv.block, tr.channel, tr.bit) if hasattr(tr, "channel") else (tr.conv.block, tr.index)

    def _value(self):
        if self.cur is None:
            return 1.0
        return float(1000 * self.cur.conv.block + (100 * self.cur.channel + self.cur.bit if hasattr(self.cur, "channel")
                                                   else self.cur.index))

    def forward(self, x):
        self.log.append(("forward", x))
        return self._value(), torch.zeros(2, dtype=torch.int32)

    def score(self, logits, y, row):
        row[0] += logits
        row[3] += 1

    def score_kl(self, logits, y, ref, row, kl_row):
        row[0] += logits
        row[2] += 1
        row[3] += 1
        kl_row[0] += ref
        kl_row[1] += 1

    def slow(self, tr):
        return -1.0

    # what suffix.enter calls
    def block_of(self, conv):
        return conv.block

    def block_name(self, j):
        return "block%d" % j

    def kept_bytes(self, x, j):
        return self.nbytes

    def fill(self, x, j):
        self.log.append(("fill", j, x))
        return None if j in self.not_resumable else _kept(self.nbytes)

    def resume(self, kept, j):
        self.log.append(("resume", j))
        if self.cur is not None and self._key(self.cur) == self.raise_at:
            raise KeyboardInterrupt("stop")
        return self._value() + (0.5 if j in self.wrong else 0.0), torch.zeros(2, dtype=torch.int32)

    def sync(self):
        pass


BATCHES = [("x0", "y0"), ("x1", "y1")]


def _trials(conv, channels=(0, 1), bits=(8,), col=0):
    from smpq.sensitivity import Trial
    return [Trial(col + i, 1, conv, c, b) for i, (c, b) in enumerate((c, b) for c in channels for b in bits)]


def _counts():
    return {"patched": 0, "overflowed": 0, "slow": {}, "constant": [], "rows_patched": 0, "max_rows": 0}


def _run(groups, hooks, plan, got=None):
    from smpq import sensitivity
    got = {} if got is None else got
    counts = _counts()
    sensitivity.sweep(groups, BATCHES, hooks, "cpu", lambda tr, loss, slow, row: got.__setitem__(hooks._key(tr), (loss, slow)),
                      counts, plan=plan)
    return got, counts


def test_sweep_fills_once_per_block_in_block_order(built_lib):
    from smpq import suffix
    c5a, c5b, c2, c7 = FakeConv(5), FakeConv(5), FakeConv(2), FakeConv(7)
    hooks = FakeHooks()
    plan = suffix.Plan(None, [2.0, 0.0, 0.0, 2.0], first=3)
    releases = []
    real = plan.store.release
    plan.store.release = lambda: (releases.append(plan.store.block), real())[1]
    groups = [(True, _trials(c7)), (True, _trials(c5a)), (True, _trials(c2)), (True, _trials(c5b, channels=(3,)))]
    got, counts = _run(groups, hooks, plan)
    assert counts["patched"] == 7
    assert got[(5, 0, 8)] == ((5000 + 8.0), False) and got[(7, 1, 8)] == (7108.0, False) and got[(2, 1, 8)] == (2108.0, False)
    # block order: 2 (below the cut: replay, no fill), then 5 (both convs, ONE fill), then 7
    patches = [e[1][0] for e in hooks.log if e[0] == "patch"]
    assert patches == [2, 2, 5, 5, 5, 7, 7]
    fills = [e[1] for e in hooks.log if e[0] == "fill"]
    assert fills == [5, 5, 7, 7]  # one pass over the two batches per block
    assert [e for e in hooks.log if e[0] == "forward"] == [("forward", "x0"), ("forward", "x1")] * 2  # block 2's trials
    # per block: 2 self-check resumes, then 2 per trial
    assert [e[1] for e in hooks.log if e[0] == "resume"] == [5] * (2 + 3 * 2) + [7] * (2 + 2 * 2)
    # released on every change of block and at the end (None: nothing was held)
    assert releases == [None, None, 5, 7]
    rep = plan.report()
    assert [(b["block"], b["used"], b["resumable"], b["kept"], b["full"], b["bytes"], b["self_check"]) for b in rep["blocks"]] == \
        [(2, False, None, 0, None, 0, None), (5, True, True, 2, 0, 20, True), (7, True, True, 2, 0, 20, True)]
    assert rep["blocks"][1]["name"] == "block5" and rep["first_block"] == 3
    assert plan.store.entries == [] and plan.store.block is None


def test_sweep_without_a_plan_keeps_the_given_order(built_lib):
    c7, c2 = FakeConv(7), FakeConv(2)
    hooks = FakeHooks()
    _run([(True, _trials(c7)), (True, _trials(c2))], hooks, None)
    assert [e[1][0] for e in hooks.log if e[0] == "patch"] == [7, 7, 2, 2]
    assert not [e for e in hooks.log if e[0] in ("fill", "resume")]


def test_a_block_that_cannot_be_resumed_falls_back_and_is_counted(built_lib):
    from smpq import suffix
    c4, c6 = FakeConv(4), FakeConv(6)
    hooks = FakeHooks(not_resumable={4})
    plan = suffix.Plan(None, [2.0, 0.0, 0.0, 2.0], first=0)
    got, counts = _run([(True, _trials(c4)), (True, _trials(c6))], hooks, plan)
    assert counts["patched"] == 4 and got[(4, 1, 8)] == (4108.0, False)
    assert [e[1] for e in hooks.log if e[0] == "fill"] == [4, 6, 6]  # the first refusal ends block 4's filling
    assert [e[1] for e in hooks.log if e[0] == "resume"] == [6] * 6
    assert len([e for e in hooks.log if e[0] == "forward"]) == 4  # block 4's two trials, two batches each
    b4, b6 = plan.report()["blocks"]
    assert (b4["resumable"], b4["kept"], b4["full"], b4["bytes"], b4["self_check"]) == (False, 0, 2, 0, None)
    assert (b6["resumable"], b6["kept"], b6["full"], b6["self_check"]) == (True, 2, 0, True)


def test_budget_keeps_what_fits_and_forwards_the_rest(built_lib):
    from smpq import suffix
    c6 = FakeConv(6)
    hooks = FakeHooks(nbytes=10)
    plan = suffix.Plan(15, [2.0, 0.0, 0.0, 2.0], first=0)
    got, _ = _run([(True, _trials(c6, channels=(0,)))], hooks, plan)
    assert got[(6, 0, 8)] == (6008.0, False)
    seq = [e[0] if e[0] != "forward" else e for e in hooks.log if e[0] in ("resume", "forward")]
    assert seq == ["resume", ("forward", "x1")] * 2  # the self-check, then the trial
    (b6,) = plan.report()["blocks"]
    assert (b6["kept"], b6["full"], b6["bytes"], b6["resumable"]) == (1, 1, 10, True)
    hooks = FakeHooks(nbytes=10)
    plan = suffix.Plan(0, [2.0, 0.0, 0.0, 2.0], first=0)
    _run([(True, _trials(c6, channels=(0,)))], hooks, plan)
    assert not [e for e in hooks.log if e[0] in ("fill", "resume")]
    assert plan.report()["blocks"][0]["kept"] == 0 and plan.report()["blocks"][0]["full"] == 2


def test_the_store_is_released_on_an_exception(built_lib):
    from smpq import suffix
    c6 = FakeConv(6)
    hooks = FakeHooks(raise_at=(6, 1, 8))
    plan = suffix.Plan(None, [2.0, 0.0, 0.0, 2.0], first=0)
    with pytest.raises(KeyboardInterrupt):
        _run([(True, _trials(c6))], hooks, plan)
    assert hooks.log[-3:] == [("patch", (6, 1, 8)), ("resume", 6), ("restore", (6, 1, 8))]
    assert c6._content_gen == 1
    assert plan.store.entries == [] and plan.store.block is None and plan.store.bytes == 0


def test_a_failed_self_check_raises_and_releases(built_lib):
    from smpq import suffix
    c6 = FakeConv(6)
    hooks = FakeHooks(wrong={6})
    plan = suffix.Plan(None, [2.0, 0.0, 0.0, 2.0], first=0)
    with pytest.raises(RuntimeError, match="does not reproduce"):
        _run([(True, _trials(c6))], hooks, plan)
    assert not [e for e in hooks.log if e[0] == "patch"]  # no trial ran on it
    assert plan.report()["blocks"][0]["self_check"] is False
    assert plan.store.entries == [] and plan.store.block is None


def test_sweep_rows_checks_the_kl_statistics_too(built_lib):
    from smpq import sensitivity, suffix
    c3, c6 = FakeConv(3), FakeConv(6)

    def sems(conv, idx):
        s = sensitivity.Semilayer(idx, 1, conv, [0, 1], [8, 8], 64)
        return s

    refs = [0.25, 0.5]
    for base_kl, ok in (([0.75, 2.0], True), ([0.5, 2.0], False)):
        hooks = FakeHooks()
        plan = suffix.Plan(None, [2.0, 0.0, 2.0, 2.0], base_kl, first=0)
        got = {}

        def out(sem, loss, acc, klv, slow, row, kl_row):
            got[sem.index] = (loss, klv)

        args = ([(True, [sems(c6, 0)]), (True, [sems(c3, 1)])], BATCHES, refs, hooks, "cpu", out, _counts())
        if ok:
            sensitivity.sweep_rows(*args, plan=plan)
            assert [e[1][0] for e in hooks.log if e[0] == "patch"] == [3, 6]  # block order
            assert got == {1: (3001.0, 0.375), 0: (6000.0, 0.375)}
            assert [b["self_check"] for b in plan.report()["blocks"]] == [True, True]
        else:
            with pytest.raises(RuntimeError):
                sensitivity.sweep_rows(*args, plan=plan)
        assert plan.store.entries == []


# ---- the switches ----------------------------------------------------------------------------------
def test_env_switch_parsing(built_lib, monkeypatch, capsys):
    from smpq import suffix
    assert suffix._gb(None) is None and suffix._gb("") is None and suffix._gb(" ") is None
    assert suffix._gb("0") == 0 and suffix._gb("1") == 1 << 30 and suffix._gb("0.5") == 1 << 29
    for bad in ("-1", "nan"):
        with pytest.raises(ValueError):
            suffix._gb(bad)
    with pytest.raises(ValueError):
        suffix._gb("many")
    try:
        monkeypatch.delenv("SMPQ_TRIAL_SUFFIX", raising=False)
        monkeypatch.delenv("SMPQ_TRIAL_SUFFIX_GB", raising=False)
        importlib.reload(suffix)
        assert suffix.TRIAL_SUFFIX == [False] and suffix.TRIAL_SUFFIX_BYTES == [None]  # off by default
        assert suffix.switch() == (False, None)
        assert capsys.readouterr().err == ""  # nothing is announced while it is off
        monkeypatch.setenv("SMPQ_TRIAL_SUFFIX", "1")
        monkeypatch.setenv("SMPQ_TRIAL_SUFFIX_GB", "2")
        importlib.reload(suffix)
        assert suffix.TRIAL_SUFFIX == [True] and suffix.TRIAL_SUFFIX_BYTES == [2 << 30]
        assert suffix.switch() == (True, 2 << 30)
        assert "SMPQ_TRIAL_SUFFIX=1" in capsys.readouterr().err
        assert suffix.switch() == (True, 2 << 30) and capsys.readouterr().err == ""  # announced once
        assert suffix.switch(False) == (False, 2 << 30) and suffix.switch(None, 7) == (True, 7)
        with pytest.raises(ValueError):
            suffix.switch(True, -1)
        monkeypatch.setenv("SMPQ_TRIAL_SUFFIX", "yes")  # only "1" turns it on, as for the other switches
        importlib.reload(suffix)
        assert suffix.TRIAL_SUFFIX == [False]
    finally:
        monkeypatch.undo()
        importlib.reload(suffix)


def test_tables_take_the_arguments_and_still_refuse_other_modes(built_lib):
    import resnet
    from smpq import engine, sensitivity
    net = resnet.resnet18().eval()
    x = [(torch.zeros(1, 3, 32, 32), torch.zeros(1, dtype=torch.long))]
    with pytest.raises(ValueError):  # a model on the CPU, whatever the switch
        sensitivity.delta_loss_table(net, x, suffix=True, suffix_bytes=0)
    with pytest.raises(ValueError):
        sensitivity.semilayer_table(net, x, [(1, [0], 4)], suffix=True)
    engine.set_range_mode("dynamic")
    try:
        with pytest.raises(ValueError):
            sensitivity.delta_loss_table(net, [], suffix=True)
    finally:
        engine.set_range_mode("static")
