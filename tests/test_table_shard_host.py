"""Sharded sensitivity tables on the host: the assignment of columns to ranks, the
merge of partial tables and what it refuses, write_csv of a partial table, the failure protocol of
dp.sharded_delta_loss_table over a world-2 gloo CPU group with an injected table function (the
ranks run as tests/test_dist.py's do), and the command line's argument checks. No GPU needed."""
import datetime
import math
import os
import socket
import time
import types

import numpy as np
import pytest
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.join(os.path.dirname(HERE), "semilayer-wise-mixed-precision-quantization_amd")
GROUP_TIMEOUT_S = 60


# ---- the assignment ------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [1, 2, 3, 8])
@pytest.mark.parametrize("channels", [None, [0, 3, 5, 9, 63], {1: [1, 2, 3], 16: range(0, 512, 7)}])
def test_shard_owner_covers_every_column_once(world, channels):
    import resnet
    from smpq import sensitivity
    net = resnet.resnet18()
    lnums = [1, 7, 16]
    cols = sensitivity._select(net, lnums, channels)
    lnum = [ln for ln, _, _ in cols]
    owner = sensitivity.shard_owner(world, lnum=lnum)
    assert owner.shape == (len(cols),) and owner.min() >= 0 and owner.max() < world
    # every (lnum, channel) belongs to exactly one rank, and position i of a conv's list to i % world
    masks = [owner == r for r in range(world)]
    assert (np.sum(masks, axis=0) == 1).all()
    at = {}
    for col, (ln, _, c) in enumerate(cols):
        assert owner[col] == at.get(ln, 0) % world, (ln, c)
        at[ln] = at.get(ln, 0) + 1
    for ln in lnums:  # balanced per conv: the ranks' shares differ by at most one column
        share = [int((owner[np.asarray(lnum) == ln] == r).sum()) for r in range(world)]
        assert max(share) - min(share) <= 1, (ln, share)


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_owner_semilayers(world):
    from smpq import sensitivity
    for n in (0, 1, 4, 17):
        owner = sensitivity.shard_owner(world, count=n)
        assert owner.tolist() == [i % world for i in range(n)]
        assert (np.sum([owner == r for r in range(world)], axis=0) == 1).all()


def test_shard_arguments():
    from smpq import sensitivity
    assert sensitivity.check_shard(None) is None and sensitivity.check_shard((1, 2)) == (1, 2)
    for bad in ((0, 0), (-1, 2), (2, 2), (0, -1), (0,), "ab"):
        with pytest.raises(ValueError):
            sensitivity.check_shard(bad)
    with pytest.raises(ValueError):
        sensitivity.shard_owner(0, count=3)
    with pytest.raises(ValueError):
        sensitivity.shard_owner(2)
    with pytest.raises(ValueError):
        sensitivity.shard_owner(2, lnum=[1], count=1)


# ---- hand-made tables ----------------------------------------------------------------------------
LNUM = [1, 1, 1, 5, 5, 9]
CNUM = [0, 7, 9, 2, 3, 4]
BITS = (8, 2)
CONST_COL = 4  # (lnum 5, channel 3): nan in the whole table too
BASE, EVAL = 6.907755278982137, 6.9077552789821375  # (one ulp apart)


def _whole():
    from smpq import sensitivity
    rng = np.random.default_rng(3)
    delta = {b: rng.standard_normal(len(LNUM)) for b in BITS}
    stats = {b: rng.standard_normal((len(LNUM), 4)) for b in BITS}
    stats[2][2] = np.nan  # a slow trial: a delta, no statistics
    for b in BITS:
        delta[b][CONST_COL] = np.nan
        stats[b][CONST_COL] = np.nan
    rep = {"trials": 12, "patched": 9, "overflowed": 1, "slow": {"overflow": 1}, "constant": [(5, 3, 8), (5, 3, 2)],
           "baseline_s": 1.0, "trials_s": 2.0}
    t = sensitivity.DeltaLossTable("resnet18", LNUM, CNUM, BITS, delta, BASE, EVAL, rep)
    t.stats = stats
    return t


def _parts(world, whole=None):
    """``whole`` cut into the tables ``world`` sharded calls would return."""
    from smpq import sensitivity
    whole = _whole() if whole is None else whole
    owner = sensitivity.shard_owner(world, lnum=LNUM)
    parts = []
    for r in range(world):
        mine = owner == r
        delta = {b: np.where(mine, whole.delta[b], np.nan) for b in BITS}
        const = [c for c in whole.report()["constant"] if mine[CONST_COL]]
        slow = {"overflow": 1} if mine[2] else {}
        n = int(mine.sum())
        rep = {"trials": n * len(BITS), "patched": n * len(BITS) - len(const) - len(slow), "overflowed": len(slow),
               "slow": slow, "constant": const, "baseline_s": 1.0 + r, "trials_s": 2.0 - 0.5 * r, "shard": [r, world]}
        t = sensitivity.DeltaLossTable("resnet18", LNUM, CNUM, BITS, delta, BASE, EVAL, rep)
        t.stats = {b: np.where(mine[:, None], whole.stats[b], np.nan) for b in BITS}
        t.owned = mine
        parts.append(t)
    return parts


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_merge_reproduces_the_whole(world):
    from smpq import sensitivity
    whole = _whole()
    parts = _parts(world, whole)
    if world == 8:
        assert not parts[7].owned.any()  # a rank that owns nothing still has a valid part
    got = sensitivity.merge_delta_loss(parts)
    assert got.owned is None and got.arch == whole.arch and got.bits == whole.bits
    assert np.array_equal(got.lnum, whole.lnum) and np.array_equal(got.cnum, whole.cnum)
    for b in BITS:
        assert np.array_equal(got.delta[b], whole.delta[b], equal_nan=True)
        assert np.array_equal(got.stats[b], whole.stats[b], equal_nan=True)
        assert np.isnan(got.delta[b][CONST_COL]) and np.isnan(got.stats[b][CONST_COL]).all()
    assert got.base_loss == BASE and got.eval_loss == EVAL
    rep, want = got.report(), whole.report()
    for k in ("trials", "patched", "overflowed", "slow"):
        assert rep[k] == want[k], k
    assert rep["constant"] == sorted(want["constant"])
    assert rep["world"] == world and rep["ranks"] == [p.report() for p in parts]
    assert rep["baseline_s"] == 1.0 + (world - 1) and rep["trials_s"] == 2.0


def test_merge_refusals():
    from smpq import sensitivity
    parts = _parts(2)
    parts[1].owned = parts[1].owned.copy()
    parts[1].owned[0] = True
    with pytest.raises(ValueError, match="column 0 is owned by part 0 and part 1"):
        sensitivity.merge_delta_loss(parts)
    parts = _parts(2)
    parts[0].owned = parts[0].owned.copy()
    parts[0].owned[2] = False
    with pytest.raises(ValueError, match="column 2 is owned by no part"):
        sensitivity.merge_delta_loss(parts)
    parts = _parts(2)
    parts[1].base_loss = float(np.nextafter(BASE, math.inf))
    with pytest.raises(ValueError, match="part 1 has base_loss"):
        sensitivity.merge_delta_loss(parts)
    parts = _parts(2)
    parts[1].eval_loss = float(np.nextafter(EVAL, -math.inf))
    with pytest.raises(ValueError, match="part 1 has eval_loss"):
        sensitivity.merge_delta_loss(parts)
    parts = _parts(2)
    parts[1].bits = (8, 4)
    with pytest.raises(ValueError, match="part 1 has bit-widths"):
        sensitivity.merge_delta_loss(parts)
    parts = _parts(2)
    parts[1].cnum = parts[1].cnum.copy()
    parts[1].cnum[3] = 11
    with pytest.raises(ValueError, match="column 3"):
        sensitivity.merge_delta_loss(parts)
    parts = _parts(2)
    parts[1].arch = "resnet34"
    with pytest.raises(ValueError, match="part 1"):
        sensitivity.merge_delta_loss(parts)
    with pytest.raises(ValueError, match="rank order"):
        sensitivity.merge_delta_loss(_parts(2)[::-1])
    with pytest.raises(ValueError):
        sensitivity.merge_delta_loss(_parts(3)[:2])
    with pytest.raises(ValueError):
        sensitivity.merge_delta_loss([])


def test_write_csv_refuses_a_partial_table(tmp_path):
    from smpq import sensitivity
    parts = _parts(2)
    with pytest.raises(ValueError, match="partial"):
        sensitivity.write_csv(parts[0], str(tmp_path / "part.csv"))
    assert not (tmp_path / "part.csv").exists()
    a, b = str(tmp_path / "merged.csv"), str(tmp_path / "whole.csv")
    sensitivity.write_csv(sensitivity.merge_delta_loss(parts), a)
    sensitivity.write_csv(_whole(), b)
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()
    sensitivity.write_csv(_parts(1)[0], a)  # world 1: owned is all true


def _sem_tables(world):
    from smpq import sensitivity
    spec = [(1, [0, 2], [4, 4]), (1, [1], [8]), (5, [3, 4, 5], [2, 2, 2]), (5, [0], [6]), (9, [7, 8], [4, 2])]
    rng = np.random.default_rng(5)
    vals = {k: rng.standard_normal(len(spec)) for k in ("loss", "acc", "kl")}
    stats, kl_stats = rng.standard_normal((len(spec), 4)), rng.standard_normal((len(spec), 2))
    slow = np.array([False, False, False, True, False])
    stats[3], kl_stats[3] = np.nan, np.nan
    for k in vals:  # semilayer 2 has a constant channel
        vals[k][2] = np.nan
    stats[2], kl_stats[2] = np.nan, np.nan

    def table(mine, rep):
        sems = [types.SimpleNamespace(lnum=ln, channels=ch, bits=bt, param=float(sum(9 * (32 - b) / 32 for b in bt)))
                for ln, ch, bt in spec]
        t = sensitivity.SemilayerTable("resnet18", sems, BASE, EVAL, rep)
        for k in vals:
            getattr(t, k)[mine] = vals[k][mine]
        t.stats[mine], t.kl_stats[mine], t.slow[mine] = stats[mine], kl_stats[mine], slow[mine]
        return t
    every = np.ones(len(spec), dtype=bool)
    whole = table(every, {"trials": 5, "patched": 3, "overflowed": 0, "slow": {"not_patchable": 1}, "constant": [(5, 4, 2)],
                          "rows_patched": 5, "max_rows": 2, "baseline_s": 1.0, "trials_s": 1.0})
    owner = sensitivity.shard_owner(world, count=len(spec))
    parts = []
    for r in range(world):
        mine = owner == r
        ok = [i for i in np.flatnonzero(mine) if i not in (2, 3)]
        rep = {"trials": int(mine.sum()), "patched": len(ok), "overflowed": 0, "slow": {"not_patchable": 1} if mine[3] else {},
               "constant": [(5, 4, 2)] if mine[2] else [], "rows_patched": sum(len(spec[i][1]) for i in ok),
               "max_rows": max([len(spec[i][1]) for i in ok], default=0), "baseline_s": 1.0, "trials_s": 0.5 + r,
               "shard": [r, world]}
        t = table(mine, rep)
        t.owned = mine
        parts.append(t)
    return whole, parts


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_merge_semilayers(world):
    from smpq import sensitivity
    whole, parts = _sem_tables(world)
    got = sensitivity.merge_semilayers(parts)
    assert got.owned is None and got.channels == whole.channels and got.bits == whole.bits
    assert np.array_equal(got.lnum, whole.lnum) and np.array_equal(got.param, whole.param)
    for k in ("loss", "acc", "kl", "stats", "kl_stats"):
        assert np.array_equal(getattr(got, k), getattr(whole, k), equal_nan=True), k
    assert np.array_equal(got.slow, whole.slow)
    assert got.base_loss == BASE and got.eval_loss == EVAL
    rep, want = got.report(), whole.report()
    for k in ("trials", "patched", "overflowed", "slow", "constant", "rows_patched", "max_rows"):
        assert rep[k] == want[k], k
    assert rep["world"] == world and len(rep["ranks"]) == world and rep["trials_s"] == 0.5 + world - 1
    if world > 1:
        parts[1].owned = parts[1].owned.copy()
        parts[1].owned[0] = True
        with pytest.raises(ValueError, match="semilayer 0 is owned by part 0 and part 1"):
            sensitivity.merge_semilayers(parts)
        _, parts = _sem_tables(world)
        parts[1].bits[2] = [2, 2, 4]
        with pytest.raises(ValueError, match="semilayer 2 of part 1"):
            sensitivity.merge_semilayers(parts)


# ---- the failure protocol: two live gloo ranks on the CPU ------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, failing, q, claim=None):
    """One rank: dp.sharded_delta_loss_table with sensitivity.delta_loss_table replaced by a function
    that returns this rank's hand-made part, or raises on the ranks in ``failing``. ``claim``:
    {rank: the rank argument it passes instead of its own}."""
    import sys
    for p in (PKG_DIR, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=GROUP_TIMEOUT_S))
    try:
        from smpq import dp, sensitivity
        calls = []

        def fake(net, batches, shard=None, **kw):
            calls.append((shard, kw))
            if shard[0] in failing:
                raise ZeroDivisionError("injected on rank %d" % shard[0])
            return _parts(shard[1])[shard[0]]
        sensitivity.delta_loss_table = fake
        t0 = time.monotonic()
        try:
            table = dp.sharded_delta_loss_table(None, [], (claim or {}).get(rank, rank), world, bits=BITS)
            res = ("table", {b: table.delta[b].tolist() for b in BITS}, table.report()["world"], table.owned is None)
        except RuntimeError as e:
            res = ("RuntimeError", str(e))
        q.put((rank, res, calls == [((rank, world), {"bits": BITS})], time.monotonic() - t0))
    finally:
        dist.destroy_process_group()


def _run_ranks(failing, claim=None):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank, args=(r, world, port, failing, q, claim)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict((r, rest) for r, *rest in (q.get(timeout=2 * GROUP_TIMEOUT_S) for _ in range(world)))
        for p in procs:
            p.join(timeout=GROUP_TIMEOUT_S)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return res


def test_wrapper_returns_the_merged_table_on_every_rank():
    res = _run_ranks(())
    whole = _whole()
    for r in (0, 1):
        (kind, delta, world, complete), called_once, _ = res[r]
        assert kind == "table" and world == 2 and complete and called_once
        for b in BITS:
            assert np.array_equal(np.asarray(delta[b]), whole.delta[b], equal_nan=True)


@pytest.mark.parametrize("failing", [(0,), (1,), (0, 1)])
def test_one_rank_raises_and_every_rank_raises_naming_it(failing):
    res = _run_ranks(failing)
    for r in (0, 1):
        (kind, text), called_once, seconds = res[r]
        assert kind == "RuntimeError" and called_once
        for f in (0, 1):
            named = "rank %d (ZeroDivisionError: injected on rank %d)" % (f, f) in text
            assert named == (f in failing), text
        assert seconds < GROUP_TIMEOUT_S  # nothing waited for the group's time limit


def test_a_wrong_rank_argument_fails_every_rank_and_none_waits():
    """Rank 1 calls as rank 0: its mistake goes through the gather, rank 0 (whose sweep ran) raises too."""
    res = _run_ranks((), claim={1: 0})
    for r in (0, 1):
        (kind, text), called_once, seconds = res[r]
        assert kind == "RuntimeError" and called_once == (r == 0)
        assert "rank 1 (ValueError: called as rank 0, but it is rank 1 of the group)" in text and "rank 0 (" not in text
        assert seconds < GROUP_TIMEOUT_S


def test_world_1_needs_no_process_group(monkeypatch):
    from smpq import dp, sensitivity
    monkeypatch.setattr(sensitivity, "delta_loss_table", lambda net, batches, shard=None, **kw: _parts(shard[1])[shard[0]])
    table = dp.sharded_delta_loss_table(None, [], 0, 1, bits=BITS)
    assert table.owned is None and table.report()["world"] == 1
    for b in BITS:
        assert np.array_equal(table.delta[b], _whole().delta[b], equal_nan=True)

    def boom(net, batches, shard=None, **kw):
        raise ZeroDivisionError("injected")
    monkeypatch.setattr(sensitivity, "delta_loss_table", boom)
    with pytest.raises(RuntimeError, match=r"rank 0 \(ZeroDivisionError: injected\)"):
        dp.sharded_delta_loss_table(None, [], 0, 1)


def test_wrapper_argument_errors():
    """Refused before any work or collective: a ResidentSet with an image shard, a missing group."""
    from smpq import dp
    from smpq.batches import ResidentSet
    with pytest.raises(ValueError, match="whole set"):
        dp.sharded_delta_loss_table(None, ResidentSet([], shard=(0, 2)), 0, 2)
    with pytest.raises(ValueError, match="process group"):
        dp.sharded_delta_loss_table(None, [], 0, 2)
    with pytest.raises(ValueError):
        dp.sharded_semilayer_table(None, [], [], 2, 2)


# ---- the command line ---------------------------------------------------------------------------------
def test_cli_arguments(capsys):
    from smpq import sharded_table
    base = ["--arch", "resnet18", "--weights", "m.smpq", "--out", "t.csv"]
    a = sharded_table.parse(base + ["--gpus", "4"])
    assert a.devices == [0, 1, 2, 3] and a.bits == [8, 6, 4] and a.lnums is None and a.rank is None
    assert not a.suffix and not a.rows and a.suffix_gb is None and a.report is None
    a = sharded_table.parse(base + ["--gpus", "2", "--devices", "0,0", "--bits", "8,2", "--lnums", "1,13", "--suffix",
                                    "--rows", "--suffix-gb", "1.5", "--report", "r.json", "--timeout", "30"])
    assert a.devices == [0, 0] and a.bits == [8, 2] and a.lnums == [1, 13] and a.suffix and a.rows
    assert a.suffix_gb == 1.5 and a.report == "r.json" and a.timeout == 30.0
    assert sharded_table.parse(base + ["--gpus", "16"]).devices == list(range(16))
    for bad in (base + ["--gpus", "17"], base + ["--gpus", "0"], base + ["--gpus", "2", "--devices", "0"],
                base + ["--gpus", "2", "--devices", "0,1,2"], base + ["--gpus", "2", "--devices", "0,-1"],
                base + ["--gpus", "2", "--devices", "a,b"], base + ["--gpus", "2", "--pretrained"],
                ["--arch", "resnet18", "--out", "t.csv", "--gpus", "2"], base + ["--gpus", "2", "--rank", "0"],
                ["--arch", "vgg", "--pretrained", "--out", "t.csv", "--gpus", "2"]):
        with pytest.raises(SystemExit) as e:
            sharded_table.parse(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()


class _Proc:
    """A child as supervise sees it: exits with ``code`` at poll number ``at`` (never: None)."""

    def __init__(self, code, at):
        self.code, self.at, self.polls, self.killed, self.returncode = code, at, 0, False, None

    def poll(self):
        self.polls += 1
        if self.returncode is None and self.at is not None and self.polls >= self.at:
            self.returncode = self.code
        return self.returncode

    def kill(self):
        self.killed, self.returncode = True, -9

    def wait(self):
        return self.returncode


def test_cli_supervision_kills_the_survivors_and_restarts_nothing():
    from smpq import sharded_table
    now = [0.0]

    def sleep(s):
        now[0] += s
    procs = [_Proc(0, 2), _Proc(0, 3)]
    assert sharded_table.supervise(procs, 10, clock=lambda: now[0], sleep=sleep) == 0 and not any(p.killed for p in procs)
    procs = [_Proc(3, 2), _Proc(0, None), _Proc(0, 1)]
    assert sharded_table.supervise(procs, 10, clock=lambda: now[0], sleep=sleep) == 3
    assert [p.killed for p in procs] == [False, True, False]
    procs = [_Proc(0, 1), _Proc(0, None)]
    assert sharded_table.supervise(procs, 1, clock=lambda: now[0], sleep=sleep) == 124
    assert [p.killed for p in procs] == [False, True]
