"""Sensitivity tables with their trials shared among live processes: the ranks of a
gloo group on cuda:0 (tests/table_shard_worker.py) each run their share of the trials of
dp.sharded_delta_loss_table / dp.sharded_semilayer_table, gather once, and the merged table every
rank gets back must be the table this process computes alone, bit for bit: deltas and trial
statistics, baseline losses, counters. Also the command line, python -m smpq.sharded_table, whose
CSV must be byte for byte the single-process table's."""
import importlib
import json
import os
import pickle
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = os.path.join(os.path.dirname(HERE), "semilayer-wise-mixed-precision-quantization_amd")
ZERO = {"calibrations": 0, "graph_captures": 0, "repack": 0}


@pytest.fixture
def knobs():
    """Range mode, graph switch and limb count as they were, whatever a test sets."""
    from smpq import engine, ops
    saved = engine.get_range_mode(), engine.USE_GRAPH[0], ops.get_act_limbs()
    yield
    engine.set_range_mode(saved[0])
    engine.USE_GRAPH[0] = saved[1]
    ops.set_act_limbs(saved[2])


def _worker_module():
    if HERE not in sys.path:
        sys.path.insert(0, HERE)
    import table_shard_worker
    return importlib.reload(table_shard_worker)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _wait_all(procs, seconds):
    """Return codes of ``procs``, every wait under a time limit; whatever still runs is killed."""
    try:
        return [p.wait(timeout=seconds) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()


def _run_ranks(case, world, tmp_path):
    """Start the case's ranks and return the merged table each of them saved."""
    port = _free_port()
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "table_shard_worker.py"), str(r), str(world), str(port),
                               str(tmp_path), case], env=env) for r in range(world)]
    rcs = _wait_all(procs, 300)
    assert rcs == [0] * world, rcs
    tables = []
    for r in range(world):
        with open(os.path.join(tmp_path, "%s_rank%d.pkl" % (case, r)), "rb") as f:
            tables.append(pickle.load(f))
    return tables


def _same_delta_tables(a, b):
    assert a.arch == b.arch and a.bits == b.bits and a.owned is None and b.owned is None
    assert np.array_equal(a.lnum, b.lnum) and np.array_equal(a.cnum, b.cnum)
    for bit in a.bits:
        assert np.array_equal(a.delta[bit], b.delta[bit], equal_nan=True), bit
        assert np.array_equal(a.stats[bit], b.stats[bit], equal_nan=True), bit
    assert a.base_loss == b.base_loss and a.eval_loss == b.eval_loss


def _check_counters(merged, alone, world, extra=()):
    rep, want = merged.report(), alone.report()
    for k in ("trials", "patched", "overflowed", "slow") + tuple(extra):
        assert rep[k] == want[k], (k, rep[k], want[k])
    assert rep["constant"] == sorted(tuple(c) for c in want["constant"])
    assert rep["world"] == world and [r["shard"] for r in rep["ranks"]] == [[r, world] for r in range(world)]
    assert sum(r["trials"] for r in rep["ranks"]) == want["trials"]
    for r in rep["ranks"]:
        if not r["slow"]:  # a rank that ran no slow trial: nothing but patch, forward, restore
            assert r["during_trials"] == ZERO, r
    return rep


def _delta_case(gpu, tmp_path, case):
    w = _worker_module()
    w.knobs()
    world = w.CASES[case]["world"]
    alone = w.single(case, w.model(gpu), w.batches(gpu))
    tables = _run_ranks(case, world, tmp_path)
    for t in tables:  # every rank returns the same merged table, and it is the single-process one
        _same_delta_tables(t, alone)
        assert json.dumps(t.report()["constant"]) == json.dumps(tables[0].report()["constant"])
        assert [t.report()[k] for k in ("trials", "patched", "overflowed", "slow", "world")] == \
            [tables[0].report()[k] for k in ("trials", "patched", "overflowed", "slow", "world")]
    return w, alone, _check_counters(tables[0], alone, world)


def test_world2_delta_loss_table_is_the_single_process_table(gpu, knobs, tmp_path):
    """Patched trials of a layer-1 conv and of layer4.0's two convs, slow trials of the fully
    quantized conv 3, a constant channel: 5 channels per conv at 8 and 2 bits over two ranks."""
    w, alone, rep = _delta_case(gpu, tmp_path, "delta_w2")
    want = alone.report()
    assert want["trials"] == 40 and want["slow"] == {"not_patchable": 10} and want["patched"] == 28
    assert sorted(want["constant"]) == [(13, 100, 2), (13, 100, 8)]
    cols = {(int(l), int(c)): i for i, (l, c) in enumerate(zip(alone.lnum, alone.cnum))}
    for bit in w.BITS:
        assert np.isnan(alone.delta[bit][cols[w.CONSTANT]])
        assert np.isfinite(np.delete(alone.delta[bit], cols[w.CONSTANT])).all()
        slow = [cols[(3, c)] for c in w.CHANNELS[3]]
        assert np.isnan(alone.stats[bit][slow]).all() and np.isfinite(alone.delta[bit][slow]).all()
    assert [r["trials"] for r in rep["ranks"]] == [24, 16]  # 3 and 2 of every conv's 5 channels
    assert [r["slow"] for r in rep["ranks"]] == [{"not_patchable": 6}, {"not_patchable": 4}]


def test_world2_with_suffix_and_rows(gpu, knobs, tmp_path):
    """The same over layer4.0's convs with the suffix and rows routes on: every rank pays its own
    prefix pass and self-checks, and they pass."""
    w, alone, rep = _delta_case(gpu, tmp_path, "suffix_w2")
    assert alone.report()["trials"] == 20 and alone.report()["patched"] == 18 and not alone.report()["slow"]
    for r in rep["ranks"] + [alone.report()]:
        blocks = r["suffix"]["blocks"]
        assert [b["name"] for b in blocks] == ["layer4.0"], blocks
        b = blocks[0]
        assert b["used"] and b["kept"] == 2 and b["self_check"] is True, b
        assert b["rows"] == "used" and b["rows_self_check"] is True, b
        assert r["during_trials"] == ZERO
    # conv 14 is the block's last: its owned trials took the rows route (3 / 2 channels x 2 bits)
    assert [r["suffix"]["blocks"][0]["rows_trials"] for r in rep["ranks"]] == [6, 4]


def test_world3_with_a_rank_that_owns_nothing(gpu, knobs, tmp_path):
    w, alone, rep = _delta_case(gpu, tmp_path, "delta_w3")
    assert alone.report()["trials"] == 16
    assert [r["trials"] for r in rep["ranks"]] == [8, 8, 0]
    idle = rep["ranks"][2]
    assert idle["patched"] == 0 and not idle["slow"] and not idle["constant"] and idle["during_trials"] == ZERO
    assert idle["baseline"]["calibrations"] == 1  # it still paid the baseline


def test_world2_semilayer_table(gpu, knobs, tmp_path):
    w = _worker_module()
    w.knobs()
    alone = w.single("semi_w2", w.model(gpu), w.batches(gpu))
    tables = _run_ranks("semi_w2", 2, tmp_path)
    for t in tables:
        assert t.owned is None and t.channels == alone.channels and t.bits == alone.bits
        assert np.array_equal(t.lnum, alone.lnum) and np.array_equal(t.param, alone.param)
        for k in ("loss", "acc", "kl", "stats", "kl_stats"):
            assert np.array_equal(getattr(t, k), getattr(alone, k), equal_nan=True), k
        assert np.array_equal(t.slow, alone.slow)
        assert t.base_loss == alone.base_loss and t.eval_loss == alone.eval_loss
    assert alone.report()["patched"] == 4 and np.isfinite(alone.kl).all()
    rep = _check_counters(tables[0], alone, 2, extra=("rows_patched", "max_rows"))
    assert [r["trials"] for r in rep["ranks"]] == [2, 2]


def test_command_line_csv_is_the_single_process_csv(gpu, knobs, tmp_path, monkeypatch):
    from smpq import checkpoint, sensitivity
    from smpq.batches import ResidentSet
    w = _worker_module()
    w.knobs()
    weights = str(tmp_path / "model.smpq")
    checkpoint.save_packed(w.model(gpu), weights)
    out, report = str(tmp_path / "table.csv"), str(tmp_path / "report.json")
    # the command line leaves graphs and limbs to the environment: name what w.knobs() sets here
    env = dict(os.environ, PYTHONUNBUFFERED="1", SMPQ_SYNTHETIC="1", SMPQ_SYNTH_IMAGES="16", SMPQ_BATCH="8",
               SMPQ_GRAPH="1", SMPQ_ACT_LIMBS="3",
               PYTHONPATH=os.pathsep.join([PKG_DIR] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else [])))
    for k in ("SMPQ_RESIDENT_VAL", "SMPQ_TRIAL_SUFFIX", "SMPQ_TRIAL_ROWS"):
        env.pop(k, None)
    cli = subprocess.Popen([sys.executable, "-m", "smpq.sharded_table", "--arch", "resnet18", "--weights", weights,
                            "--gpus", "2", "--devices", "0,0", "--bits", "8,2", "--lnums", "1,2", "--out", out,
                            "--report", report, "--timeout", "240"], env=env, cwd=str(tmp_path))
    # meanwhile, the same table in this process: the same file, the same loader
    import resnet
    monkeypatch.setenv("SMPQ_SYNTHETIC", "1")
    import imagenet
    net = resnet.resnet18().to(gpu).eval()
    checkpoint.load_packed(net, weights)
    try:
        alone = sensitivity.delta_loss_table(net, ResidentSet(imagenet.SyntheticImageNet(16, 8), device=gpu), bits=(8, 2),
                                             lnums=[1, 2])
    finally:
        rcs = _wait_all([cli], 300)
    assert rcs == [0], rcs
    want = str(tmp_path / "alone.csv")
    sensitivity.write_csv(alone, want)
    with open(out, "rb") as f, open(want, "rb") as g:
        assert f.read() == g.read()
    with open(report) as f:
        rep = json.load(f)
    assert rep["world"] == 2 and rep["trials"] == alone.report()["trials"] == 256
    assert rep["patched"] == alone.report()["patched"] == 256 and [r["trials"] for r in rep["ranks"]] == [128, 128]
