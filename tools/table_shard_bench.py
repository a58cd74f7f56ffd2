#!/usr/bin/env python3
"""What sharding a delta-loss table's TRIALS over processes costs and gains
(smpq.dp.sharded_delta_loss_table), against the same table computed unsharded in one
process (the parent commit's behaviour and the baseline).

    python tools/table_shard_bench.py [--worlds 2,4,8] [--out profiles/table_shard.json]

Workload: tools/suffix_bench.py's model and data (ResNet-50, seeded pristine weights with the
r50_mixed_cal BatchNorm statistics, --batches batches of --batch synthetic on-grid images, graphs
on, 3 limbs, suffix on with the shipped cut) over a fixed subset of trials: 32 channels of each of
lnum 1, 24, 40 and 48 at 8 and 4 bits, 256 trials. Rank r of a run uses GPU r mod (GPUs the box
shows). On a box with ONE GPU only world 2 is run, to record the overhead: its two ranks share the
GPU, no speedup can be expected, and scaling across GPUs is then not measured.

Per configuration --warmups untimed runs, then --reps timed ones. A run is: this process (which
never opens the GPU) starts the fresh rank processes, they build model and data, compute the table
and rank 0 saves the merged table; its wall time is from just before the first process is started
to the moment rank 0 holds the merged table (time.time() on both sides: one host clock). Beside it
the maximum over ranks of the sweep's own ``trials_s`` and ``baseline_s`` (report()), which show
the part that shrinks with the world and the part every rank pays again, and the efficiency
trials_s(1) / (world * max over ranks of trials_s), from the medians. Every run's merged table is
compared with the first unsharded table bit for bit (deltas, trial statistics, base and eval
losses); a difference ends the tool.

Time limits: every run is ended after --run-timeout seconds (its processes killed, the tool exits
nonzero, nothing is retried), the whole tool stops starting runs after --timeout seconds.
"""
import argparse
import json
import os
import pickle
import socket
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

LNUMS = (1, 24, 40, 48)
BITS = (8, 4)
PER_CONV = 32


def summary(xs):
    import numpy as np
    xs = [float(x) for x in xs]
    return {"reps_s": [round(x, 6) for x in xs], "median_s": round(float(np.median(xs)), 6),
            "min_s": round(min(xs), 6), "max_s": round(max(xs), 6)}


def rank_main(args):
    """One process of a run: rank --rank of --world (world 1: the unsharded call, no process group)."""
    import torch
    from delta_loss_bench import build_net
    from smpq import assignments, dp, engine, ops, sensitivity
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    torch.set_num_threads(max(1, 16 // args.world))
    engine.set_range_mode("static")
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)
    net = build_net(dev)
    lut = ops.u8lut_table()
    g = torch.Generator().manual_seed(2024)
    batches = [(ops.u8lut_decode(torch.randint(0, 256, (args.batch, 3, 224, 224), generator=g, dtype=torch.uint8), lut).to(dev),
                torch.randint(0, 1000, (args.batch,), generator=g).to(dev)) for _ in range(args.batches)]
    channels = {}
    for ln in LNUMS:
        cout = assignments.conv_for_lnum(net, ln).out_channels
        channels[ln] = list(range(0, cout, cout // PER_CONV))[:PER_CONV]
    kw = dict(bits=BITS, lnums=LNUMS, channels=channels, suffix=True)
    if args.world == 1:
        table = sensitivity.delta_loss_table(net, batches, **kw)
        done_at = time.time()
    else:
        import datetime

        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(args.port)
        dist.init_process_group("gloo", rank=args.rank, world_size=args.world,
                                timeout=datetime.timedelta(seconds=args.run_timeout))
        try:
            table = dp.sharded_delta_loss_table(net, batches, args.rank, args.world, **kw)
            done_at = time.time()  # (before the group's teardown: the merged table is held here)
        finally:
            dist.destroy_process_group()
    if args.rank == 0:
        with open(args.result, "wb") as f:
            pickle.dump({"table": table, "done_at": done_at, "gpus": torch.cuda.device_count(),
                         "device": torch.cuda.get_device_name(dev), "streams": engine.STREAMS[0]}, f)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def one_run(args, world, gpus, tmp):
    """Start the ranks of one run, wait for them under the run's limit: (wall seconds, rank 0's result)."""
    result = os.path.join(tmp, "result.pkl")
    if os.path.exists(result):
        os.remove(result)
    port = free_port()
    cmd = [sys.executable, os.path.abspath(__file__), "--role", "rank", "--world", str(world), "--port", str(port),
           "--result", result, "--batches", str(args.batches), "--batch", str(args.batch),
           "--run-timeout", str(args.run_timeout)]
    t0 = time.time()
    procs = [subprocess.Popen(cmd + ["--rank", str(r), "--device", str(r % gpus)]) for r in range(world)]
    end = time.monotonic() + args.run_timeout
    try:
        rcs = [p.wait(timeout=max(0.1, end - time.monotonic())) for p in procs]
    except subprocess.TimeoutExpired:
        sys.exit("table_shard_bench: a world-%d run exceeded %d s and was ended" % (world, args.run_timeout))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    if any(rcs):
        sys.exit("table_shard_bench: a world-%d run's ranks exited with %r" % (world, rcs))
    with open(result, "rb") as f:
        res = pickle.load(f)
    return res["done_at"] - t0, res


def same(a, b):
    import numpy as np
    ok = a.bits == b.bits and np.array_equal(a.lnum, b.lnum) and np.array_equal(a.cnum, b.cnum)
    for bit in a.bits:
        ok = ok and np.array_equal(a.delta[bit], b.delta[bit], equal_nan=True)
        ok = ok and np.array_equal(a.stats[bit], b.stats[bit], equal_nan=True)
    return bool(ok and a.base_loss == b.base_loss and a.eval_loss == b.eval_loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=1080, help="seconds after which no further run is started")
    ap.add_argument("--run-timeout", type=int, default=240, help="seconds for one run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "table_shard.json"))
    ap.add_argument("--role", default="parent", help=argparse.SUPPRESS)
    ap.add_argument("--rank", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--world", type=int, default=1, help=argparse.SUPPRESS)
    ap.add_argument("--port", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--device", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--result", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.role == "rank":
        return rank_main(args)

    import __graft_entry__
    __graft_entry__.build()  # (host work: the ranks find the library built)
    started = time.monotonic()
    worlds = [int(w) for w in args.worlds.split(",") if w]
    if any(not 2 <= w <= 16 for w in worlds):
        sys.exit("table_shard_bench: --worlds within 2..16")
    rows, skipped = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        reference, gpus, device, streams = None, 1, None, None
        for world in [1] + worlds:
            if world > 1 and gpus == 1 and world != 2:
                skipped.append({"world": world, "why": "the box shows one GPU: only world 2 is run, for the overhead"})
                continue
            wall, trials_s, baseline_s, last = [], [], [], None
            for rep in range(args.warmups + args.reps):
                if time.monotonic() - started > args.timeout:
                    break
                dt, res = one_run(args, world, gpus, tmp)
                table = res["table"]
                if reference is None:
                    reference, gpus, device, streams = table, res["gpus"], res["device"], res["streams"]
                    r = table.report()
                    assert r["trials"] == r["patched"] == len(LNUMS) * PER_CONV * len(BITS) and not r["slow"], r
                assert same(table, reference), "world %d, run %d: the table is not the unsharded table bit for bit" % (world, rep)
                r = table.report()
                ranks = r.get("ranks", [r])
                assert len(ranks) == world and sum(k["trials"] for k in ranks) == reference.report()["trials"]
                print("world %d run %d: wall %.2f s, max trials_s %.2f, max baseline_s %.2f" % (
                    world, rep, dt, r["trials_s"], r["baseline_s"]), flush=True)
                if rep >= args.warmups:
                    wall.append(dt)
                    trials_s.append(r["trials_s"])
                    baseline_s.append(r["baseline_s"])
                    last = ranks
            if not wall:
                skipped.append({"world": world, "why": "the tool's --timeout passed before its timed runs"})
                continue
            rows[world] = {"world": world, "gpus_used": min(world, gpus), "timed_runs": len(wall),
                           "wall_spawn_to_table": summary(wall), "max_rank_trials_s": summary(trials_s),
                           "max_rank_baseline_s": summary(baseline_s),
                           "per_rank_last_run": [{"trials": k["trials"], "trials_s": round(k["trials_s"], 6),
                                                  "baseline_s": round(k["baseline_s"], 6),
                                                  "suffix_blocks": [{f: b[f] for f in ("name", "used", "kept", "self_check")} |
                                                                    {"prefix_pass_s": round(b["prefix_pass_s"], 6),
                                                                     "self_check_s": round(b["self_check_s"], 6)}
                                                                    for b in k["suffix"].get("blocks", [])]} for k in last]}
    if 1 not in rows:
        sys.exit("table_shard_bench: no timed unsharded run")
    t1 = rows[1]["max_rank_trials_s"]["median_s"]
    for world, row in rows.items():
        if world > 1:
            row["trials_efficiency"] = round(t1 / (world * row["max_rank_trials_s"]["median_s"]), 4)
            row["wall_over_unsharded"] = round(row["wall_spawn_to_table"]["median_s"] / rows[1]["wall_spawn_to_table"]["median_s"], 4)
    doc = {
        "tool": "tools/table_shard_bench.py", "device": device, "gpus_on_the_box": gpus,
        "workload": {"arch": "resnet50", "bn": "r50_mixed_cal", "batches": args.batches, "batch": args.batch,
                     "trials": len(LNUMS) * PER_CONV * len(BITS), "lnums": list(LNUMS), "channels_per_conv": PER_CONV,
                     "bits": list(BITS), "graphs": True, "act_limbs": 3, "suffix": True, "streams": streams},
        "protocol": {"warmups": args.warmups, "reps": args.reps,
                     "wall": "time.time() just before the first rank process is started to rank 0 holding the merged table: "
                             "interpreter start, imports, model, data, baseline, trials, gather and merge",
                     "trials_s / baseline_s": "the sweep's own report(), the maximum over the ranks of a run",
                     "trials_efficiency": "median trials_s(world 1) / (world * median of max-rank trials_s)",
                     "bitwise_equal_to_unsharded": True},
        "unsharded": rows[1], "sharded": [rows[w] for w in sorted(rows) if w > 1], "not_run": skipped,
        "scaling_across_gpus_measured": bool(gpus > 1 and any(w > 1 for w in rows)),
        "not_measured": "a whole table, real data, other batch sizes, ResNet-18/34, a semilayer table, more than one node"
                        + ("" if gpus > 1 else "; scaling across GPUs (the box shows one GPU: the two ranks shared it)"),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"out": args.out, "gpus": gpus, "unsharded_wall_s": rows[1]["wall_spawn_to_table"]["median_s"],
                      "sharded": {str(w): {"wall_s": rows[w]["wall_spawn_to_table"]["median_s"],
                                           "trials_efficiency": rows[w]["trials_efficiency"]} for w in rows if w > 1}}))


if __name__ == "__main__":
    main()
