#!/usr/bin/env python3
"""What one delta-loss trial costs when it forwards only the blocks from the patched conv on
(smpq.sensitivity.delta_loss_table(..., suffix=True): eager, from block inputs kept by one prefix
pass per block) and when it replays the full-batch graphs (suffix=False, the parent's
behaviour and the baseline).

    python tools/suffix_bench.py [--batches 4] [--batch 256] [--out profiles/trial_suffix.json]

Workload: tools/delta_loss_bench.py's. ResNet-50, seeded pristine weights with the r50_mixed_cal
BatchNorm statistics, --batches batches of --batch synthetic on-grid images on the device, graphs
on, 3 limbs; the same 64 trials: 8 channels of each of lnum 1, 24, 40 and 48 (blocks 0, 7, 13 and
15 of 16) at 8 and 4 bits. Every block is resumed in the suffix route (smpq.suffix.MIN_SKIPPED = 0
for the measurement), so that the cut can be chosen from the figures. Both routes in one run,
alternating; --warmups untimed repetitions, then --reps timed ones; host wall time, a device
synchronise on both sides of a table, the time of each conv's 16 trials taken at the table's
progress callback (which follows that conv's host read). The suffix route's figure per trial leaves
out its block's prefix pass and self-check, which are paid once per block and table and reported
beside it. The tool asserts that the two routes' statistics are equal bit for bit.

Time limits: the measurement runs in a child process which the parent ends after --timeout
seconds; in the child a watchdog ends the process when one repetition takes longer than
--rep-timeout seconds.
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)

LNUMS = (1, 24, 40, 48)
BITS = (8, 4)


def summary(xs):
    import numpy as np
    xs = [float(x) for x in xs]
    return {"reps_s": [round(x, 6) for x in xs], "median_s": round(float(np.median(xs)), 6),
            "min_s": round(min(xs), 6), "max_s": round(max(xs), 6)}


class Watchdog:
    """Ends the process (status 124) when a repetition outlives its limit, a hung device call included."""

    def __init__(self, seconds):
        self.seconds, self.timer = seconds, None

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, lambda: (print("suffix_bench: a repetition exceeded %d s" % self.seconds,
                                                                  file=sys.stderr, flush=True), os._exit(124)))
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()


def one_table(net, batches, channels, use_suffix):
    """One table of the 64 trials: (wall seconds, table, {lnum: seconds of that conv's 16 trials})."""
    import torch
    from smpq import sensitivity
    marks = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = sensitivity.delta_loss_table(net, batches, bits=BITS, lnums=LNUMS, channels=channels,
                                         progress=lambda done, counts: marks.append(time.perf_counter()), suffix=use_suffix)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    rep = table.report()
    assert rep["patched"] == 64 and not rep["slow"] and not rep["constant"], rep
    assert rep["during_trials"] == {"calibrations": 0, "graph_captures": 0, "repack": 0}, rep
    assert len(marks) == len(LNUMS)
    starts = [t1 - rep["trials_s"]] + marks[:-1]  # (the trials' phase ends where the table returns)
    return t1 - t0, table, {ln: m - s for ln, s, m in zip(LNUMS, starts, marks)}


def worker(args):
    import numpy as np
    import torch

    import __graft_entry__
    __graft_entry__.build()
    if not torch.cuda.is_available():
        sys.exit("suffix_bench: needs a GPU (nothing is measured without one)")
    from delta_loss_bench import build_net
    from smpq import assignments, engine, ops, prefix, suffix
    dev = torch.device("cuda:0")
    engine.set_range_mode("static")
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)
    shipped_cut = suffix.MIN_SKIPPED[0]
    suffix.MIN_SKIPPED[0] = 0.0  # resume every block: the measurement decides the cut
    net = build_net(dev)
    names = prefix.block_names(net)
    lut = ops.u8lut_table()
    g = torch.Generator().manual_seed(2024)
    batches = [(ops.u8lut_decode(torch.randint(0, 256, (args.batch, 3, 224, 224), generator=g, dtype=torch.uint8), lut).to(dev),
                torch.randint(0, 1000, (args.batch,), generator=g).to(dev)) for _ in range(args.batches)]
    channels, block = {}, {}
    for ln in LNUMS:
        conv = assignments.conv_for_lnum(net, ln)
        channels[ln] = list(range(0, conv.out_channels, conv.out_channels // 8))[:8]
        block[ln] = suffix.block_of(net, conv)
    per_conv = len(BITS) * 8

    replay = {ln: [] for ln in LNUMS}
    resumed = {ln: [] for ln in LNUMS}
    prefix_s = {ln: [] for ln in LNUMS}
    check_s = {ln: [] for ln in LNUMS}
    calls = {"replay": [], "suffix": []}
    last = None
    for rep in range(args.warmups + args.reps):
        with Watchdog(args.rep_timeout):
            dt_r, t_r, conv_r = one_table(net, batches, channels, False)
            dt_s, t_s, conv_s = one_table(net, batches, channels, True)
        for bit in BITS:  # the two routes compute the same thing
            assert np.array_equal(t_r.stats[bit].view(np.uint64), t_s.stats[bit].view(np.uint64)), (rep, bit)
        assert t_r.base_loss == t_s.base_loss
        rows = {b["block"]: b for b in t_s.report()["suffix"]["blocks"]}
        assert all(rows[block[ln]]["kept"] == args.batches and rows[block[ln]]["self_check"] is True for ln in LNUMS), rows
        if rep >= args.warmups:
            calls["replay"].append(dt_r)
            calls["suffix"].append(dt_s)
            for ln in LNUMS:
                row = rows[block[ln]]
                replay[ln].append(conv_r[ln] / per_conv)
                resumed[ln].append((conv_s[ln] - row["prefix_pass_s"] - row["self_check_s"]) / per_conv)
                prefix_s[ln].append(row["prefix_pass_s"])
                check_s[ln].append(row["self_check_s"])
        last = t_s.report()["suffix"]
        print("rep %d: replay %.3f s, suffix %.3f s; per trial (ms) %s" % (
            rep, dt_r, dt_s, ", ".join("lnum %d: %.2f / %.2f" % (ln, 1e3 * conv_r[ln] / per_conv,
                                                                 1e3 * (conv_s[ln] - rows[block[ln]]["prefix_pass_s"]
                                                                        - rows[block[ln]]["self_check_s"]) / per_conv)
                                       for ln in LNUMS)), flush=True)

    # conv launches of one resumed batch per block, and of one full eager forward for scale
    from smpq import stats
    cal = engine.model_state(net).ranges
    launches = {}
    with torch.no_grad():
        c = stats["hip_conv"]
        engine._static_eager(net, batches[0][0], cal)
        full = stats["hip_conv"] - c
        for ln in LNUMS:
            kept = suffix.fill(net, batches[0][0], cal, block[ln])
            c = stats["hip_conv"]
            suffix.resume(net, kept, cal, block[ln])
            launches[ln] = stats["hip_conv"] - c
            del kept
    torch.cuda.synchronize()

    per_lnum, wins = {}, []
    for ln in LNUMS:
        r, s = summary(replay[ln]), summary(resumed[ln])
        spread = max(r["max_s"] - r["min_s"], s["max_s"] - s["min_s"])
        win = r["median_s"] - s["median_s"] > spread
        if win:
            wins.append(block[ln])
        per_lnum[str(ln)] = {
            "block": block[ln], "name": names[block[ln]], "blocks_skipped_share": round(block[ln] / len(names), 4),
            "replay_per_trial": r, "suffix_per_trial": s, "suffix_over_replay": round(s["median_s"] / r["median_s"], 4),
            "spread_s": round(spread, 6), "suffix_wins": bool(win),
            "prefix_pass_once_per_block": summary(prefix_s[ln]), "self_check_once_per_block": summary(check_s[ln]),
            "kept_bytes": rows[block[ln]]["bytes"],
            "conv_launches_per_resumed_batch": launches[ln], "conv_launches_per_full_batch": full}
    # the cut: the shallowest measured block from which on every measured block wins
    cut = None
    for ln in sorted(LNUMS, reverse=True):
        if not per_lnum[str(ln)]["suffix_wins"]:
            break
        cut = block[ln]
    doc = {
        "tool": "tools/suffix_bench.py", "device": torch.cuda.get_device_name(0),
        "workload": {"arch": "resnet50", "bn": "r50_mixed_cal", "batches": args.batches, "batch": args.batch, "trials": 64,
                     "lnums": list(LNUMS), "channels": {str(k): v for k, v in channels.items()}, "bits": list(BITS),
                     "graphs": bool(engine.USE_GRAPH[0]), "act_limbs": ops.get_act_limbs(), "streams": engine.STREAMS[0],
                     "slices_per_batch": len(suffix.slices(args.batch))},
        "protocol": {"warmups": args.warmups, "reps": args.reps,
                     "clock": "host perf_counter; a device synchronise on both sides of a table, a conv's 16 trials end at "
                              "its host read; both routes in one run, alternating; every block resumed (MIN_SKIPPED 0)",
                     "per_trial": "a conv's time over its 16 trials; the suffix route's without its block's prefix pass "
                                  "and self-check, which are listed beside it",
                     "wins": "replay median - suffix median > the larger of the two routes' max - min over the reps",
                     "statistics_bitwise_equal": True},
        "table_call": {"replay": summary(calls["replay"]), "suffix": summary(calls["suffix"])},
        "per_lnum": per_lnum,
        "suffix_totals_last_rep": {k: last[k] for k in ("resumed_forwards", "resumed_conv_launches")},
        "cut": {"shallowest_winning_measured_block": cut, "name": None if cut is None else names[cut],
                "share_of_blocks_skipped": None if cut is None else round(cut / len(names), 4),
                "min_skipped_shipped": shipped_cut,
                "note": "blocks between two measured ones were not measured; the shipped rule uses the suffix from the "
                        "shallowest measured winner on"},
        "not_measured": "a whole table, real data, other batch sizes, ResNet-18/34, a semilayer table",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"cut": doc["cut"]["name"], "suffix_over_replay": {k: v["suffix_over_replay"] for k, v in per_lnum.items()},
                      "out": args.out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=480, help="seconds for the whole run")
    ap.add_argument("--rep-timeout", type=int, default=90, help="seconds for one repetition (both routes)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trial_suffix.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the measurement in a fresh child under the whole run's limit (this process never opens the GPU)
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:], timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        sys.exit("suffix_bench: the run exceeded %d s and was ended" % args.timeout)
    sys.exit(rc)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
