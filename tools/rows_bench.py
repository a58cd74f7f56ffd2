#!/usr/bin/env python3
"""What one delta-loss trial of a block's LAST conv costs on the rows route
(smpq.sensitivity.delta_loss_table(..., suffix=True, rows=True): the patched output channel alone is
recomputed into the kept input of the next block and the forward resumes there) and on
the suffix route (suffix=True, rows=False: the whole block again, then the rest; the parent's
behaviour and the baseline).

    python tools/rows_bench.py [--batches 4] [--batch 256] [--out profiles/trial_rows.json]

Workload: tools/suffix_bench.py's. ResNet-50 and ResNet-18, seeded pristine weights with the
r50_mixed_cal / r18_u8_cal BatchNorm statistics, --batches batches of --batch synthetic on-grid
images on the device, graphs on, 3 limbs; 8 channels at 8 and 4 bits of the last convs lnum 24, 27,
39, 42, 45 (ResNet-50: layer3.0, 3.1, 3.5, layer4.0, 4.1) and 10, 12, 14 (ResNet-18: layer3.0, 3.1,
layer4.0), each in a block of its own; a conv whose block is not eligible is reported and left out
of the decision. Both routes in one run, alternating; --warmups untimed repetitions, then --reps
timed ones; host wall time, a device synchronise on both sides of a table, the time of each conv's 16
trials taken at the table's progress callback (which follows that conv's host read). A per-trial
figure leaves out what its block pays once per table (the prefix pass and the self-checks), which is
reported beside it. The tool asserts that the two routes' statistics are equal bit for bit.

Time limits: the measurement runs in a child process which the parent ends after --timeout seconds;
in the child a watchdog ends the process when one repetition takes longer than --rep-timeout seconds.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)

LNUMS = {"resnet50": (24, 27, 39, 42, 45), "resnet18": (10, 12, 14)}
BN = {"resnet50": "r50_mixed_cal", "resnet18": "r18_u8_cal"}
BITS = (8, 4)
ZERO = {"calibrations": 0, "graph_captures": 0, "repack": 0}


def build_net(arch, dev):
    import numpy as np
    import torch

    import resnet
    torch.manual_seed(0)
    net = getattr(resnet, arch)()
    g = np.load(os.path.join(REPO, "tests", "golden", "model_goldens.npz"), allow_pickle=False)
    sd = net.state_dict()
    head = BN[arch] + "/bn/"
    for k in g.files:
        if k.startswith(head):
            sd[k[len(head):]].copy_(torch.from_numpy(g[k]))
    return net.to(dev).eval()


def one_table(net, batches, lnums, channels, rows):
    """One table of the trials: (wall seconds, table, {lnum: seconds of that conv's 16 trials})."""
    import torch
    from smpq import sensitivity
    marks = []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    table = sensitivity.delta_loss_table(net, batches, bits=BITS, lnums=lnums, channels=channels, suffix=True, rows=rows,
                                         progress=lambda done, counts: marks.append(time.perf_counter()))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    rep = table.report()
    assert rep["patched"] == 16 * len(lnums) and not rep["slow"] and not rep["constant"], rep
    assert rep["during_trials"] == ZERO, rep
    assert len(marks) == len(lnums)
    starts = [t1 - rep["trials_s"]] + marks[:-1]  # (the trials' phase ends where the table returns)
    return t1 - t0, table, {ln: m - s for ln, s, m in zip(lnums, starts, marks)}


def measure(arch, args, dev):
    import numpy as np
    import torch
    from suffix_bench import Watchdog, summary
    from smpq import assignments, ops, prefix, suffix
    net = build_net(arch, dev)
    names = prefix.block_names(net)
    lut = ops.u8lut_table()
    g = torch.Generator().manual_seed(2024)
    batches = [(ops.u8lut_decode(torch.randint(0, 256, (args.batch, 3, 224, 224), generator=g, dtype=torch.uint8), lut).to(dev),
                torch.randint(0, 1000, (args.batch,), generator=g).to(dev)) for _ in range(args.batches)]
    lnums = LNUMS[arch]
    channels, block = {}, {}
    for ln in lnums:
        conv = assignments.conv_for_lnum(net, ln)
        channels[ln] = list(range(0, conv.out_channels, conv.out_channels // 8))[:8]
        block[ln] = suffix.block_of(net, conv)
        assert conv is suffix.last_conv(net, block[ln])[0]
    assert len(set(block.values())) == len(lnums)  # one conv per block: every conv's time holds its block's fill
    per_conv = len(BITS) * 8
    t_sfx = {ln: [] for ln in lnums}
    t_rows = {ln: [] for ln in lnums}
    once = {ln: {k: [] for k in ("prefix_pass_s", "self_check_s", "rows_self_check_s")} for ln in lnums}
    once_sfx = {ln: {k: [] for k in ("prefix_pass_s", "self_check_s")} for ln in lnums}
    calls = {"suffix": [], "rows": []}
    rows_r = None
    for rep in range(args.warmups + args.reps):
        with Watchdog(args.rep_timeout):
            dt_s, tab_s, conv_s = one_table(net, batches, lnums, channels, False)
            dt_r, tab_r, conv_r = one_table(net, batches, lnums, channels, True)
        for bit in BITS:  # the two routes compute the same thing
            assert np.array_equal(tab_s.stats[bit].view(np.uint64), tab_r.stats[bit].view(np.uint64)), (rep, bit)
        assert tab_s.base_loss == tab_r.base_loss
        rows_s = {b["block"]: b for b in tab_s.report()["suffix"]["blocks"]}
        rows_r = {b["block"]: b for b in tab_r.report()["suffix"]["blocks"]}
        fixed = ("prefix_pass_s", "self_check_s", "rows_self_check_s")
        cur = {ln: ((conv_s[ln] - sum(rows_s[block[ln]][k] for k in fixed)) / per_conv,
                    (conv_r[ln] - sum(rows_r[block[ln]][k] for k in fixed)) / per_conv) for ln in lnums}
        if rep >= args.warmups:
            calls["suffix"].append(dt_s)
            calls["rows"].append(dt_r)
            for ln in lnums:
                t_sfx[ln].append(cur[ln][0])
                t_rows[ln].append(cur[ln][1])
                for k in once[ln]:
                    once[ln][k].append(rows_r[block[ln]][k])
                for k in once_sfx[ln]:
                    once_sfx[ln][k].append(rows_s[block[ln]][k])
        print("%s rep %d: suffix %.3f s, rows %.3f s; per trial (ms) %s" % (
            arch, rep, dt_s, dt_r, ", ".join("lnum %d: %.2f / %.2f" % (ln, 1e3 * cur[ln][0], 1e3 * cur[ln][1])
                                             for ln in lnums)), flush=True)
    per_lnum, decisive = {}, []
    for ln in lnums:
        b = rows_r[block[ln]]
        s, r = summary(t_sfx[ln]), summary(t_rows[ln])
        spread = max(s["max_s"] - s["min_s"], r["max_s"] - r["min_s"])
        used = b["rows"] == "used" and b["rows_trials"] == per_conv
        win = bool(used and s["median_s"] - r["median_s"] > spread)
        if used:
            decisive.append(win)
        per_lnum[str(ln)] = {
            "block": block[ln], "name": names[block[ln]], "rows": b["rows"], "rows_trials": b["rows_trials"],
            "suffix_per_trial": s, "rows_per_trial": r, "rows_over_suffix": round(r["median_s"] / s["median_s"], 4),
            "saved_per_trial_s": round(s["median_s"] - r["median_s"], 6), "spread_s": round(spread, 6), "rows_wins": win,
            "once_per_block_rows_route": {k: summary(v) for k, v in once[ln].items()},
            "once_per_block_suffix_route": {k: summary(v) for k, v in once_sfx[ln].items()},
            "kept_bytes": b["bytes"], "of_which_rows_bytes": b["rows_bytes"]}
    return {"workload": {"arch": arch, "bn": BN[arch], "batches": args.batches, "batch": args.batch,
                         "trials": per_conv * len(lnums), "lnums": list(lnums),
                         "channels": {str(k): v for k, v in channels.items()}, "bits": list(BITS),
                         "slices_per_batch": len(suffix.slices(args.batch))},
            "table_call": {"suffix": summary(calls["suffix"]), "rows": summary(calls["rows"])},
            "per_lnum": per_lnum}, decisive


def worker(args):
    import torch

    import __graft_entry__
    __graft_entry__.build()
    if not torch.cuda.is_available():
        sys.exit("rows_bench: needs a GPU (nothing is measured without one)")
    from smpq import engine, ops, suffix
    dev = torch.device("cuda:0")
    engine.set_range_mode("static")
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)
    archs, decisive = {}, []
    for arch in args.archs.split(","):
        archs[arch], d = measure(arch, args, dev)
        decisive += d
        torch.cuda.empty_cache()
    default_on = bool(decisive) and all(decisive)
    doc = {
        "tool": "tools/rows_bench.py", "device": torch.cuda.get_device_name(0),
        "settings": {"graphs": bool(engine.USE_GRAPH[0]), "act_limbs": ops.get_act_limbs(), "streams": engine.STREAMS[0],
                     "min_skipped": suffix.MIN_SKIPPED[0]},
        "protocol": {"warmups": args.warmups, "reps": args.reps,
                     "clock": "host perf_counter; a device synchronise on both sides of a table, a conv's 16 trials end at "
                              "its host read; both routes in one run, alternating",
                     "per_trial": "a conv's time, without its block's prefix pass and self-checks (listed beside it), over "
                                  "its 16 trials",
                     "wins": "suffix median - rows median > the larger of the two routes' max - min over the reps",
                     "statistics_bitwise_equal": True},
        "archs": archs,
        "decision": {"rule": "SMPQ_TRIAL_ROWS defaults to on under the suffix only if the rows route wins for every "
                             "measured block that used it", "every_measured_block_wins": default_on,
                     "shipped_default": bool(suffix.TRIAL_ROWS[0])},
        "not_measured": "a whole table, real data, other batch sizes, 2 limbs, graphs off, ResNet-34, BasicBlock nets "
                        "beyond ResNet-18",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"every_measured_block_wins": default_on, "out": args.out,
                      "rows_over_suffix": {a: {k: v["rows_over_suffix"] for k, v in d["per_lnum"].items()}
                                           for a, d in archs.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=1)
    ap.add_argument("--archs", default="resnet50,resnet18")
    ap.add_argument("--timeout", type=int, default=540, help="seconds for the whole run")
    ap.add_argument("--rep-timeout", type=int, default=90, help="seconds for one repetition (both routes)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trial_rows.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the measurement in a fresh child under the whole run's limit (this process never opens the GPU)
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:], timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        sys.exit("rows_bench: the run exceeded %d s and was ended" % args.timeout)
    sys.exit(rc)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
