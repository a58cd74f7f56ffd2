#!/usr/bin/env python3
"""What the weight-stationary 1x1 tiles with 3 weight limbs + ReLU (tile kind TILE_RESIDENT1X1_W,
SMPQ_RESIDENT_W) change for a model under search, against the parent's behaviour (the knob at 0).

    python tools/search_tiles_bench.py [--batches 4] [--batch 256] [--out profiles/search_tiles.json]

Workload: tools/delta_loss_bench.py's. ResNet-50, seeded pristine weights with the r50_mixed_cal
BatchNorm statistics, --batches batches of --batch synthetic on-grid images on the device, graphs
on, 3 limbs, the batch in 2 slices. One model per setting, both in this one run. The tile cache keeps
the two settings apart by itself (an eligible call is cached under the variant "resw" with the knob
on and under "nohalo" with it off), every other shape runs the same tile in both, and the knob is
set to a model's own value before anything is run on it. Per setting --warmups untimed repetitions,
then --reps timed ones, the settings alternating; host wall time with a device synchronise on both
sides.

  (a) per eligible conv shape at the slice batch: the autotuner's median (ops.TUNE_LOG) of the best
      kind-6 tile against the best other tile, from the tuning of the knob-on model;
  (b) the graph-replayed forward per batch (--passes passes over the batches per repetition);
  (c) the 64-trial delta_loss_table call through the replay (8 channels of each of lnum 1, 24, 40 and
      48 at 8 and 4 bits); the two settings' tables are asserted equal bit for bit.

The default of SMPQ_RESIDENT_W follows (b): 1 only if the median with the kind is below the median
without it by more than the spread of the repetitions (the larger max - min of the two settings).

Time limits: the measurement runs in a child process which the parent ends after --timeout seconds.
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

LNUMS = (1, 24, 40, 48)
BITS = (8, 4)


def summary(xs):
    import numpy as np
    xs = [float(x) for x in xs]
    return {"reps_s": [round(x, 6) for x in xs], "median_s": round(float(np.median(xs)), 6),
            "min_s": round(min(xs), 6), "max_s": round(max(xs), 6)}


def timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def tune_rows(ops):
    """(a): per eligible call key (variant "resw"), the best kind-6 median and the best other one."""
    rows = []
    for key, log in sorted(ops.TUNE_LOG.items()):
        if not key.endswith("|resw"):
            continue
        w = {c: t for c, t in log.items() if ops.tile_kind(c) == ops.TILE_RESIDENT1X1_W}
        o = {c: t for c, t in log.items() if ops.tile_kind(c) != ops.TILE_RESIDENT1X1_W}
        if not w or not o:
            continue
        f = key.split("|")
        bw, bo = min(w, key=w.get), min(o, key=o.get)
        rows.append({"key": key, "n": int(f[0]), "hw": int(f[1]), "cin": int(f[3]), "cout": int(f[4]),
                     "residual_q": bool(int(f[14])), "best_kind6": {"cfg": bw, "us": w[bw]},
                     "best_other": {"cfg": bo, "us": o[bo], "kind": ops.tile_kind(bo)},
                     "kind6_over_other": round(w[bw] / o[bo], 4), "all_kind6_us": {str(c): t for c, t in sorted(w.items())}})
    return rows


def worker(args):
    import numpy as np
    import torch

    import __graft_entry__
    __graft_entry__.build()
    if not torch.cuda.is_available():
        sys.exit("search_tiles_bench: needs a GPU (nothing is measured without one)")
    from delta_loss_bench import build_net
    from smpq import assignments, engine, ops, sensitivity, suffix
    dev = torch.device("cuda:0")
    engine.set_range_mode("static")
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)
    lut = ops.u8lut_table()
    g = torch.Generator().manual_seed(2024)
    batches = [(ops.u8lut_decode(torch.randint(0, 256, (args.batch, 3, 224, 224), generator=g, dtype=torch.uint8), lut).to(dev),
                torch.randint(0, 1000, (args.batch,), generator=g).to(dev)) for _ in range(args.batches)]
    nets = {1: build_net(dev), 0: build_net(dev)}
    channels = {}
    for ln in LNUMS:
        cout = assignments.conv_for_lnum(nets[1], ln).out_channels
        channels[ln] = list(range(0, cout, cout // 8))[:8]

    def forward_pass(net):
        with torch.no_grad():
            for _ in range(args.passes):
                for x, _y in batches:
                    net(x)

    def table(net):
        t = sensitivity.delta_loss_table(net, batches, bits=BITS, lnums=LNUMS, channels=channels, suffix=False)
        r = t.report()
        assert r["patched"] == 64 and not r["slow"] and not r["constant"], r
        assert r["during_trials"] == {"calibrations": 0, "graph_captures": 0, "repack": 0}, r
        return t

    fwd = {1: [], 0: []}
    tab = {1: [], 0: []}
    trials = {1: [], 0: []}
    last = {}
    for rep in range(args.warmups + args.reps):
        for knob in (1, 0):
            ops.RESIDENT_W[0] = bool(knob)
            net = nets[knob]
            if rep == 0:
                with torch.no_grad():  # calibration, tuning and captures before anything is timed
                    for x, _y in batches:
                        net(x)
                    for x, _y in batches:
                        net(x)
            dt_f, _ = timed(lambda: forward_pass(net))
            dt_t, t = timed(lambda: table(net))
            last[knob] = t
            if rep >= args.warmups:
                fwd[knob].append(dt_f / (args.passes * len(batches)))
                tab[knob].append(dt_t)
                trials[knob].append(t.report()["trials_s"])
            print("rep %d knob %d: forward %.3f ms per batch, table call %.3f s (trials %.3f s)"
                  % (rep, knob, 1e3 * dt_f / (args.passes * len(batches)), dt_t, t.report()["trials_s"]), flush=True)
        ta, tb = last[1], last[0]
        assert ta.base_loss == tb.base_loss and ta.eval_loss == tb.eval_loss
        for bit in BITS:  # the two settings compute the same thing
            assert np.array_equal(np.asarray(ta.stats[bit]).view(np.uint64), np.asarray(tb.stats[bit]).view(np.uint64)), (rep, bit)
            assert np.array_equal(np.asarray(ta.delta[bit]).view(np.uint64), np.asarray(tb.delta[bit]).view(np.uint64)), (rep, bit)

    on_kind6 = sorted({(k[0][3], k[0][4]) for k, v in ops._TUNED.items()
                       if isinstance(k[0], tuple) and k[1] == "resw" and ops.tile_kind(v) == ops.TILE_RESIDENT1X1_W})
    f1, f0 = summary(fwd[1]), summary(fwd[0])
    spread = max(f1["max_s"] - f1["min_s"], f0["max_s"] - f0["min_s"])
    wins = f0["median_s"] - f1["median_s"] > spread
    doc = {
        "tool": "tools/search_tiles_bench.py", "device": torch.cuda.get_device_name(0),
        "workload": {"arch": "resnet50", "bn": "r50_mixed_cal", "weights": "seeded, pristine", "batches": args.batches,
                     "batch": args.batch, "graphs": bool(engine.USE_GRAPH[0]), "act_limbs": ops.get_act_limbs(),
                     "slices_per_batch": len(suffix.slices(args.batch)), "streams": engine.STREAMS[0],
                     "trials": 64, "lnums": list(LNUMS), "channels": {str(k): v for k, v in channels.items()},
                     "bits": list(BITS)},
        "protocol": {"warmups": args.warmups, "reps": args.reps, "passes_per_forward_rep": args.passes,
                     "tune_reps": ops.TUNE_REPS[0],
                     "clock": "host perf_counter, device synchronise on both sides; one model per setting in one run, "
                              "the settings alternating, SMPQ_RESIDENT_W=1 first in each repetition",
                     "baseline": "SMPQ_RESIDENT_W=0: the parent's candidates and tiles",
                     "tables_bitwise_equal": True},
        "a_autotuner_medians_per_eligible_shape": tune_rows(ops),
        "shapes_the_tuner_put_on_kind6": [list(s) for s in on_kind6],
        "b_forward_per_batch": {"resident_w_1": f1, "resident_w_0": f0, "with_over_without": round(f1["median_s"] / f0["median_s"], 4),
                                "spread_s": round(spread, 6)},
        "c_table_call_64_trials": {"resident_w_1": summary(tab[1]), "resident_w_0": summary(tab[0]),
                                   "trials_only_1": summary(trials[1]), "trials_only_0": summary(trials[0])},
        "default": {"rule": "1 only if (b)'s median without the kind minus the median with it exceeds the spread "
                            "(the larger max - min of the two settings over the reps)",
                    "kind_wins": bool(wins), "SMPQ_RESIDENT_W": 1 if wins else 0},
        "not_measured": "ResNet-18 / 34 (BasicBlock nets have no eligible conv), 2 limbs, real data, a whole table",
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"forward_ms_with": 1e3 * f1["median_s"], "forward_ms_without": 1e3 * f0["median_s"],
                      "spread_ms": 1e3 * spread, "default": doc["default"]["SMPQ_RESIDENT_W"], "out": args.out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=1)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=560, help="seconds for the whole run")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_tiles.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    # the measurement in a fresh child under the whole run's limit (this process never opens the GPU)
    try:
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"] + sys.argv[1:], timeout=args.timeout).returncode
    except subprocess.TimeoutExpired:
        sys.exit("search_tiles_bench: the run exceeded %d s and was ended" % args.timeout)
    sys.exit(rc)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
