#!/usr/bin/env python3
"""What one delta-loss trial costs through smpq.sensitivity.delta_loss_table (a packed weight row
patched in place, the captured graphs replayed) and through the public API one trial at a time
(functions.channel_wise_quantizationperchan on the weight, functions.evaluate_loss, the weight put
back with checkpoint.restore_), which is what the package offered before and is the baseline.

    python tools/delta_loss_bench.py [--batches 4] [--batch 256] [--out profiles/delta_loss_sweep.json]

Workload: ResNet-50, seeded pristine weights with the r50_mixed_cal BatchNorm statistics
(tests/golden/model_goldens.npz), --batches batches of --batch synthetic on-grid images on the
device. Both routes run the same 64 trials: 8 channels of each of lnum 1, 24, 40 and 48, at 8 and 4
bits. Per route: --warmups untimed repetitions, then --reps timed ones, host wall time with a device
synchronise on both sides, median and range reported; both routes in this one run, alternating.
The sweep's time is split into its baseline (one evaluation and one unpatched pass, paid once per
table) and its trials. The figures for a whole ResNet-50 table are the per-trial medians times
67 968 trials: a scaling, not a measurement. The tool asserts what makes a patched trial cheap:
the 64 trials add 0 calibrations, 0 graph captures and 0 repacks.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

LNUMS = (1, 24, 40, 48)
BITS = (8, 4)
TABLE_TRIALS = 22656 * 3  # every channel of ResNet-50's 48 searched convs at 8, 6 and 4 bits


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(xs):
    xs = [float(x) for x in xs]
    return {"reps_s": [round(x, 6) for x in xs], "median_s": round(float(np.median(xs)), 6),
            "min_s": round(min(xs), 6), "max_s": round(max(xs), 6)}


def build_net(dev):
    import resnet
    torch.manual_seed(0)
    net = resnet.resnet50()
    g = np.load(os.path.join(REPO, "tests", "golden", "model_goldens.npz"), allow_pickle=False)
    sd = net.state_dict()
    for k in g.files:
        if k.startswith("r50_mixed_cal/bn/"):
            sd[k[len("r50_mixed_cal/bn/"):]].copy_(torch.from_numpy(g[k]))
    return net.to(dev).eval()


def api_route(net, dev, batches, trials, state):
    """The public API, one trial at a time: {(lnum, channel, bit): loss}."""
    import functions
    from smpq import assignments, checkpoint
    out = {}
    for ln, c, bit in trials:
        conv = assignments.conv_for_lnum(net, ln)
        functions.channel_wise_quantizationperchan(conv.weight.data, bit, c)
        out[(ln, c, bit)] = functions.evaluate_loss(net, dev, batches)
        checkpoint.restore_(net, state)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "delta_loss_sweep.json"))
    args = ap.parse_args()
    __graft_entry__.build()
    if not torch.cuda.is_available():
        sys.exit("delta_loss_bench: needs a GPU (nothing is measured without one)")
    import functions
    from smpq import assignments, checkpoint, engine, ops, sensitivity, stats
    dev = torch.device("cuda:0")
    net = build_net(dev)
    lut = ops.u8lut_table()
    g = torch.Generator().manual_seed(2024)
    batches = [(ops.u8lut_decode(torch.randint(0, 256, (args.batch, 3, 224, 224), generator=g, dtype=torch.uint8), lut).to(dev),
                torch.randint(0, 1000, (args.batch,), generator=g).to(dev)) for _ in range(args.batches)]
    channels = {}
    for ln in LNUMS:
        cout = assignments.conv_for_lnum(net, ln).out_channels
        channels[ln] = list(range(0, cout, cout // 8))[:8]
    trials = [(ln, c, bit) for ln in LNUMS for c in channels[ln] for bit in BITS]
    assert len(trials) == 64
    state = checkpoint.snapshot(net)
    base_eval = functions.evaluate_loss(net, dev, batches)

    sweep_t, sweep_base_t, sweep_trials_t, api_t = [], [], [], []
    table = api = None
    for rep in range(args.warmups + args.reps):
        dt_s, table = timed(lambda: sensitivity.delta_loss_table(net, batches, bits=BITS, lnums=LNUMS, channels=channels))
        r = table.report()
        # the structural claim: a patched trial touches no model tensor, so nothing is rebuilt
        assert r["patched"] == 64 and not r["slow"] and not r["constant"], r
        assert r["during_trials"] == {"calibrations": 0, "graph_captures": 0, "repack": 0}, r
        dt_a, api = timed(lambda: api_route(net, dev, batches, trials, state))
        if rep >= args.warmups:
            sweep_t.append(dt_s)
            sweep_base_t.append(r["baseline_s"])
            sweep_trials_t.append(r["trials_s"])
            api_t.append(dt_a)
        print("rep %d: sweep %.3f s (baseline %.3f, trials %.3f), public API %.3f s"
              % (rep, dt_s, r["baseline_s"], r["trials_s"], dt_a), flush=True)
    before = {k: stats[k] for k in ("calibrations", "graph_captures", "repack")}
    api_route(net, dev, batches, trials[:8], state)
    api_counts = {k: (stats[k] - before[k]) / 8.0 for k in before}

    cols = {(int(l), int(c)): i for i, (l, c) in enumerate(zip(table.lnum, table.cnum))}
    diffs = [abs(float(table.delta[bit][cols[(ln, c)]]) - (api[(ln, c, bit)] - base_eval)) for ln, c, bit in trials]
    sign_same = sum((float(table.delta[bit][cols[(ln, c)]]) > 0) == (api[(ln, c, bit)] - base_eval > 0)
                    for ln, c, bit in trials)
    per_trial_sweep = float(np.median(sweep_trials_t)) / 64
    per_trial_api = float(np.median(api_t)) / 64
    doc = {
        "tool": "tools/delta_loss_bench.py", "device": torch.cuda.get_device_name(0),
        "workload": {"arch": "resnet50", "bn": "r50_mixed_cal", "batches": args.batches, "batch": args.batch,
                     "trials": 64, "lnums": list(LNUMS), "channels": channels, "bits": list(BITS),
                     "graphs": bool(engine.USE_GRAPH[0]), "act_limbs": ops.get_act_limbs()},
        "protocol": {"warmups": args.warmups, "reps": args.reps,
                     "clock": "host perf_counter, device synchronise on both sides; both routes in one run, alternating"},
        "sweep": {"call": summary(sweep_t), "baseline_once_per_table": summary(sweep_base_t),
                  "trials_64": summary(sweep_trials_t), "per_trial_s": round(per_trial_sweep, 6),
                  "added_by_the_64_trials": table.report()["during_trials"], "asserted_zero": True},
        "public_api_baseline": {"trials_64": summary(api_t), "per_trial_s": round(per_trial_api, 6),
                                "per_trial_counters": api_counts},
        "agreement": {"max_abs_delta_difference": max(diffs), "same_sign": "%d of 64" % sign_same,
                      "note": "the sweep's trials run under the baseline's ranges, the public route calibrates afresh"},
        "scaled_to_a_resnet50_table": {
            "trials": TABLE_TRIALS, "sweep_hours": round(per_trial_sweep * TABLE_TRIALS / 3600, 2),
            "public_api_hours": round(per_trial_api * TABLE_TRIALS / 3600, 2),
            "note": "per-trial medians of this workload times 67 968: a scaling, not a measured table"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"per_trial_sweep_s": doc["sweep"]["per_trial_s"], "per_trial_api_s": doc["public_api_baseline"]["per_trial_s"],
                      "out": args.out}))


if __name__ == "__main__":
    main()
