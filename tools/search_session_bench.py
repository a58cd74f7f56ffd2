#!/usr/bin/env python3
"""What one main-loop trial of the search costs through smpq.search.Session (the semilayer's rows of
the conv's packed operand patched in place, forwarded from a kept boundary or by replay, restored)
and through the public API, which is what the package offered before and is the baseline: quantize
the semilayer (functions.channel_wise_quantizationperchan per channel), functions.evaluate_acc_loss_softmax
+ functions.KLdiv, checkpoint.restore_, and the drivers' "debug" evaluation of the restored state
with the evaluation memo off.

    python tools/search_session_bench.py [--batches 4] [--batch 256] [--out profiles/search_session.json]

Workload (DESIGN.md 5g's): ResNet-50, seeded pristine weights with the r50_mixed_cal BatchNorm
statistics (tests/golden/model_goldens.npz), --batches batches of --batch synthetic on-grid images on
the device, graphs on, 3 limbs. Standing state: pristine plus three accepted 8-bit semilayers, the
even and the odd channels of lnum 1 (which completes that conv: its operand is 'exact8') and the even
channels of lnum 24. The 12 trials: the completed conv at 6 bits (even, odd: the exact8 patch), a
quarter of lnum 24, the even and the odd channels of lnum 40 and 48 at 8 and at 6 bits, and last
the trial that completes lnum 24 (odd channels at 8 bits: the slow route). Both routes run the same
12 trials in one run, alternating per repetition; --warmups untimed repetitions, then --reps timed
ones; host wall time with a device synchronise on both sides of every trial; median and range
reported. A session runs once with the default boundaries and once with none (the replay), so a
resumed trial has its replayed twin. Asserted: patched trials add 0 calibrations, 0 graph captures and 0 repacks. Reported,
not asserted: everything else.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402
from semilayer_bench import build_net, summary, timed  # noqa: E402

ZERO = {"calibrations": 0, "graph_captures": 0, "repack": 0}


def standing_and_trials(net):
    from smpq import assignments
    cout = {ln: assignments.conv_for_lnum(net, ln).out_channels for ln in (1, 24, 40, 48)}
    accepted = [(1, list(range(0, cout[1], 2)), 8), (1, list(range(1, cout[1], 2)), 8), (24, list(range(0, cout[24], 2)), 8)]
    trials = [(1, list(range(0, cout[1], 2)), 6), (1, list(range(1, cout[1], 2)), 6), (24, list(range(1, cout[24], 4)), 8)]
    for ln in (40, 48):
        for bit in (8, 6):
            trials += [(ln, list(range(0, cout[ln], 2)), bit), (ln, list(range(1, cout[ln], 2)), bit)]
    trials.append((24, list(range(1, cout[24], 2)), 8))  # completes lnum 24: the slow route, and a rebase after it
    assert len(trials) == 12
    return accepted, trials


def api_trial(net, dev, batches, trial, state, reference):
    """The parent's main-loop trial: (acc, loss, kl) of the quantized model; then the restore and the
    "debug" evaluation of the restored state."""
    import functions
    from smpq import assignments, checkpoint
    ln, channels, bit = trial
    conv = assignments.conv_for_lnum(net, ln)
    for c in channels:
        conv.weight.data = functions.channel_wise_quantizationperchan(conv.weight.data, bit, c)
    acc, loss, after = functions.evaluate_acc_loss_softmax(net, dev, batches)
    kl = functions.KLdiv(reference, after)
    checkpoint.restore_(net, state)
    functions.evaluate_acc_loss_softmax(net, dev, batches)
    return acc, loss, kl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmups", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "search_session.json"))
    args = ap.parse_args()
    __graft_entry__.build()
    if not torch.cuda.is_available():
        sys.exit("search_session_bench: needs a GPU (nothing is measured without one)")
    import functions
    from smpq import assignments, checkpoint, engine, memo, ops, search
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)
    memo.disable()
    dev = torch.device("cuda:0")
    net = build_net(dev)
    lut = ops.u8lut_table()
    g = torch.Generator().manual_seed(2024)
    batches = [(ops.u8lut_decode(torch.randint(0, 256, (args.batch, 3, 224, 224), generator=g, dtype=torch.uint8), lut).to(dev),
                torch.randint(0, 1000, (args.batch,), generator=g).to(dev)) for _ in range(args.batches)]
    _, _, reference = functions.evaluate_acc_loss_softmax(net, dev, batches)
    reference = [r.clone() for r in reference]
    accepted, trials = standing_and_trials(net)
    for ln, channels, bit in accepted:
        conv = assignments.conv_for_lnum(net, ln)
        for c in channels:
            conv.weight.data = functions.channel_wise_quantizationperchan(conv.weight.data, bit, c)
    state = checkpoint.snapshot(net)

    n = len(trials)
    times = {"resumed": [[] for _ in range(n)], "replay": [[] for _ in range(n)], "api": [[] for _ in range(n)]}
    rebase_t = {"resumed": [], "replay": []}
    last = {}
    for rep in range(args.warmups + args.reps):
        keep = rep >= args.warmups
        results = {"resumed": [], "replay": [], "api": []}
        for name, boundaries in (("resumed", None), ("replay", ())):
            dt, s = timed(lambda: search.Session(net, batches, reference_outputs=reference, boundaries=boundaries))
            if keep:
                rebase_t[name].append(dt)
            for i, trial in enumerate(trials):  # (the slow trial is the last one: no rebase falls into a timed trial)
                dt, r = timed(lambda: s.trial(*trial))
                results[name].append(r)
                if keep:
                    times[name][i].append(dt)
            rp = s.report()
            assert rp["patched_trials"] == ZERO, rp  # the structural claim: a patched trial rebuilds nothing
            last[name] = (rp, s.base)
            s.close()
        for i, trial in enumerate(trials):
            dt, r = timed(lambda: api_trial(net, dev, batches, trial, state, reference))
            results["api"].append(r)
            if keep:
                times["api"][i].append(dt)
        last["results"] = results
        print("rep %d done" % rep, flush=True)

    results = last["results"]
    base = last["resumed"][1]
    rows = []
    for i, (ln, channels, bit) in enumerate(trials):
        r, p, a = results["resumed"][i], results["replay"][i], results["api"][i]
        row = {"lnum": ln, "rows": len(channels), "bit": bit, "route": r.route, "resumed_from": r.resumed_from,
               "session_s": summary(times["resumed"][i]), "session_no_boundaries_s": summary(times["replay"][i]),
               "public_api_s": summary(times["api"][i]),
               "acc": {"session": r.acc, "public_api": a[0]}, "kl": {"session": r.kl, "public_api": a[2]},
               "decision_keep": {"session": bool(r.acc >= base.acc), "public_api": bool(a[0] >= base.acc)},
               "same_statistics_resumed_and_replayed": r.stats == p.stats and r.kl_stats == p.kl_stats}
        row["decisions_agree"] = row["decision_keep"]["session"] == row["decision_keep"]["public_api"]
        row["kl_abs_difference"] = abs(r.kl - a[2])
        if r.resumed_from is not None:  # the 5h rule: resumed below the replay by more than the spread of the 5
            sp = max(row["session_s"]["max_s"] - row["session_s"]["min_s"],
                     row["session_no_boundaries_s"]["max_s"] - row["session_no_boundaries_s"]["min_s"])
            row["resumed_beats_replay_by_more_than_the_spread"] = bool(
                row["session_no_boundaries_s"]["median_s"] - row["session_s"]["median_s"] > sp)
        rows.append(row)
    by_route = {}
    for row in rows:
        key = "%s from %s" % (row["route"], row["resumed_from"]) if row["route"].startswith("patched") else row["route"]
        by_route.setdefault(key, []).append(row)
    per_route = {k: {"trials": len(v),
                     "session_median_ms": round(1e3 * float(np.median([x["session_s"]["median_s"] for x in v])), 3),
                     "session_no_boundaries_median_ms": round(1e3 * float(np.median([x["session_no_boundaries_s"]["median_s"] for x in v])), 3),
                     "public_api_median_ms": round(1e3 * float(np.median([x["public_api_s"]["median_s"] for x in v])), 3)}
                 for k, v in by_route.items()}
    doc = {
        "tool": "tools/search_session_bench.py", "device": torch.cuda.get_device_name(0),
        "workload": {"arch": "resnet50", "bn": "r50_mixed_cal", "batches": args.batches, "batch": args.batch,
                     "graphs": bool(engine.USE_GRAPH[0]), "act_limbs": ops.get_act_limbs(),
                     "standing_state": [{"lnum": ln, "rows": len(ch), "bit": bit} for ln, ch, bit in accepted],
                     "evaluation_memo": "off"},
        "protocol": {"warmups": args.warmups, "reps": args.reps,
                     "clock": "host perf_counter, device synchronise on both sides of every trial; the three routes "
                              "in one run, alternating per repetition",
                     "baseline": "per trial: quantize through the public API, evaluate_acc_loss_softmax + KLdiv, "
                                 "checkpoint.restore_, the debug evaluation of the restored state"},
        "trials": rows, "per_route": per_route,
        "rebase": {"default_boundaries_s": summary(rebase_t["resumed"]), "no_boundaries_s": summary(rebase_t["replay"]),
                   "note": "a session's construction on the standing state: paid once per accepted state and per "
                           "slow trial, not once per trial",
                   "boundaries": last["resumed"][0]["boundaries"]},
        "session_report": {k: v for k, v in last["resumed"][0].items() if k != "boundaries"},
        "agreement": {"decisions_agree": all(r["decisions_agree"] for r in rows),
                      "max_kl_abs_difference": max(r["kl_abs_difference"] for r in rows),
                      "resumed_and_replayed_statistics_equal": all(r["same_statistics_resumed_and_replayed"] for r in rows),
                      "base_acc": base.acc,
                      "note": "a patched trial runs under the standing state's ranges and none of its forwards is a "
                              "calibration forward; the public route calibrates afresh on its first batch"},
        "patched_trials_added": ZERO, "asserted_zero": True,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps({"per_route": per_route, "decisions_agree": doc["agreement"]["decisions_agree"],
                      "max_kl_abs_difference": doc["agreement"]["max_kl_abs_difference"],
                      "rebase_default_median_s": doc["rebase"]["default_boundaries_s"]["median_s"], "out": args.out}))


if __name__ == "__main__":
    main()
