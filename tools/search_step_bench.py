#!/usr/bin/env python3
"""What the search's repeat work costs with and without the evaluation memo (smpq.memo) and the
pristine-model pool (smpq.models): the three operations of a search step that the two switches
touch, timed with both switches off (the unchanged code path) and with both on.

    python tools/search_step_bench.py [--batches 8] [--batch 256] [--out profiles/search_step_memo.json]

Workload: ResNet-50 with the published mixed assignment (r50_mixed) on a smpq.batches.ResidentSet of
--batches on-grid batches of --batch images, built as tools/eval_host_batches.py builds them. Per
repetition (2 warm-ups, then 5 timed, every one reported):

  miss    a weight change (half of one layer3 conv3 re-quantized at 3 bits, another conv each
          repetition, so that the state is new), then functions.evaluate_acc_loss_softmax;
  debug   net.load_state_dict(saved accepted state), then the re-evaluation of
          resnet50_main.py:236 (with the memo: a hit);
  fresh   resnet.resnet50(pretrained='imagenet') from a local file (resnet50_main.py:231,
          functions.py:528), then its evaluation (with the memo: a hit, the pristine state having
          been evaluated before, as the driver's initial evaluation does).

Evaluation times are also scaled linearly to the 196 batches of ImageNet val (batch 256), the way
tools/driver_quant_cost.py scales: for a hit that is an upper bound (the key's cost does not grow
with the set, only the clones of the softmax batches do). The weight file is a seeded ResNet-50
state dict written to a temporary directory. A timed search was not run: the share of a search
quoted in DESIGN.md 5d comes from the counts of the reference's published trace.
"""
import argparse
import gc
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__  # noqa: E402

WARMUPS, REPS = 2, 5
COUNTERS = ("hip_conv", "calibrations", "graph_captures", "graph_replays")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(xs):
    xs = [float(x) for x in xs]
    return {"reps_s": [round(x, 5) for x in xs], "median_s": round(float(np.median(xs)), 5),
            "min_s": round(min(xs), 5), "max_s": round(max(xs), 5)}


def run(on, args, dev, host, weights_dir):
    import functions
    import resnet
    from smpq import assignments, memo, models, quantize_layer_, stats
    from smpq.batches import ResidentSet
    memo.clear()
    models.clear_pristine_pool()
    (memo.enable if on else memo.disable)()
    models.set_pristine_pool(on)
    os.environ["SMPQ_PRETRAINED_DIR"] = weights_dir
    rs = ResidentSet(host, device=dev)
    pristine = resnet.resnet50(pretrained="imagenet")
    for _ in range(3):  # the driver's initial evaluation: fills the set, then graphs on its staging buffers
        functions.evaluate_acc_loss_softmax(pristine, dev, rs)
    net = resnet.resnet50(pretrained="imagenet").to(dev).eval()
    assignments.apply_assignment(net, "r50_mixed")
    for _ in range(2):
        accepted = functions.evaluate_acc_loss_softmax(net, dev, rs)
    pth = os.path.join(weights_dir, "accepted.pth")
    torch.save(net.state_dict(), pth)
    t = {k: [] for k in ("miss_eval", "debug_load", "debug_eval", "fresh_build", "fresh_eval")}
    launches = {"debug_eval": [], "fresh_eval": []}
    checks = {"debug_equals_accepted": True, "fresh_equals_pristine": True}
    first_pristine = functions.evaluate_acc_loss_softmax(pristine, dev, rs)
    for rep in range(WARMUPS + REPS):
        conv = net.layer3[rep % 6].conv3
        bits = np.zeros(conv.out_channels, dtype=np.int64)
        bits[:conv.out_channels // 2] = 3 - rep // 6  # (a conv met a second time gets another width)
        quantize_layer_(conv, bits)
        dt_miss, _ = timed(lambda: functions.evaluate_acc_loss_softmax(net, dev, rs))
        dt_load, _ = timed(lambda: net.load_state_dict(torch.load(pth, weights_only=True)))
        s0 = {k: stats[k] for k in COUNTERS}
        dt_dbg, dbg = timed(lambda: functions.evaluate_acc_loss_softmax(net, dev, rs))
        l_dbg = {k: stats[k] - s0[k] for k in COUNTERS}
        checks["debug_equals_accepted"] &= dbg[:2] == accepted[:2] and all(
            torch.equal(a, b) for a, b in zip(dbg[2], accepted[2]))
        dt_build, fresh = timed(lambda: resnet.resnet50(num_classes=1000, pretrained="imagenet"))
        s0 = {k: stats[k] for k in COUNTERS}
        dt_fresh, fr = timed(lambda: functions.evaluate_acc_loss_softmax(fresh, dev, rs))
        l_fresh = {k: stats[k] - s0[k] for k in COUNTERS}
        checks["fresh_equals_pristine"] &= fr[:2] == first_pristine[:2] and all(
            torch.equal(a, b) for a, b in zip(fr[2], first_pristine[2]))
        del fresh, fr, dbg
        gc.collect()
        if rep >= WARMUPS:
            for k, v in (("miss_eval", dt_miss), ("debug_load", dt_load), ("debug_eval", dt_dbg),
                         ("fresh_build", dt_build), ("fresh_eval", dt_fresh)):
                t[k].append(v)
            launches["debug_eval"].append(l_dbg)
            launches["fresh_eval"].append(l_fresh)
        print("on" if on else "off", rep, "miss %.4f load %.4f debug %.4f build %.4f fresh-eval %.4f s"
              % (dt_miss, dt_load, dt_dbg, dt_build, dt_fresh), l_dbg, flush=True)
    res = {k: summary(v) for k, v in t.items()}
    scale = 196.0 / args.batches
    for k in ("miss_eval", "debug_eval", "fresh_eval"):
        res[k]["median_s_scaled_196_batches"] = round(res[k]["median_s"] * scale, 4)
    res["engine_events"] = launches
    res["checks"] = checks
    res["memo_report"] = memo.report()
    res["pool_report"] = models.pristine_pool_report()
    res["accepted"] = list(accepted[:2])
    memo.disable()
    memo.clear()
    models.set_pristine_pool(False)
    models.clear_pristine_pool()
    del net, pristine, rs
    gc.collect()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    __graft_entry__.build()
    import resnet
    from smpq import ops
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    lut = ops.u8lut_table()
    host = [(ops.u8lut_decode(torch.randint(0, 256, (args.batch, 3, 224, 224), generator=g, dtype=torch.uint8), lut)
             .pin_memory(), torch.randint(0, 1000, (args.batch,), generator=g).pin_memory())
            for _ in range(args.batches)]
    res = {"workload": "resnet50 r50_mixed, ResidentSet of %d on-grid batches of %d, functions.evaluate_acc_loss_softmax"
                       % (args.batches, args.batch),
           "timing": "%d warm-up repetitions, then %d timed; host wall time around each operation with a device "
                     "synchronize before and after; *_scaled_196_batches = median * 196 / %d" % (WARMUPS, REPS, args.batches),
           "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads()}
    with tempfile.TemporaryDirectory() as d:
        torch.manual_seed(0)
        sd = {k: v for k, v in resnet.resnet50().state_dict().items()
              if not k.endswith(("qbits", "qstep", "num_batches_tracked"))}
        torch.save(sd, os.path.join(d, os.path.basename(resnet.MODEL_URLS["resnet50"])))
        del sd
        res["switches_off"] = run(False, args, dev, host, d)
        res["switches_on"] = run(True, args, dev, host, d)
    off, on = res["switches_off"], res["switches_on"]
    res["same_results"] = off["accepted"] == on["accepted"] and all(off["checks"].values()) and all(on["checks"].values())
    res["hit_launches_no_forward"] = all(not any(e.values()) for k in ("debug_eval", "fresh_eval")
                                         for e in on["engine_events"][k])
    res["ratios_on_over_off"] = {k: round(on[k]["median_s"] / off[k]["median_s"], 4) for k in
                                 ("miss_eval", "debug_load", "debug_eval", "fresh_build", "fresh_eval")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    assert res["same_results"] and res["hit_launches_no_forward"], (res["same_results"], res["hit_launches_no_forward"])


if __name__ == "__main__":
    main()
