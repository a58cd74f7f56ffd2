#!/usr/bin/env python3
"""Throughput of the drop-in evaluation loop (functions.evaluate_acc_loss_softmax, the reference's
functions.py:84-129) when the batches come from the host, as the reference's DataLoader delivers
them (pin_memory=True, imagenet.py), against the same loop on device-resident fp32 batches and on a
smpq.batches.ResidentSet (the set kept on the device as uint8 and decoded batch by batch).

    python tools/eval_host_batches.py [--batches 8] [--batch 256] [--config r50_mixed] [--out PATH]

All four loaders serve the same batches, which lie on the ToTensor / Normalize grid as a real
ImageNet loader's do: random uint8 through ops.u8lut_table(). Prints one JSON object: images/s for
device batches, pinned host batches, pageable host batches and the resident uint8 set (each from
--reps evaluations after one warm-up evaluation that calibrates, captures graphs and, for the
resident set, reads the loader; every repetition's time is kept), the ratios, the engine's graph
events per loader, and the decode kernel's own time from device events around a batch of launches.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import __graft_entry__  # noqa: E402

ARCH = {"r50_mixed": "resnet50", "r18_u8": "resnet18", "r34_4bit": "resnet34"}


def decode_kernel_time(ops, dev, batch, launches=50):
    """ops.u8lut_decode at [batch, 3, 224, 224] between two device events: mean us per launch and
    bytes/s over the 5 bytes per element it moves (1 read, 4 written)."""
    lut = ops.u8lut_table().to(dev)
    u = torch.randint(0, 256, (batch, 3, 224, 224), dtype=torch.uint8, device=dev)
    x = torch.empty(u.shape, dtype=torch.float32, device=dev)
    for _ in range(5):
        ops.u8lut_decode(u, lut, out=x)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    runs = []
    for _ in range(3):
        e0.record()
        for _ in range(launches):
            ops.u8lut_decode(u, lut, out=x)
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / launches)
    us = min(runs)
    return {"shape": list(u.shape), "launches": launches, "us_per_launch_runs": [round(r, 2) for r in runs],
            "us": round(us, 2), "bytes": 5 * u.numel(), "TB_s": round(5 * u.numel() / (us * 1e-6) / 1e12, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--config", default="r50_mixed")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    __graft_entry__.build()
    import functions
    import resnet
    from smpq import assignments, engine, ops, stats
    from smpq.batches import ResidentSet
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = getattr(resnet, ARCH[args.config])().to(dev).eval()
    assignments.apply_assignment(net, args.config)
    g = torch.Generator().manual_seed(5)
    lut = ops.u8lut_table()
    host = [(ops.u8lut_decode(torch.randint(0, 256, (args.batch, 3, 224, 224), generator=g, dtype=torch.uint8), lut),
             torch.randint(0, 1000, (args.batch,), generator=g)) for _ in range(args.batches)]
    pinned = [(x.pin_memory(), y.pin_memory()) for x, y in host]
    device = [(x.to(dev), y.to(dev)) for x, y in host]
    res = {"workload": "%s, %d batches of %d images on the uint8 grid, functions.evaluate_acc_loss_softmax" % (
        args.config, args.batches, args.batch)}
    accs = {}
    keys = ("calibrations", "overflow_reruns", "stale_reruns", "graph_captures", "graph_replays")

    class Stamped:
        """The loader, with the host time at which each batch is handed out."""
        def __init__(self, items):
            self.items, self.t = items, []

        def __iter__(self):
            for it in self.items:
                self.t.append(time.perf_counter())
                yield it
    resident = ResidentSet(pinned, device=dev)
    for name, loader in (("device", device), ("pinned_host", pinned), ("pageable_host", host),
                         ("resident_u8", resident)):
        # every loader starts with all of the model's per-address graph slots free, as if it were the
        # only one the process evaluates (the slots are not reclaimed from an earlier loader's inputs)
        engine.model_state(net).graphs.forget(fallback=False)
        first = functions.evaluate_acc_loss_softmax(net, dev, loader)  # calibration + graph captures (+ the fill)
        if loader is resident:
            # the second evaluation is the first served from the device: it captures the graphs on
            # the two staging addresses
            assert functions.evaluate_acc_loss_softmax(net, dev, loader)[:2] == first[:2]
        best, times = None, []
        for _ in range(args.reps):
            # (the resident set is evaluated as it is: functions iterates it directly, without the
            # prefetching DeviceBatches wrapper any other iterable gets)
            st = loader if loader is resident else Stamped(loader)
            s0 = {k: stats[k] for k in keys}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc, loss, _ = functions.evaluate_acc_loss_softmax(net, dev, st)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            times.append(el)
            if best is None or el < best:
                best = el
                res[name + "_engine_events"] = {k: stats[k] - s0[k] for k in keys}
                if loader is not resident:
                    res[name + "_batch_ms"] = [round((b - a) * 1e3, 2) for a, b in zip([t0] + st.t, st.t + [t0 + el])]
        accs[name] = (acc, loss)
        images = args.batches * args.batch
        res[name + "_img_s"] = round(images / best, 1)
        res[name + "_rep_img_s"] = [round(images / t, 1) for t in times]
        # the spread of this loader's own repetitions, relative to its best
        res[name + "_rep_spread"] = round(max(times) / min(times) - 1, 4)
        print(name, res[name + "_img_s"], "img/s", res[name + "_rep_img_s"], res[name + "_engine_events"],
              res.get(name + "_batch_ms"), flush=True)
    # same results bit for bit, whichever way the batches reach the device
    assert accs["pinned_host"] == accs["device"] == accs["pageable_host"] == accs["resident_u8"], accs
    res["resident_report"] = resident.report()
    res["pinned_over_device"] = round(res["pinned_host_img_s"] / res["device_img_s"], 4)
    res["pageable_over_device"] = round(res["pageable_host_img_s"] / res["device_img_s"], 4)
    res["resident_over_device"] = round(res["resident_u8_img_s"] / res["device_img_s"], 4)
    res["resident_over_pinned"] = round(res["resident_u8_img_s"] / res["pinned_host_img_s"], 4)
    # the noise of the comparison below: the larger of the spreads the two loaders it compares show
    # between their own repetitions (slowest time over fastest, minus one)
    res["rep_spread_max"] = max(res[n + "_rep_spread"] for n in ("pinned_host", "resident_u8"))
    res["decode_kernel"] = decode_kernel_time(ops, dev, args.batch)
    res["timing"] = "best of %d evaluations after the warm-up evaluations of each loader; *_rep_img_s has every one" % args.reps
    # the resident set must not be slower than pinned host batches by more than the run's own noise
    res["resident_not_below_pinned"] = bool(res["resident_u8_img_s"] * (1 + res["rep_spread_max"])
                                            >= res["pinned_host_img_s"])
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    assert res["resident_not_below_pinned"], (res["resident_u8_img_s"], res["pinned_host_img_s"], res["rep_spread_max"])


if __name__ == "__main__":
    main()
