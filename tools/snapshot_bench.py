#!/usr/bin/env python3
"""Save / rollback cost of the search loop on the device: the bit-packed snapshot against the
state-dict files ("Bit-packed weight store").

The search saves the model on every accepted semilayer (resnet50_main.py:212
``torch.save(net.state_dict(), pthname)``) and reloads it on every rejected one (:233-234
``net.load_state_dict(torch.load(pthname))``). On a ResNet-50 with the published mixed 8/6/4
assignment, on cuda:0, this times, each warm, repeated, median of the repeats, every repeat
ending in a device synchronise:

  * checkpoint.snapshot(net) and checkpoint.restore_(net, state) (csrc/bitpack.hip);
  * checkpoint.save_checkpoint / load_checkpoint (the .pth + sidecar this package had before);
  * the driver's own two lines, torch.save(state_dict) and load_state_dict(torch.load(...)),
    with the file in --dir (default: a fresh temporary directory, removed afterwards);
  * checkpoint.save_packed / load_packed, with both files' sizes.

After every restore the state dict is compared bitwise with the one saved. Prints one JSON line.

usage: python tools/snapshot_bench.py [--model resnet50] [--assignment r50_mixed] [--reps 15]
                                      [--warmup 3] [--dir D] [--out F.json] [--device cuda:0]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)

import torch  # noqa: E402


def _sync():
    if torch.cuda.is_initialized():
        torch.cuda.synchronize()


def timed(fn, warmup, reps):
    """Milliseconds of fn(), each call bracketed by device synchronises: median, min, max."""
    ts = []
    for i in range(warmup + reps):
        _sync()
        t0 = time.perf_counter()
        fn()
        _sync()
        if i >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--assignment", default="r50_mixed")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--device", default="cuda:0", help="cpu: a rehearsal of the script, not a measurement")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    import resnet
    from smpq import assignments, checkpoint
    dev = torch.device(args.device)
    assert dev.type == "cpu" or torch.cuda.is_available(), "snapshot_bench measures on the GPU"
    torch.manual_seed(0)
    net = getattr(resnet, args.model)().to(dev).eval()
    assignments.apply_assignment(net, args.assignment)
    sd0 = {k: v.clone() for k, v in net.state_dict().items()}

    def same():
        sd = net.state_dict()
        return all(torch.equal(sd[k].view(torch.int32) if v.dtype == torch.float32 else sd[k],
                               v.view(torch.int32) if v.dtype == torch.float32 else v) for k, v in sd0.items())

    def scramble():
        with torch.no_grad():
            for p in net.parameters():
                p.zero_()

    tmp = args.dir or tempfile.mkdtemp(prefix="smpq_snapshot_bench_")
    os.makedirs(tmp, exist_ok=True)
    pth, side_pth, packed = (os.path.join(tmp, n) for n in ("driver.pth", "sidecar.pth", "packed.smpq"))
    res = {"model": args.model, "assignment": args.assignment, "reps": args.reps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(dev) if dev.type == "cuda" else "cpu (rehearsal)"}
    try:
        holder = {}
        res["snapshot"] = timed(lambda: holder.__setitem__("st", checkpoint.snapshot(net)), args.warmup, args.reps)
        st = holder["st"]
        rep = checkpoint.packed_report(st)["total"]
        res["report"] = rep
        scramble()
        res["restore"] = timed(lambda: checkpoint.restore_(net, st), args.warmup, args.reps)
        res["restore_bitwise"] = same()
        res["restore_write_GBps"] = round(rep["fp32_bytes"] / (res["restore"]["median_ms"] * 1e-3) / 1e9, 1)

        res["driver_torch_save"] = timed(lambda: torch.save(net.state_dict(), pth), args.warmup, args.reps)
        scramble()
        res["driver_load_state_dict"] = timed(lambda: net.load_state_dict(torch.load(pth)), args.warmup, args.reps)
        res["driver_bitwise"] = same()

        res["save_checkpoint"] = timed(lambda: checkpoint.save_checkpoint(net, side_pth), args.warmup, args.reps)
        scramble()
        res["load_checkpoint"] = timed(lambda: checkpoint.load_checkpoint(net, side_pth, map_location=dev),
                                       args.warmup, args.reps)
        res["load_checkpoint_bitwise"] = same()

        res["save_packed"] = timed(lambda: checkpoint.save_packed(net, packed), args.warmup, args.reps)
        scramble()
        res["load_packed"] = timed(lambda: checkpoint.load_packed(net, packed, map_location=dev), args.warmup, args.reps)
        res["load_packed_bitwise"] = same()
        res["file_bytes"] = {"driver_pth": os.path.getsize(pth), "packed": os.path.getsize(packed),
                             "save_checkpoint_pth": os.path.getsize(side_pth),
                             "save_checkpoint_sidecar": os.path.getsize(checkpoint.sidecar_path(side_pth))}
    finally:
        if args.dir is None:
            shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
