"""Time the 3x3 small-channel stem (ops.image_quantize_c4 + ops.stem_conv3_q, csrc/conv_stem3.hip) per call at
batch 256 on 32^2 and 64^2 RGB images, 64 output channels, against the route such a stem took
before: fp32 F.conv2d + F.batch_norm + ReLU on torch, the NHWC copy and ops.act_absmax (engine.stem_forward's
torch branch with nn.Identity for the pool; the act_quantize pass the next conv then still needs is not in
its figure). Variants:
  torch_stem    the fp32 route above
  c4_calib      act_absmax(x) + image_quantize_c4 + stem_conv3_q writing fp32 y and y_absmax (calibration / dynamic)
  c4_static     act_absmax(x) + image_quantize_c4 + stem_conv3_q writing the limb planes only (lean epilogue)
  c4_lean_conv  that last launch alone
Device events, the variants alternating, 5 repetitions of LAUNCHES calls each; sorted times per variant."""
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "semilayer-wise-mixed-precision-quantization_amd"))
from smpq import ops  # noqa: E402

dev = torch.device("cuda:0")
N, COUT, REPS, LAUNCHES = 256, 64, 5, 2000  # windows of 40 ms (the lean conv at 32^2) to 0.9 s
out = []


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / LAUNCHES


for h in (32, 64):
    g = torch.Generator().manual_seed(h)
    w = (torch.randn(COUT, 3, 3, 3, generator=g) * 0.2).to(dev)
    x = torch.randn(N, 3, h, h, generator=g).to(dev)
    mean, var = torch.zeros(COUT, device=dev), torch.ones(COUT, device=dev)
    gamma, beta = torch.linspace(0.5, 1.5, COUT, device=dev), torch.linspace(-0.1, 0.1, COUT, device=dev)
    codes, wscale, _ = ops.pack_weights_stem3(w)
    inv = torch.rsqrt(var + 1e-5) * gamma
    cs, sh = (wscale * inv).contiguous(), (beta - mean * inv).contiguous()
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    yam = torch.zeros(N, device=dev)

    def torch_stem():
        y = F.relu(F.batch_norm(F.conv2d(x.contiguous(memory_format=torch.channels_last), w, None, 1, 1), mean, var,
                                gamma, beta, False, 0.0, 1e-5))
        y = y.permute(0, 2, 3, 1).contiguous()
        return y, ops.act_absmax(y)

    ref = torch_stem()[0]
    rng = float(ref.max()) * 1.25
    am = ops.act_absmax(x)
    xq = ops.image_quantize_c4(x, am)

    def c4(**kw):
        a = ops.act_absmax(x)
        return ops.stem_conv3_q(ops.image_quantize_c4(x, a), a, codes, cs, sh, relu=True, **kw)

    lean = dict(emit_range=rng, overflow=ovf, want_f32=False)
    fns = {
        "torch_stem": torch_stem,
        "c4_calib": lambda: c4(y_absmax=yam),
        "c4_static": lambda: c4(**lean),
        "c4_lean_conv": lambda: ops.stem_conv3_q(xq, am, codes, cs, sh, relu=True, **lean),
    }
    for fn in fns.values():  # warm-up: code objects, MIOpen's algorithm choice
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    # host enqueue alone (no synchronise inside the window): a call time below it is enqueue bound
    torch.cuda.synchronize()
    enq = {}
    for k in ("c4_static", "c4_lean_conv"):
        t0 = time.perf_counter()
        for _ in range(LAUNCHES):
            fns[k]()
        enq[k] = (time.perf_counter() - t0) * 1e3 / LAUNCHES
        torch.cuda.synchronize()
    y = c4()
    err = float((y - ref).abs().max() / ref.abs().max())
    work = ops.alg_work(N, h, h, 4, COUT, 3, 3, h, h, 3, 3, False, True, False, False)
    lean_ms = sorted(ms["c4_lean_conv"])[REPS // 2]
    row = {"h": h, "n": N, "cout": COUT, "rel_err_vs_fp32": err, "overflow": int(ovf.item()), "enqueue_ms": enq,
           "lean_conv_bytes": work["bytes"], "lean_conv_GBps": work["bytes"] / lean_ms / 1e6,
           "ms": {k: sorted(v) for k, v in ms.items()}}
    print(json.dumps(row), flush=True)
    out.append(row)
if len(sys.argv) > 1:  # optional: a file for the rows
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
