"""Time ops.conv2d_dilated_q in its static limb-plane mode (limb planes in, limb planes out, BN scale / ReLU /
requantize fused) on the dilated conv2 shapes of ResNet-50 replace_stride_with_dilation=[False, True, True]
at 224^2, batch 64, against
  (a) F.relu(F.conv2d(..., dilation=d)) in fp32, the route such a conv took before, and
  (b) ops.tuned_conv2d_q on the same tensors with dilation 1 / pad 1: the same MACs on the project's own
      undilated kernels (the halo 3x3 tiles for exact codes), the fair yardstick.
Device events, the variants alternating, 5 repetitions of LAUNCHES launches each; sorted times per variant."""
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
N, REPS, LAUNCHES = 64, 5, 300
# (channels, H, dilation)
SHAPES = [(256, 28, 2), (512, 28, 2), (512, 28, 4)]
out = []


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / LAUNCHES


for c, h, d in SHAPES:
    g = torch.Generator().manual_seed(c + h + d)
    w = (torch.randn(c, c, 3, 3, generator=g) * 0.02).to(dev)
    x = torch.relu(torch.randn(N, h, h, c, generator=g)).to(dev)
    am = ops.act_absmax(x)
    xq = ops.act_quantize(x, am, 3)
    sh = torch.zeros(c, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    c3, _, s3, _ = ops.pack_weights_ex(w, None, 3)
    wq = w.clone()
    step = ops.quantize_channels_(wq.reshape(c, -1), [8] * c)
    c1, o1, s1, _ = ops.pack_weights_ex(wq, step, 1)
    xn = x.permute(0, 3, 1, 2)  # the NCHW view of NHWC the parent's fallback hands F.conv2d
    ref = F.relu(F.conv2d(xn, w, None, 1, d, d))
    rng = float(ref.max()) * 1.25
    lean = dict(relu=True, emit_range=rng, overflow=ovf, want_f32=False)
    fns = {
        "f_conv2d_relu": lambda: F.relu(F.conv2d(xn, w, None, 1, d, d)),
        "dilated_fixed24": lambda: ops.conv2d_dilated_q(xq, am, c3, None, d, s3, sh, **lean),
        "dilated_exact8": lambda: ops.conv2d_dilated_q(xq, am, c1, o1, d, s1, sh, **lean),
        "undilated_fixed24": lambda: ops.tuned_conv2d_q(xq, am, c3, None, 3, 3, 1, 1, s3, sh, **lean),
        "undilated_exact8": lambda: ops.tuned_conv2d_q(xq, am, c1, o1, 3, 3, 1, 1, s1, sh, **lean),
    }
    for fn in fns.values():  # warm-up: code objects, MIOpen's algorithm choice, the tile choice
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    # host enqueue alone (no synchronise inside the window): a kernel time below it is enqueue bound
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(LAUNCHES):
        fns["dilated_exact8"]()
    enqueue_ms = (time.perf_counter() - t0) * 1e3 / LAUNCHES
    torch.cuda.synchronize()
    y = ops.conv2d_dilated_q(xq, am, c3, None, d, s3, sh, relu=True)
    err = float((y.permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max())
    row = {"c": c, "h": h, "d": d, "n": N, "rel_err_vs_fp32": err, "overflow": int(ovf.item()),
           "enqueue_ms_dilated_exact8": enqueue_ms, "ms": {k: sorted(v) for k, v in ms.items()}}
    print(json.dumps(row), flush=True)
    out.append(row)
if len(sys.argv) > 1:  # optional: a file for the rows
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
