"""Time ops.conv2d_grouped_q (limb planes in, limb planes out, BN scale / ReLU / requantize fused) against
F.relu(F.conv2d(..., groups=32)) in fp32, the route such a conv took before, on the conv2 shapes of
ResNeXt-50 32x4d, batch 64. Device events, alternating, 5 repetitions of 1000 launches each."""
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "semilayer-wise-mixed-precision-quantization_amd"))
from smpq import ops  # noqa: E402

dev = torch.device("cuda:0")
N, REPS, LAUNCHES = 64, 5, 1000
# (channels, stride, H in)
SHAPES = [(128, 1, 56), (256, 2, 56), (256, 1, 28), (512, 2, 28), (512, 1, 14), (1024, 2, 14), (1024, 1, 7)]
out = []


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / LAUNCHES


for c, stride, h in SHAPES:
    g = torch.Generator().manual_seed(c + h)
    w = (torch.randn(c, c // 32, 3, 3, generator=g) * 0.1).to(dev)
    x = torch.relu(torch.randn(N, h, h, c, generator=g)).to(dev)
    am = ops.act_absmax(x)
    xq = ops.act_quantize(x, am, 3)
    sh = torch.zeros(c, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    c3, _, s3, _ = ops.pack_weights_grouped(w, None, 3, 32)
    wq = w.clone()
    step = ops.quantize_channels_(wq.reshape(c, -1), [8] * c)
    c1, o1, s1, _ = ops.pack_weights_grouped(wq, step, 1, 32)
    xn = x.permute(0, 3, 1, 2)  # the NCHW view of NHWC the parent's fallback hands F.conv2d
    ref = F.relu(F.conv2d(xn, w, None, stride, 1, 1, 32))
    rng = float(ref.max()) * 1.25
    fns = {
        "f_conv2d_relu": lambda: F.relu(F.conv2d(xn, w, None, stride, 1, 1, 32)),
        "grouped_fixed24": lambda: ops.conv2d_grouped_q(xq, am, c3, None, stride, s3, sh, relu=True, emit_range=rng,
                                                        overflow=ovf, want_f32=False),
        "grouped_exact8": lambda: ops.conv2d_grouped_q(xq, am, c1, o1, stride, s1, sh, relu=True, emit_range=rng,
                                                       overflow=ovf, want_f32=False),
    }
    for fn in fns.values():  # warm-up: code objects, MIOpen's algorithm choice
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    y = ops.conv2d_grouped_q(xq, am, c3, None, stride, s3, sh, relu=True)
    err = float((y.permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max())
    row = {"c": c, "stride": stride, "h": h, "n": N, "rel_err_vs_fp32": err, "overflow": int(ovf.item()),
           "ms": {k: sorted(v) for k, v in ms.items()}}
    print(json.dumps(row), flush=True)
    out.append(row)
if len(sys.argv) > 1:  # optional: a file for the rows
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
