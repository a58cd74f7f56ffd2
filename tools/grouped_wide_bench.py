"""Time ops.conv2d_grouped_q on wide groups (csrc/conv_grouped_wide.hip; limb planes in, limb planes out, BN scale
/ ReLU / requantize fused) on the layer-3 / layer-4 conv2 shapes of ResNeXt 32x16d and 32x32d, batch 64, against
(a) F.relu(F.conv2d(..., groups=32)) in fp32 on the NCHW view, the route such a conv took before, and
(b) ops.tuned_conv2d_q on a dense conv of the same MAC count (cin = cg, cout = og, batch x groups images): the
project's own tiles on the same arithmetic. Device events, alternating, 5 repetitions of 50
launches each; enqueue_us is the host time per call of 20 calls into an idle queue."""
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
N, G, REPS, LAUNCHES = 64, 32, 5, 50
# (channels, stride, H in): 32x16d layer 4 (cg 128); 32x32d layer 3 (cg 128) and layer 4 (cg 256)
SHAPES = [(4096, 2, 14), (4096, 1, 7), (4096, 2, 28), (4096, 1, 14), (8192, 2, 14), (8192, 1, 7)]
out = []


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / LAUNCHES


def enqueue_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / 20 * 1e6


for c, stride, h in SHAPES:
    cg = c // G
    g = torch.Generator().manual_seed(c + h)
    w = (torch.randn(c, cg, 3, 3, generator=g) * 0.1).to(dev)
    x = torch.relu(torch.randn(N, h, h, c, generator=g)).to(dev)
    am = ops.act_absmax(x)
    xq = ops.act_quantize(x, am, 3)
    sh = torch.zeros(c, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    c3, _, s3, _ = ops.pack_weights_grouped(w, None, 3, G)
    wq = w.clone()
    step = ops.quantize_channels_(wq.reshape(c, -1), [8] * c)
    c1, o1, s1, _ = ops.pack_weights_grouped(wq, step, 1, G)
    # (b): one group's weights as a dense conv on batch x groups images of cg channels
    xd = x[:, :, :, :cg].repeat(G, 1, 1, 1).contiguous()
    amd = ops.act_absmax(xd)
    xqd = ops.act_quantize(xd, amd, 3)
    d3, _, sd3, _ = ops.pack_weights_ex(w[:cg].contiguous(), None, 3)
    d1, od1, sd1, _ = ops.pack_weights_ex(wq[:cg].contiguous(), step[:cg], 1)
    shd = torch.zeros(cg, device=dev)
    del xd
    xn = x.permute(0, 3, 1, 2)  # the NCHW view of NHWC the parent's fallback hands F.conv2d
    ref = F.relu(F.conv2d(xn, w, None, stride, 1, 1, G))
    rng = float(ref.max()) * 1.25
    fns = {
        "f_conv2d_relu": lambda: F.relu(F.conv2d(xn, w, None, stride, 1, 1, G)),
        "wide_fixed24": lambda: ops.conv2d_grouped_q(xq, am, c3, None, stride, s3, sh, relu=True, emit_range=rng,
                                                     overflow=ovf, want_f32=False),
        "wide_exact8": lambda: ops.conv2d_grouped_q(xq, am, c1, o1, stride, s1, sh, relu=True, emit_range=rng,
                                                    overflow=ovf, want_f32=False),
        "dense_fixed24": lambda: ops.tuned_conv2d_q(xqd, amd, d3, None, 3, 3, stride, 1, sd3, shd, relu=True,
                                                    emit_range=rng, overflow=ovf, want_f32=False),
        "dense_exact8": lambda: ops.tuned_conv2d_q(xqd, amd, d1, od1, 3, 3, stride, 1, sd1, shd, relu=True,
                                                   emit_range=rng, overflow=ovf, want_f32=False),
    }
    for fn in fns.values():  # warm-up: code objects, MIOpen's algorithm choice, the tile choice
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    enq = {k: enqueue_us(fn) for k, fn in fns.items()}
    y = ops.conv2d_grouped_q(xq, am, c3, None, stride, s3, sh, relu=True)
    err = float((y.permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max())
    row = {"c": c, "cg": cg, "stride": stride, "h": h, "n": N, "rel_err_vs_fp32": err, "overflow": int(ovf.item()),
           "ms": {k: sorted(v) for k, v in ms.items()}, "enqueue_us": enq}
    print(json.dumps(row), flush=True)
    out.append(row)
    del x, xq, xqd, xn, ref, y, w, wq
    torch.cuda.empty_cache()
if len(sys.argv) > 1:  # optional: a file for the rows
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
