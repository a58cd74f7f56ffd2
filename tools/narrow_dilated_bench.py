"""Time ops.conv2d_narrow_dilated_q (csrc/conv_narrow_dilated.hip; limb planes in, limb planes out, BN scale / ReLU /
requantize fused) per call at batch 64 on the dilated conv2 shapes a width-scaled ResNet-50 has on cin % 64 != 0:
layer 2 of replace_stride_with_dilation=[True, True, True] (width 2 * width_per_group, d 2, 56 x 56) at
width_per_group 16, 48, 80 and 112, and the 48 one at d 4 (a dilation no torchvision-style model pairs with such a
width: layers 3 and 4 are 4 and 8 times width_per_group, multiples of 64), against
(a) F.relu(F.conv2d(..., dilation=d)) in fp32 on the NCHW view, the route such a conv took before, and
(b) ops.conv2d_dilated_q on channels zero-padded to the next multiple of 64 (5o has the same
    comparison for the narrow kernel).
Device events, alternating, 5 repetitions of 20 launches each (the median is the middle of the sorted list);
enqueue_us is the host time per call of 20 calls into an idle queue."""
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
N, REPS, LAUNCHES = 64, 5, 20
# (channels, d, H)
SHAPES = [(32, 2, 56), (96, 2, 56), (160, 2, 56), (224, 2, 56), (96, 4, 56)]
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


for c, d, h in SHAPES:
    cp = (c + 63) // 64 * 64
    g = torch.Generator().manual_seed(c + d + h)
    w = (torch.randn(c, c, 3, 3, generator=g) * 0.1).to(dev)
    x = torch.relu(torch.randn(N, h, h, c, generator=g)).to(dev)
    am = ops.act_absmax(x)
    xq = ops.act_quantize(x, am, 3)
    sh = torch.zeros(c, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    c3, _, s3, _ = ops.pack_weights_narrow(w, None, 3, 1)
    wq = w.clone()
    step = ops.quantize_channels_(wq.reshape(c, -1), [8] * c)
    c1, o1, s1, _ = ops.pack_weights_narrow(wq, step, 1, 1)
    # (b): the same conv with input and output channels zero-padded to cp (padded rows: step 1, zero codes)
    xqp = F.pad(xq, (0, cp - c)).contiguous()
    wp, wqp = F.pad(w, (0, 0, 0, 0, 0, cp - c, 0, cp - c)), F.pad(wq, (0, 0, 0, 0, 0, cp - c, 0, cp - c))
    stepp = torch.cat([step.reshape(-1), torch.ones(cp - c, device=dev)])
    p3, _, sp3, _ = ops.pack_weights_ex(wp.contiguous(), None, 3)
    p1, po1, sp1, _ = ops.pack_weights_ex(wqp.contiguous(), stepp, 1)
    shp = torch.zeros(cp, device=dev)
    xn = x.permute(0, 3, 1, 2)  # the NCHW view of NHWC the parent's fallback hands F.conv2d
    ref = F.relu(F.conv2d(xn, w, None, 1, d, d))
    rng = float(ref.max()) * 1.25
    fns = {
        "f_conv2d_relu": lambda: F.relu(F.conv2d(xn, w, None, 1, d, d)),
        "nd_fixed24": lambda: ops.conv2d_narrow_dilated_q(xq, am, c3, None, d, s3, sh, relu=True, emit_range=rng,
                                                          overflow=ovf, want_f32=False),
        "nd_exact8": lambda: ops.conv2d_narrow_dilated_q(xq, am, c1, o1, d, s1, sh, relu=True, emit_range=rng,
                                                         overflow=ovf, want_f32=False),
        "padded_fixed24": lambda: ops.conv2d_dilated_q(xqp, am, p3, None, d, sp3, shp, relu=True, emit_range=rng,
                                                       overflow=ovf, want_f32=False),
        "padded_exact8": lambda: ops.conv2d_dilated_q(xqp, am, p1, po1, d, sp1, shp, relu=True, emit_range=rng,
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
    enq = {k: enqueue_us(fn) for k, fn in fns.items()}
    y = ops.conv2d_narrow_dilated_q(xq, am, c3, None, d, s3, sh, relu=True)
    yp = ops.conv2d_dilated_q(xqp, am, p3, None, d, sp3, shp, relu=True)
    err = float((y.permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max())
    row = {"c": c, "c_padded": cp, "d": d, "h": h, "n": N, "rel_err_vs_fp32": err,
           "max_abs_diff_vs_padded": float((y - yp[..., :c]).abs().max()), "overflow": int(ovf.item()),
           "ms": {k: sorted(v) for k, v in ms.items()}, "enqueue_us": enq}
    print(json.dumps(row), flush=True)
    out.append(row)
    del x, xq, xqp, xn, ref, y, yp, w, wq
    torch.cuda.empty_cache()
if len(sys.argv) > 1:  # optional: a file for the rows
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
