"""Time ops.conv2d_narrow_q in its static limb-plane mode (limb planes in, limb planes out, BN scale / ReLU /
requantize fused, no residual) on the narrow conv2 and conv3 shapes of ResNet-50 width_per_group=48 at 224^2,
batch 64, against
  (a) F.relu(F.conv2d(...)) in fp32 on the same tensors, the route such a conv took before, and
  (b) ops.tuned_conv2d_q on the same problem with the input channels zero-padded to the next multiple of 64:
      what padding the channels instead would cost (the producer's extra stores not counted).
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
N, REPS, LAUNCHES = 64, 5, 200
# (cin, cout, k, stride, H): layer1 conv2 / conv3, layer2 block 0 conv2, layer2 conv2 / conv3
SHAPES = [(48, 48, 3, 1, 56), (48, 256, 1, 1, 56), (96, 96, 3, 2, 56), (96, 96, 3, 1, 28), (96, 512, 1, 1, 28)]
out = []


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(LAUNCHES):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / LAUNCHES


for cin, cout, k, stride, h in SHAPES:
    g = torch.Generator().manual_seed(cin + cout + k + h)
    pad, cpad = k // 2, (cin + 63) // 64 * 64
    w = (torch.randn(cout, cin, k, k, generator=g) * 0.05).to(dev)
    x = torch.relu(torch.randn(N, h, h, cin, generator=g)).to(dev)
    am = ops.act_absmax(x)
    xq = ops.act_quantize(x, am, 3)
    xqp = F.pad(xq, (0, cpad - cin)).contiguous()
    sh = torch.zeros(cout, device=dev)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    wq = w.clone()
    step = ops.quantize_channels_(wq.reshape(cout, -1), [8] * cout)
    n3, _, s3, _ = ops.pack_weights_narrow(w, None, 3, stride)
    n1, o1, s1, _ = ops.pack_weights_narrow(wq, step, 1, stride)
    p3, _, t3, _ = ops.pack_weights_ex(F.pad(w, (0, 0, 0, 0, 0, cpad - cin)).contiguous(), None, 3)
    p1, q1, t1, _ = ops.pack_weights_ex(F.pad(wq, (0, 0, 0, 0, 0, cpad - cin)).contiguous(), step, 1)
    xn = x.permute(0, 3, 1, 2)  # the NCHW view of NHWC the parent's fallback hands F.conv2d
    ref = F.relu(F.conv2d(xn, w, None, stride, pad))
    rng = float(ref.max()) * 1.25
    lean = dict(relu=True, emit_range=rng, overflow=ovf, want_f32=False)
    fns = {
        "f_conv2d_relu": lambda: F.relu(F.conv2d(xn, w, None, stride, pad)),
        "narrow_fixed24": lambda: ops.conv2d_narrow_q(xq, am, n3, None, s3, sh, **lean),
        "narrow_exact8": lambda: ops.conv2d_narrow_q(xq, am, n1, o1, s1, sh, **lean),
        "padded_fixed24": lambda: ops.tuned_conv2d_q(xqp, am, p3, None, k, k, stride, pad, t3, sh, **lean),
        "padded_exact8": lambda: ops.tuned_conv2d_q(xqp, am, p1, q1, k, k, stride, pad, t1, sh, **lean),
    }
    for fn in fns.values():  # warm-up: code objects, MIOpen's algorithm choice, the tile choice
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in fns}
    for _ in range(REPS):
        for name, fn in fns.items():
            ms[name].append(timed(fn))
    # host enqueue alone (no synchronise inside the window): a kernel time below it is enqueue bound
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(LAUNCHES):
        fns["narrow_exact8"]()
    enqueue_ms = (time.perf_counter() - t0) * 1e3 / LAUNCHES
    torch.cuda.synchronize()
    y = ops.conv2d_narrow_q(xq, am, n3, None, s3, sh, relu=True)
    err = float((y.permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max())
    _, yn = fns["narrow_exact8"]()
    _, yp = fns["padded_exact8"]()
    row = {"cin": cin, "cout": cout, "k": k, "stride": stride, "h": h, "n": N, "rel_err_vs_fp32": err,
           "overflow": int(ovf.item()), "exact8_equals_padded": bool(torch.equal(yn, yp)),
           "enqueue_ms_narrow_exact8": enqueue_ms, "ms": {name: sorted(v) for name, v in ms.items()}}
    print(json.dumps(row), flush=True)
    out.append(row)
if len(sys.argv) > 1:  # optional: a file for the rows
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
