"""One rank of tests/test_gpu_table_shard.py (not a test module): a process of a gloo group on
cuda:0 that runs its share of a sensitivity table's trials (dp.sharded_delta_loss_table /
dp.sharded_semilayer_table) and saves the merged table it got back.

    python tests/table_shard_worker.py RANK WORLD PORT OUTDIR CASE

Model and data are tests/test_gpu_sensitivity.py's: a seeded ResNet-18 with the r18_u8_cal
BatchNorm statistics and 2 batches of 8 seeded 224 x 224 images; static ranges, graphs on, 3 limbs.
Conv 3 is fully quantized (its trials take the slow route) and one channel of conv 13 is constant.
"""
import os
import pickle
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "semilayer-wise-mixed-precision-quantization_amd"))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

IMG_SEED, LABEL_SEED = 77, 182
BITS = (8, 2)
# one layer-1 conv, the fully quantized conv 3, and layer4.0's conv1 / conv2 (block 6 of 8: past the
# suffix cut; conv 14 is the block's last conv, the rows route's)
CHANNELS = {1: [0, 5, 17, 40, 63], 3: [0, 5, 9, 33, 63], 13: [0, 3, 100, 257, 511], 14: [1, 2, 200, 300, 510]}
QUANTIZED_LNUM = 3
CONSTANT = (13, 100)
SEMILAYERS = [(2, list(range(0, 64, 2)), 8), (15, list(range(1, 512, 2)), 2), (15, [3, 60], (8, 2)), (2, list(range(63)), 4)]
CASES = {
    "delta_w2": {"world": 2, "kw": {"bits": BITS, "lnums": [1, 3, 13, 14], "channels": CHANNELS}},
    "suffix_w2": {"world": 2, "kw": {"bits": BITS, "lnums": [13, 14], "channels": CHANNELS, "suffix": True, "rows": True}},
    # 2 channels per conv over 3 ranks: rank 2 owns nothing of any conv
    "delta_w3": {"world": 3, "kw": {"bits": BITS, "lnums": [1, 3, 13, 14],
                                    "channels": {1: [0, 63], 3: [0, 63], 13: [3, 100], 14: [1, 510]}}},
    "semi_w2": {"world": 2, "semilayers": SEMILAYERS, "kw": {}},
}


def knobs():
    from smpq import engine, ops
    engine.set_range_mode("static")
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)


def model(dev):
    import resnet
    from smpq import assignments, quant
    torch.manual_seed(0)
    net = resnet.resnet18()
    g = np.load(os.path.join(REPO, "tests", "golden", "model_goldens.npz"), allow_pickle=False)
    sd = net.state_dict()
    for k in g.files:
        if k.startswith("r18_u8_cal/bn/"):
            sd[k[len("r18_u8_cal/bn/"):]].copy_(torch.from_numpy(g[k]))
    net = net.to(dev).eval()
    with torch.no_grad():
        assignments.conv_for_lnum(net, CONSTANT[0]).weight[CONSTANT[1]] = 0.0078125
    conv = assignments.conv_for_lnum(net, QUANTIZED_LNUM)
    quant.quantize_layer_(conv, np.full(conv.out_channels, 8))
    return net


def batches(dev, n=8, count=2):
    g = torch.Generator().manual_seed(IMG_SEED)
    xs = [torch.randn(n, 3, 224, 224, generator=g) for _ in range(count)]
    ys = torch.randint(0, 1000, (n * count,), generator=torch.Generator().manual_seed(LABEL_SEED))
    return [(x.to(dev), ys[i * n:(i + 1) * n].to(dev)) for i, x in enumerate(xs)]


def single(case, net, data):
    """The case's table in one process, unsharded."""
    from smpq import sensitivity
    c = CASES[case]
    if "semilayers" in c:
        return sensitivity.semilayer_table(net, data, c["semilayers"], **c["kw"])
    return sensitivity.delta_loss_table(net, data, **c["kw"])


def main():
    rank, world, port, outdir, case = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    import datetime

    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=240))
    try:
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        from smpq import dp
        knobs()
        c = CASES[case]
        assert c["world"] == world
        net, data = model(dev), batches(dev)
        if "semilayers" in c:
            table = dp.sharded_semilayer_table(net, data, c["semilayers"], rank, world, **c["kw"])
        else:
            table = dp.sharded_delta_loss_table(net, data, rank, world, **c["kw"])
        with open(os.path.join(outdir, "%s_rank%d.pkl" % (case, rank)), "wb") as f:
            pickle.dump(table, f)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
