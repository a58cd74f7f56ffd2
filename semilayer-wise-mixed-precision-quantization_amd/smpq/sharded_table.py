"""A delta-loss table with its trials shared among the GPUs of one node.

    python -m smpq.sharded_table --arch resnet18|resnet34|resnet50 (--weights FILE | --pretrained) --gpus N
        [--devices 0,1,...] [--bits 8,6,4] [--lnums 1,2,...] [--suffix] [--rows] [--suffix-gb X]
        --out CSV [--report JSON] [--timeout S]

The parent process never opens the GPU. It starts N fresh child processes of this module, one per
entry of ``--devices`` (default 0..N-1; an index may repeat, so two ranks can share a GPU), gives
them a gloo rendezvous on 127.0.0.1 on a free port, used only for the one gather of the parts (host
objects), and polls them: when a child exits nonzero, or ``--timeout`` seconds have passed, the
others are killed and the parent exits nonzero. Nothing is ever restarted.

Each child builds the model (``--weights``: a ``.smpq`` file through checkpoint.load_packed, any
other through checkpoint.load_checkpoint), takes the WHOLE evaluation set from ``imagenet.val_loader``
as the environment defines it (SMPQ_SYNTHETIC, SMPQ_IMAGENET_ROOT, ...), kept on its device as a
ResidentSet, runs dp.sharded_delta_loss_table and, as rank 0, writes the table
(sensitivity.write_csv) and the merged report.

Of the engine's knobs the command line sets only the static range mode (the tables need it). The
graph switch (SMPQ_GRAPH, default on), the activation limb count (SMPQ_ACT_LIMBS, default 3), tile
table, streams and chunk are the environment's, inherited by every rank, as they are for a
delta_loss_table call in a process of one's own; without --suffix / --rows, SMPQ_TRIAL_SUFFIX /
SMPQ_TRIAL_ROWS decide. A table to compare with must be computed under the same settings.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

MAX_GPUS = 16  # (a rank is a process with a GPU open)
ARCHS = ("resnet18", "resnet34", "resnet50")


def _ints(text):
    try:
        return [int(v) for v in text.split(",") if v.strip() != ""]
    except ValueError:
        raise argparse.ArgumentTypeError("a comma-separated list of integers, not %r" % text) from None


def parser():
    ap = argparse.ArgumentParser(prog="python -m smpq.sharded_table", description=__doc__.split("\n\n")[0])
    ap.add_argument("--arch", required=True, choices=ARCHS)
    w = ap.add_mutually_exclusive_group(required=True)
    w.add_argument("--weights", help=".smpq: checkpoint.load_packed, anything else: checkpoint.load_checkpoint")
    w.add_argument("--pretrained", action="store_true")
    ap.add_argument("--gpus", type=int, required=True, help="number of ranks (at most %d)" % MAX_GPUS)
    ap.add_argument("--devices", type=_ints, default=None, help="device index of each rank (default 0..N-1)")
    ap.add_argument("--bits", type=_ints, default=[8, 6, 4])
    ap.add_argument("--lnums", type=_ints, default=None)
    ap.add_argument("--suffix", action="store_true")
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--suffix-gb", type=float, default=None)
    ap.add_argument("--out", required=True, help="the table, in the reference's csv layout")
    ap.add_argument("--report", default=None, help="the merged report as json")
    ap.add_argument("--timeout", type=float, default=86400.0, help="seconds for the whole run")
    ap.add_argument("--rank", type=int, default=None, help=argparse.SUPPRESS)  # a child's: set by the parent
    ap.add_argument("--port", type=int, default=None, help=argparse.SUPPRESS)
    return ap


def parse(argv=None):
    """The arguments, checked: 1 <= --gpus <= 16, one --devices entry per rank (default 0..N-1),
    none negative, a --timeout above 0. (argparse reports a violation and exits with status 2.)"""
    ap = parser()
    args = ap.parse_args(argv)
    if not 1 <= args.gpus <= MAX_GPUS:
        ap.error("--gpus must be within 1..%d, not %d" % (MAX_GPUS, args.gpus))
    if args.devices is None:
        args.devices = list(range(args.gpus))
    if len(args.devices) != args.gpus:
        ap.error("--devices lists %d devices for --gpus %d" % (len(args.devices), args.gpus))
    if min(args.devices) < 0:
        ap.error("--devices must not be negative")
    if not args.bits:
        ap.error("--bits is empty")
    if not args.timeout > 0:
        ap.error("--timeout must be above 0")
    if (args.rank is None) != (args.port is None) or (args.rank is not None and not 0 <= args.rank < args.gpus):
        ap.error("--rank and --port are set by the parent process")
    return args


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def supervise(procs, timeout, poll_s=0.1, clock=time.monotonic, sleep=time.sleep):
    """Poll ``procs`` until all have exited with 0 (returns 0), one has exited nonzero (returns its
    status) or ``timeout`` seconds have passed (returns 124); whatever still runs then is killed and
    reaped. Nothing is restarted."""
    end = clock() + timeout
    rc = 0
    try:
        while True:
            codes = [p.poll() for p in procs]
            bad = [c for c in codes if c not in (None, 0)]
            if bad:
                rc = bad[0]
                return rc
            if all(c == 0 for c in codes):
                return 0
            if clock() >= end:
                rc = 124
                return rc
            sleep(poll_s)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()


def parent(args, argv):
    pkg_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONUNBUFFERED="1")
    env["PYTHONPATH"] = os.pathsep.join([pkg_dir] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    port = free_port()
    procs = [subprocess.Popen([sys.executable, "-m", "smpq.sharded_table"] + list(argv) +
                              ["--rank", str(r), "--port", str(port)], env=env) for r in range(args.gpus)]
    rc = supervise(procs, args.timeout)
    if rc:
        print("smpq.sharded_table: status %d (a rank failed, or --timeout of %g s passed: 124); the ranks still "
              "running were ended, nothing is retried" % (rc, args.timeout), file=sys.stderr)
    return rc


def _plain(v):
    """json.dump's default: numpy scalars and arrays in a report."""
    import numpy as np
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, np.ndarray):
        return v.tolist()
    return str(v)


def child(args):
    import datetime

    import torch
    import torch.distributed as dist

    rank, world = args.rank, args.gpus
    torch.set_num_threads(max(1, 16 // world))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(args.port)
    # gloo on purpose: the one collective gathers host objects
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=args.timeout))
    try:
        dev = torch.device("cuda", args.devices[rank])
        torch.cuda.set_device(dev)
        import imagenet
        import resnet
        from smpq import checkpoint, dp, engine, sensitivity
        from smpq.batches import ResidentSet
        engine.set_range_mode("static")
        if args.pretrained:
            net = getattr(resnet, args.arch)(pretrained=True)
        else:
            net = getattr(resnet, args.arch)()
        net = net.to(dev).eval()
        if args.weights is not None:
            load = checkpoint.load_packed if args.weights.endswith(".smpq") else checkpoint.load_checkpoint
            load(net, args.weights)
        data = imagenet.val_loader
        if not isinstance(data, ResidentSet):
            data = ResidentSet(data, device=dev)
        table = dp.sharded_delta_loss_table(
            net, data, rank, world, bits=tuple(args.bits), lnums=args.lnums,
            suffix=True if args.suffix else None, rows=True if args.rows else None,  # (None: the environment's)
            suffix_bytes=None if args.suffix_gb is None else int(args.suffix_gb * (1 << 30)))
        if rank == 0:
            sensitivity.write_csv(table, args.out)
            if args.report is not None:
                with open(args.report, "w") as f:
                    json.dump(table.report(), f, indent=1, default=_plain)
                    f.write("\n")
    finally:
        dist.destroy_process_group()
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse(argv)
    return child(args) if args.rank is not None else parent(args, argv)


if __name__ == "__main__":
    sys.exit(main())
