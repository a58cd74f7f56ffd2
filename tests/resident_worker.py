"""Child process of tests/test_gpu_u8lut.py: the drop-in ``imagenet`` module under
SMPQ_RESIDENT_VAL=1 SMPQ_SYNTHETIC=1. Evaluates ResNet-18 twice on ``imagenet.val_loader`` (the
resident set) and twice on the plain synthetic loader it wraps, and prints one JSON line with a
digest of each evaluation (accuracy, loss, SHA-256 of every softmax tensor's bytes)."""
import hashlib
import json

import torch

import __graft_entry__

__graft_entry__.build()

import functions  # noqa: E402
import imagenet  # noqa: E402
import resnet  # noqa: E402
from smpq import assignments  # noqa: E402
from smpq.batches import ResidentSet  # noqa: E402


def digest(result):
    acc, loss, outs = result
    h = hashlib.sha256()
    for p in outs:
        h.update(p.cpu().numpy().tobytes())
    return [acc, loss, len(outs), h.hexdigest()]


def main():
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    net = resnet.resnet18().to(dev).eval()
    assignments.apply_assignment(net, "r18_u8")
    rs = imagenet.val_loader
    assert isinstance(rs, ResidentSet) and isinstance(rs.loader, imagenet.SyntheticImageNet)
    resident = [digest(functions.evaluate_acc_loss_softmax(net, dev, rs)) for _ in range(2)]
    plain = [digest(functions.evaluate_acc_loss_softmax(net, dev, rs.loader)) for _ in range(2)]
    print(json.dumps({"resident": resident, "plain": plain, "report": rs.report(), "max_bytes": rs.max_bytes}))


if __name__ == "__main__":
    main()
