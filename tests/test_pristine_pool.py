"""The pristine-model pool of smpq.models (SMPQ_PRISTINE_POOL / set_pristine_pool): later
``resnetNN(pretrained=...)`` calls for the same local weight file build the module tree without
parameter initialisation and load a private host copy of the first call's state. The ground truth
is the normally constructed model (pool off)."""
import os

import numpy as np
import pytest
import torch


def _write_weights(dirname, seed):
    """A seeded ResNet-18 state dict under the file name the pretrained branch reads, in the form
    of the published checkpoint: no quantization metadata, no num_batches_tracked."""
    import resnet
    torch.manual_seed(seed)
    sd = {k: v for k, v in resnet.resnet18().state_dict().items()
          if not k.endswith(("qbits", "qstep", "num_batches_tracked"))}
    g = torch.Generator().manual_seed(seed + 1)
    for k, v in sd.items():  # BN statistics that are not the constructor's constants
        if k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    path = os.path.join(dirname, os.path.basename(resnet.MODEL_URLS["resnet18"]))
    torch.save(sd, path)
    return path


@pytest.fixture
def pool(tmp_path, monkeypatch):
    from smpq import models
    monkeypatch.setenv("SMPQ_PRETRAINED_DIR", str(tmp_path))
    _write_weights(str(tmp_path), 7)
    models.clear_pristine_pool()
    models.set_pristine_pool(True)
    yield models
    models.set_pristine_pool(False)
    models.clear_pristine_pool()


def _same_state(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].shape == sb[k].shape and sa[k].device == sb[k].device, k
        assert torch.equal(sa[k], sb[k]), k


def _ptrs(m):
    return {t.data_ptr() for t in m.state_dict().values()}


def test_pooled_model_equals_the_normal_one(pool):
    import resnet
    pool.set_pristine_pool(False)
    normal = resnet.resnet18(pretrained="imagenet")
    assert pool.pristine_pool_report()["entries"] == 0 and pool.pristine_pool_report()["misses"] == 0
    pool.set_pristine_pool(True)
    first = resnet.resnet18(pretrained="imagenet")
    rep = pool.pristine_pool_report()
    assert rep["misses"] == 1 and rep["hits"] == 0 and rep["entries"] == 1 and rep["bytes"] > 4 * 11e6
    rng = torch.get_rng_state()
    second = resnet.resnet18(pretrained="imagenet")
    third = resnet.resnet18(pretrained="imagenet")
    assert torch.equal(rng, torch.get_rng_state())  # the pooled path draws nothing from the global generator
    assert pool.pristine_pool_report()["hits"] == 2
    for m in (first, second, third):
        _same_state(m, normal)
        assert all(t.device.type == "cpu" for t in m.state_dict().values())
        for c in m.modules():
            if isinstance(c, pool.QConv2d):
                assert c._bits_host.dtype == np.int16 and c._bits_host.shape == (c.out_channels,)
                assert not c._bits_host.any() and not c.qbits.any() and not c.qstep.any()
    assert second.bn1.num_batches_tracked.item() == 0 and second.bn1.num_batches_tracked.dtype == torch.int64
    assert second.training == normal.training and type(second) is type(normal)
    assert [n for n, _ in second.named_modules()] == [n for n, _ in normal.named_modules()]
    # no storage shared: among the models, or with the master
    master = next(iter(pool._POOL.values()))
    sets = [_ptrs(first), _ptrs(second), _ptrs(third), {t.data_ptr() for t in master.values()}]
    for i in range(len(sets)):
        for j in range(i + 1, len(sets)):
            assert sets[i].isdisjoint(sets[j]), (i, j)
    with torch.no_grad():
        for t in second.state_dict().values():
            t.add_(1)
    _same_state(third, normal)
    _same_state(resnet.resnet18(pretrained="imagenet"), normal)  # the master is unchanged
    # the quantizer finds a pooled model's convs (QConv2d's registry), as it finds a normal one's
    from smpq.qconv import find_owner
    conv = third.layer1[0].conv1
    assert find_owner(conv.weight.data) is conv


def test_keyword_arguments_are_part_of_the_key(pool):
    import resnet
    a = resnet.resnet18(pretrained="imagenet")
    b = resnet.resnet18(pretrained="imagenet", num_classes=1000)
    c = resnet.resnet18(pretrained="imagenet", zero_init_residual=True)
    rep = pool.pristine_pool_report()
    assert rep["entries"] == 3 and rep["misses"] == 3 and rep["hits"] == 0
    _same_state(a, b)
    _same_state(a, c)
    resnet.resnet18(pretrained="imagenet", num_classes=1000)
    assert pool.pristine_pool_report()["hits"] == 1


def test_rewritten_file_is_read_again(pool, tmp_path):
    import resnet
    a = resnet.resnet18(pretrained="imagenet")
    path = _write_weights(str(tmp_path), 8)
    st = os.stat(path)
    os.utime(path, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))  # whatever the clock's grain
    b = resnet.resnet18(pretrained="imagenet")
    assert not torch.equal(a.conv1.weight, b.conv1.weight)
    rep = pool.pristine_pool_report()
    assert rep["misses"] == 2 and rep["entries"] == 1  # the old file's master is dropped
    pool.set_pristine_pool(False)
    _same_state(b, resnet.resnet18(pretrained="imagenet"))
    pool.set_pristine_pool(True)
    _same_state(resnet.resnet18(pretrained="imagenet"), b)
    assert pool.pristine_pool_report()["hits"] == 1


def test_unpretrained_models_are_untouched(pool):
    import resnet
    torch.manual_seed(3)
    on = resnet.resnet18()
    on_rng = torch.get_rng_state()
    pool.set_pristine_pool(False)
    torch.manual_seed(3)
    off = resnet.resnet18()
    assert torch.equal(on_rng, torch.get_rng_state())
    _same_state(on, off)
    rep = pool.pristine_pool_report()
    assert rep["entries"] == 0 and rep["hits"] == 0 and rep["misses"] == 0


def test_pool_off_is_the_parent_path(pool):
    """Off: every call initialises (the global generator advances) and reads the file; nothing is kept."""
    import resnet
    pool.set_pristine_pool(False)
    torch.manual_seed(5)
    a = resnet.resnet18(pretrained="imagenet")
    rng = torch.get_rng_state()
    b = resnet.resnet18(pretrained="imagenet")
    assert not torch.equal(rng, torch.get_rng_state())
    _same_state(a, b)
    assert pool.pristine_pool_report() == {"hits": 0, "misses": 0, "enabled": False, "entries": 0, "bytes": 0}
    torch.manual_seed(5)
    pool.ResNet(pool.BasicBlock, [2, 2, 2, 2])  # the initialisation _resnet runs before it loads the file
    assert torch.equal(rng, torch.get_rng_state())


@pytest.mark.gpu
def test_pooled_model_hits_the_first_models_memo_entry(gpu, pool):
    """A pooled fresh model's evaluation is answered from the entry the first model left, and it
    equals the first model's unmemoised evaluation bit for bit."""
    import functions
    import resnet
    from smpq import memo, ops, stats
    from smpq.batches import ResidentSet
    g = torch.Generator().manual_seed(41)
    lut = ops.u8lut_table()
    host = [(ops.u8lut_decode(torch.randint(0, 256, (8, 3, 224, 224), generator=g, dtype=torch.uint8), lut),
             torch.randint(0, 1000, (8,), generator=g)) for _ in range(2)]
    first = resnet.resnet18(pretrained="imagenet")
    was = memo.enabled()
    memo.clear()
    try:
        memo.disable()
        rs = ResidentSet(host, device=gpu)
        want = functions.evaluate_acc_loss_softmax(first, gpu, rs)  # unmemoised; fills the set
        memo.enable()
        assert _same_eval(functions.evaluate_acc_loss_softmax(first, gpu, rs), want)  # a miss, recorded
        assert memo.report()["misses"] == 1 and memo.report()["entries"] == 1
        fresh = resnet.resnet18(pretrained="imagenet")
        assert pool.pristine_pool_report()["hits"] == 1
        convs = stats["hip_conv"]
        got = functions.evaluate_acc_loss_softmax(fresh, gpu, rs)
        assert memo.report()["hits"] == 1 and stats["hip_conv"] == convs
        assert _same_eval(got, want)
        memo.disable()
        assert _same_eval(functions.evaluate_acc_loss_softmax(fresh, gpu, rs), want)  # its own forward
    finally:
        memo.clear()
        memo.enable() if was else memo.disable()


def _same_eval(r, want):
    return r[0] == want[0] and r[1] == want[1] and len(r[2]) == len(want[2]) and \
        all(torch.equal(a, b) for a, b in zip(r[2], want[2]))
