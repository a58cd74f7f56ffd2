"""uint8 images through a per-channel table on the device (csrc/u8lut.hip) and the resident
evaluation set built on it (smpq.batches.ResidentSet).

The kernels run on views at every byte alignment inside a larger pre-filled byte buffer: bit for
bit against the host twins, every byte outside the view untouched, the same result under two
fills. ResidentSet under ResNet-18: three evaluations read the loader once and equal the plain
loader's bit for bit; raw batches, abandoned passes, max_bytes, shards, and the drop-in
``imagenet`` switch in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import u8lut_ref as ref
from conftest import PKG_DIR, REPO

pytestmark = pytest.mark.gpu

PAD = 256            # guard bytes on each side of a view (the views start at PAD + offset)
FILLS = (0x5A, 0xC3)


def _arena(gpu, nbytes, fill):
    buf = torch.full((2 * PAD + 16 + nbytes,), fill, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    return buf


def _outside_untouched(buf, start, nbytes, fill):
    return bool(((buf[:start] == fill).all() & (buf[start + nbytes:] == fill).all()).item())


@pytest.mark.parametrize("c", ref.CS)
@pytest.mark.parametrize("n", ref.NS)
def test_device_kernels_match_host_twins_at_every_alignment(gpu, n, c):
    from smpq import ops
    for hw in ref.HWS:
        u, x, lut = ref.on_grid_case(n, c, hw)
        if hw == 33 and c == 4 and n == 2:
            x, lut, _, _ = ref.off_grid_case()  # the off-grid kinds, on the device too
        tl = torch.from_numpy(lut)
        xh = torch.from_numpy(x)
        h_u, h_bad = ops.u8lut_encode(xh, tl)           # the host twins: the expected bits
        h_x = ops.u8lut_decode(h_u, tl)
        numel = x.size
        ld, xd = tl.to(gpu), xh.to(gpu)
        want_u, want_x = h_u.to(gpu), h_x.to(gpu).view(torch.int32)  # (bits: x may hold a NaN)
        src = _arena(gpu, numel, 0)
        for uo in range(16):
            # encode into a uint8 view at byte offset uo
            got = []
            for fill in FILLS:
                buf = _arena(gpu, numel, fill)
                out = buf[PAD + uo:PAD + uo + numel].view(x.shape)
                res, bad = ops.u8lut_encode(xd, ld, out=out)
                assert res is out and int(bad.item()) == int(h_bad.item())
                assert _outside_untouched(buf, PAD + uo, numel, fill), ("encode", hw, uo, fill)
                got.append(out.clone())
            assert torch.equal(got[0], got[1]) and torch.equal(got[0], want_u), ("encode", hw, uo)
            # decode from a uint8 view at byte offset uo into fp32 views at byte offsets 0, 4, 8, 12
            uin = src[PAD + uo:PAD + uo + numel].view(x.shape)
            uin.copy_(want_u)
            for xo in (0, 4, 8, 12):
                got = []
                for fill in FILLS:
                    buf = _arena(gpu, 4 * numel, fill)
                    out = buf[PAD + xo:PAD + xo + 4 * numel].view(torch.float32).view(x.shape)
                    assert ops.u8lut_decode(uin, ld, out=out) is out
                    assert _outside_untouched(buf, PAD + xo, 4 * numel, fill), ("decode", hw, uo, xo, fill)
                    got.append(out.view(torch.int32).clone())
                assert torch.equal(got[0], got[1]) and torch.equal(got[0], want_x), ("decode", hw, uo, xo)
            assert torch.equal(uin, want_u)  # the input is only read


def test_device_wrappers_validate(gpu):
    from smpq import ops
    lut = ops.u8lut_table().to(gpu)
    u = torch.zeros(2, 3, 8, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        ops.u8lut_decode(u.cpu(), lut)                      # images and table on different devices
    with pytest.raises(ValueError):
        ops.u8lut_decode(u, lut, out=torch.zeros(2, 3, 8))  # out on another device
    bad = lut.clone()
    bad[2, 9] = bad[2, 8]
    with pytest.raises(ValueError):
        ops.u8lut_decode(u, bad)                            # a device table is validated on the host
    assert ops.u8lut_decode(u, lut).device == u.device


# ---- ResidentSet under ResNet-18 -----------------------------------------------------------------
SIZES = (4, 4, 2)  # 10 images of 3 x 64 x 64


class Counting:
    """A list loader that counts how often it is iterated."""

    def __init__(self, items):
        self.items, self.iterations = items, 0

    def __iter__(self):
        self.iterations += 1
        return iter(self.items)


def _on_grid_batches(seed=3):
    from smpq import ops
    lut = ops.u8lut_table()
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in SIZES:
        u = torch.randint(0, 256, (b, 3, 64, 64), generator=g, dtype=torch.uint8)
        out.append((ops.u8lut_decode(u, lut), torch.randint(0, 1000, (b,), generator=g)))
    return out


@pytest.fixture(scope="module")
def r18(gpu):
    from test_gpu import build_model
    return build_model(gpu, "resnet18", "r18_u8")


@pytest.fixture(scope="module")
def plain(gpu, r18):
    """The on-grid batches and three evaluations of them as a plain list loader: the reference the
    resident set has to reproduce bit for bit (computed once, never changed)."""
    import functions
    host = _on_grid_batches()
    return host, [functions.evaluate_acc_loss_softmax(r18, gpu, host) for _ in range(3)]


def _same(r, want):
    return r[0] == want[0] and r[1] == want[1] and len(r[2]) == len(want[2]) and \
        all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(r[2], want[2]))


def test_resident_set_reads_the_loader_once_and_replays_bitwise(gpu, r18, plain):
    import functions
    from smpq.batches import ResidentSet
    host, want = plain
    loader = Counting(host)
    rs = ResidentSet(loader, device=gpu)
    for k in range(3):
        assert _same(functions.evaluate_acc_loss_softmax(r18, gpu, rs), want[k]), k
    assert loader.iterations == 1
    rep = rs.report()
    nchw = 10 * 3 * 64 * 64
    assert rep["images"] == 10 and rep["u8_batches"] == 3 and rep["raw_batches"] == 0
    assert rep["resident_bytes"] == nchw and rep["fp32_bytes"] == 4 * nchw
    assert rep["off_grid_elements"] == 0
    assert rep["loader_passes"] == 1 and rep["resident_passes"] == 2
    # a pass by hand: at most two addresses, the short batch a leading view, clones equal the loader's
    ptrs, clones = [], []
    for x, y in rs:
        ptrs.append(x.data_ptr())
        clones.append((x.clone(), y.clone()))
        assert x.is_cuda and y.is_cuda and x.is_contiguous()
    assert len(set(ptrs)) <= 2 and ptrs[2] == ptrs[0]
    assert loader.iterations == 1 and rs.report()["resident_passes"] == 3
    for (x, y), (hx, hy) in zip(clones, host):
        assert torch.equal(x.cpu().view(torch.int32), hx.view(torch.int32)) and torch.equal(y.cpu(), hy)
    # invalidate(): the next pass reads the loader again and caches again
    rs.invalidate()
    assert rs.report()["resident_bytes"] == 0
    assert _same(functions.evaluate_acc_loss_softmax(r18, gpu, rs), want[0])
    assert loader.iterations == 2 and rs.report()["u8_batches"] == 3


def test_off_grid_batch_is_kept_raw(gpu, r18):
    import functions
    from smpq.batches import ResidentSet
    host = [(x.clone(), y) for x, y in _on_grid_batches()]
    px = host[1][0]
    px[2, 1, 17, 5] = float(np.nextafter(np.float32(px[2, 1, 17, 5].item()), np.float32(np.inf)))  # one pixel, one ulp
    want = [functions.evaluate_acc_loss_softmax(r18, gpu, host) for _ in range(2)]
    loader = Counting(host)
    rs = ResidentSet(loader, device=gpu)
    for k in range(2):
        assert _same(functions.evaluate_acc_loss_softmax(r18, gpu, rs), want[k])
    rep = rs.report()
    assert loader.iterations == 1
    assert rep["u8_batches"] == 2 and rep["raw_batches"] == 1 and rep["off_grid_elements"] == 1
    one = 3 * 64 * 64
    assert rep["resident_bytes"] == (4 + 2) * one + 4 * 4 * one and rep["fp32_bytes"] == 4 * 10 * one
    got = [x.clone() for x, _ in rs]
    for a, (hx, _) in zip(got, host):
        assert torch.equal(a.cpu().view(torch.int32), hx.view(torch.int32))


def test_abandoned_first_pass_caches_nothing(gpu, plain):
    from smpq.batches import ResidentSet
    host, _ = plain
    loader = Counting(host)
    rs = ResidentSet(loader, device=gpu)
    it = iter(rs)
    x, _ = next(it)
    assert torch.equal(x.cpu(), host[0][0])
    it.close()
    rep = rs.report()
    assert not rep["resident"] and rep["loader_passes"] == 0 and rep["resident_passes"] == 0
    assert len(list(rs)) == 3 and loader.iterations == 2  # started over from the loader
    assert rs.report()["resident"] and rs.report()["loader_passes"] == 1
    assert len(list(rs)) == 3 and loader.iterations == 2


def test_max_bytes_one_short_falls_back_to_the_loader(gpu, r18, plain, capfd):
    import functions
    from smpq.batches import ResidentSet
    host, want = plain
    nchw = 10 * 3 * 64 * 64
    loader = Counting(host)
    rs = ResidentSet(loader, device=gpu, max_bytes=nchw - 1)
    for k in range(2):
        assert _same(functions.evaluate_acc_loss_softmax(r18, gpu, rs), want[k])  # it does not raise
    assert loader.iterations == 2
    rep = rs.report()
    assert rep["fallback"] and not rep["resident"] and rep["resident_bytes"] == 0
    assert rep["loader_passes"] == 2 and rep["resident_passes"] == 0
    err = capfd.readouterr().err
    assert err.count("max_bytes") == 1, err  # one line, once
    # exactly enough is kept
    fits = ResidentSet(Counting(host), device=gpu, max_bytes=nchw)
    list(fits)
    assert fits.report()["resident"] and fits.report()["resident_bytes"] == nchw


def test_shards_concatenate_to_the_whole_set(gpu, plain):
    from smpq import dp
    from smpq.batches import ResidentSet
    host, _ = plain
    loader = Counting(host)
    halves = [ResidentSet(loader, device=gpu, shard=(r, 2)) for r in range(2)]
    for _ in range(2):  # the filling pass, then a resident one
        parts = [[(x.clone(), y.clone()) for x, y in rs] for rs in halves]
        for (x0, y0), (x1, y1), (hx, hy) in zip(parts[0], parts[1], host):
            assert x0.shape[0] == dp.shard_range(hx.shape[0], 0, 2)[1]
            assert torch.equal(torch.cat([x0, x1]).cpu().view(torch.int32), hx.view(torch.int32))
            assert torch.equal(torch.cat([y0, y1]).cpu(), hy)
    assert loader.iterations == 2  # once per rank
    assert sum(rs.report()["resident_bytes"] for rs in halves) == 10 * 3 * 64 * 64
    with pytest.raises(ValueError):
        ResidentSet(loader, device=gpu, shard=(2, 2))


def test_sharded_eval_takes_a_resident_set(gpu, r18, plain):
    from smpq import dp
    from smpq.batches import ResidentSet
    host, want = plain
    loader = Counting(host)
    rs = ResidentSet(loader, device=gpu, shard=(0, 1))
    for k in range(2):
        assert _same(dp.sharded_eval(r18, rs, 0, 1, device=gpu), want[k])
    assert loader.iterations == 1
    assert _same(dp.sharded_eval(r18, ResidentSet(Counting(host), device=gpu), 0, 1, device=gpu), want[0])  # no shard = (0, 1)
    with pytest.raises(ValueError):
        dp.sharded_eval(r18, ResidentSet(loader, device=gpu, shard=(1, 2)), 0, 1, device=gpu)
    with pytest.raises(ValueError):
        dp.sharded_eval(r18, rs, 0, 2, device=gpu)
    assert loader.iterations == 1  # refused before any batch was read


def test_imagenet_resident_switch_in_a_child_process(gpu):
    """SMPQ_RESIDENT_VAL=1 SMPQ_SYNTHETIC=1: two evaluations of imagenet.val_loader in a fresh child
    equal, bit for bit, those of the plain synthetic loader the module serves without the switch,
    and the loader was read once."""
    env = dict(os.environ, SMPQ_SYNTHETIC="1", SMPQ_RESIDENT_VAL="1", SMPQ_SYNTH_IMAGES="6", SMPQ_BATCH="4",
               SMPQ_RESIDENT_MAX_GB="1", PYTHONPATH=os.pathsep.join([PKG_DIR, REPO]))
    p = subprocess.run([sys.executable, os.path.join(REPO, "tests", "resident_worker.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "SMPQ_RESIDENT_VAL=1" in p.stderr and "SMPQ_SYNTHETIC=1" in p.stderr
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["resident"] == out["plain"] and len(out["plain"]) == 2
    assert out["report"]["loader_passes"] == 1 and out["report"]["resident_passes"] == 1
    assert out["report"]["images"] == 6 and out["report"]["raw_batches"] == 2  # N(0,1) images: off the grid
    assert out["max_bytes"] == 10 ** 9
