"""uint8 images through a per-channel table on the host (include/smpq.h; smpq.ops u8lut_*): the
table against torch's own ToTensor / Normalize operators bit for bit, the native host twins against
the numpy restatement of tests/u8lut_ref.py with a bitwise round trip, every kind of off-grid
input counted exactly once, and the refusals."""
import numpy as np
import pytest
import torch

import u8lut_ref as ref
from u8lut_ref import u32


def _shapes():
    return [(n, c, hw) for c in ref.CS for n in ref.NS for hw in ref.HWS]


def test_table_is_torch_totensor_normalize_bit_for_bit(built_lib):
    from smpq import ops
    lut = ops.u8lut_table()
    assert lut.dtype == torch.float32 and lut.shape == (3, 256) and lut.is_contiguous()
    # torchvision's ToTensor (uint8 -> float32, div(255)) then Normalize (sub_(mean), div_(std)) on
    # an image holding every pixel value in every channel
    img = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 256).repeat(3, 1, 1)  # [c, h, w]
    mean = torch.as_tensor(ref.MEAN, dtype=torch.float32).view(-1, 1, 1)
    std = torch.as_tensor(ref.STD, dtype=torch.float32).view(-1, 1, 1)
    want = img.to(torch.float32).div(255).sub_(mean).div_(std).reshape(3, 256)
    assert np.array_equal(u32(lut.numpy()), u32(want.numpy()))
    assert np.array_equal(u32(lut.numpy()), u32(ref.np_table()))
    assert bool((lut[:, 1:] > lut[:, :-1]).all())  # strictly increasing: injective
    assert tuple(ops.IMAGENET_MEAN) == ref.MEAN and tuple(ops.IMAGENET_STD) == ref.STD
    # the check can fail: the fused affine form of the same formula is a different table
    fused = ref.np_table_fused()
    differ = int((u32(fused) != u32(lut.numpy())).sum())
    assert differ > 384, differ
    # other constants, one channel
    one = ops.u8lut_table([0.5], [0.25])
    assert one.shape == (1, 256) and np.array_equal(u32(one.numpy()), u32(ref.np_table([0.5], [0.25])))


@pytest.mark.parametrize("n,c,hw", _shapes(), ids=["n%d-c%d-hw%d" % s for s in _shapes()])
def test_host_twins_match_numpy_and_round_trip(built_lib, n, c, hw):
    from smpq import ops
    u, x, lut = ref.on_grid_case(n, c, hw)
    tl = torch.from_numpy(lut)
    got_x = ops.u8lut_decode(torch.from_numpy(u), tl)
    assert got_x.dtype == torch.float32 and got_x.shape == u.shape
    assert np.array_equal(u32(got_x.numpy()), u32(x))
    got_u, bad = ops.u8lut_encode(torch.from_numpy(x), tl)
    n_u, n_bad = ref.np_encode(x, lut)
    assert got_u.dtype == torch.uint8 and got_u.shape == x.shape
    assert n_bad == 0 and int(bad.item()) == 0
    assert np.array_equal(got_u.numpy(), u) and np.array_equal(n_u, u)
    # out=: written in place and returned
    out_u = torch.full(x.shape, 77, dtype=torch.uint8)
    out_x = torch.full(x.shape, 7.0)
    assert ops.u8lut_encode(torch.from_numpy(x), tl, out=out_u)[0] is out_u and np.array_equal(out_u.numpy(), u)
    assert ops.u8lut_decode(out_u, tl, out=out_x) is out_x and np.array_equal(u32(out_x.numpy()), u32(x))


def test_image_shaped_batches(built_lib):
    """[n, c, h, w] tensors: hw is everything after the channel axis."""
    from smpq import ops
    u, x, lut = ref.on_grid_case(2, 3, 35)
    u4, x4 = u.reshape(2, 3, 5, 7), x.reshape(2, 3, 5, 7)
    tl = torch.from_numpy(lut)
    assert np.array_equal(u32(ops.u8lut_decode(torch.from_numpy(u4), tl).numpy()), u32(x4))
    got, bad = ops.u8lut_encode(torch.from_numpy(x4), tl)
    assert np.array_equal(got.numpy(), u4) and int(bad.item()) == 0


def test_off_grid_elements_are_counted_once_each(built_lib):
    from smpq import ops
    x, lut, want, nbad = ref.off_grid_case()
    n_u, n_bad = ref.np_encode(x, lut)
    assert n_bad == nbad and np.array_equal(n_u, want)  # the restatement agrees with the plan
    got, bad = ops.u8lut_encode(torch.from_numpy(x), torch.from_numpy(lut))
    assert np.array_equal(got.numpy(), want)
    assert int(bad.item()) == nbad
    # *bad is increased, not overwritten (the C entry point, on a counter that already holds 5)
    from smpq import _lib
    counter = torch.full((1,), 5, dtype=torch.int32)
    out = torch.empty(x.shape, dtype=torch.uint8)
    P = _lib.ptr
    xt, lt = torch.from_numpy(x), torch.from_numpy(lut)
    assert built_lib.smpq_u8lut_encode_host(P(xt), 2, 4, 33, P(lt), P(out), P(counter)) == 0
    assert int(counter.item()) == 5 + nbad and np.array_equal(out.numpy(), want)


@pytest.mark.parametrize("kind", ["equal", "decreasing", "nan", "inf"])
def test_bad_tables_are_refused(built_lib, kind):
    from smpq import _lib, ops
    lut = ref.case_table(3).copy()
    if kind == "equal":
        lut[1][40] = lut[1][39]
    elif kind == "decreasing":
        lut[2][255] = lut[2][200]
    elif kind == "nan":
        lut[0][0] = np.nan
    else:
        lut[2][255] = np.inf
    tl = torch.from_numpy(lut)
    u = torch.zeros(1, 3, 4, dtype=torch.uint8)
    x = torch.zeros(1, 3, 4)
    with pytest.raises(ValueError):
        ops.u8lut_decode(u, tl)
    with pytest.raises(ValueError):
        ops.u8lut_encode(x, tl)
    # the native twins validate for themselves
    P = _lib.ptr
    bad = torch.zeros(1, dtype=torch.int32)
    assert built_lib.smpq_u8lut_decode_host(P(u), 1, 3, 4, P(tl), P(x)) == _lib.SMPQ_E_INVALID
    assert built_lib.smpq_u8lut_encode_host(P(x), 1, 3, 4, P(tl), P(u), P(bad)) == _lib.SMPQ_E_INVALID
    # and a table changed in place after it was accepted is checked again
    good = torch.from_numpy(ref.case_table(3).copy())
    ops.u8lut_decode(u, good)
    good[1, 7] = good[1, 6]
    with pytest.raises(ValueError):
        ops.u8lut_decode(u, good)


def test_bad_shapes_and_dtypes(built_lib):
    from smpq import _lib, ops
    tl = torch.from_numpy(ref.case_table(3))
    u = torch.zeros(2, 3, 8, dtype=torch.uint8)
    x = torch.zeros(2, 3, 8)
    bad_calls = [
        lambda: ops.u8lut_decode(x, tl),                                   # fp32 where uint8 is due
        lambda: ops.u8lut_decode(u.to(torch.int8), tl),
        lambda: ops.u8lut_encode(u, tl),                                   # uint8 where fp32 is due
        lambda: ops.u8lut_encode(x.double(), tl),
        lambda: ops.u8lut_decode(torch.zeros(2, 4, 8, dtype=torch.uint8), tl),  # 4 channels, 3 rows
        lambda: ops.u8lut_decode(torch.zeros(6, dtype=torch.uint8), tl),   # no channel axis
        lambda: ops.u8lut_decode(torch.zeros(0, 3, 8, dtype=torch.uint8), tl),  # empty
        lambda: ops.u8lut_decode(u.transpose(0, 2), tl),                   # not contiguous
        lambda: ops.u8lut_encode(x[:, :, ::2], tl),
        lambda: ops.u8lut_decode(u, tl.double()),
        lambda: ops.u8lut_decode(u, tl[:, :255]),
        lambda: ops.u8lut_decode(u, tl.reshape(-1)),
        lambda: ops.u8lut_decode(u[:, :1], torch.zeros(5, 256)),           # c above 4
        lambda: ops.u8lut_decode(u, tl, out=torch.zeros(2, 3, 9)),         # out: wrong shape
        lambda: ops.u8lut_decode(u, tl, out=torch.zeros(2, 3, 8, dtype=torch.float64)),
        lambda: ops.u8lut_encode(x, tl, out=torch.zeros(2, 3, 8)),         # out: wrong dtype
        lambda: ops.u8lut_encode(x, tl, out=torch.zeros(2, 3, 16, dtype=torch.uint8)[:, :, ::2]),
        lambda: ops.u8lut_table([0.5, 0.5], [0.25]),
        lambda: ops.u8lut_table([0.5], [0.0]),                             # rows of inf / NaN
        lambda: ops.u8lut_table([0.5], [-0.25]),                           # decreasing rows
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % i)
    # the C entry points: sizes outside the contract are SMPQ_E_SHAPE before anything runs
    P = _lib.ptr
    cnt = torch.zeros(1, dtype=torch.int32)
    for n, c, hw in [(0, 3, 8), (2, 0, 8), (2, 5, 8), (2, 3, 0), (-1, 3, 8), (1 << 15, 4, 1 << 14)]:
        assert built_lib.smpq_u8lut_decode_host(P(u), n, c, hw, P(tl), P(x)) == _lib.SMPQ_E_SHAPE, (n, c, hw)
        assert built_lib.smpq_u8lut_encode_host(P(x), n, c, hw, P(tl), P(u), P(cnt)) == _lib.SMPQ_E_SHAPE
        # the device entry points check sizes on the host too, before any launch (no GPU needed)
        assert built_lib.smpq_u8lut_decode(P(u), n, c, hw, P(tl), P(x), None) == _lib.SMPQ_E_SHAPE
        assert built_lib.smpq_u8lut_encode(P(x), n, c, hw, P(tl), P(u), P(cnt), None) == _lib.SMPQ_E_SHAPE
