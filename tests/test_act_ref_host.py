"""The references of tests/act_ref.py checked against themselves (no GPU): the limb codec on every
code, quantize_ref inside the float64 bound of quantize_ideal, the restated absmax launch at the
shapes the GPU tests rely on, the max pool against torch in float64, and the image layouts."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from act_ref import (absmax_boundaries, absmax_launch, absmax_positions, c4_ref, check_quantized, edge_images,
                     maxpool_ref, quantize_ideal, quantize_ref, s2d_ref)
from lean_ref import decode, encode
from test_gpu import LIMB_QMAX, s2d_to_image_planes


def carry_codes(limbs):
    """The codes whose digits carry: +-QMAX, a low digit of -128 / 127, a negative code with zero low
    digits, and their neighbours."""
    qmax = int(LIMB_QMAX[limbs])
    base = [0, 127, 128, 129, 255, 256, 32767, 32768, 32896, 65536, 65536 - 128, 65536 + 127, 8323072 - 256]
    c = {s * (b + d) for b in base + [qmax] for d in (-1, 0, 1) for s in (-1, 1)}
    return np.array(sorted(q for q in c if abs(q) <= qmax), np.int64)


@pytest.mark.parametrize("limbs", [1, 2, 3])
def test_codec_round_trip(limbs):
    qmax = int(LIMB_QMAX[limbs])
    q = np.arange(-qmax, qmax + 1, 1 if limbs < 3 else 997, dtype=np.int64)
    q = np.concatenate([q, carry_codes(limbs)])
    planes = encode(q, limbs)
    assert planes.dtype == np.int8 and planes.shape == (limbs, q.size)
    np.testing.assert_array_equal(decode(planes), q)
    if limbs > 1:  # the carry cases really are among them
        assert (planes[0] == -128).any() and (planes[0] == 127).any()
        assert ((q < 0) & (planes[:-1] == 0).all(0)).any()
    assert decode(encode(np.array([qmax]), limbs))[0] == qmax and decode(encode(np.array([-qmax]), limbs))[0] == -qmax


@pytest.mark.parametrize("limbs", [1, 2, 3])
def test_quantize_ref_within_ideal_bound(limbs):
    g = np.random.default_rng(limbs)
    x = (g.standard_normal((4, 4096)) * np.array([1.0, 30.0, 1e-3, 1e-25])[:, None]).astype(np.float32)
    am = np.abs(x).max(1)
    check_quantized(quantize_ref(x, am, limbs), x, am, limbs)
    assert np.abs(quantize_ref(x, am, limbs)).max() == LIMB_QMAX[limbs]
    xe, ame = edge_images(64, limbs)
    codes = quantize_ref(xe, ame, limbs)
    check_quantized(codes, xe, ame, limbs)
    # ties round half to even: the scale of image 0 is exactly 1
    z, _ = quantize_ideal(xe, ame, limbs)
    np.testing.assert_array_equal(codes[0], np.rint(z[0]).astype(np.int64))
    assert (codes[0] % 2 == 0).all()
    qmax = int(LIMB_QMAX[limbs])
    assert set(codes[1][np.abs(xe[1]) > 3.0]) == {-qmax, qmax}
    assert not codes[3].any()
    np.testing.assert_array_equal(codes[4], np.sign(xe[4]).astype(np.int64) * qmax)  # the tiny range
    assert np.abs(codes[5]).max() == qmax and (np.abs(codes[5]) == qmax).sum() > 1    # the static range clamps


def test_absmax_launch_values():
    # the shapes of test_gpu_act_helpers.py: between them every loop of absmax_kernel runs twice
    want = {(1024, 9728): ("vector", 2, 2), (300, 16384): ("vector", 1, 0), (3, 2240): ("vector", 0, 1),
            (2, 4551): ("scalar", 0, 4), (1, 12): ("vector", 0, 1)}
    want.update({(5, per): ("scalar", 0, 1) for per in (1, 2, 3, 5, 7)})
    for (n, per), exp in want.items():
        assert absmax_launch(n, per) == exp, (n, per)
    # (1024, 9728): one block per image, stride 1024; the second remainder pass reaches half the threads
    assert absmax_boundaries(1024, 9728) == list(range(1024, 9728, 1024)) and 9728 % 1024 == 512
    assert absmax_positions(1024, 9728)[:4] == [0, 1023, 1024, 2047] and absmax_positions(1024, 9728)[-1] == 9727
    assert absmax_boundaries(300, 16384) == [4096, 8192, 12288]
    assert absmax_boundaries(2, 4551) == [1280, 2560, 3840]
    assert absmax_positions(5, 1) == [0] and absmax_positions(3, 2240) == [0, 2239]
    # the R50 bench's input images run the unrolled body (the issue's production case)
    assert absmax_launch(256, 3 * 224 * 224)[1] >= 2


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (2, 2), (2, 9), (17, 22), (8, 8)])
def test_maxpool_ref_is_torch(hw):
    h, w = hw
    x = torch.randn(3, h, w, 5, generator=torch.Generator().manual_seed(h * 31 + w), dtype=torch.float64)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    np.testing.assert_array_equal(maxpool_ref(x.numpy()), ref)
    got32 = maxpool_ref(x.float().numpy())
    assert got32.dtype == np.float64
    np.testing.assert_array_equal(got32, F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("c", [1, 2, 3, 4])
@pytest.mark.parametrize("hw", [(2, 2), (3, 5), (40, 36)])
def test_image_layouts(hw, c):
    h, w = hw
    g = np.random.default_rng(c)
    codes = g.integers(-8323072, 8323073, (2, c, h, w))
    planes = s2d_ref(codes, 3)
    assert planes.shape == (3, 2, (h + 1) // 2, (w + 1) // 2, 16)
    img = decode(s2d_to_image_planes(planes))  # the layout as test_gpu.py states it
    np.testing.assert_array_equal(img[:, :h, :w, :c], codes.transpose(0, 2, 3, 1))
    assert not img[..., c:].any() and not img[:, h:].any() and not img[:, :, w:].any()
    p4 = c4_ref(codes)
    assert p4.shape == (3, 2, h, w, 4)
    np.testing.assert_array_equal(decode(p4)[..., :c], codes.transpose(0, 2, 3, 1))
    assert not decode(p4)[..., c:].any()
