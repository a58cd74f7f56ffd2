"""Helpers of tests/test_gpu_act_helpers.py and tests/test_act_ref_host.py (not a test module): plain
numpy references of the activation-side helper kernels of csrc/conv.hip and csrc/conv_stem3.hip.

  * quantize_ref / quantize_ideal: the activation quantizer to the bit (the kernels' fp32 arithmetic
    restated) and in float64 with a derived bound;
  * absmax_launch / absmax_boundaries: the launch of smpq_act_absmax restated, so that a test can
    assert which loops of absmax_kernel its shape runs;
  * maxpool_ref: the 3x3 / stride 2 / pad 1 max pool on NHWC in float64;
  * s2d_ref / c4_ref: the limb planes of image_quantize_s2d and image_quantize_c4 from NCHW codes;
  * edge_images: the edge values every quantizer kernel is run on.

Limb planes <-> codes are lean_ref.encode / lean_ref.decode, the guard regions lean_ref.run_guarded.
"""
import numpy as np

from lean_ref import encode
from test_gpu import LIMB_QMAX

TINY = np.float32(2.0 ** -64)   # per-image ranges below it are scaled by 2^64 before the division
SCALE_UP = np.float32(2.0 ** 64)


def _per_image(v, x):
    return np.asarray(v, np.float32).reshape((-1,) + (1,) * (x.ndim - 1))


def quantize_ref(x, absmax, limbs):
    """The quantizer kernels' arithmetic in np.float32, in their order: int64 codes shaped like x
    (x fp32 [n, ...], absmax fp32 [n]).

        pre = 2^64 if am < 2^-64 else 1            (exact: a power of two)
        inv = fl32(qmax / fl32(am * pre)) if am > 0 else 0
        code = clamp(rint(fl32(fl32(x * pre) * inv)), -QMAX, QMAX)     rint: half to even

    With pre = 1 this is qmax / am and x * inv; below 2^-64 the scaling keeps qmax / am (past FLT_MAX
    from about 2.4e-32 at 3 limbs) finite. NaN and Inf inputs are not defined."""
    x = np.asarray(x, np.float32)
    am = _per_image(absmax, x)
    assert am.shape[0] == x.shape[0] and np.isfinite(x).all() and np.isfinite(am).all() and (am >= 0).all()
    qmax = np.float32(LIMB_QMAX[limbs])
    pre = np.where(am < TINY, SCALE_UP, np.float32(1.0)).astype(np.float32)
    ams = (am * pre).astype(np.float32)
    inv = np.where(am > 0, qmax / np.where(am > 0, ams, np.float32(1.0)), np.float32(0.0)).astype(np.float32)
    with np.errstate(over="ignore"):  # a value far past a tiny range: inf, clamped
        t = ((x * pre).astype(np.float32) * inv).astype(np.float32)
    assert not np.isnan(t).any()
    return np.clip(np.rint(t), -qmax, qmax).astype(np.int64)


def quantize_ideal(x, absmax, limbs):
    """(z, tol): z = x * QMAX / am in float64 (0 where am == 0) and the bound a kernel code obeys,
    |code - clip(z, -QMAX, QMAX)| <= tol = 0.5 + |z| * (2^-23 + 2^-47).

    Derivation. The kernel computes c = fl32(x' * fl32(QMAX / am')) with x' = x * pre, am' = am * pre
    exact (pre a power of two), so x' / am' = x / am. Each of the two fp32 roundings has relative
    error at most u = 2^-24 (round to nearest, normal results): c = z (1 + d1)(1 + d2), |d1|, |d2| <=
    u, hence |c - z| <= |z| (2 u + u^2) = |z| (2^-23 + 2^-48) <= |z| (2^-23 + 2^-47). rint moves c by at
    most 0.5, and the clamp to [-QMAX, QMAX] is monotone and 1-Lipschitz, so it moves code and
    clip(z) no further apart. (The float64 evaluation of z itself errs by 2^-52 |z|: inside the
    margin between 2^-48 and 2^-47.) Nothing here is measured."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    am = _per_image(absmax, x64).astype(np.float64)
    qmax = LIMB_QMAX[limbs]
    z = np.where(am > 0, x64 * qmax / np.where(am > 0, am, 1.0), 0.0)
    return z, 0.5 + np.abs(z) * (2.0 ** -23 + 2.0 ** -47)


def check_quantized(codes, x, absmax, limbs):
    """codes (int64, shaped like x) against both references: equal to quantize_ref to the bit, inside
    the float64 bound of quantize_ideal, and 0 wherever x is +-0."""
    codes = np.asarray(codes)
    x = np.asarray(x, np.float32)
    assert codes.shape == x.shape, (codes.shape, x.shape)
    exp = quantize_ref(x, absmax, limbs)
    if not np.array_equal(codes, exp):
        bad = codes != exp
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%d of %d codes differ from quantize_ref: first at %s, x %r, code %d, expected %d"
                             % (bad.sum(), bad.size, i, float(x[i]), codes[i], exp[i]))
    z, tol = quantize_ideal(x, absmax, limbs)
    qmax = LIMB_QMAX[limbs]
    err = np.abs(codes - np.clip(z, -qmax, qmax))
    if (err > tol).any():
        i = tuple(int(v) for v in np.argwhere(err > tol)[0])
        raise AssertionError("%d codes outside the float64 bound: first at %s, x %r, code %d, ideal %.3f, bound %.3f"
                             % ((err > tol).sum(), i, float(x[i]), codes[i], z[i], tol[i]))
    assert not codes[x == 0].any(), "a zero activation must code to 0"


# ---- smpq_act_absmax's launch -------------------------------------------------------------------
def _absmax_grid(n, per_image):
    chunks = min((1024 + n - 1) // n, (per_image // 4 + 255) // 256)
    return max(chunks, 1)


def absmax_launch(n, per_image):
    """(path, unrolled_bodies, remainder_passes) of absmax_kernel's thread 0 for n images of
    per_image elements: the launcher's dim3(chunks, n) blocks of 256 threads restated. 'vector'
    (per_image % 4 == 0): each load of a thread is a float4 and the threads of an image cover
    stride = chunks * 1024 elements per load; the 4-load body runs while i + 3 stride < per_image,
    the one-load remainder loop takes the rest (its last pass may reach only some threads). 'scalar':
    one element per load, stride chunks * 256, no unrolled body."""
    chunks = _absmax_grid(n, per_image)
    if per_image % 4 == 0:
        stride = chunks * 1024
        i = bodies = 0
        while i + 3 * stride < per_image:
            bodies += 1
            i += 4 * stride
        return "vector", bodies, len(range(i, per_image, stride))
    return "scalar", 0, len(range(0, per_image, chunks * 256))


def absmax_boundaries(n, per_image):
    """The element indices at which another load of absmax_kernel begins (the multiples of the
    stride inside the image): the loop boundaries absmax_launch counts, body loads and remainder
    passes alike, and the first element no thread of the last pass's full width would reach."""
    path, bodies, rem = absmax_launch(n, per_image)
    stride = _absmax_grid(n, per_image) * (1024 if path == "vector" else 256)
    b = list(range(stride, per_image, stride))
    assert len(b) == max(4 * bodies + rem - 1, 0)
    return b


def absmax_positions(n, per_image):
    """Where the tests put an image's maximum: 0, per_image - 1 and both sides of every boundary."""
    pos = {0, per_image - 1}
    for b in absmax_boundaries(n, per_image):
        pos.update((b - 1, b))
    return sorted(pos)


# ---- max pool -----------------------------------------------------------------------------------
def maxpool_ref(x):
    """MaxPool2d(3, stride 2, pad 1) on NHWC [n, h, w, c] in float64 -> [n, ho, wo, c] (padding never
    wins: every window holds its centre (2 oh, 2 ow))."""
    x = np.asarray(x)
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = np.full((n, ho, wo, c), -np.inf, np.float64)
    for dr in (-1, 0, 1):
        for dc in (-1, 0, 1):
            # outputs whose tap (2 oh + dr, 2 ow + dc) is inside the image
            oh0, ow0 = (1 if dr < 0 else 0), (1 if dc < 0 else 0)
            oh1, ow1 = min(ho, (h - 1 - dr) // 2 + 1), min(wo, (w - 1 - dc) // 2 + 1)
            if oh1 <= oh0 or ow1 <= ow0:
                continue
            tap = x[:, 2 * oh0 + dr:2 * (oh1 - 1) + dr + 1:2, 2 * ow0 + dc:2 * (ow1 - 1) + dc + 1:2]
            np.maximum(out[:, oh0:oh1, ow0:ow1], tap.astype(np.float64), out=out[:, oh0:oh1, ow0:ow1])
    assert np.isfinite(out).all()
    return out


# ---- image layouts ------------------------------------------------------------------------------
def c4_ref(codes, limbs=3):
    """NCHW codes [n, c <= 4, h, w] -> image_quantize_c4's planes int8 [limbs, n, h, w, 4]: byte ch of
    a pixel = channel ch, zero for ch >= c."""
    codes = np.asarray(codes, np.int64)
    n, c, h, w = codes.shape
    assert 1 <= c <= 4
    img = np.zeros((n, h, w, 4), np.int64)
    img[..., :c] = codes.transpose(0, 2, 3, 1)
    return encode(img, limbs)


def s2d_ref(codes, limbs):
    """NCHW codes [n, c <= 4, h, w] -> image_quantize_s2d's planes int8 [limbs, n, ceil(h/2),
    ceil(w/2), 16]: channel (dy * 2 + dx) * 4 + ch of pixel (i, j) = image pixel (2 i + dy, 2 j + dx),
    channel ch; zero for ch >= c and for the row / column past an odd h / w."""
    codes = np.asarray(codes, np.int64)
    n, c, h, w = codes.shape
    assert 1 <= c <= 4
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    img = np.zeros((n, 2 * h2, 2 * w2, 4), np.int64)
    img[:, :h, :w, :c] = codes.transpose(0, 2, 3, 1)
    s2d = img.reshape(n, h2, 2, w2, 2, 4).transpose(0, 1, 3, 2, 4, 5).reshape(n, h2, w2, 16)
    return encode(s2d, limbs)


# ---- edge values --------------------------------------------------------------------------------
EDGE_IMAGES = 6


def edge_images(per_image, limbs, seed=0):
    """(x fp32 [6, per_image], absmax fp32 [6]): the values a quantizer kernel can get wrong, each
    image's pattern repeated to per_image (>= 64) elements.

      0  ties k + 0.5 under absmax = QMAX (the scale is exactly 1): k even and odd, both signs, next to
         0 and next to QMAX;
      1  values at 1.5 x and 100 x the range, both signs (codes exactly +-QMAX), among in-range ones;
      2  +0.0 and -0.0 among ordinary values;
      3  an all-zero image with absmax 0;
      4  absmax 1e-33: zeros and +-1e-33 (QMAX / absmax is past FLT_MAX at 3 limbs);
      5  a passed range half the data's maximum, as the static mode passes."""
    assert per_image >= 64
    qmax = LIMB_QMAX[limbs]
    ks = np.array([0, 1, 2, 3, 4, 5, 126, qmax - 2, qmax - 1], np.float64)
    ties = np.concatenate([ks + 0.5, -(ks + 0.5)])
    assert ((ties.astype(np.float32)).astype(np.float64) == ties).all()  # exact in fp32
    rng = np.random.default_rng(seed)
    tiny = np.float32(1e-33)
    pats = [
        ties,
        np.array([4.5, -4.5, 300.0, -300.0, 3.0, -3.0, 1.0, -2.9999998, 0.25, 3.0000002]),
        np.array([0.0, -0.0, 0.5, -0.0, 0.0, -1.0, 1e-30, -0.0]),
        np.zeros(1),
        np.array([0.0, tiny, -tiny, -0.0, 0.0, tiny, 0.0, -tiny]),
        rng.standard_normal(64),
    ]
    x = np.stack([np.resize(p, per_image) for p in pats]).astype(np.float32)
    am = np.array([qmax, 3.0, 1.0, 0.0, tiny, 0.5 * np.abs(x[5]).max()], np.float32)
    assert x.shape[0] == EDGE_IMAGES and np.signbit(x[2]).any() and (np.abs(x[5]) > am[5]).any()
    return x, am
