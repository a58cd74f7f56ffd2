"""numpy restatement of the uint8 <-> fp32 table kernels (include/smpq.h, csrc/u8lut.hip), and the
shapes and inputs the host and GPU tests share.

Independent of the library: the table from numpy fp32 scalars, encode by ``searchsorted`` per
plane (the largest v with lut[ch][v] <= x), the grid test on bit patterns.
"""
import numpy as np

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
CS = (1, 3, 4)
NS = (1, 2)
# below, at and above the 16-element vector and the wave; odd; past one 4096-element tile
HWS = (1, 3, 15, 16, 17, 31, 33, 255, 257, 4099)


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def np_table(mean=MEAN, std=STD):
    """(u / 255 - mean) / std in fp32, one rounding per operator: ToTensor then Normalize."""
    t = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.stack([(t - np.float32(m)) / np.float32(s) for m, s in zip(mean, std)]).astype(np.float32)


def np_table_fused(mean=MEAN, std=STD):
    """The one-multiply-add affine restatement u * (1 / (255 std)) - mean / std, in fp32: what a
    kernel that recomputed instead of looking up would produce."""
    u = np.arange(256, dtype=np.float32)
    return np.stack([u * np.float32(1.0 / (255.0 * s)) + np.float32(-m / s) for m, s in zip(mean, std)]).astype(
        np.float32)


def case_table(c):
    """A valid table for any c in 1..4: the ImageNet rows, then a row through +0.0 with a step that
    is no power of two."""
    rows = [np_table()[i] for i in range(3)] + [((np.arange(256, dtype=np.float32) - 100) * np.float32(0.37))]
    return np.ascontiguousarray(np.stack(rows[:c] if c != 1 else rows[3:4]), dtype=np.float32)


def np_decode(u, lut):
    n, c = u.shape[:2]
    flat = u.reshape(n, c, -1)
    x = np.empty(flat.shape, np.float32)
    for ch in range(c):
        x[:, ch] = lut[ch][flat[:, ch]]
    return x.reshape(u.shape)


def np_encode(x, lut):
    """(u, bad): u = largest v with lut[ch][v] <= x, 0 if none or NaN; bad = count of elements
    whose bits differ from lut[ch][u]'s."""
    n, c = x.shape[:2]
    flat = x.reshape(n, c, -1)
    u = np.empty(flat.shape, np.uint8)
    for ch in range(c):
        v = flat[:, ch]
        idx = np.searchsorted(lut[ch], v, side="right").astype(np.int64) - 1  # NaN sorts last: fixed below
        idx = np.where(np.isnan(v), 0, np.clip(idx, 0, 255))
        u[:, ch] = idx.astype(np.uint8)
    back = np_decode(u.reshape(x.shape), lut)
    return u.reshape(x.shape), int((u32(back) != u32(x)).sum())


def on_grid_case(n, c, hw, seed=0):
    """(u, x, lut) numpy arrays: random codes (0 and 255 included) and their table values."""
    rng = np.random.default_rng(seed + 1000 * n + 100 * c + hw)
    lut = case_table(c)
    u = rng.integers(0, 256, size=(n, c, hw), dtype=np.uint8)
    u.reshape(-1)[:: max(1, u.size // 7)] = 255
    u.reshape(-1)[1:: max(1, u.size // 5)] = 0
    return u, np_decode(u, lut), lut


def off_grid_case():
    """(x [2, 4, 33], lut, expected u, expected bad): an on-grid batch with one off-grid element
    of every kind planted in it. Channel 3's row contains +0.0 at v = 100."""
    u, x, lut = on_grid_case(2, 4, 33, seed=7)
    x = x.copy()
    want = u.copy()
    inf = np.float32(np.inf)
    plants = [
        # (n, ch, e, value, expected code)
        (0, 0, 0, np.nextafter(lut[0][17], inf), 17),     # one ulp above an entry
        (0, 0, 5, np.nextafter(lut[0][17], -inf), 16),    # one ulp below it
        (0, 1, 32, np.nextafter(lut[1][0], -inf), 0),     # below the row
        (0, 2, 16, np.nextafter(lut[2][255], inf), 255),  # above the row
        (1, 0, 15, np.float32(np.nan), 0),
        (1, 1, 17, inf, 255),
        (1, 2, 1, -inf, 0),
        (1, 3, 31, np.float32(-0.0), 100),                # -0.0 against the +0.0 entry: off the grid
        (0, 3, 2, np.float32(0.0), 100),                  # +0.0 itself: ON the grid (not counted)
    ]
    for i, ch, e, v, code in plants:
        x[i, ch, e] = v
        want[i, ch, e] = code
    assert u32(lut[3][100:101])[0] == 0  # the entry is +0.0
    return x, lut, want, len(plants) - 1
