"""Helpers of tests/test_bitpack_host.py and tests/test_gpu_bitpack.py (not a test module).

  * np_pack / np_unpack: an independent numpy implementation of format smpq-packed/1
    (include/smpq.h): the six packing conditions in numpy fp32 arithmetic, the payload through
    np.packbits(..., bitorder="little") on the per-code bit matrix;
  * the deterministic input tensors both suites share, built once per process.
"""
import functools

import numpy as np
import torch

KS = (1, 9, 27, 63, 64, 65, 576, 1153)
COUT = 12
# bits 1..8 mixed within a tensor, two channels left unquantized; rotated per k, so every width
# meets every k somewhere in the row of tensors and the odd k meet b = 3, 5, 6, 7
BITS = (1, 2, 3, 4, 5, 6, 7, 8, 0, 7, 0, 5)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def np_plan_channel(v, b, s):
    """(packed?, base, int64 codes) of one channel: conditions 1-6, each spelled out."""
    v = np.asarray(v, dtype=np.float32)
    s = np.float32(s)
    if not (1 <= b <= 8):
        return False, 0, None
    if not (np.isfinite(s) and s > 0):
        return False, 0, None
    if not np.isfinite(v).all():
        return False, 0, None
    with np.errstate(over="ignore"):
        m = np.rint(v / s)  # fp32 / fp32: IEEE fp32 division; rint: half to even
    assert m.dtype == np.float32
    if not (np.abs(m) <= 2.0 ** 23).all():
        return False, 0, None
    mi = m.astype(np.int64)
    back = mi.astype(np.float32) * s
    if not np.array_equal(u32(back), u32(v)):
        return False, 0, None
    if mi.max() - mi.min() > (1 << b) - 1:
        return False, 0, None
    return True, int(mi.min()), mi


def np_pack(w, qbits, step):
    """(mode int8 [cout], base int32 [cout], word_off int64 [cout + 1], payload uint32 [total])."""
    w = np.asarray(w, dtype=np.float32)
    cout, k = w.shape
    mode, base, chunks = np.zeros(cout, np.int8), np.zeros(cout, np.int32), []
    for c in range(cout):
        b = int(qbits[c])
        ok, m0, mi = np_plan_channel(w[c], b, step[c])
        if not ok:
            chunks.append(u32(w[c]).copy())
            continue
        mode[c], base[c] = b, m0
        u = (mi - m0).astype(np.uint32)
        bitmat = ((u[:, None] >> np.arange(b, dtype=np.uint32)) & 1).astype(np.uint8)  # [k, b], low bit first
        stream = np.zeros(-(-k * b // 32) * 32, np.uint8)
        stream[:k * b] = bitmat.reshape(-1)
        chunks.append(np.packbits(stream, bitorder="little").view("<u4").astype(np.uint32))
        assert chunks[-1].size == -(-k * b // 32)
    off = np.zeros(cout + 1, np.int64)
    off[1:] = np.cumsum([c.size for c in chunks])
    return mode, base, off, np.concatenate(chunks)


def np_unpack(payload, cout, k, mode, base, step, off):
    out = np.empty((cout, k), np.float32)
    for c in range(cout):
        words = np.asarray(payload[off[c]:off[c + 1]], dtype="<u4")
        b = int(mode[c])
        if b == 0:
            out[c] = words.view(np.float32)
            continue
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:k * b].reshape(k, b).astype(np.int64)
        u = (bits << np.arange(b)).sum(axis=1)
        out[c] = (np.int64(base[c]) + u).astype(np.float32) * np.float32(step[c])
    return out


def payload_words(t):
    """uint32 words of an ops payload (int8 bytes, any device)."""
    return t.detach().cpu().numpy().view(np.uint8).view("<u4").astype(np.uint32)


@functools.lru_cache(maxsize=None)
def quantized_tensor(k):
    """(w fp32 [COUT, k], qbits int8, step fp32), host tensors, never modified afterwards: seeded
    Gaussian channels through ops.quantize_channels_ (host quantizer, CPU semantics) at BITS
    rotated by the k's index. k = 1 cannot go through the quantizer (a one-element channel is
    constant: functions.py:40 divides by zero), so its quantized channels are put on a grid by
    hand: w = fl32(m * step) for a seeded integer m and a power-of-two-free step.

    Every quantized channel has a zero point z = round(mn / scale) != 0 (asserted here, on the
    Gaussian input; the 1-bit channels get a negative mean for it). With z == 0 the quantizer's
    rintf(t / s + 0.0) - 0.0 turns every small negative weight into -0.0, which the format keeps
    raw by its condition 5 (zero_point_zero_channel is that case)."""
    from smpq import ops
    i = KS.index(k)
    bits = np.roll(np.asarray(BITS), i)
    g = torch.Generator().manual_seed(1000 + k)
    w = (torch.randn(COUT, k, generator=g) * 0.05).contiguous()
    w[torch.from_numpy(bits == 1)] -= 0.2
    if k > 1:
        for c in np.nonzero(bits)[0]:
            mn, mx = float(w[c].min()), float(w[c].max())
            assert round(mn / ((mx - mn) / (2 ** int(bits[c]) - 1))) != 0, (k, c)
    if k == 1:
        rng = np.random.default_rng(7)
        step = np.where(bits > 0, np.float32(0.0123), np.float32(0)).astype(np.float32)
        m = rng.integers(-200, 200, size=COUT)
        wq = w.numpy().copy()
        sel = bits > 0
        wq[sel, 0] = (m[sel].astype(np.float32) * step[sel])
        return torch.from_numpy(wq), torch.from_numpy(bits.astype(np.int8)), torch.from_numpy(step)
    step = ops.quantize_channels_(w, bits.tolist(), semantics="cpu")
    return w, torch.from_numpy(bits.astype(np.int8)), step.contiguous()


@functools.lru_cache(maxsize=None)
def zero_point_zero_channel():
    """(w [2, 27], qbits, step): channel 0 a 1-bit quantization whose zero point is 0 (mn < 0 < mx,
    |mn| < mx), straight from the quantizer: its negative weights become -0.0; channel 1 the same
    values with the sign of zero cleared, which packs."""
    from smpq import ops
    v = torch.randn(27, generator=torch.Generator().manual_seed(5)) * 0.05
    if -float(v.min()) > float(v.max()):
        v = -v
    assert float(v.min()) < 0 < -float(v.min()) < float(v.max())
    w = v.reshape(1, -1).repeat(2, 1).contiguous()
    step = ops.quantize_channels_(w, [1, 1], semantics="cpu")
    assert (u32(w[0].numpy()) == 0x80000000).any()
    w[1] = w[1] + 0.0  # -0.0 + 0.0 = +0.0
    assert not (u32(w[1].numpy()) == 0x80000000).any()
    return w, torch.tensor([1, 1], dtype=torch.int8), step.contiguous()


FALLBACK_B = 3
FALLBACK_NAMES = ("control", "negative zero", "one ulp off", "span 2^b", "nan", "inf", "qbits 9", "step 0",
                  "step nan", "step inf", "control 8 bit")


@functools.lru_cache(maxsize=None)
def fallback_tensor():
    """(w [11, 27], qbits, step, raw mask): channels 0 and 10 pack; every other one breaks exactly
    one condition and must go raw."""
    from smpq import ops
    k = 27
    n = len(FALLBACK_NAMES)
    g = torch.Generator().manual_seed(77)
    w = (torch.randn(n, k, generator=g) * 0.05).contiguous()
    bits = np.array([4, 4, 4, 0, 4, 4, 4, 4, 4, 4, 8])
    step = ops.quantize_channels_(w, bits.tolist(), semantics="cpu").numpy().copy()
    w = w.numpy().copy()
    qbits = bits.astype(np.int8)
    # 1: the code 0 unpacks to +0.0, so a -0.0 must not pack. Put the channel on a grid through 0.
    step[1] = np.float32(0.25)
    w[1] = (np.arange(k) % 9 - 4).astype(np.float32) * step[1]
    w[1, 4] = np.float32(-0.0)
    assert u32(w[1, 4:5])[0] == 0x80000000
    # 2: one value one ulp off its grid point
    w[2, 5] = np.nextafter(w[2, 5], np.float32(np.inf), dtype=np.float32)
    # 3: codes 0 .. 2^b (2^b + 1 levels) under recorded bit b
    qbits[3] = FALLBACK_B
    step[3] = np.float32(0.125)
    w[3] = (np.arange(k) % ((1 << FALLBACK_B) + 1)).astype(np.float32) * step[3]
    w[4, 3] = np.float32(np.nan)
    w[5, 26] = np.float32(-np.inf)
    qbits[6] = 9
    step[7] = np.float32(0)
    step[8] = np.float32(np.nan)
    step[9] = np.float32(np.inf)
    raw = np.ones(n, bool)
    raw[[0, 10]] = False
    return torch.from_numpy(w), torch.from_numpy(qbits), torch.from_numpy(step), raw
