#!/usr/bin/env python3
"""LDS bank conflicts of the narrow-channel conv kernel's activation fragment reads
(csrc/conv_narrow.hip), by the enumeration of tools/halo_conflicts.py: for a channel slab of cwc 16-B
chunks, a kernel size and a stride, every K step and pixel fragment, the worst extra LDS cycles of one
ds_read_b128 over the gfx950 lane groups, for the patch image the kernel stages: pixel (pr, pc) at
16 * (pr * RP + pc * PP). narrow_pitch() restates the kernel's choice of (PP, RP): of pixel pitches
cwc .. cwc + 2 and up to 15 chunks of row padding, the pair with the fewest conflicts, then the
smallest image that fits 160 KB. Pure host arithmetic, no GPU.

    python tools/narrow_conflicts.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from halo_conflicts import extra_cycles  # noqa: E402

LDS_MAX = 160 * 1024


def patch_edge(taps, stride):
    return 8 if taps == 1 else 7 * stride + 3


def worst(cwc, taps, stride, pp, rp):
    w = 0
    for j in range((taps * cwc + 3) // 4):
        for pf in range(4):
            def addr(lane):
                frow, kk = lane & 15, 4 * j + (lane >> 4)
                tap, sub = divmod(kk, cwc)
                off = (tap // 3) * rp + (tap % 3) * pp + sub if tap < taps else 0
                return 16 * (stride * (2 * pf + (frow >> 3)) * rp + stride * (frow & 7) * pp + off)
            w = max(w, extra_cycles(addr))
    return w


def patch_bytes(pw, rp):
    return (3 * pw * rp * 16 + 1023) // 1024 * 1024


def narrow_pitch(cwc, taps, stride):
    pw = patch_edge(taps, stride)
    cand = [(worst(cwc, taps, stride, p, r), r, p) for p in range(cwc, cwc + 3) for r in range(pw * p, pw * p + 16)
            if patch_bytes(pw, r) <= LDS_MAX]
    return min(cand, key=lambda c: (c[0], c[1])) if cand else None


if __name__ == "__main__":
    for taps, stride in ((9, 1), (9, 2), (1, 1)):
        pw = patch_edge(taps, stride)
        for cwc in range(1, 14):
            best = narrow_pitch(cwc, taps, stride)
            if best is None:
                print("taps %d stride %d slab %3d ch: no patch image fits LDS (the kernel walks narrower slabs)"
                      % (taps, stride, 16 * cwc))
                continue
            extra, rp, pp = best
            print("taps %d stride %d slab %3d ch: pitch (%2d, %3d) chunks, %3d KB, extra cycles %d (unpadded: %d)"
                  % (taps, stride, 16 * cwc, pp, rp, patch_bytes(pw, rp) // 1024, extra,
                     worst(cwc, taps, stride, cwc, pw * cwc)))
