#!/usr/bin/env python3
"""LDS bank conflicts of the wide-group 3x3 kernel's B-fragment reads (csrc/conv_grouped_wide.hip), counted as
tools/halo_conflicts.py counts them: for both strides, every tap, pixel fragment and ds_read_b128 lane group of
gfx950, the extra LDS cycles of the stage image [ri][ci][64 B] with the 16-B chunk c at c ^ 2 (ri & 1), where
patch row pr is image row pr (stride 1) or 9 (pr & 1) + (pr >> 1) (stride 2, columns likewise); next to it the
plain row-major image without the XOR. Pure host arithmetic, no GPU.

    python tools/grouped_wide_conflicts.py"""
from halo_conflicts import extra_cycles


def idx(stride, p):
    return p if stride == 1 else 9 * (p & 1) + (p >> 1)


def worst(stride, kernel_image):
    pw = 7 * stride + 3
    w = 0
    for pf in range(4):
        for kr in range(3):
            for kc in range(3):
                def addr(lane):
                    frow, grp = lane & 15, lane >> 4
                    pr, pc = stride * (2 * pf + (frow >> 3)) + kr, stride * (frow & 7) + kc
                    if not kernel_image:
                        return (pr * pw + pc) * 64 + 16 * grp
                    ri, ci = idx(stride, pr), idx(stride, pc)
                    return (ri * pw + ci) * 64 + 16 * (grp ^ (2 * (ri & 1)))
                w = max(w, extra_cycles(addr))
    return w


if __name__ == "__main__":
    for stride in (1, 2):
        print("stride %d: extra cycles per read, worst case: %d (plain row-major image: %d)"
              % (stride, worst(stride, True), worst(stride, False)))
