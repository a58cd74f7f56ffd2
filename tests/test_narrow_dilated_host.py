"""Dilated narrow-channel 3x3 conv on the host: the appended C-ABI entries and their support rule."""
import pytest


def test_narrow_dilated_symbols_exported_abi_unchanged(built_lib):
    from smpq import _lib
    for s in ("smpq_conv2d_narrow_dilated_supported", "smpq_conv2d_narrow_dilated_fwd_q"):
        assert hasattr(built_lib, s) and s in _lib.EXPORTED_SYMBOLS, s
    assert built_lib.smpq_abi_version() == 7 == _lib.ABI_VERSION


def test_stride1_slab_boundary(built_lib):
    # the kernel runs on narrow_geo(cin, 3x3, stride 1): 34 chunks (cin 544) are the widest single slab, 35 are
    # slabs of 34 + 1 (the GPU test's two slab-boundary shapes)
    steps = [built_lib.smpq_weights_narrow_expand_bytes(3, 16, 16 * cc, 3, 3, 1) // (3 * 1024) for cc in (34, 35)]
    assert steps == [77, 77 + 3]


# (cin, cout, kh, kw, stride, pad, dilation, limbs, wlimbs) -> supported here, by the dense dilated kernel.
# cin 64 and cin 192 = 3 * 64 (the layer-3 width at width_per_group 48) are the dense dilated kernel's and stay
# there; 96 is that model's layer-2 width
@pytest.mark.parametrize("geo,want,dense", [
    ((48, 48, 3, 3, 1, 2, 2, 3, 1), 1, 0), ((96, 96, 3, 3, 1, 4, 4, 3, 3), 1, 0), ((16, 16, 3, 3, 1, 8, 8, 3, 1), 1, 0),
    ((64, 64, 3, 3, 1, 2, 2, 3, 1), 0, 1), ((192, 192, 3, 3, 1, 4, 4, 3, 3), 0, 1), ((24, 64, 3, 3, 1, 2, 2, 3, 1), 0, 0),
    ((48, 40, 3, 3, 1, 2, 2, 3, 1), 0, 0), ((48, 48, 3, 3, 1, 3, 3, 3, 1), 0, 0), ((48, 48, 3, 3, 1, 1, 2, 3, 1), 0, 0),
    ((48, 48, 3, 3, 2, 2, 2, 3, 1), 0, 0), ((48, 48, 1, 1, 1, 2, 2, 3, 1), 0, 0), ((48, 48, 3, 3, 1, 2, 2, 2, 1), 0, 0),
    ((48, 48, 3, 3, 1, 2, 2, 3, 2), 0, 0)])
def test_narrow_dilated_supported_rule(built_lib, geo, want, dense):
    assert built_lib.smpq_conv2d_narrow_dilated_supported(*geo) == want
    assert built_lib.smpq_conv2d_dilated_supported(*geo) == dense  # what it was: no conv has two kernels
