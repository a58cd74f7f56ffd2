"""3x3 small-channel stem on the host: the appended C-ABI entries and their support rule."""
import pytest


def test_stem3_symbols_exported_abi_unchanged(built_lib):
    from smpq import _lib
    for s in ("smpq_stem3_supported", "smpq_image_quantize_c4", "smpq_stem_conv3_q"):
        assert hasattr(built_lib, s) and s in _lib.EXPORTED_SYMBOLS, s
    assert built_lib.smpq_abi_version() == 7 == _lib.ABI_VERSION


# (cin, cout, kh, kw, stride, pad, limbs, wlimbs) -> supported
@pytest.mark.parametrize("geo,want", [((3, 64, 3, 3, 1, 1, 3, 3), 1), ((1, 128, 3, 3, 1, 1, 3, 3), 1),
                                      ((4, 64 * 1001, 3, 3, 1, 1, 3, 3), 1), ((5, 64, 3, 3, 1, 1, 3, 3), 0),
                                      ((0, 64, 3, 3, 1, 1, 3, 3), 0), ((3, 80, 3, 3, 1, 1, 3, 3), 0),
                                      ((3, 64, 3, 3, 2, 1, 3, 3), 0), ((3, 64, 3, 3, 1, 0, 3, 3), 0),
                                      ((3, 64, 7, 7, 1, 1, 3, 3), 0), ((3, 64, 3, 1, 1, 1, 3, 3), 0),
                                      ((3, 64, 3, 3, 1, 1, 2, 3), 0), ((3, 64, 3, 3, 1, 1, 3, 1), 0)])
def test_stem3_supported_rule(built_lib, geo, want):
    assert built_lib.smpq_stem3_supported(*geo) == want
