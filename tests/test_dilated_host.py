"""Dilated conv on the host: the appended C-ABI entries and their support rule."""
import pytest


def test_dilated_symbols_exported_abi_unchanged(built_lib):
    from smpq import _lib
    for s in ("smpq_conv2d_dilated_supported", "smpq_conv2d_dilated_fwd_q"):
        assert hasattr(built_lib, s) and s in _lib.EXPORTED_SYMBOLS, s
    assert built_lib.smpq_abi_version() == 7 == _lib.ABI_VERSION


# (cin, cout, kh, kw, stride, pad, dilation, limbs, wlimbs) -> supported
@pytest.mark.parametrize("geo,want", [((256, 256, 3, 3, 1, 2, 2, 3, 1), 1), ((512, 512, 3, 3, 1, 4, 4, 3, 3), 1),
                                      ((64, 128, 3, 3, 1, 8, 8, 3, 3), 1), ((256, 256, 3, 3, 1, 1, 1, 3, 1), 0),
                                      ((256, 256, 3, 3, 1, 3, 3, 3, 1), 0), ((256, 256, 3, 3, 1, 16, 16, 3, 1), 0),
                                      ((256, 256, 3, 3, 2, 2, 2, 3, 1), 0), ((256, 256, 3, 3, 1, 1, 2, 3, 1), 0),
                                      ((256, 256, 5, 5, 1, 2, 2, 3, 1), 0), ((256, 256, 3, 1, 1, 2, 2, 3, 1), 0),
                                      ((96, 256, 3, 3, 1, 2, 2, 3, 1), 0), ((256, 80, 3, 3, 1, 2, 2, 3, 1), 0),
                                      ((256, 256, 3, 3, 1, 2, 2, 2, 1), 0), ((256, 256, 3, 3, 1, 2, 2, 3, 2), 0)])
def test_dilated_supported_rule(built_lib, geo, want):
    assert built_lib.smpq_conv2d_dilated_supported(*geo) == want
