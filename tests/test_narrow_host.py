"""Narrow-channel conv on the host: the appended C-ABI entries and their support rule."""
import pytest


def test_narrow_symbols_exported_abi_unchanged(built_lib):
    from smpq import _lib
    for s in ("smpq_conv2d_narrow_supported", "smpq_weights_narrow_expand_bytes", "smpq_weights_narrow_expand",
              "smpq_conv2d_narrow_fwd_q"):
        assert hasattr(built_lib, s) and s in _lib.EXPORTED_SYMBOLS, s
    assert built_lib.smpq_abi_version() == 7 == _lib.ABI_VERSION


# (cin, cout, kh, kw, stride, pad, limbs, wlimbs) -> supported
@pytest.mark.parametrize("geo,want", [((48, 48, 3, 3, 1, 1, 3, 1), 1), ((96, 96, 3, 3, 2, 1, 3, 3), 1),
                                      ((16, 64, 1, 1, 1, 0, 3, 1), 1), ((336, 336, 3, 3, 2, 1, 3, 3), 1),
                                      ((16 * 1001, 16, 3, 3, 2, 1, 3, 1), 1), ((64, 64, 3, 3, 1, 1, 3, 1), 0),
                                      ((24, 64, 3, 3, 1, 1, 3, 1), 0), ((48, 100, 3, 3, 1, 1, 3, 1), 0),
                                      ((48, 64, 5, 5, 1, 2, 3, 1), 0), ((48, 64, 1, 1, 2, 0, 3, 1), 0),
                                      ((48, 64, 3, 3, 1, 0, 3, 1), 0), ((48, 64, 3, 1, 1, 1, 3, 1), 0),
                                      ((48, 64, 3, 3, 1, 1, 2, 1), 0), ((48, 64, 3, 3, 1, 1, 3, 2), 0)])
def test_narrow_supported_rule(built_lib, geo, want):
    assert built_lib.smpq_conv2d_narrow_supported(*geo) == want


def test_narrow_expand_bytes_follow_the_slabs(built_lib):
    # [planes][cout / 16][NK] KiB: one slab of ceil(9 * 3 / 4) steps; 1x1 with the all-ones plane; at stride 2
    # cin = 208 is slabs of 11 and 2 chunks, ceil(99 / 4) + ceil(18 / 4) steps; an unsupported operand
    assert built_lib.smpq_weights_narrow_expand_bytes(3, 32, 48, 3, 3, 1) == 3 * 2 * 7 * 1024
    assert built_lib.smpq_weights_narrow_expand_bytes(1, 16, 96, 1, 1, 1) == 2 * 1 * 2 * 1024
    assert built_lib.smpq_weights_narrow_expand_bytes(3, 16, 208, 3, 3, 2) == 3 * 1 * (25 + 5) * 1024
    assert built_lib.smpq_weights_narrow_expand_bytes(3, 16, 64, 3, 3, 1) == 0
