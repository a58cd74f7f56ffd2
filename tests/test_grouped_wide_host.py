"""Wide-group 3x3 conv on the host: the support rule of smpq_conv2d_grouped_supported for cin / groups >= 128
(csrc/conv_grouped_wide.hip), the size of the expanded weight copy, the unchanged ABI."""
import pytest


# (cin, cout, groups, k, stride, pad, limbs, wlimbs) -> supported
@pytest.mark.parametrize("geo,want", [((256, 256, 2, 3, 1, 1, 3, 1), 1), ((4096, 4096, 32, 3, 1, 1, 3, 3), 1),
                                      ((256, 512, 2, 3, 2, 1, 3, 3), 1), ((1024, 64, 4, 3, 1, 1, 3, 3), 0),
                                      ((96, 96, 2, 3, 1, 1, 3, 3), 0), ((256, 256, 2, 3, 1, 1, 3, 2), 0),
                                      ((256, 256, 2, 3, 1, 1, 2, 1), 0), ((256, 256, 2, 5, 1, 2, 3, 3), 0)])
def test_grouped_wide_supported_rule(built_lib, geo, want):
    cin, cout, groups, k, stride, pad, limbs, wlimbs = geo
    assert built_lib.smpq_conv2d_grouped_supported(cin, cout, groups, k, k, stride, pad, limbs, wlimbs) == want
    if want:  # test_grouped_host's formula with S = cg: 9 cg / 64 whole steps per fragment
        cg = cin // groups
        nbytes = built_lib.smpq_weights_grouped_expand_bytes(wlimbs, cout, cg, groups)
        assert nbytes == (wlimbs + (wlimbs == 1)) * (cout // 16) * ((9 * cg + 63) // 64) * 1024


def test_grouped_wide_abi_unchanged(built_lib):
    from smpq import _lib
    assert built_lib.smpq_abi_version() == 7 == _lib.ABI_VERSION
