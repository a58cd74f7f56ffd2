"""Grouped conv on the host: the appended C-ABI entries, and the trial planners' view of a grouped conv."""
import pytest

GROUPED_SYMBOLS = ("smpq_conv2d_grouped_supported", "smpq_pack_weights_grouped", "smpq_weights_grouped_expand_bytes",
                   "smpq_weights_grouped_expand", "smpq_conv2d_grouped_fwd_q")


def test_grouped_symbols_exported_abi_unchanged(built_lib):
    from smpq import _lib
    for s in GROUPED_SYMBOLS:
        assert hasattr(built_lib, s) and s in _lib.EXPORTED_SYMBOLS, s
    assert built_lib.smpq_abi_version() == 7 == _lib.ABI_VERSION


# (cin, cout, groups, k, stride, pad, limbs, wlimbs) -> supported
@pytest.mark.parametrize("geo,want", [((128, 128, 32, 3, 1, 1, 3, 1), 1), ((1024, 1024, 32, 3, 2, 1, 3, 3), 1),
                                      ((128, 256, 2, 3, 1, 1, 3, 3), 1), ((128, 128, 32, 3, 1, 1, 2, 1), 0),
                                      ((128, 128, 32, 3, 1, 1, 3, 2), 0), ((128, 128, 1, 3, 1, 1, 3, 1), 0),
                                      ((64, 64, 4, 5, 1, 2, 3, 3), 0), ((96, 96, 2, 3, 1, 1, 3, 3), 0),
                                      ((128, 128, 32, 3, 3, 1, 3, 1), 0), ((1024, 64, 4, 3, 2, 1, 3, 3), 0)])
def test_grouped_supported_rule(built_lib, geo, want):
    cin, cout, groups, k, stride, pad, limbs, wlimbs = geo
    assert built_lib.smpq_conv2d_grouped_supported(cin, cout, groups, k, k, stride, pad, limbs, wlimbs) == want
    nbytes = built_lib.smpq_weights_grouped_expand_bytes(wlimbs, cout, cin // groups, groups)
    if want:  # [planes][cout / 16][ceil(9 S / 64)][1024], one more plane (the group indicator) with one weight limb
        cg, og = cin // groups, cout // groups
        S = cg * max(1, 16 // og)
        assert nbytes == (wlimbs + (wlimbs == 1)) * (cout // 16) * ((9 * S + 63) // 64) * 1024


def test_trial_planners_do_not_patch_a_grouped_conv(built_lib):
    from smpq import trials
    from smpq.qconv import QConv2d
    conv = QConv2d(128, 128, 3, padding=1, groups=32, bias=False)
    assert trials._operand(conv, None) is None
    assert not trials.patchable(conv, None) and not trials.patchable_rows(conv, None, [0, 1])
    assert not trials.patchable_rows_x8(conv, None, [0, 1], 4)
