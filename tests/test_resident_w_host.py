"""The weight-stationary 1x1 tiles with 3 weight limbs + ReLU (tile kind TILE_RESIDENT1X1_W) on the
host: the appended configurations and their shape rule through the C-ABI, the untouched numbering of
the 51 configurations before them, ops.tuned_conv2d_q's candidate gate with SMPQ_RESIDENT_W, and the
tile cache being looked up before the candidate list is built (no GPU needed)."""
from collections import Counter

import pytest
import torch

# (cw, wp) of the four geometries and the K sizes each runs with 3 weight limbs: the geometry's K
# mask cut by the register budget (3 * K / 64 * cw <= 32 weight fragments per wave)
GEOMS = [((4, 2), (64,)), ((4, 1), (64, 128)), ((1, 1), (64, 128, 256, 512)), ((2, 1), (64, 128, 256))]
W_BASE = 51


@pytest.fixture
def ops(built_lib):
    """smpq.ops with its knobs put back afterwards, whatever a test sets."""
    from smpq import ops
    saved = ops.RESIDENT_W[0], ops.AUTOTUNE[0]
    yield ops
    ops.RESIDENT_W[0], ops.AUTOTUNE[0] = saved


def test_four_configurations_appended(ops, built_lib):
    assert built_lib.smpq_conv2d_num_tile_configs() == 55
    assert ops.TILE_RESIDENT1X1_W == 6
    assert [built_lib.smpq_conv2d_tile_kind(c) for c in range(W_BASE, 55)] == [6] * 4
    tiles = ops.tile_configs()
    for i, ((cw, wp), _) in enumerate(GEOMS):  # the same four geometries as kind 5, in its order
        assert tiles[W_BASE + i] == (16 * wp, 64 * cw, 256)
        assert tiles[W_BASE + i] == tiles[W_BASE - 4 + i]
    assert built_lib.smpq_abi_version() == 7
    assert built_lib.smpq_conv2d_tile_kind(55) < 0


def test_earlier_configurations_keep_their_kinds(ops, built_lib):
    kinds = [built_lib.smpq_conv2d_tile_kind(c) for c in range(W_BASE)]
    assert Counter(kinds) == {ops.TILE_LDS_DMA: 26, ops.TILE_LDS_DMA_K128: 11, ops.TILE_HALO3X3: 10,
                              ops.TILE_RESIDENT1X1: 4}
    assert kinds[47:] == [ops.TILE_RESIDENT1X1] * 4 and kinds[37:47] == [ops.TILE_HALO3X3] * 10
    assert all(k in (ops.TILE_LDS_DMA, ops.TILE_LDS_DMA_K128) for k in kinds[:37])
    # kind 5's own rule is as it was: 3 weight limbs up to K 512 on the 64-channel slab, 1 limb to K 1024
    assert ops._tile_fits(49, 3, 3, 512, 256, 1) and ops._tile_fits(49, 3, 1, 256, 1024, 1)
    assert not ops._tile_fits(49, 3, 3, 256, 1024, 1)


def test_tile_supported_follows_the_rule(ops):
    for i, ((cw, wp), ks) in enumerate(GEOMS):
        c = W_BASE + i
        slab = 64 * cw
        for k in (64, 128, 192, 256, 320, 512, 1024, 2048, 96):
            for cout in (64, 128, 192, 256, 512, 1024, 2048, 32):
                want = k in ks and cout % slab == 0
                assert ops._tile_fits(c, 3, 3, cout, k, 1) == want, (c, k, cout)
        k, cout = ks[0], 4 * slab
        assert ops._tile_fits(c, 3, 3, cout, k, 1)
        assert not ops._tile_fits(c, 3, 1, cout, k, 1) and not ops._tile_fits(c, 3, 2, cout, k, 1)
        assert not ops._tile_fits(c, 2, 3, cout, k, 1) and not ops._tile_fits(c, 2, 2, cout, k, 1)
        assert not ops._tile_fits(c, 3, 3, cout, k, 3)
        assert not ops._tile_fits(c, 3, 3, cout, 1024, 1)
    # the eligible 1x1 convs of a ResNet-50 under search each have a configuration; K 1024 / 2048 none
    for cin, cout in ((64, 64), (256, 64), (64, 256), (256, 128), (512, 128), (128, 512), (512, 256), (256, 1024),
                      (512, 2048)):
        assert any(ops._tile_fits(c, 3, 3, cout, cin, 1) for c in range(W_BASE, 55)), (cin, cout)
    for cin, cout in ((1024, 256), (1024, 512), (2048, 512)):
        assert not any(ops._tile_fits(c, 3, 3, cout, cin, 1) for c in range(W_BASE, 55)), (cin, cout)


def _gates(ops, **over):
    """ops._conv_tile_gates for a Bottleneck conv1 of a model under search, with overrides."""
    a = dict(kh=1, kw=1, stride=1, pad=0, wlimbs=3, offset=None, residual=None, relu=True, y_absmax=None, out=None,
             emit_range=4.0, want_f32=False, residual_q=None)
    a.update(over)
    return ops._conv_tile_gates(**a)


def _w_cands(ops, gates, cin=256, cout=64, k=1, wlimbs=3):
    return [c for c in ops._conv_tile_candidates(3, wlimbs, cout, cin, k, gates)
            if ops.tile_kind(c) == ops.TILE_RESIDENT1X1_W]


def test_candidate_gate(ops):
    t = torch.zeros(1)
    ops.RESIDENT_W[0] = True
    g = _gates(ops)
    assert g == (False, False, True) and ops._conv_tile_variant(g) == "resw"
    assert _w_cands(ops, g) == [53]  # 256 -> 64: the 64-channel slab only
    assert _w_cands(ops, g, cin=64, cout=256) == [51, 52, 53, 54]
    assert _w_cands(ops, _gates(ops, residual_q=t), cin=512, cout=2048) == [53]
    # the other candidates of the call are the ones it had: no kind-5 tile (3 weight limbs + ReLU)
    others = [c for c in ops._conv_tile_candidates(3, 3, 256, 64, 1, g) if ops.tile_kind(c) != ops.TILE_RESIDENT1X1_W]
    assert others and all(ops.tile_kind(c) in (ops.TILE_LDS_DMA, ops.TILE_LDS_DMA_K128) for c in others)
    ops.RESIDENT_W[0] = False
    assert others == ops._conv_tile_candidates(3, 3, 256, 64, 1, _gates(ops))
    ops.RESIDENT_W[0] = True
    # each condition of the gate, one at a time
    for over in (dict(relu=False), dict(emit_range=None), dict(want_f32=True), dict(residual=t), dict(y_absmax=t),
                 dict(out=t), dict(offset=t), dict(kh=3, kw=3, pad=1), dict(pad=1), dict(stride=2), dict(wlimbs=1),
                 dict(wlimbs=2)):
        g2 = _gates(ops, **over)
        assert not g2[2], over
        assert ops._conv_tile_variant(g2) != "resw"
        assert _w_cands(ops, g2, cin=64, cout=256, k=over.get("kh", 1), wlimbs=over.get("wlimbs", 3)) == [], over
    # the knob: off, the call is the parent's (its candidates and its cache variant)
    ops.RESIDENT_W[0] = False
    g3 = _gates(ops)
    assert g3 == (False, False, False) and ops._conv_tile_variant(g3) == "nohalo"
    assert _w_cands(ops, g3, cin=64, cout=256) == []
    # the existing kinds' gates do not move with the knob
    for knob in (False, True):
        ops.RESIDENT_W[0] = knob
        assert _gates(ops, relu=False) == (False, True, False)  # a downsample: kind 5
        assert _gates(ops, wlimbs=1, offset=t) == (False, True, False)
        assert _gates(ops, kh=3, kw=3, pad=1, wlimbs=1) == (True, False, False)
        assert ops._conv_tile_variant(_gates(ops, relu=False)) is None


def test_cache_is_looked_up_before_the_candidates_are_built(ops, monkeypatch, tmp_path):
    """The second tuned_conv2d_q call of a key asks libsmpq about no tile configuration (the first
    asks about each once); the tile comes from a table here, so nothing is launched or timed."""
    import json
    calls, launched = [], []
    real_fits = ops._tile_fits

    def counted(*a, **kw):
        calls.append(a)
        return real_fits(*a, **kw)
    monkeypatch.setattr(ops, "_tile_fits", counted)
    monkeypatch.setattr(ops, "conv2d_q", lambda *a, tile_cfg=-1, **kw: launched.append(tile_cfg))
    xq = torch.zeros(3, 2, 7, 7, 256, dtype=torch.int8)
    codes = torch.zeros(3, 64, 256, dtype=torch.int8)
    am, cs = torch.ones(2), torch.ones(64)
    key = (2, 7, 7, 256, 64, 1, 1, 1, 0, 3, 3, False, True, False, False)
    table = tmp_path / "tiles.json"
    table.write_text(json.dumps({"tiles": {ops.key_str(key): 53}}))
    saved = dict(ops._TUNED)
    try:
        ops._TUNED.clear()
        ops.load_tile_table(str(table))
        for knob, want, variant in ((True, 53, "resw"), (False, -1, "nohalo")):
            ops.RESIDENT_W[0] = knob
            ops.AUTOTUNE[0] = False
            del calls[:], launched[:]
            kw = dict(relu=True, emit_range=4.0, overflow=torch.zeros(1, dtype=torch.int32), want_f32=False)
            ops.tuned_conv2d_q(xq, am, codes, None, 1, 1, 1, 0, cs, cs, **kw)
            assert launched == [want]
            assert len(calls) == 55  # one question per configuration, the first time
            if knob:
                assert ops._TUNED == {(key, variant): 53}
                del calls[:]
                ops.tuned_conv2d_q(xq, am, codes, None, 1, 1, 1, 0, cs, cs, **kw)
                assert launched == [53, 53] and calls == []
            else:  # the table's tile is no candidate with the knob off: nothing cached under this variant
                assert (key, variant) not in ops._TUNED
    finally:
        ops._TUNED.clear()
        ops._TUNED.update(saved)
        ops.load_tile_table()
