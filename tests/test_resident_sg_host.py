"""The grid and the block -> (slab, tile) order of the weight-stationary 1x1 launches with slab groups
(csrc/conv_resident.hip res_grid / res_block_map, through smpq_resident_sg_grid / _sg_map): for every
grid the launcher can choose, every (slab, tile) pair is visited exactly once, and the super-slabs
that share a pixel tile sit at block indices 8 apart (one XCD under the block % 8 dispatch rule)
wherever 8 tile walkers fill a round. No GPU needed: the same function runs in the kernel.

A launch's grid is the launcher's own arithmetic on a budget of resident workgroups (CUs x
workgroups per CU), so the grids asked for (1, 7, 8, 9, 256 MINW, ntiles nslabs / SG blocks) are
budgets here: the launcher rounds each to a multiple of the super-slabs, at most ntiles for each."""
import ctypes
import itertools

import pytest

NSLABS = (2, 4, 16)
SGS = (1, 2, 4)
NTILES = (1, 5, 33)
CASES = [(ns, sg, nt) for ns, sg, nt in itertools.product(NSLABS, SGS, NTILES) if ns % sg == 0]


def budgets(ntiles, nss):
    return sorted({1, 7, 8, 9, 256, 512, ntiles * nss})


def grid(lib, budget, ntiles, nss):
    blocks = lib.smpq_resident_sg_grid(budget, ntiles, nss)
    assert blocks > 0 and blocks % nss == 0 and 1 <= blocks // nss <= ntiles
    # as many as the budget holds (never fewer than one walker per super-slab)
    assert blocks // nss == max(1, min(ntiles, budget // nss))
    return int(blocks)


def block_map(lib, blocks, nss):
    out = []
    for b in range(blocks):
        ss, t0 = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.smpq_resident_sg_map(b, blocks, nss, ctypes.byref(ss), ctypes.byref(t0)) == 0
        out.append((ss.value, t0.value))
    return out


@pytest.mark.parametrize("nslabs,sg,ntiles", CASES)
def test_every_slab_and_tile_once(built_lib, nslabs, sg, ntiles):
    nss = nslabs // sg
    for budget in budgets(ntiles, nss):
        blocks = grid(built_lib, budget, ntiles, nss)
        stride = blocks // nss
        seen = {}
        for b, (ss, t0) in enumerate(block_map(built_lib, blocks, nss)):
            assert 0 <= ss < nss and 0 <= t0 < stride, (budget, b, ss, t0)
            for t in range(t0, ntiles, stride):      # the kernel's tile walk
                for g in range(sg):                  # wave group g: slab sg * ss + g
                    key = (ss * sg + g, t)
                    assert key not in seen, (budget, b, key, seen[key])
                    seen[key] = b
        assert len(seen) == nslabs * ntiles and set(seen) == set(itertools.product(range(nslabs), range(ntiles)))


@pytest.mark.parametrize("nslabs,sg,ntiles", CASES)
def test_sibling_super_slabs_share_an_xcd(built_lib, nslabs, sg, ntiles):
    nss = nslabs // sg
    for budget in budgets(ntiles, nss):
        blocks = grid(built_lib, budget, ntiles, nss)
        stride = blocks // nss
        by_walker = {}
        for b, (ss, t0) in enumerate(block_map(built_lib, blocks, nss)):
            by_walker.setdefault(t0, {})[ss] = b
        assert sorted(by_walker) == list(range(stride))
        rounds = stride // 8 * 8  # walkers in whole rounds of 8: the grid allows it for these
        for t0, sibs in by_walker.items():
            assert sorted(sibs) == list(range(nss))
            bs = [sibs[s] for s in range(nss)]
            if t0 < rounds:
                # one XCD, adjacent in its launch order: 8 apart, in super-slab order
                assert all(b1 - b0 == 8 for b0, b1 in zip(bs, bs[1:])), (budget, t0, bs)
                assert bs[0] % 8 == t0 % 8
            else:
                assert all(b1 - b0 == 1 for b0, b1 in zip(bs, bs[1:])), (budget, t0, bs)
        # the shapes this is for: 256 CUs, 8 and 2 super-slabs -> every walker in a whole round
        if budget in (256, 512) and stride == budget // nss:
            assert rounds == stride


def test_map_refuses_bad_arguments(built_lib):
    ss, t0 = ctypes.c_int(), ctypes.c_int()
    for b, blocks, nss in ((-1, 8, 2), (8, 8, 2), (0, 7, 2), (0, 1, 2), (0, 8, 0)):
        assert built_lib.smpq_resident_sg_map(b, blocks, nss, ctypes.byref(ss), ctypes.byref(t0)) != 0
    assert built_lib.smpq_resident_sg_map(0, 8, 2, None, ctypes.byref(t0)) != 0
    assert built_lib.smpq_resident_sg_grid(256, 0, 2) < 0


def test_sg_support_rule(built_lib):
    sup = built_lib.smpq_conv2d_chain_sg_supported
    for shape in ((64, 256, 64, 1), (128, 512, 256, 2), (256, 1024, 512, 2)):
        assert sup(*shape, 3, 0, 1) == 1 and sup(*shape, 3, 1, 1) == 1 and sup(*shape, 3, 0, 4) == 0
    assert sup(256, 1024, 512, 2, 3, 0, 2) == 1 and sup(256, 1024, 512, 2, 3, 1, 2) == 1
    assert sup(128, 512, 256, 2, 3, 0, 2) == 1 and sup(128, 512, 256, 2, 3, 1, 2) == 0  # (would spill)
    assert sup(64, 256, 64, 1, 3, 0, 2) == 0 and sup(128, 512, 256, 1, 3, 0, 2) == 0


def test_tile_table_picks_the_slab_groups(built_lib, tmp_path):
    """conv_chain_q's default: the table's chain|... entry where that is built, else one group."""
    import json
    from smpq import ops
    l3 = (128, 14, 14, 256, 1024, 512, 2)
    l2 = (128, 28, 28, 128, 512, 256, 2)
    table = tmp_path / "tiles.json"
    table.write_text(json.dumps({"format": "smpq-tiles/1", "tiles": {
        ops.key_str(ops.chain_sg_key(*l3, False)): 2, ops.key_str(ops.chain_sg_key(*l2, True)): 2,
        ops.key_str(ops.chain_sg_key(*l2, False)): 4}}))
    try:
        ops.load_tile_table(str(table))
        assert ops._chain_sg(*l3, False) == 2
        assert ops._chain_sg(*l3, True) == 1    # not listed
        assert ops._chain_sg(*l2, True) == 1    # listed, not built (would spill)
        assert ops._chain_sg(*l2, False) == 1   # listed with a count that is not built
        ops.load_tile_table("off")
        assert ops._chain_sg(*l3, False) == 1
        ops.load_tile_table(ops.TILE_TABLE_DEFAULT)  # the committed table: the bench's slice shapes
        assert ops._chain_sg(*l3, False) == 2 and ops._chain_sg(*l3, True) == 2 and ops._chain_sg(*l2, False) == 2
    finally:
        ops.load_tile_table()
