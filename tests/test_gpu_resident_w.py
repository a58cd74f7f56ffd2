"""Weight-stationary 1x1 tiles with 3 weight limbs + ReLU (tile kind TILE_RESIDENT1X1_W: the 1x1 convs
of a model under search, whose operand is 24-bit fixed point while a channel is free): limb planes and
overflow flag equal the default LDS-DMA tile's bit for bit, with and without a limb-plane residual, in
range and overflowing, partial last tiles, K 64 .. 512, several tiles per persistent workgroup, more
images than the per-image scale table, a patched operand row; one case against the float64
reference of tests/lean_ref.py; the calls the kind does not run are refused before launching; and a
pristine ResNet-50's logits and delta-loss table do not move when the kind runs its eligible convs.
Every call goes through the C-ABI."""
import json

import pytest
import torch

import lean_ref
from lean_ref import FACTORS, ConvCase
from test_gpu import build_model

pytestmark = pytest.mark.gpu


def _w_cfgs(ops, cin, cout):
    return [c for c in ops.tile_configs()
            if ops.tile_kind(c) == ops.TILE_RESIDENT1X1_W and ops._tile_fits(c, 3, 3, cout, cin, 1)]


def _operands(gpu, cin, cout, n, h, seed):
    from smpq import ops
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(cout, cin, 1, 1, generator=g) * 0.1).to(gpu)
    codes, _, wscale, _ = ops.pack_weights_ex(w, None, 3)
    x = torch.relu(torch.randn(n, h, h, cin, generator=g)).to(gpu)
    x[0] *= 3.0
    am = ops.act_absmax(x)
    xq = ops.act_quantize(x, am, 3)
    shift = torch.linspace(-0.5, 0.5, cout, device=gpu)
    return w, codes, wscale, xq, am, shift, g


def _conv(ops, gpu, xq, am, codes, scale, shift, cfg, rng, **kw):
    ovf = torch.zeros(1, dtype=torch.int32, device=gpu)
    _, yq = ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=True, tile_cfg=cfg, emit_range=rng,
                         overflow=ovf, want_f32=False, **kw)
    return yq, ovf


def _compare(ops, gpu, cfgs, xq, am, codes, scale, shift, rng, want_ovf=None, launches=2, **kw):
    yq0, ovf0 = _conv(ops, gpu, xq, am, codes, scale, shift, -1, rng, **kw)
    if want_ovf is not None:
        assert int(ovf0.item()) == want_ovf
    for c in cfgs:
        for _ in range(launches):  # repeated: no race between a tile's DMA and the last tile's reads
            yq, ovf = _conv(ops, gpu, xq, am, codes, scale, shift, c, rng, **kw)
            assert torch.equal(yq, yq0), (c, rng)
            assert torch.equal(ovf, ovf0), (c, rng)
    return yq0


# (cin, cout): the kind-6 configurations that take the shape (51: slab 256 / 32 px, 52: slab 256 / 16 px,
# 53: slab 64, 54: slab 128)
FITTING = {(64, 256): [51, 52, 53, 54], (256, 64): [53], (128, 512): [52, 53, 54], (512, 128): [53],
           (256, 1024): [53, 54], (512, 2048): [53]}


@pytest.mark.parametrize("cin,cout,n,h", [(64, 256, 1, 5), (256, 64, 2, 9), (128, 512, 1, 9), (512, 128, 1, 7)])
def test_relu_equals_lds_dma(gpu, cin, cout, n, h):
    """A Bottleneck conv1 under search (ReLU only): a partial last tile, four K chunks on the
    64-channel slab, K 512 (on the 64-channel slab only: 128 channels are over the register budget)."""
    from smpq import ops
    cfgs = _w_cfgs(ops, cin, cout)
    assert cfgs == FITTING[(cin, cout)]
    _, codes, scale, xq, am, shift, _ = _operands(gpu, cin, cout, n, h, 7 * n + h + cin)
    ref = ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=True)
    for frac in (2.0, 0.4):
        _compare(ops, gpu, cfgs, xq, am, codes, scale, shift, float(ref.abs().max()) * frac, 1 if frac < 1 else 0)


@pytest.mark.parametrize("cin,cout,n,h", [(64, 256, 2, 13), (256, 1024, 2, 7), (512, 2048, 1, 7)])
def test_relu_residual_equals_lds_dma(gpu, cin, cout, n, h):
    """A Bottleneck conv3 under search (ReLU + the limb-plane identity, which arrives by LDS-DMA one
    tile ahead): residual range above, just above and far above the residual's maximum, in range and
    overflowing."""
    from smpq import ops
    cfgs = _w_cfgs(ops, cin, cout)
    assert cfgs == FITTING[(cin, cout)]
    _, codes, scale, xq, am, shift, g = _operands(gpu, cin, cout, n, h, 3 * n + h + cin)
    r = torch.relu(torch.randn(n, h, h, cout, generator=g)).to(gpu)
    rmax = float(r.abs().max())
    for rr in (rmax * 1.5, rmax * 1.01, 40.0):
        rq = ops.act_quantize(r, torch.full((n,), rr, device=gpu), 3)
        ref = ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=True, residual_q=rq, residual_range=rr)
        for frac in (2.0, 0.4):
            _compare(ops, gpu, cfgs, xq, am, codes, scale, shift, float(ref.abs().max()) * frac,
                     1 if frac < 1 else 0, residual_q=rq, residual_range=rr)


def test_several_tiles_per_persistent_workgroup(gpu):
    """1 176 tiles of 16 pixels (588 of 32): more than 256 CUs x 4 workgroups, so each walks several."""
    from smpq import ops
    cin, cout, n, h = 64, 256, 24, 28
    cfgs = _w_cfgs(ops, cin, cout)
    assert cfgs == FITTING[(cin, cout)] and n * h * h // 16 > 256 * 4
    _, codes, scale, xq, am, shift, _ = _operands(gpu, cin, cout, n, h, 91)
    ref = ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=True)
    for frac in (2.0, 0.4):
        _compare(ops, gpu, cfgs, xq, am, codes, scale, shift, float(ref.abs().max()) * frac, 1 if frac < 1 else 0)


def test_more_images_than_the_scale_table(gpu):
    """260 images with scales that differ past the 256th: the per-image scale is read from memory
    inside the tile loop (with the residual)."""
    from smpq import ops
    cin, cout, n, h = 64, 256, 260, 3
    cfgs = _w_cfgs(ops, cin, cout)
    assert cfgs == FITTING[(cin, cout)]
    _, codes, scale, _, _, shift, g = _operands(gpu, cin, cout, 1, 1, 17)
    x = torch.relu(torch.randn(n, h, h, cin, generator=g))
    x *= (1.0 + 0.01 * torch.arange(n).float()).reshape(n, 1, 1, 1)
    x = x.to(gpu)
    am = ops.act_absmax(x)
    a = am.cpu().tolist()
    assert len(set(a[256:])) == 4 and not set(a[256:]) & set(a[:256])
    xq = ops.act_quantize(x, am, 3)
    r = torch.relu(torch.randn(n, h, h, cout, generator=g)).to(gpu)
    rr = float(r.abs().max()) * 1.5
    rq = ops.act_quantize(r, torch.full((n,), rr, device=gpu), 3)
    ref = ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=True, residual_q=rq, residual_range=rr)
    for frac in (2.0, 0.4):
        _compare(ops, gpu, cfgs, xq, am, codes, scale, shift, float(ref.abs().max()) * frac, 1 if frac < 1 else 0,
                 residual_q=rq, residual_range=rr)


def test_patched_operand_row(gpu):
    """The kernel reads codes / the K-major copy at every launch: a row patched in place
    (ops.trial_row_patch, a delta-loss trial) is seen as the LDS-DMA kernel sees it, and the restored
    operand gives the unpatched planes again."""
    from smpq import ops
    cin, cout, n, h = 256, 64, 2, 9
    cfgs = _w_cfgs(ops, cin, cout)
    assert cfgs == FITTING[(cin, cout)]
    w, codes, wscale, xq, am, shift, g = _operands(gpu, cin, cout, n, h, 29)
    km = codes._smpq_km
    assert km is not None
    bn_a = (torch.rand(cout, generator=g) + 0.5).to(gpu)
    col_scale = (wscale * bn_a).contiguous()
    ref = ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, col_scale, shift, relu=True)
    rng = float(ref.abs().max()) * 2.0
    y_plain = _compare(ops, gpu, cfgs, xq, am, codes, col_scale, shift, rng, 0)
    orig = [t.clone() for t in (codes, km, wscale, col_scale)]
    save = torch.zeros(ops.trial_save_bytes(3, cin), dtype=torch.int8, device=gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    row = 37
    ops.trial_row_patch(w, row, 4, bn_a, codes, wscale, col_scale, save, status, km=km)
    assert int(status) == 0 and not torch.equal(codes, orig[0]) and not torch.equal(km, orig[1])
    y_patched = _compare(ops, gpu, cfgs, xq, am, codes, col_scale, shift, rng)
    assert not torch.equal(y_patched[..., row], y_plain[..., row])
    keep = [c for c in range(cout) if c != row]
    assert torch.equal(y_patched[..., keep], y_plain[..., keep])
    ops.trial_row_restore(row, codes, wscale, col_scale, save, km=km)
    for t, o in zip((codes, km, wscale, col_scale), orig):
        assert torch.equal(t.view(torch.int8), o.view(torch.int8))
    assert torch.equal(_compare(ops, gpu, cfgs, xq, am, codes, col_scale, shift, rng, 0), y_plain)


def test_refuses_what_it_does_not_run(gpu):
    """SMPQ_E_INVALID before launching ("resident" in the message): the refused calls leave their
    overflow flag untouched."""
    from smpq import _lib, ops
    from test_gpu import make_layer
    cin, cout, n, h = 64, 256, 1, 8
    c = _w_cfgs(ops, cin, cout)[0]
    _, codes, scale, xq, am, shift, g = _operands(gpu, cin, cout, n, h, 3)
    ovf = torch.zeros(1, dtype=torch.int32, device=gpu)
    lean = dict(tile_cfg=c, emit_range=1.0, overflow=ovf, want_f32=False)
    ok = ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=True,  # the call the kind does run
                      **dict(lean, overflow=torch.zeros(1, dtype=torch.int32, device=gpu)))[1]
    assert ok.shape == (3, n, h, h, cout)
    _, _, codes1, _ = make_layer(gpu, cin, cout, 1, seed=3, bits_choice=(6, 4))
    with pytest.raises(_lib.SmpqError, match="resident"):  # one weight limb
        ops.conv2d_q(xq, am, codes1, None, 1, 1, 1, 0, scale, shift, relu=True, **lean)
    with pytest.raises(_lib.SmpqError, match="resident"):  # no ReLU
        ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=False, **lean)
    with pytest.raises(_lib.SmpqError, match="resident"):  # fp32 output
        ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=True, tile_cfg=c)
    with pytest.raises(_lib.SmpqError, match="resident"):  # fp32 output beside the limb planes
        ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=True, tile_cfg=c, emit_range=1.0,
                     overflow=ovf, want_f32=True)
    with pytest.raises(_lib.SmpqError, match="resident"):  # an fp32 residual
        ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 0, scale, shift, relu=True,
                     residual=torch.zeros(n, h, h, cout, device=gpu), **lean)
    off = torch.zeros(cout, dtype=torch.int32, device=gpu)
    off[3] = 5
    with pytest.raises(_lib.SmpqError, match="resident"):  # weight offsets
        ops.conv2d_q(xq, am, codes, off, 1, 1, 1, 0, scale, shift, relu=True, **lean)
    with pytest.raises(_lib.SmpqError, match="resident"):  # pad 1
        ops.conv2d_q(xq, am, codes, None, 1, 1, 1, 1, scale, shift, relu=True, **lean)
    with pytest.raises(_lib.SmpqError, match="resident"):  # stride 2
        ops.conv2d_q(xq, am, codes, None, 1, 1, 2, 0, scale, shift, relu=True, **lean)
    w2 = (torch.randn(cout, cin, 1, 1, generator=g) * 0.1).to(gpu)
    codes2, _, scale2, _ = ops.pack_weights_ex(w2, None, 2)
    x2 = ops.act_quantize(torch.ones(n, h, h, cin, device=gpu), torch.ones(n, device=gpu), 2)
    with pytest.raises(_lib.SmpqError, match="resident"):  # 2 activation limbs
        ops.conv2d_q(x2, torch.ones(n, device=gpu), codes2, None, 1, 1, 1, 0, scale2, shift, relu=True, **lean)
    assert int(ovf.item()) == 0


def test_relu_residual_vs_float64_reference(gpu):
    """Independent of kernel against kernel: conv3 64 -> 256 with 3 weight limbs, ReLU and the
    limb-plane identity on every configuration of the kind, guarded launches, against the float64
    reference of the same operation within tests/lean_ref.py's own bound; in range and overflowing."""
    from smpq import ops
    case = ConvCase(gpu, 64, 256, 1, 1, 5, 5, 3, 3, wl=3, seed=311, residual=True, relu=True)
    cfgs = lean_ref._kind_cfgs((ops.TILE_RESIDENT1X1_W,), 3, 3, 256, 64, 1)
    assert cfgs == FITTING[(64, 256)]
    for f in FACTORS:
        for c in cfgs:
            yq, ovf = case.launch(c, f)
            case.check(yq, ovf, f, "resident 1x1, 3 weight limbs + ReLU + residual")
        assert int(case.reference(f)[2]) == (1 if f < 1 else 0)


# ---- a model under search ---------------------------------------------------------------------------
ELIGIBLE = {(64, 64), (256, 64), (64, 256), (256, 128), (512, 128), (128, 512), (512, 256), (256, 1024), (512, 2048)}


@pytest.fixture
def tile_state():
    """Tile table, tile cache, the kind's knob, autotune switch, graph switch, range mode and limb
    count as they were, whatever a test sets."""
    from smpq import engine, ops
    saved = (ops.RESIDENT_W[0], ops.AUTOTUNE[0], engine.USE_GRAPH[0], engine.get_range_mode(), ops.get_act_limbs(),
             dict(ops._TUNED), dict(ops._TABLE))
    try:
        yield
    finally:
        ops.RESIDENT_W[0], ops.AUTOTUNE[0], engine.USE_GRAPH[0] = saved[:3]
        engine.set_range_mode(saved[3])
        ops.set_act_limbs(saved[4])
        ops._TUNED.clear()
        ops._TUNED.update(saved[5])
        ops._TABLE.clear()
        ops._TABLE.update(saved[6])


def _forced_table(ops, tmp_path, n, hw):
    """A tile table that puts every eligible 1x1 conv of a ResNet-50 forward of n images of hw x hw
    on a kind-6 configuration (the last that takes the shape); table keys: ops.tuned_conv2d_q's, at
    the sizes of the slices the engine runs a batch as."""
    from smpq import suffix
    tiles = {}
    sizes = sorted({e - s for s, e in suffix.slices(n)})
    side = {1: hw // 4, 2: hw // 8, 3: hw // 16, 4: hw // 32}
    for layer, planes in ((1, 64), (2, 128), (3, 256), (4, 512)):
        s, up = side[layer], side[layer] * 2
        first_in = 64 if layer == 1 else 2 * planes
        # conv1 of the first block (reads the previous stage's output at its size), of the others,
        # conv3 (+ limb-plane identity)
        shapes = [(up if layer > 1 else s, first_in, planes, False), (s, 4 * planes, planes, False),
                  (s, planes, 4 * planes, True)]
        for h, cin, cout, res in shapes:
            cfgs = _w_cfgs(ops, cin, cout)
            for m in sizes if cfgs else ():
                key = (m, h, h, cin, cout, 1, 1, 1, 0, 3, 3, False, True, False, res)
                tiles[ops.key_str(key)] = cfgs[-1]
    path = tmp_path / "tiles_forced.json"
    path.write_text(json.dumps({"tiles": tiles}))
    return str(path), tiles


def _on_kind6(ops):
    return {(k[0][3], k[0][4]) for k, v in ops._TUNED.items()
            if isinstance(k[0], tuple) and k[1] == "resw" and ops.tile_kind(v) == ops.TILE_RESIDENT1X1_W}


def test_model_forward_and_table_do_not_move(gpu, tile_state, tmp_path):
    """A pristine ResNet-50 (every searched conv packed as 24-bit fixed point), 2 batches of 8 images
    at 64 x 64, graphs on, 3 limbs: with the kind forced for every eligible shape through a tile table
    and with the kind off, the logits are equal bit for bit, and so is a delta-loss table over 2
    channels of lnum 1 (a conv1 the kind runs) and lnum 3 (a conv3 it runs) at 8 and 4 bits."""
    from smpq import engine, ops, sensitivity
    engine.set_range_mode("static")
    engine.USE_GRAPH[0] = True
    ops.set_act_limbs(3)
    ops.AUTOTUNE[0] = False  # a shape's tile: the table's, else the C-ABI default
    g = torch.Generator().manual_seed(77)
    xs = [torch.randn(8, 3, 64, 64, generator=g).to(gpu) for _ in range(2)]
    ys = [torch.randint(0, 1000, (8,), generator=g).to(gpu) for _ in range(2)]
    batches = list(zip(xs, ys))
    path, tiles = _forced_table(ops, tmp_path, 8, 64)
    out = {}
    for knob in (True, False):
        ops.RESIDENT_W[0] = knob
        ops._TUNED.clear()
        ops.load_tile_table(path)
        net = build_model(gpu, "resnet50", None, "r50_mixed_cal")
        with torch.no_grad():
            net(xs[0])  # calibration
            logits = [net(x).clone() for x in xs] + [net(x).clone() for x in xs]  # captures, then replays
        table = sensitivity.delta_loss_table(net, batches, bits=(8, 4), lnums=[1, 3], channels={1: [0, 63], 3: [5, 255]})
        rep = table.report()
        assert rep["trials"] == 8 and rep["patched"] == 8 and not rep["slow"] and not rep["constant"], rep
        ran = _on_kind6(ops)
        if knob:
            assert ran >= ELIGIBLE, sorted(ELIGIBLE - ran)
            assert ops._TABLE["hits"] >= len(ELIGIBLE)
        else:
            assert not ran and not any(ops.tile_kind(v) == ops.TILE_RESIDENT1X1_W for v in ops._TUNED.values())
        out[knob] = (logits, table)
    (la, ta), (lb, tb) = out[True], out[False]
    for a, b in zip(la, lb):
        assert torch.equal(a, b)
    assert torch.equal(la[0], la[2]) and torch.equal(la[1], la[3]) and not torch.equal(la[0], la[1])
    assert ta.base_loss == tb.base_loss and ta.eval_loss == tb.eval_loss
    for bit in (8, 4):
        assert (ta.delta[bit] == tb.delta[bit]).all(), bit
        assert (ta.stats[bit] == tb.stats[bit]).all(), bit
        assert (ta.delta[bit] != 0).any()
