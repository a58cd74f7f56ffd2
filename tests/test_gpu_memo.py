"""smpq.memo under the drop-in evaluation (functions.evaluate_acc_loss_softmax / evaluate_loss) on
the GPU: ResNet-18 on a ResidentSet of two batches of 8 images at 224 x 224. The ground truth of
every comparison is the same call with the memo disabled (``_plain``), never the memo itself."""
import os

import pytest
import torch

from test_gpu import build_model

pytestmark = pytest.mark.gpu

COUNTERS = ("hip_conv", "calibrations", "graph_replays", "graph_captures")


class Counting:
    def __init__(self, items):
        self.items, self.iterations = items, 0

    def __iter__(self):
        self.iterations += 1
        return iter(self.items)


def _host_batches(seed=41):
    from smpq import ops
    lut = ops.u8lut_table()
    g = torch.Generator().manual_seed(seed)
    return [(ops.u8lut_decode(torch.randint(0, 256, (8, 3, 224, 224), generator=g, dtype=torch.uint8), lut),
             torch.randint(0, 1000, (8,), generator=g)) for _ in range(2)]


def _same(r, want):
    return r[0] == want[0] and r[1] == want[1] and len(r[2]) == len(want[2]) and \
        all(torch.equal(a, b) for a, b in zip(r[2], want[2]))


def _eval(net, gpu, loader):
    import functions
    return functions.evaluate_acc_loss_softmax(net, gpu, loader)


def _plain(net, gpu, loader, fn="evaluate_acc_loss_softmax"):
    """The unmemoised call: the ground truth."""
    import functions
    from smpq import memo
    on = memo.enabled()
    memo.disable()
    try:
        return getattr(functions, fn)(net, gpu, loader)
    finally:
        if on:
            memo.enable()


@pytest.fixture(scope="module")
def host(gpu):
    return _host_batches()


@pytest.fixture(scope="module")
def net(gpu):
    return build_model(gpu, "resnet18", "r18_u8", "r18_u8_cal")


@pytest.fixture(scope="module")
def pristine(net):
    """The module model's state, put back after every test that changes it (never changed itself)."""
    return {k: v.detach().clone() for k, v in net.state_dict().items()}


@pytest.fixture
def memo_on(net, pristine):
    from smpq import engine, memo, ops
    memo.clear()
    memo.enable(entries=4)
    mode, limbs = engine.get_range_mode(), ops.get_act_limbs()
    yield memo
    memo.disable()
    memo.clear()
    memo.enable(entries=int(os.environ.get("SMPQ_EVAL_MEMO_ENTRIES", "4")))
    if os.environ.get("SMPQ_EVAL_MEMO", "0") != "1":
        memo.disable()
    engine.set_range_mode(mode)
    ops.set_act_limbs(limbs)
    net.load_state_dict(pristine)


def _snap(rs):
    from smpq import stats
    return [stats[k] for k in COUNTERS] + [rs.report()["resident_passes"], rs.report()["loader_passes"]]


def _engine_caches(net):
    """Identity of everything the engine keeps for ``net``: its state's fields, and the graph
    cache's per-address entries, fallback entry and pool."""
    from smpq import engine
    st = engine.model_state(net)
    out = {k: id(getattr(st, k)) for k in st.__slots__}
    out.update({k: id(getattr(st.graphs, k)) for k in ("entries", "fallback", "pool")})
    out.update({k: id(v) for k, v in net.__dict__.items() if k.startswith("_smpq")})
    return out


def _hit(memo, net, gpu, rs):
    """An evaluation that must be answered from the memo, launching nothing."""
    h, m, before = memo.report()["hits"], memo.report()["misses"], _snap(rs)
    cached = _engine_caches(net)
    r = _eval(net, gpu, rs)
    assert memo.report()["hits"] == h + 1 and memo.report()["misses"] == m
    assert _snap(rs) == before
    assert _engine_caches(net) == cached
    return r


def _miss(memo, net, gpu, rs, fn=_eval):
    h, m = memo.report()["hits"], memo.report()["misses"]
    r = fn(net, gpu, rs)
    assert memo.report()["hits"] == h and memo.report()["misses"] == m + 1
    return r


# ---- 1 -------------------------------------------------------------------------------------------
def test_hit_is_bitwise_and_launches_nothing(gpu, net, host, memo_on, capfd, monkeypatch):
    from smpq import stats
    from smpq.batches import ResidentSet
    monkeypatch.setattr(memo_on, "_ANNOUNCED", [False])
    capfd.readouterr()
    loader = Counting(host)
    rs = ResidentSet(loader, device=gpu)
    e0 = rs.report()["epoch"]
    h0, m0 = stats["memo_hits"], stats["memo_misses"]
    filled = _miss(memo_on, net, gpu, rs)  # the filling pass: a miss, recorded once the set is resident
    assert rs.report()["resident"] and rs.report()["epoch"] == e0 + 1
    assert memo_on.report()["entries"] == 1
    hit = _hit(memo_on, net, gpu, rs)
    rep = memo_on.report()
    assert rep["hits"] == 1 and rep["misses"] == 1 and rep["bypasses"] == 0
    assert rep["prob_bytes"] == 2 * 8 * 1000 * 4
    assert stats["memo_hits"] == h0 + 1 and stats["memo_misses"] == m0 + 1
    want = _plain(net, gpu, rs)
    assert type(hit[0]) is float and type(hit[1]) is float
    assert _same(hit, want) and _same(filled, want)
    assert loader.iterations == 1
    assert all(o.is_cuda and o.dtype == torch.float32 for o in hit[2])
    lines = [ln for ln in capfd.readouterr().err.splitlines() if "SMPQ_EVAL_MEMO" in ln]
    assert len(lines) == 1, lines  # one line at the (here: pretended) first hit of the process
    _hit(memo_on, net, gpu, rs)
    assert "SMPQ_EVAL_MEMO" not in capfd.readouterr().err


# ---- 2 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["static", "dynamic"])
def test_driver_step_restore_is_a_hit(gpu, host, memo_on, tmp_path, mode):
    """resnet50_main.py:176-237: accept a semilayer and save; quantize half of another conv, evaluate
    (a miss), reject: load the saved state and re-evaluate (:236) — a hit that equals the accepted
    evaluation and the same evaluation recomputed with the memo off."""
    from smpq import engine
    from smpq.batches import ResidentSet
    from test_gpu_driver import _quantize_semilayer
    model = build_model(gpu, "resnet18", None, "r18_u8_cal")
    rs = ResidentSet(host, device=gpu)
    engine.set_range_mode(mode)
    _miss(memo_on, model, gpu, rs)  # the initial evaluation fills the set
    conv = model.layer2[0].conv1
    _quantize_semilayer(conv, 4, range(conv.out_channels))
    accepted = _miss(memo_on, model, gpu, rs)
    pth = os.path.join(tmp_path, "step.pth")
    torch.save(model.state_dict(), pth)
    conv2 = model.layer3[1].conv2
    _quantize_semilayer(conv2, 4, range(conv2.out_channels // 2))
    trial = _miss(memo_on, model, gpu, rs)
    assert not _same(trial, accepted)
    model.load_state_dict(torch.load(pth, weights_only=True))
    debug = _hit(memo_on, model, gpu, rs)
    assert _same(debug, accepted)
    assert _same(debug, _plain(model, gpu, rs))


# ---- 3 -------------------------------------------------------------------------------------------
def test_key_is_content_only_and_entries_serve_both_functions(gpu, net, host, memo_on):
    import functions
    import resnet
    from smpq.batches import ResidentSet
    rs = ResidentSet(host, device=gpu)
    first = _miss(memo_on, net, gpu, rs)
    torch.manual_seed(99)
    other = resnet.resnet18().to(gpu).eval()  # separately constructed, other weights
    other.load_state_dict(net.state_dict())
    assert {t.data_ptr() for t in other.state_dict().values()}.isdisjoint(
        {t.data_ptr() for t in net.state_dict().values()})
    got = _hit(memo_on, other, gpu, rs)
    assert _same(got, first) and _same(got, _plain(other, gpu, rs))
    # evaluate_loss after evaluate_acc_loss_softmax of the same state: served from that entry, and
    # equal to the unmemoised evaluate_loss (the statistics do not depend on want_probs)
    h, before = memo_on.report()["hits"], _snap(rs)
    loss = functions.evaluate_loss(net, gpu, rs)
    assert memo_on.report()["hits"] == h + 1 and _snap(rs) == before
    assert type(loss) is float and loss == _plain(net, gpu, rs, "evaluate_loss") and loss == first[1]
    # the other way round: an entry without probabilities serves evaluate_loss only; the softmax
    # evaluation is a miss that upgrades it
    net.fc.bias.data[3] += 0.5
    l2 = _miss(memo_on, net, gpu, rs, functions.evaluate_loss)
    assert l2 == _plain(net, gpu, rs, "evaluate_loss")
    assert memo_on.report()["prob_bytes"] == 2 * 8 * 1000 * 4  # the first state's only
    up = _miss(memo_on, net, gpu, rs)
    assert up[1] == l2 and _same(up, _plain(net, gpu, rs))
    assert memo_on.report()["entries"] == 2 and memo_on.report()["prob_bytes"] == 2 * 2 * 8 * 1000 * 4
    assert _same(_hit(memo_on, net, gpu, rs), up)


# ---- 4 -------------------------------------------------------------------------------------------
def _w_elem(net):
    net.layer1[0].conv1.weight.data[3, 2, 1, 1] += 0.25


def _bn_var(net):
    net.layer2[0].bn1.running_var[5] *= 1.5


def _fc_bias(net):
    net.fc.bias.data[7] += 1.0


def _qstep(net):
    net.layer3[0].conv2.qstep[3] *= 2.0


def _bits_host(net):
    conv = net.layer1[1].conv2
    assert int(conv.qbits[3]) > 0
    conv._bits_host[3] = 0  # disagrees with qbits: the packing kind is chosen from this mirror


def _limbs(net):
    from smpq import ops
    ops.set_act_limbs(2 if ops.get_act_limbs() != 2 else 3)


def _range_mode(net):
    from smpq import engine
    engine.set_range_mode("dynamic" if engine.get_range_mode() == "static" else "static")


@pytest.mark.parametrize("change", [_w_elem, _bn_var, _fc_bias, _qstep, _bits_host, _limbs, _range_mode])
def test_every_change_is_a_miss_equal_to_the_unmemoised_result(gpu, net, host, memo_on, change):
    from smpq.batches import ResidentSet
    rs = ResidentSet(host, device=gpu)
    base = _miss(memo_on, net, gpu, rs)
    assert _same(_hit(memo_on, net, gpu, rs), base)
    with torch.no_grad():
        change(net)
    got = _miss(memo_on, net, gpu, rs)
    assert _same(got, _plain(net, gpu, rs))
    assert _same(_hit(memo_on, net, gpu, rs), got)


def test_invalidate_and_refill_is_a_miss(gpu, net, host, memo_on):
    from smpq.batches import ResidentSet
    loader = Counting(host)
    rs = ResidentSet(loader, device=gpu)
    base = _miss(memo_on, net, gpu, rs)
    _hit(memo_on, net, gpu, rs)
    e = rs.report()["epoch"]
    rs.invalidate()
    assert rs.report()["epoch"] == e + 1
    got = _miss(memo_on, net, gpu, rs)  # reads the loader again
    assert loader.iterations == 2 and rs.report()["epoch"] == e + 2
    assert memo_on.report()["entries"] == 1  # the earlier epoch's entry is gone
    assert _same(got, base) and _same(got, _plain(net, gpu, rs))
    _hit(memo_on, net, gpu, rs)


# ---- 5 -------------------------------------------------------------------------------------------
def _bypass(memo, net, gpu, loader):
    r0 = memo.report()
    got = _eval(net, gpu, loader)
    r1 = memo.report()
    assert r1["bypasses"] == r0["bypasses"] + 1
    assert (r1["hits"], r1["misses"], r1["entries"]) == (r0["hits"], r0["misses"], r0["entries"])
    return got


def test_bypasses(gpu, net, host, memo_on, monkeypatch):
    import torch.distributed as dist
    from smpq import engine
    from smpq.batches import ResidentSet
    want = _plain(net, gpu, host)
    for _ in range(2):
        assert _same(_bypass(memo_on, net, gpu, host), want)           # a plain list: nothing vouches for it
    sharded = ResidentSet(host, device=gpu, shard=(0, 1))
    for _ in range(3):
        assert _same(_bypass(memo_on, net, gpu, sharded), want)        # filling pass and resident passes
    small = ResidentSet(host, device=gpu, max_bytes=1)
    assert _same(_miss(memo_on, net, gpu, small), want)                 # (falls back during this pass)
    assert small.report()["fallback"] and memo_on.report()["entries"] == 0
    for _ in range(2):
        assert _same(_bypass(memo_on, net, gpu, small), want)
    rs = ResidentSet(host, device=gpu)
    assert _same(_miss(memo_on, net, gpu, rs), want)
    assert _same(_hit(memo_on, net, gpu, rs), want)
    assert not dist.is_initialized()
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)  # a single-rank group, as tests/test_dist.py makes them
    try:
        engine.set_dp_group(dist.group.WORLD)
        assert _same(_bypass(memo_on, net, gpu, rs), want)               # even for a recorded state
    finally:
        engine.set_dp_group(None)
        dist.destroy_process_group()
    assert memo_on.report()["entries"] == 1
    assert _same(_hit(memo_on, net, gpu, rs), want)


# ---- 6 -------------------------------------------------------------------------------------------
def test_pending_constant_channel_raises_on_a_would_be_hit(gpu, net, host, memo_on, monkeypatch):
    import functions
    from smpq import quant
    from smpq.batches import ResidentSet
    monkeypatch.setattr(quant, "DEFER", [True])
    rs = ResidentSet(host, device=gpu)
    conv = net.layer2[1].conv1
    conv.weight.data[5] = 0.125  # a constant channel (functions.py:40 divides by its zero range)
    base = _miss(memo_on, net, gpu, rs)
    assert _same(_hit(memo_on, net, gpu, rs), base)
    conv.weight.data = functions.channel_wise_quantizationperchan(conv.weight.data, 4, 5)  # deferred: no raise yet
    h = memo_on.report()["hits"]
    with pytest.raises(ZeroDivisionError):
        _eval(net, gpu, rs)
    assert memo_on.report()["hits"] == h
    # the failed call changed nothing and its metadata is put back: the state is the recorded one
    assert _same(_hit(memo_on, net, gpu, rs), base)
    assert _same(base, _plain(net, gpu, rs))


# ---- 7 -------------------------------------------------------------------------------------------
def test_lru_and_returned_tensors_are_private(gpu, net, host, memo_on):
    """Capacity 2, states A, B, A (a hit, which refreshes A), C (evicts B): A is still held and B is
    not. A is probed first: the miss on B is recorded in its turn and evicts the older of the two
    held then."""
    from smpq.batches import ResidentSet
    memo_on.enable(entries=2)
    rs = ResidentSet(host, device=gpu)
    bias = net.fc.bias.data
    a0 = bias.clone()

    def state(name):
        bias.copy_(a0)
        if name == "B":
            bias[0] += 1.0
        elif name == "C":
            bias[1] += 1.0
    state("A")
    ra = _miss(memo_on, net, gpu, rs)
    state("B")
    rb = _miss(memo_on, net, gpu, rs)
    state("A")
    assert _same(_hit(memo_on, net, gpu, rs), ra)
    state("C")
    _miss(memo_on, net, gpu, rs)
    assert memo_on.report()["entries"] == 2 and memo_on.report()["evictions"] == 1
    state("A")
    got = _hit(memo_on, net, gpu, rs)
    assert _same(got, ra)
    for o in got[2]:
        o.zero_()  # a caller scribbling over what it was given
    again = _hit(memo_on, net, gpu, rs)
    assert _same(again, ra) and _same(again, _plain(net, gpu, rs))
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(again[2], got[2]))
    state("B")
    assert _same(_miss(memo_on, net, gpu, rs), rb)
    assert memo_on.report()["evictions"] == 2
