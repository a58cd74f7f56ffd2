"""smpq.prefix on the host: the boundary keys (with fake per-tensor digests standing in for the
device fingerprints), the refill rule as a state machine over key sequences, and the byte budget."""
import pytest
import torch


@pytest.fixture(scope="module", params=["resnet50", "resnet18"])
def net(request):
    import resnet
    torch.manual_seed(0)
    with torch.device("meta"):  # names, shapes and the module tree only: the digests are fake
        return getattr(resnet, request.param)().eval()


def _convs(net):
    from smpq.qconv import QConv2d
    return [(name, m) for name, m in net.named_modules() if isinstance(m, QConv2d)]


class Keys:
    """boundary_keys of ``net`` under fake digests and ranges that single entries of can be moved."""

    def __init__(self, net):
        self.net = net
        self.digests = {k: 1000 + i for i, k in enumerate(net.state_dict())}
        self.ranges = {id(m): 1.0 + i for i, (_, m) in enumerate(_convs(net))}
        self.set_key = (7, 1)

    def __call__(self, name):
        from smpq import prefix
        j = prefix.block_index(self.net, name)
        return prefix.boundary_keys(self.net, [j], self.ranges, set_key=self.set_key,
                                    digest=lambda net, named: [self.digests[k] for k, _ in named])[j]


def _is_upstream(name, net, boundary):
    from smpq import prefix
    ups = ("conv1", "bn1") + tuple(prefix.block_names(net)[:prefix.block_index(net, boundary)])
    return any(name.startswith(p + ".") or name == p for p in ups)


# ---- 1: key locality -----------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", ["layer4.0", "layer3.0"])
def test_key_changes_when_and_only_when_something_upstream_changes(net, boundary):
    from smpq import prefix
    keys = Keys(net)
    k0 = keys(boundary)
    assert k0 == keys(boundary)
    up = down = 0
    for name in net.state_dict():  # every tensor's digest
        keys.digests[name] += 1
        if _is_upstream(name, net, boundary):
            assert keys(boundary) != k0, name
            up += 1
        else:
            assert keys(boundary) == k0, name
            down += 1
        keys.digests[name] -= 1
    assert up > 0 and down > 0
    names = [n for n in net.state_dict() if not _is_upstream(n, net, boundary)]
    assert any(n.startswith("fc.") for n in names) and any(n.startswith("layer4.") for n in names)
    assert not any(n.startswith(("conv1.", "bn1.", "layer1.", "layer2.")) for n in names)
    assert any(n.startswith("layer3.") for n in names) == (boundary == "layer3.0")
    for name, conv in _convs(net):  # every conv's range and bit-width mirror
        keys.ranges[id(conv)] *= 1.5
        assert (keys(boundary) != k0) == _is_upstream(name, net, boundary), name
        keys.ranges[id(conv)] /= 1.5
        old = int(conv._bits_host[0])
        conv._bits_host[0] = 4 if old != 4 else 6
        assert (keys(boundary) != k0) == _is_upstream(name, net, boundary), name
        conv._bits_host[0] = old
    assert keys(boundary) == k0
    assert k0 != keys("layer3.0" if boundary == "layer4.0" else "layer4.0")  # the boundary's name is in its key
    keys.set_key = (7, 2)  # the set's epoch
    assert keys(boundary) != k0
    keys.set_key = (7, 1)
    assert keys(boundary) == k0
    with pytest.raises(ValueError):
        prefix.block_index(net, "layer4.9")
    with pytest.raises(ValueError):
        prefix.block_index(net, "fc")


def test_key_changes_with_settings_and_upstream_structure(net, monkeypatch):
    from smpq import engine, ops
    keys = Keys(net)
    k0 = keys("layer4.0")
    monkeypatch.setattr(ops, "_ACT_LIMBS", [2 if ops.get_act_limbs() != 2 else 3])
    assert keys("layer4.0") != k0
    monkeypatch.undo()
    monkeypatch.setattr(engine, "STREAMS", [engine.STREAMS[0] + 1])
    assert keys("layer4.0") != k0
    monkeypatch.undo()
    monkeypatch.setattr(engine, "USE_GRAPH", [not engine.USE_GRAPH[0]])
    assert keys("layer4.0") != k0
    monkeypatch.undo()
    assert keys("layer4.0") == k0
    blk = net.layer2[0]
    conv = blk.conv2 if hasattr(blk, "conv3") else blk.conv1   # the stage's strided conv
    assert conv.stride == (2, 2)
    monkeypatch.setattr(conv, "stride", (1, 1))          # upstream geometry
    assert keys("layer4.0") != k0
    monkeypatch.undo()
    conv = net.layer4[1].conv1
    monkeypatch.setattr(conv, "stride", (2, 2))          # downstream geometry
    assert keys("layer4.0") == k0


def test_key_is_content_only():
    """The same upstream state in another model object, at other addresses, gives the same key."""
    import hashlib

    import resnet
    from smpq import prefix

    def digest(net, named):
        return [int.from_bytes(hashlib.sha256(t.contiguous().numpy().tobytes()).digest()[:8], "little")
                for _, t in named]
    torch.manual_seed(0)
    a = resnet.resnet18(num_classes=10).eval()
    torch.manual_seed(5)
    b = resnet.resnet18(num_classes=10).eval()
    j = prefix.block_index(a, "layer4.0")

    def key(m):
        ranges = {id(c): 2.0 + i for i, (_, c) in enumerate(_convs(m))}
        return prefix.boundary_keys(m, [j], ranges, set_key=(1, 1), digest=digest)[j]
    assert key(a) != key(b)
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    for k in sd:
        if k.startswith(("layer4.", "fc.")):  # what lies downstream may differ
            sd[k] = b.state_dict()[k].clone()
    b.load_state_dict(sd)
    assert key(a) == key(b)


# ---- 2: the refill rule --------------------------------------------------------------------------
def _play(b, keys, ok=True):
    """Run the key sequence through the state machine as an evaluation loop would; returns the
    verdicts."""
    out = []
    for k in keys:
        v = b.decide(k)
        if v == "fill":
            b.begin_fill(k)
            b.end_fill(ok)
        out.append(v)
    return out


def test_refill_rule():
    from smpq.prefix import Boundary
    b = Boundary("layer4.0", 13)
    assert _play(b, ["A"]) == ["fill"] and b.valid and b.key == "A"       # an empty boundary fills at once
    # a sensitivity pass: one-off trial states never replace the pristine prefix
    assert _play(b, ["B", "A", "C", "A"]) == ["skip", "hit", "skip", "hit"] and b.key == "A" and b.valid
    # an acceptance: B replaces A during the second B, and is resumed from afterwards
    assert _play(b, ["B", "B", "B"]) == ["skip", "fill", "hit"] and b.key == "B" and b.valid
    # a pass that does not compute the boundary in full (it resumed downstream) cannot fill it
    assert b.decide("C", in_full=False) == "skip" and b.decide("C", in_full=False) == "skip" and b.key == "B"
    assert b.decide("C") == "fill"


def test_abandoned_fill_leaves_the_boundary_invalid():
    from smpq.prefix import Boundary
    b = Boundary("layer3.0", 7)
    _play(b, ["A"])
    assert b.decide("B") == "skip" and b.decide("B") == "fill"
    b.begin_fill("B")
    assert not b.valid                       # invalid first: an interrupted pass leaves nothing usable
    assert b.decide("A") != "hit"            # ... and not A either
    b.end_fill(False)
    assert not b.valid and b.key is None
    assert _play(b, ["C"]) == ["fill"] and b.valid and b.key == "C"       # empty: the next pass fills at once


# ---- 3: budget -----------------------------------------------------------------------------------
def test_bytes_per_image():
    import resnet
    from smpq import prefix
    with torch.device("meta"):
        r50, r18 = resnet.resnet50(), resnet.resnet18()
    for net, name, want in ((r50, "layer3.0", 1204224), (r50, "layer4.0", 602112), (r18, "layer4.0", 150528)):
        limbs, n, h, w, c = prefix.boundary_shape(net, prefix.block_index(net, name), 1, 224, 224, 3)
        assert (limbs, n) == (3, 1)
        assert prefix.boundary_bytes(limbs, c, h, w, 1) == limbs * c * h * w == want
        assert prefix.boundary_bytes(limbs, c, h, w, 50000) == 50000 * want
        assert prefix.boundary_bytes(2, c, h, w, 3) * 3 == prefix.boundary_bytes(3, c, h, w, 3) * 2
    assert prefix.boundary_shape(r50, 0, 5, 224, 224, 3) == (3, 5, 56, 56, 64)
    assert prefix.boundary_shape(r50, prefix.block_index(r50, "layer2.0"), 2, 225, 193, 2) == (2, 2, 57, 49, 256)
    assert round(50000 * 1204224 / 1e9, 1) == 60.2 and round(50000 * 602112 / 1e9, 1) == 30.1


def test_admission_is_deepest_first():
    from smpq.prefix import admit
    sizes = [(7, 1204224 * 100), (13, 602112 * 100)]
    assert admit(sizes, sum(nb for _, nb in sizes)) == ([13, 7], [])
    assert admit(sizes, 1204224 * 100) == ([13], [7])                  # the deepest first, although the other fits alone
    assert admit(sizes, 602112 * 100 - 1) == ([], [13, 7])             # nothing fits: refused and counted, no error
    assert admit([(3, 10), (7, 50), (13, 20)], 35) == ([13, 3], [7])   # a refusal does not stop the shallower ones
    assert admit([], 10) == ([], [])
