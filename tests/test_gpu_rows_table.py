"""The rows route of smpq.suffix on the GPU: delta-loss tables whose trials of a
block's last conv recompute only the patched output channel into the kept input of the next block
(rows=True) against the same tables without it (rows=False), both with suffix=True, bit for bit; which
trials took the route; what a table leaves behind. Models, batches and fixtures are
tests/test_gpu_suffix.py's."""
import numpy as np
import pytest
import torch

from test_gpu import build_model
from test_gpu_sensitivity import _operands, knobs  # noqa: F401  (knobs: a fixture)
from test_gpu_suffix import CAL, ZERO, _counts, _delta, _mixed_batches, _same_bits, _set

pytestmark = pytest.mark.gpu

BITS = (8, 4)
# ResNet-18: lnum 12 = layer3.1.conv2 and 14 = layer4.0.conv2 (last convs: 3x3, K = 2304 and 4608 =
# the kernel's longest row), 13 = layer4.0.conv1 (not a last conv, same block as 14)
R18 = {12: [0, 255], 13: [7], 14: [1, 511]}
R18_LAST = {12: "layer3.1", 14: "layer4.0"}
# ResNet-50: lnum 27 = layer3.1.conv3, 39 = layer3.5.conv3 (the next block is a stage entry),
# 45 = layer4.1.conv3 (the next block is the net's last), 25 = layer3.1.conv1 (not a last conv)
R50 = {25: [3], 27: [0, 1023], 39: [512], 45: [2047]}
R50_LAST = {27: "layer3.1", 39: "layer3.5", 45: "layer4.1"}

_BASE = {}


def _without_rows(gpu, arch, graph, limbs, sizes, channels):
    """The suffix route's table of one case (rows=False), computed once and shared (never written to)."""
    key = (arch, graph, limbs, sizes)
    if key not in _BASE:
        _set(graph, limbs)
        net = build_model(gpu, arch, None, CAL[arch])
        _BASE[key] = _delta(net, _mixed_batches(gpu, sizes), channels, BITS, suffix=True, rows=False)
    return _BASE[key]


def _check(gpu, arch, graph, limbs, sizes, channels, last):
    from smpq import sensitivity
    off = _without_rows(gpu, arch, graph, limbs, sizes, channels)
    _set(graph, limbs)
    net = build_model(gpu, arch, None, CAL[arch])
    dev = _mixed_batches(gpu, sizes)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    on = _delta(net, dev, channels, BITS, suffix=True, rows=True)
    # the same table, bit for bit: delta, eval_loss, the statistics and the flags' consequences
    assert on.bits == off.bits and on.lnum.tolist() == off.lnum.tolist() and on.cnum.tolist() == off.cnum.tolist()
    for bit in off.bits:
        assert np.isfinite(off.stats[bit]).all()
        assert _same_bits(on.stats[bit], off.stats[bit]), (bit, on.stats[bit], off.stats[bit])
        assert _same_bits(on.delta[bit], off.delta[bit]), bit
    assert _same_bits(on.base_loss, off.base_loss) and _same_bits(on.eval_loss, off.eval_loss)
    ron, roff = on.report(), off.report()
    assert _counts(ron) == _counts(roff), (ron, roff)
    assert ron["patched"] == ron["trials"] and not ron["slow"] and not ron["overflowed"] and not ron["constant"], ron
    assert ron["during_trials"] == ZERO and roff["during_trials"] == ZERO
    # rows trials for the last convs only
    rows = {b["name"]: b for b in ron["suffix"]["blocks"]}
    expect = {}
    for ln, name in last.items():
        expect[name] = expect.get(name, 0) + len(channels[ln]) * len(BITS)
    for name, b in rows.items():
        assert b["rows"] == "used" and b["rows_self_check"] is True and b["self_check"] is True, b
        assert b["rows_kept"] == b["kept"] == len(sizes) and b["rows_bytes"] > 0 and b["rows_self_check_s"] > 0, b
        assert b["bytes"] == b["rows_bytes"] + sum(_kept_bytes(net, x, b["block"]) for x, _ in dev), b
        assert b["rows_trials"] == expect.get(name, 0), (name, b)
    assert sum(b["rows_trials"] for b in rows.values()) == sum(len(channels[ln]) for ln in last) * len(BITS)
    for b in roff["suffix"]["blocks"]:
        assert b["rows"] == "off" and b["rows_trials"] == 0 and b["rows_bytes"] == 0 and b["rows_self_check"] is None
    # the model is as it was, and an ordinary evaluation after the table equals the one before it
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert _same_bits(sensitivity.ordinary_loss(net, dev), on.eval_loss)
    return on


def _kept_bytes(net, x, j):
    from smpq import suffix
    return suffix.kept_bytes(net, x, j)


@pytest.mark.parametrize("graph,limbs", [(True, 3), (False, 3), (True, 2)])
def test_rows_table_equals_the_suffix_route_resnet18(gpu, knobs, graph, limbs):  # noqa: F811
    on = _check(gpu, "resnet18", graph, limbs, (8, 8), R18, R18_LAST)
    assert [b["name"] for b in on.report()["suffix"]["blocks"]] == ["layer3.1", "layer4.0"]


@pytest.mark.parametrize("graph,limbs", [(True, 3), (False, 3), (True, 2)])
def test_rows_table_equals_the_suffix_route_resnet50(gpu, knobs, graph, limbs):  # noqa: F811
    on = _check(gpu, "resnet50", graph, limbs, (4, 4), R50, R50_LAST)
    assert [b["name"] for b in on.report()["suffix"]["blocks"]] == ["layer3.1", "layer3.5", "layer4.1"]


def test_the_last_block_and_the_budget_keep_the_suffix_route(gpu, knobs):  # noqa: F811
    """lnum 16 is the last conv of ResNet-18's last block (its output is fp32: no rows route); with a
    budget of one batch's block input no batch fits with the extra tensors, so layer4.0's are kept
    without them. Both tables equal the unbounded one."""
    from smpq import suffix
    _set(True, 3)
    channels = {14: [1], 16: [0]}
    dev = _mixed_batches(gpu, (8, 8))
    tables = []
    for budget in (None, "two"):
        net = build_model(gpu, "resnet18", None, CAL["resnet18"])
        nb = 2 * suffix.kept_bytes(net, dev[0][0], 6) if budget else None
        tables.append(_delta(net, dev, channels, (4,), suffix=True, rows=True, suffix_bytes=nb))
    full, tight = tables
    assert _same_bits(full.stats[4], tight.stats[4]) and np.isfinite(full.stats[4]).all()
    rows = {b["name"]: b for b in full.report()["suffix"]["blocks"]}
    assert (rows["layer4.0"]["rows"], rows["layer4.0"]["rows_trials"]) == ("used", 1)
    assert (rows["layer4.1"]["rows"], rows["layer4.1"]["rows_trials"], rows["layer4.1"]["kept"]) == ("last_block", 0, 2)
    rows = {b["name"]: b for b in tight.report()["suffix"]["blocks"]}
    assert (rows["layer4.0"]["rows"], rows["layer4.0"]["rows_trials"], rows["layer4.0"]["kept"]) == ("budget", 0, 2)
    assert rows["layer4.0"]["rows_bytes"] == 0 and rows["layer4.0"]["bytes"] == 2 * suffix.kept_bytes(net, dev[0][0], 6)


def test_the_switch_is_off_by_default_and_needs_the_suffix(gpu, knobs):  # noqa: F811
    _set(True, 3)
    dev = _mixed_batches(gpu, (8, 8))
    net = build_model(gpu, "resnet18", None, CAL["resnet18"])
    default = _delta(net, dev, {14: [1]}, (4,), suffix=True)
    assert [b["rows"] for b in default.report()["suffix"]["blocks"]] == ["off"]
    alone = _delta(net, dev, {14: [1]}, (4,), suffix=False, rows=True)
    assert alone.report()["suffix"] == {} and _same_bits(alone.stats[4], default.stats[4])
