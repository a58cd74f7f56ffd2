"""engine.GraphCache on the host: which inputs get a graph of their own, which go to the fallback,
and when captured graphs are released, driven with a fake capture on CPU tensors."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "semilayer-wise-mixed-precision-quantization_amd"))

from smpq import engine  # noqa: E402

BASE, BASE2 = ("sig", 1), ("sig", 2)


class FakeGraph:
    def __init__(self):
        self.replays = 0

    def replay(self):
        self.replays += 1


class FakeCtx:
    overflow = torch.zeros(2, dtype=torch.int32)


class Driver:
    """A GraphCache with a fake capture and a fake eager forward that record what they saw."""

    def __init__(self):
        self.cache = engine.GraphCache()
        self.captured = []          # the tensors a graph was captured on
        self.fallback_at_eager = []  # the cache's fallback entry at each eager forward
        self.overflow = 0

    def capture(self, x_in):
        self.captured.append(x_in)
        return engine.GraphEntry(FakeGraph(), FakeCtx(), torch.full((1,), float(len(self.captured))))

    def eager(self):
        self.fallback_at_eager.append(self.cache.fallback)
        return torch.zeros(1), torch.tensor([self.overflow, 0], dtype=torch.int32)

    def forward(self, x, base=BASE, capture=True):
        return self.cache.forward(x, base, self.eager, self.capture if capture else None)


@pytest.fixture
def slots():
    old = engine.GRAPHS_PER_MODEL[0]
    engine.GRAPHS_PER_MODEL[0] = 2
    yield 2
    engine.GRAPHS_PER_MODEL[0] = old


def test_addresses_get_entries_then_the_fallback(slots):
    d = Driver()
    xs = [torch.zeros(2, 3) for _ in range(3)]
    for x in xs:
        assert not d.cache.ready(x, BASE) and d.cache.lookup(x, BASE) is None
        d.forward(x)  # eager, then the capture
    assert len(d.fallback_at_eager) == 3 and len(d.captured) == 3
    assert len(d.cache.entries) == slots and d.captured[0] is xs[0] and d.captured[1] is xs[1]
    # the third address: a static copy of the input, captured as the fallback
    fb = d.cache.fallback
    assert fb is not None and fb.static_x is d.captured[2] and fb.static_x is not xs[2]
    assert all(e.static_x is None for e in d.cache.entries.values())
    # replays: each address its own graph; any further input of the shape through the fallback's copy
    x4 = torch.ones(2, 3)
    for x, entry in ((xs[0], d.cache.entries[engine._addr_key(xs[0])]), (xs[2], fb), (x4, fb)):
        n = entry.graph.replays
        assert d.cache.ready(x, BASE) and d.cache.lookup(x, BASE) is entry
        y, ovf = d.forward(x)
        assert entry.graph.replays == n + 1 and torch.equal(y, entry.logits) and y is not entry.logits
        assert ovf is FakeCtx.overflow
    assert torch.equal(fb.static_x, x4)  # the fallback read x4 from its static buffer
    assert len(d.fallback_at_eager) == 3 and len(d.captured) == 3  # nothing ran eagerly since


def test_each_shape_has_its_own_count(slots):
    d = Driver()
    a = [torch.zeros(2, 3) for _ in range(2)]
    b = [torch.zeros(4, 3) for _ in range(2)]
    for x in a + b:
        assert d.cache.has_slot(x)
        d.forward(x)
    assert len(d.cache.entries) == 4 and d.cache.fallback is None
    assert not d.cache.has_slot(torch.zeros(2, 3)) and not d.cache.has_slot(torch.zeros(4, 3))
    assert d.cache.has_slot(torch.zeros(5, 3))
    assert d.cache.has_slot(torch.zeros(2, 3, dtype=torch.float64))  # another dtype: another count


def test_non_contiguous_view_of_a_cached_address_never_matches(slots):
    d = Driver()
    x = torch.zeros(4, 4)
    d.forward(x)
    view = x.t()
    assert view.data_ptr() == x.data_ptr() and view.shape == x.shape and not view.is_contiguous()
    assert engine._addr_key(view) is None and not d.cache.has_slot(view)
    assert not d.cache.ready(view, BASE) and d.cache.lookup(view, BASE) is None
    d.forward(view)  # eager, then the fallback on a contiguous copy; x's entry is not replayed
    assert d.cache.entries[engine._addr_key(x)].graph.replays == 0
    assert d.cache.fallback.static_x.is_contiguous() and len(d.cache.entries) == 1
    assert d.cache.lookup(view, BASE) is d.cache.fallback


def test_changed_base_drops_the_entries_and_keeps_the_pool(slots):
    d = Driver()
    pool = d.cache.pool_for(torch.device("cpu"))
    xs = [torch.zeros(2, 3) for _ in range(3)]
    for x in xs:
        d.forward(x)
    old_entries, old_fallback = dict(d.cache.entries), d.cache.fallback
    assert len(old_entries) == 2 and old_fallback is not None
    # release point 1: the first call with another base drops every per-address entry at once
    assert not d.cache.ready(xs[0], BASE2)
    assert d.cache.entries == {} and d.cache.base == BASE2
    assert d.cache.pool_for(torch.device("cpu")) is pool
    # the old base's fallback matches nothing, and a free slot leaves it alone (release point 3)
    assert d.cache.fallback is old_fallback and d.cache.lookup(xs[2], BASE2) is None
    d.forward(xs[0], BASE2)
    assert d.cache.fallback is old_fallback and list(d.cache.entries) == [engine._addr_key(xs[0])]
    # a non-contiguous input does not get as far as release point 1 in ready(); lookup does
    assert not d.cache.ready(torch.zeros(5, 2).t(), BASE) and d.cache.base == BASE2
    assert d.cache.lookup(torch.zeros(5, 2).t(), BASE) is None and d.cache.base == BASE and d.cache.entries == {}
    assert d.cache.pool_for(torch.device("cpu")) is pool


def test_fallback_cleared_before_eager_only_without_a_free_slot(slots):
    d = Driver()
    xs = [torch.zeros(2, 3) for _ in range(3)]
    for x in xs:
        d.forward(x)
    fb = d.cache.fallback
    # another shape with its slots free: the (now unmatched) fallback survives the eager forward
    y = torch.zeros(4, 3)
    d.forward(y)
    assert d.fallback_at_eager[-1] is fb and d.cache.fallback is fb
    # the slots of that shape used up, the fallback of another key: cleared BEFORE the eager
    # forward (release point 3), replaced after the capture (release point 2)
    d.forward(torch.zeros(4, 3))
    assert d.cache.fallback is fb
    d.forward(torch.zeros(4, 3))
    assert d.fallback_at_eager[-1] is None
    fb2 = d.cache.fallback
    assert fb2 is not None and fb2 is not fb and tuple(fb2.static_x.shape) == (4, 3)
    # an overflowing eager forward, or capture left to the caller: no capture, the cleared
    # fallback stays cleared
    d.overflow = 1
    n = len(d.captured)
    d.forward(torch.zeros(2, 3))
    assert d.fallback_at_eager[-1] is None and d.cache.fallback is None and len(d.captured) == n
    d.overflow = 0
    x = torch.zeros(2, 3)
    d.forward(x, capture=False)
    assert d.cache.fallback is None and len(d.captured) == n
    d.cache.capture_for(x, BASE, d.capture)  # the caller's deferred capture
    assert d.cache.fallback is not None and len(d.captured) == n + 1


def test_no_slots_sends_everything_to_the_fallback():
    old = engine.GRAPHS_PER_MODEL[0]
    engine.GRAPHS_PER_MODEL[0] = 0
    try:
        d = Driver()
        pool = d.cache.pool_for(torch.device("cpu"))
        xs = [torch.full((2, 3), float(i)) for i in range(3)]
        for x in xs:
            d.forward(x)
        assert d.cache.entries == {} and len(d.captured) == 1 and len(d.fallback_at_eager) == 1
        fb = d.cache.fallback
        assert fb.graph.replays == 2 and torch.equal(fb.static_x, xs[2])
        d.cache.forget()  # every graph; the pool stays
        assert d.cache.fallback is None and d.cache.entries == {} and d.cache.pool_for(torch.device("cpu")) is pool
        d.forward(xs[0])
        assert len(d.captured) == 2 and d.cache.fallback is not fb
    finally:
        engine.GRAPHS_PER_MODEL[0] = old
