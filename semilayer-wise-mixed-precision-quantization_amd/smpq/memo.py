"""Evaluation memo: a whole-set evaluation that repeats an earlier one is answered from its record.

The search drivers re-evaluate the restored model after every rejected semilayer
(resnet50_main.py:227-237). That evaluation is a function of the weights and the loader only
(tests/test_gpu_driver.py), so it repeats, bit for bit, the evaluation of the accepted state. With
the memo on (``SMPQ_EVAL_MEMO=1`` or ``enable()``; off by default), the drop-in
``functions.evaluate_acc_loss_softmax`` / ``evaluate_loss`` key every evaluation on

  * the loader: a ``smpq.batches.ResidentSet`` (the only loader whose content somebody vouches
    for), as ``(id(set), epoch)``;
  * the model's content: name, dtype, shape and device fingerprint (``smpq_fingerprint``, one
    launch over all tensors, one device-to-host read) of every tensor of ``state_dict()``, every
    conv's host mirror of its bit-widths, the module tree's types and conv geometries;
  * every process-wide setting that selects arithmetic (``settings()``),

and a hit returns the recorded statistics and clones of the recorded softmax batches without
iterating the set or launching a forward. No ``id()`` of a tensor, ``data_ptr`` or ``_version`` is
in the model's part of the key: a freshly built or reloaded model with the same state hits.

Everything else is a counted bypass that runs the unmemoised code: another kind of net or loader, a
CPU device, a data-parallel group, a sharded set, a set in ``max_bytes`` fallback.
"""
import collections
import hashlib
import os
import struct
import sys
import weakref

import torch

from .qconv import QConv2d, stats

ENABLED = [os.environ.get("SMPQ_EVAL_MEMO", "0") == "1"]
_CAPACITY = [max(1, int(os.environ.get("SMPQ_EVAL_MEMO_ENTRIES", "4")))]
stats.setdefault("memo_hits", 0)
stats.setdefault("memo_misses", 0)


class Entry:
    """What one evaluation ended with: the four float64 statistics [loss sum, correct, seen,
    batches] as host numbers and, from evaluate_acc_loss_softmax, its per-batch softmax tensors."""
    __slots__ = ("stats", "probs")

    def __init__(self, stats4, probs=None):
        self.stats = tuple(float(v) for v in stats4)
        self.probs = probs

    def nbytes(self):
        return sum(p.numel() * p.element_size() for p in self.probs or ())


class LRU:
    """``capacity`` entries, least recently used out first; a hit refreshes recency."""

    def __init__(self, capacity):
        self.capacity = max(1, int(capacity))
        self.items = collections.OrderedDict()
        self.evictions = 0

    def get(self, key):
        e = self.items.get(key)
        if e is not None:
            self.items.move_to_end(key)
        return e

    def put(self, key, entry):
        self.items[key] = entry
        self.items.move_to_end(key)
        while len(self.items) > self.capacity:
            self.items.popitem(last=False)
            self.evictions += 1

    def drop(self, pred):
        for k in [k for k in self.items if pred(k)]:
            del self.items[k]


_LRU = LRU(_CAPACITY[0])
_COUNTS = {"hits": 0, "misses": 0, "bypasses": 0}
_SETS = {}           # id(set) -> (weak reference, the epoch its entries were made at)
_FPS = weakref.WeakKeyDictionary()  # model -> (layout, Fingerprinter): rebuilt when a tensor moves
_ANNOUNCED = [False]


def enable(entries=None):
    """Switch the memo on; ``entries`` resizes the LRU (default: keep SMPQ_EVAL_MEMO_ENTRIES)."""
    if entries is not None:
        _LRU.capacity = max(1, int(entries))
        while len(_LRU.items) > _LRU.capacity:
            _LRU.items.popitem(last=False)
            _LRU.evictions += 1
    ENABLED[0] = True


def disable():
    """Switch the memo off (its entries stay until clear())."""
    ENABLED[0] = False


def enabled():
    return ENABLED[0]


def clear():
    """Drop every entry and zero the counters of report()."""
    _LRU.items.clear()
    _LRU.evictions = 0
    _SETS.clear()
    for k in _COUNTS:
        _COUNTS[k] = 0


def report():
    """hits, misses, bypasses, entries held, evictions, bytes of the cached softmax tensors."""
    r = dict(_COUNTS)
    r.update(entries=len(_LRU.items), evictions=_LRU.evictions, capacity=_LRU.capacity, enabled=ENABLED[0],
             prob_bytes=sum(e.nbytes() for e in _LRU.items.values()))
    return r


# ---- the key ------------------------------------------------------------------------------------
def settings():
    """Every process-wide setting that selects arithmetic, or that no test shows to be bitwise
    neutral: the range mode, the activation limbs, the static ranges' headroom and the knobs every
    captured graph is keyed on (engine._graph_base), plus graph replay itself."""
    from . import engine, ops
    return (("range_mode", engine.get_range_mode()), ("act_limbs", ops.get_act_limbs()),
            ("headroom", float(engine.HEADROOM)), ("chunk", engine.CHUNK[0]), ("fused_stem", engine.FUSED_STEM[0]),
            ("concurrent_ds", engine.CONCURRENT_DS[0]), ("streams", engine.STREAMS[0]), ("kmajor", ops.KMAJOR[0]),
            ("pair_1x1", engine.PAIR_1X1[0]), ("fuse_ds", engine.FUSE_DS[0]),
            ("fuse_ds_max_cin", engine.FUSE_DS_MAX_CIN[0]), ("pair_stage_entry", engine.PAIR_STAGE_ENTRY[0]),
            ("use_graph", engine.USE_GRAPH[0]), ("serial_slices", engine.SERIAL_SLICES[0]))


def structure(net, keep=None):
    """Structural signature of the module tree: each module's name and type, each conv's geometry.
    ``keep(name)``: only the modules it accepts (smpq.prefix: the modules upstream of a boundary)."""
    out = []
    for name, m in net.named_modules():
        if keep is not None and not keep(name):
            continue
        row = [name, type(m).__module__ + "." + type(m).__qualname__]
        if isinstance(m, torch.nn.Conv2d):
            row += [m.in_channels, m.out_channels, tuple(m.kernel_size), tuple(m.stride), tuple(m.padding),
                    m.groups, tuple(m.dilation), m.padding_mode]
        elif isinstance(m, torch.nn.BatchNorm2d):
            row += [m.eps, m.affine, m.track_running_stats]
        out.append(tuple(row))
    return (tuple(out), bool(getattr(net, "fused", False)), bool(net.training))


def compose_key(tensors, digests, bits_host, struct_sig, setting_items):
    """SHA-256 over, in order: (name, dtype, shape, 64-bit content digest) of every tensor,
    (name, bytes) of every conv's host bit-width mirror, the structural signature, the settings.
    ``tensors``: (name, dtype, shape) triples; ``digests``: one int per tensor."""
    h = hashlib.sha256()
    h.update(b"smpq-eval-memo/1\0")
    h.update(struct.pack("<q", len(tensors)))
    for (name, dtype, shape), d in zip(tensors, digests):
        h.update(("%s\0%s\0%s\0" % (name, dtype, tuple(shape))).encode())
        h.update(struct.pack("<Q", int(d) & 0xFFFFFFFFFFFFFFFF))
    h.update(b"\1bits\0")
    for name, b in bits_host:
        h.update(name.encode() + b"\0" + bytes(b) + b"\0")
    h.update(b"\1tree\0" + repr(struct_sig).encode())
    h.update(b"\1knobs\0" + repr(tuple(setting_items)).encode())
    return h.hexdigest()


def device_digests(net, named):
    """Fingerprints of the (non-empty) tensors of ``named`` in one launch and one host read. The
    launch tables are kept per model while no tensor moves (the restore through load_state_dict
    copies in place)."""
    from .fingerprint import Fingerprinter
    ts = [t for _, t in named if t.numel() > 0]
    if not ts:
        return [0] * len(named)
    layout = tuple((t.data_ptr(), t.numel() * t.element_size()) for t in ts)
    dev = ts[0].device
    cached = _FPS.get(net)
    if cached is not None and cached[0] == (layout, dev):
        fp = cached[1]
        now = fp.compute(fp.now)
    else:
        if any(t.device != dev for t in ts):
            raise ValueError("smpq memo: the model's tensors lie on several devices")
        fp = Fingerprinter(ts, dev)  # raises ValueError for a tensor it cannot cover
        _FPS[net] = ((layout, dev), fp)
        now = fp.ref
    it = iter(now.tolist())
    return [next(it) if t.numel() > 0 else 0 for _, t in named]


def bits_rows(net):
    """(name, dtype + shape + bytes) of every conv's host mirror of its bit-widths."""
    bits = []
    for name, m in net.named_modules():
        if isinstance(m, QConv2d):
            b = m._bits_host
            bits.append((name, ("%s%s" % (b.dtype.str, b.shape)).encode() + b.tobytes()))
    return bits


def state_key(net, digest=None):
    """The content key of ``net`` under the current settings. ``digest(net, named)`` returns one
    integer per (name, tensor) of ``state_dict()`` (default: the device fingerprints)."""
    named = [(k, v.detach()) for k, v in net.state_dict().items()]
    digests = (digest or device_digests)(net, named)
    return compose_key([(k, str(t.dtype), tuple(t.shape)) for k, t in named], digests, bits_rows(net), structure(net),
                       settings())


# ---- the evaluation's side ---------------------------------------------------------------------
class Token:
    """One memoisable evaluation between begin() and finish(): a hit (``entry`` set) or a miss."""
    __slots__ = ("digest", "rs", "epoch", "resident", "want_probs", "entry")


def _eligible(net, dev, loader):
    from . import engine
    from .batches import ResidentSet
    from .models import ResNet
    return (isinstance(net, ResNet) and dev.type == "cuda" and engine.get_dp_group() is None
            and isinstance(loader, ResidentSet) and loader.shard is None and not loader._fallback
            and (loader.dev is None or loader.dev == dev))


def _forget(sid):
    _SETS.pop(sid, None)
    _LRU.drop(lambda k: k[0] == sid)


def _set_key(rs):
    """(id(set), epoch), after dropping what was recorded for an earlier epoch of this set (or for
    a dead set whose id this one took over)."""
    sid = id(rs)
    known = _SETS.get(sid)
    if known is not None and (known[0]() is not rs or known[1] != rs._epoch):
        _forget(sid)
        known = None
    if known is None:
        _SETS[sid] = (weakref.ref(rs, lambda _r, sid=sid: _forget(sid)), rs._epoch)
    return (sid, rs._epoch)


def begin(net, dev, loader, want_probs):
    """Called by functions._run_eval after ``net.to(device)`` / ``net.eval()``. Returns None for a
    bypass (counted), else a Token: with ``entry`` set it is a hit and nothing is to be run."""
    if not _eligible(net, dev, loader):
        _COUNTS["bypasses"] += 1
        return None
    from .quant import check_pending
    check_pending()  # a deferred constant-channel ZeroDivisionError surfaces on a hit too
    try:
        digest = state_key(net)
    except ValueError:  # a tensor the fingerprint kernel cannot cover: nothing vouches for it
        _COUNTS["bypasses"] += 1
        return None
    t = Token()
    t.digest, t.rs, t.epoch, t.want_probs, t.entry = digest, loader, loader._epoch, want_probs, None
    t.resident = loader._cache is not None
    if t.resident:
        e = _LRU.get(_set_key(loader) + (digest,))
        if e is not None and (e.probs is not None or not want_probs):
            t.entry = e
            _COUNTS["hits"] += 1
            stats["memo_hits"] += 1
            if not _ANNOUNCED[0]:
                _ANNOUNCED[0] = True
                print("smpq memo: SMPQ_EVAL_MEMO=1 -> an evaluation that repeats an earlier one (same weights, "
                      "same resident set, same settings) is answered from its record, without a forward",
                      file=sys.stderr)
            return t
    _COUNTS["misses"] += 1
    stats["memo_misses"] += 1
    return t


def hit_result(token):
    """(statistics as a host float64 tensor, fresh clones of the recorded softmax batches)."""
    e = token.entry
    outs = [p.clone() for p in e.probs] if token.want_probs else []
    return torch.tensor(e.stats, dtype=torch.float64), outs


def finish(token, stats4, outputs):
    """After a miss ran to its end: record it if the set is resident now with the content the pass
    served (the filling pass installs its cache at its end, which moves the epoch once). Returns
    the statistics as a host tensor (the evaluation's one host sync happens here)."""
    host = stats4.tolist()
    rs = token.rs
    served = token.epoch if token.resident else token.epoch + 1
    if rs._cache is not None and not rs._fallback and rs._epoch == served:
        key = _set_key(rs) + (token.digest,)
        old = _LRU.items.get(key)
        probs = [p.clone() for p in outputs] if token.want_probs else (old.probs if old is not None else None)
        _LRU.put(key, Entry(host, probs))
    return torch.tensor(host, dtype=torch.float64)
