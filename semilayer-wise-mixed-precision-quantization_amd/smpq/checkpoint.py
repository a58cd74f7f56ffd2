""".pth checkpoints + bit-assignment sidecar.

The reference's drivers checkpoint and roll back with plain state dicts
(resnet50_main.py:212 ``torch.save(net.state_dict(), pthname)``, :233-234 / :426-427
``net.load_state_dict(torch.load(pthname))``). Those files carry fake-quantized fp32 weights
only: the bit-widths are implicit in the values. Our QConv2d keeps ``qbits``/``qstep`` buffers
(qconv.py), so a state dict written by this package reloads with its metadata. This module covers
the other two cases:

* ``save_checkpoint`` writes the state dict plus ``<path>.bits.json``, the per-channel bit
  assignment in the reference's own vocabulary (lnum -> per-channel bits, 0 = never quantized)
  and the exact fp32 step of every channel (its IEEE bit pattern in hex), readable without torch
  by the search drivers' bookkeeping. By default (``plain=True``) the ``.pth`` holds exactly the
  reference's keys (no ``qbits``/``qstep``), so the reference's and torchvision's
  ``load_state_dict(strict=True)`` accept it; the sidecar restores the metadata bitwise;
* ``load_checkpoint`` / ``infer_quant_`` recover the metadata of a reference-written ``.pth``
  (no ``qbits``/``qstep`` keys): per channel, the smallest bit-width b whose re-quantization
  (functions.py:25-43 restated on the native library) leaves the channel bitwise unchanged is
  recorded with its step. A sidecar, when present, restricts the search to the recorded bit.
  The packer still verifies every code bitwise (smpq_pack_weights), so a wrong inference can
  only send a channel to the fixed-point path, never change a result;
* ``snapshot`` / ``restore_`` / ``save_packed`` / ``load_packed`` / ``packed_report``: the same
  state with every QConv2d weight bit-packed (format smpq-packed/1, include/smpq.h), in memory on
  the net's device for the search's rollback, or as one file of the size the assignment promises.
"""
import json
import os

import numpy as np
import torch

from . import ops
from .assignments import addressable_convs

SIDECAR_SUFFIX = ".bits.json"
CANDIDATE_BITS = (2, 3, 4, 5, 6, 7, 8)


def sidecar_path(path):
    return str(path) + SIDECAR_SUFFIX


def bit_assignment(net):
    """{lnum: [bits per output channel]} over the addressable convs (lnum from 1, the drivers'
    numbering: resnet50_main.py:81-136, resnet18_main.py:86-115)."""
    out = {}
    for ln, conv in enumerate(addressable_convs(net), start=1):
        out[ln] = [int(b) for b in conv.qbits.detach().cpu().tolist()]
    return out


META_KEYS = (".qbits", ".qstep")


def plain_state_dict(net):
    """``net.state_dict()`` without the quantization metadata buffers: the reference's keys only."""
    return {k: v for k, v in net.state_dict().items() if not k.endswith(META_KEYS)}


def step_assignment(net):
    """{lnum: [fp32 step per output channel as its IEEE bit pattern, 8 hex digits]}."""
    out = {}
    for ln, conv in enumerate(addressable_convs(net), start=1):
        bits = conv.qstep.detach().cpu().contiguous().view(torch.int32).numpy().astype(np.uint32)
        out[ln] = ["%08x" % int(b) for b in bits]
    return out


def save_checkpoint(net, path, plain=True):
    """``torch.save(net.state_dict(), path)`` + ``<path>.bits.json`` (bits + exact steps). With
    ``plain`` the .pth carries the reference's keys only (loadable with strict=True by the
    reference's / torchvision's ResNet); otherwise it also keeps the qbits/qstep buffers."""
    from .quant import check_pending
    check_pending()
    torch.save(plain_state_dict(net) if plain else net.state_dict(), path)
    side = {"format": "smpq-bits/2", "convs": {str(k): v for k, v in bit_assignment(net).items()},
            "steps": {str(k): v for k, v in step_assignment(net).items()}}
    with open(sidecar_path(path), "w") as f:
        json.dump(side, f)


def _read_sidecar_full(path):
    p = sidecar_path(path)
    if not os.path.exists(p):
        return None, None
    with open(p) as f:
        side = json.load(f)
    fmt = side.get("format")
    if fmt not in ("smpq-bits/1", "smpq-bits/2"):
        raise ValueError("%s: unknown sidecar format %r" % (p, fmt))
    bits = {int(k): np.asarray(v, dtype=np.int64) for k, v in side["convs"].items()}
    steps = None
    if fmt == "smpq-bits/2":
        steps = {int(k): np.array([int(h, 16) for h in v], dtype=np.uint32).view(np.float32)
                 for k, v in side["steps"].items()}
    return bits, steps


def read_sidecar(path):
    """{lnum: int array of bits per channel} from ``<path>.bits.json``, or None."""
    return _read_sidecar_full(path)[0]


def read_sidecar_steps(path):
    """{lnum: fp32 array of exact steps per channel} (format smpq-bits/2), or None."""
    return _read_sidecar_full(path)[1]


def infer_quant_(conv, allowed=None):
    """Record (bit, step) for channels of ``conv`` that carry no metadata but whose weights lie on
    the reference quantizer's grid. ``allowed``: optional int array [cout] restricting channel c to
    bit allowed[c] (0 = leave). Returns the number of channels recorded."""
    w2d = conv.weight.detach().reshape(conv.out_channels, -1).to(torch.float32).contiguous()
    cout = conv.out_channels
    # channels already carrying metadata, and constant channels (the reference quantizer divides
    # by zero on them, functions.py:40), are left alone
    known = conv.qbits.detach().cpu().numpy() > 0
    known |= (w2d.amax(dim=1) == w2d.amin(dim=1)).cpu().numpy()
    found = np.zeros(cout, dtype=np.int64)
    steps = torch.zeros(cout, dtype=torch.float32, device=w2d.device)
    cands = CANDIDATE_BITS if allowed is None else sorted({int(b) for b in np.asarray(allowed) if b > 0})
    for b in cands:
        todo = ~known & (found == 0)
        if allowed is not None:
            todo &= np.asarray(allowed) == b
        if not todo.any():
            continue
        # the channel may have been written by torch on the CPU or on the GPU (functions.py:41
        # rounds differently there, ops.QSEM): either re-quantization that is a fixed point counts
        for sem in ("cpu", "device"):
            todo_s = todo & (found == 0)
            if not todo_s.any():
                break
            work = w2d.clone()
            step = ops.quantize_channels_(work, np.where(todo_s, b, 0), semantics=sem)
            same = (work == w2d).all(dim=1).cpu().numpy() & todo_s
            found[same] = b
            sel = torch.from_numpy(np.nonzero(same)[0]).to(steps.device)
            steps[sel] = step.reshape(-1).to(steps.device)[sel]
    # Re-quantization is not always idempotent (the min/max of a quantized channel round to a
    # grid shifted by an ulp): the rest get a direct grid search on the values
    lo_b = None if allowed is None else np.asarray(allowed)
    for c in np.nonzero(~known & (found == 0))[0]:
        if lo_b is not None and lo_b[c] <= 0:
            continue
        hit = _grid_search(w2d[c].detach().cpu().numpy(),
                           CANDIDATE_BITS if lo_b is None else (int(lo_b[c]),))
        if hit is not None:
            found[c] = hit[0]
            steps[int(c)] = float(hit[1])
    if (found > 0).any():
        conv.record_quant_all(found, steps)
    return int((found > 0).sum())


def _grid_search(v, bits):
    """(b, fp32 step) such that every value is fl32(m * step) for an integer m, with the code span
    of a b-bit reference quantization (2^b - 1, +-1 from rounding); None if no candidate fits."""
    nlev = np.unique(v).size
    if nlev > (1 << max(bits)) + 1:
        return None
    lo, hi = np.float64(v.min()), np.float64(v.max())
    for b in bits:
        if nlev > (1 << b) + 1:
            continue
        for n in ((1 << b) - 1, 1 << b, (1 << b) - 2):
            s = np.float32((hi - lo) / n)
            for k in (0, -1, 1, -2, 2, -3, 3, -4, 4):  # the nearest fp32 steps first
                cand = s
                for _ in range(abs(k)):
                    cand = np.nextafter(cand, np.float32(np.inf if k > 0 else 0), dtype=np.float32)
                m = np.rint(v.astype(np.float64) / np.float64(cand)).astype(np.float32)
                if np.array_equal(m * cand, v):
                    return b, cand
    return None


def _strict_ok(net, state):
    """strict=True for a plain (reference-format) state dict: only the metadata buffers, which the
    QConv2d loader tolerates as missing, may be absent."""
    want = set(net.state_dict())
    missing = {k for k in want - set(state) if not k.endswith(META_KEYS)}
    unexpected = set(state) - want
    if missing or unexpected:
        raise RuntimeError("Error(s) in loading state_dict: missing keys %s, unexpected keys %s"
                           % (sorted(missing)[:8], sorted(unexpected)[:8]))


# ---- bit-packed state, format smpq-packed/1 (include/smpq.h) -----------------------------------
# The search's save / rollback (resnet50_main.py:212 torch.save(net.state_dict(), ...) on every
# accepted semilayer, :233-234 net.load_state_dict(torch.load(...)) on every rejected one) without
# the disk and the host: snapshot() keeps every QConv2d weight as b-bit codes next to the net, on
# its device, restore_() unpacks them into the weights in place. save_packed / load_packed are the
# same state as one file, whose size is the size the bit assignment promises.
PACKED_FORMAT = "smpq-packed/1"
_CONV_FIELDS = ("shape", "qbits", "step", "mode", "base", "word_off", "payload")
_CONV_KEYS = ("weight", "qbits", "qstep")


class PackedConv:
    """One QConv2d weight in packed form: the format's arrays on one device, the payload as the
    int8 byte view of its 32-bit words, plus two host-side numbers the restore needs without a
    sync (the payload's word count and the host mirror of qbits)."""
    __slots__ = ("shape", "k", "qbits", "step", "mode", "base", "word_off", "payload", "total_words", "bits_host")

    def __init__(self, shape, qbits, step, mode, base, word_off, payload, total_words, bits_host):
        self.shape = tuple(int(s) for s in shape)
        self.k = int(np.prod(self.shape[1:], dtype=np.int64))
        self.qbits, self.step, self.mode, self.base = qbits, step, mode, base
        self.word_off, self.payload = word_off, payload
        self.total_words = int(total_words)
        self.bits_host = np.asarray(bits_host).astype(np.int16).copy()

    @property
    def cout(self):
        return self.shape[0]

    @property
    def device(self):
        return self.payload.device

    def to(self, device):
        if self.device == torch.device(device):
            return self
        return PackedConv(self.shape, *(getattr(self, f).to(device) for f in _CONV_FIELDS[1:]),
                          self.total_words, self.bits_host)


class PackedState:
    """snapshot()'s result: ``convs`` {module name: PackedConv} for every QConv2d, ``tensors``
    {state-dict key: copy} for everything else (BN, fc, conv biases), all on the net's device."""
    __slots__ = ("convs", "tensors")

    def __init__(self, convs, tensors):
        self.convs, self.tensors = convs, tensors


def _qconvs(net):
    from .qconv import QConv2d
    return [(name, m) for name, m in net.named_modules() if isinstance(m, QConv2d)]


def _weight2d(name, m):
    w = m.weight.detach()
    if w.dtype != torch.float32 or not w.is_contiguous() or m.qbits.device != w.device or m.qstep.device != w.device:
        raise ValueError("smpq-packed: %s needs a contiguous fp32 weight with its metadata on the same device" % name)
    return w.view(w.shape[0], -1)


def snapshot(net):
    """The net's whole state, QConv2d weights bit-packed, on the net's device: what
    ``torch.save(net.state_dict(), ...)`` keeps for a rollback, with no file and no host copy.
    A pending deferred quantizer error is raised first (as save_checkpoint does). Every conv is
    planned, then the payload sizes are read in one host sync, then every conv is stored."""
    from .quant import check_pending
    check_pending()
    plans = []
    with torch.no_grad():
        for name, m in _qconvs(net):
            w2d = _weight2d(name, m)
            qbits, step = m.qbits.detach().clone(), m.qstep.detach().clone()
            mode, base, words = ops.bitpack_plan(w2d, qbits, step)
            plans.append((name, m, w2d, qbits, step, mode, base, ops.bitpack_offsets(words)))
        last = [p[7][-1] for p in plans]
        if len({t.device for t in last}) == 1:
            totals = torch.stack(last).tolist()  # the one host sync
        else:  # a net spread over devices: one read per conv
            totals = [int(t) for t in last]
        convs = {}
        for i, (name, m, w2d, qbits, step, mode, base, off) in enumerate(plans):
            payload = ops.bitpack_store(w2d, mode, base, step, off, totals[i])
            convs[name] = PackedConv(m.weight.shape, qbits, step, mode, base, off, payload, totals[i], m._bits_host)
        skip = {(n + "." if n else "") + k for n in convs for k in _CONV_KEYS}
        tensors = {k: v.detach().clone() for k, v in net.state_dict().items() if k not in skip}
    return PackedState(convs, tensors)


def restore_(net, state):
    """Put a PackedState back into ``net`` in place: weights (unpacked straight into the
    Parameters' memory), qbits / qstep and their host mirror through QConv2d.restore_quant, every
    other tensor by copy_. No host sync when the state is on the net's device (a state from
    another device is moved first). The engine sees the restored content (the convs' metadata and
    content generations move). Returns ``net``."""
    convs = _qconvs(net)
    sd = net.state_dict()
    skip = {(n + "." if n else "") + k for n, _ in convs for k in _CONV_KEYS}
    if [n for n, _ in convs] != list(state.convs) or {k for k in sd if k not in skip} != set(state.tensors):
        raise ValueError("smpq-packed: the state's convs / tensors are not this net's")
    for name, m in convs:
        if tuple(m.weight.shape) != state.convs[name].shape:
            raise ValueError("smpq-packed: %s is %s, the state holds %s"
                             % (name, tuple(m.weight.shape), state.convs[name].shape))
    for k, v in state.tensors.items():
        if sd[k].shape != v.shape or sd[k].dtype != v.dtype:
            raise ValueError("smpq-packed: tensor %s does not match the net's" % k)
    with torch.no_grad():
        dst, src = [], []
        for name, m in convs:
            w2d = _weight2d(name, m)
            pc = state.convs[name].to(w2d.device)
            ops.bitpack_load(pc.payload, pc.cout, pc.k, pc.mode, pc.base, pc.step, pc.word_off, out=w2d)
            dst += [m.qbits, m.qstep]
            src += [pc.qbits, pc.step]
            m.restore_quant(pc.bits_host)
        for k, v in state.tensors.items():
            dst.append(sd[k])
            src.append(v)
        # a few hundred small tensors (metadata, BN, fc): one batched copy, not one launch each
        torch._foreach_copy_(dst, src)
    return net


def _conv_words(mode, k):
    """Per-channel payload word counts the format fixes for ``mode`` (host int array): k for a raw
    channel, ceil(k * b / 32) for a packed one."""
    mode = np.asarray(mode, dtype=np.int64)
    return np.where(mode == 0, k, (k * mode + 31) // 32)


def packed_report(state):
    """{"convs": {name: row}, "total": row}, row = fp32_bytes (the weights as fp32), packed_bytes
    (the payload), meta_bytes (the per-channel arrays), raw_channels, packed_channels; the total
    also has other_bytes (the tensors kept verbatim). The payload of every channel is checked
    against the format's word counts (ValueError otherwise)."""
    rows = {}
    total = {"fp32_bytes": 0, "packed_bytes": 0, "meta_bytes": 0, "raw_channels": 0, "packed_channels": 0}
    for name, pc in state.convs.items():
        mode = pc.mode.cpu().numpy()
        off = pc.word_off.cpu().numpy()
        if not np.array_equal(np.diff(off), _conv_words(mode, pc.k)) or off[0] != 0 \
                or pc.payload.numel() != 4 * int(off[-1]):
            raise ValueError("smpq-packed: %s: payload words do not follow the format" % name)
        meta = sum(getattr(pc, f).numel() * getattr(pc, f).element_size() for f in _CONV_FIELDS[1:6])
        rows[name] = {"fp32_bytes": 4 * pc.cout * pc.k, "packed_bytes": int(pc.payload.numel()), "meta_bytes": meta,
                      "raw_channels": int((mode == 0).sum()), "packed_channels": int((mode > 0).sum())}
        for f in total:
            total[f] += rows[name][f]
    total["other_bytes"] = sum(v.numel() * v.element_size() for v in state.tensors.values())
    return {"convs": rows, "total": total}


def save_packed(net, path):
    """``snapshot(net)`` as one file (torch.save of a flat dict of plain tensors and the format
    tag; readable with weights_only=True, no sidecar): "conv/<module>/<field>" for the packed
    convs (shape, qbits, step, mode, base, word_off, payload), "tensor/<key>" for the rest."""
    st = snapshot(net)
    doc = {"format": PACKED_FORMAT}
    for name, pc in st.convs.items():
        doc["conv/%s/shape" % name] = torch.tensor(pc.shape, dtype=torch.int64)
        for f in _CONV_FIELDS[1:]:
            doc["conv/%s/%s" % (name, f)] = getattr(pc, f).cpu()
    for k, v in st.tensors.items():
        doc["tensor/" + k] = v.cpu()
    torch.save(doc, path)
    return st


def _validate_packed(doc, net, path):
    """Everything a kernel will trust, checked on the host; returns the PackedState."""
    def bad(msg):
        raise ValueError("%s: %s" % (path, msg))
    if not isinstance(doc, dict) or doc.get("format") != PACKED_FORMAT:
        bad("not a %s file (format %r)" % (PACKED_FORMAT, doc.get("format") if isinstance(doc, dict) else None))
    names = [n for n, _ in _qconvs(net)]
    in_file = sorted({k.split("/")[1] for k in doc if k.startswith("conv/")})
    if in_file != sorted(names):
        bad("the file's convs are not this net's")
    sd = net.state_dict()
    skip = {(n + "." if n else "") + k for n in names for k in _CONV_KEYS}
    tensors = {k[len("tensor/"):]: v for k, v in doc.items() if k.startswith("tensor/")}
    if set(tensors) != {k for k in sd if k not in skip}:
        bad("the file's tensors are not this net's")
    for k, v in tensors.items():
        if not isinstance(v, torch.Tensor) or v.shape != sd[k].shape or v.dtype != sd[k].dtype:
            bad("tensor %s does not match the net's" % k)
    dtypes = {"shape": torch.int64, "qbits": torch.int8, "step": torch.float32, "mode": torch.int8,
              "base": torch.int32, "word_off": torch.int64, "payload": torch.int8}
    convs = {}
    for name, m in _qconvs(net):
        f = {}
        for field in _CONV_FIELDS:
            t = doc.get("conv/%s/%s" % (name, field))
            if not isinstance(t, torch.Tensor) or t.dtype != dtypes[field] or t.dim() != 1:
                bad("%s: %s missing or of the wrong type" % (name, field))
            f[field] = t.contiguous()
        shape = tuple(f["shape"].tolist())
        cout, k = m.weight.shape[0], m.weight[0].numel()
        if shape != tuple(m.weight.shape):
            bad("%s: cout / k of the file %s, of the conv %s" % (name, shape, tuple(m.weight.shape)))
        for field in ("qbits", "step", "mode", "base"):
            if f[field].numel() != cout:
                bad("%s: %s has %d entries for %d channels" % (name, field, f[field].numel(), cout))
        mode = f["mode"].cpu().numpy().astype(np.int64)
        if mode.min() < 0 or mode.max() > 8:
            bad("%s: mode outside 0..8" % name)
        qb = f["qbits"].cpu().numpy().astype(np.int64)
        if ((mode > 0) & (mode != qb)).any():
            bad("%s: a packed channel's mode is not its recorded bit-width" % name)
        base = f["base"].cpu().numpy().astype(np.int64)
        if np.abs(base).max() > (1 << 23) or (base[mode == 0] != 0).any():
            bad("%s: base outside the code range" % name)
        off = f["word_off"].cpu().numpy()
        if off.size != cout + 1 or off[0] != 0:
            bad("%s: word_off must be [cout + 1] and start at 0" % name)
        if not np.array_equal(np.diff(off), _conv_words(mode, k)):
            bad("%s: word_off does not advance by each channel's word count" % name)
        if f["payload"].numel() != 4 * int(off[-1]):
            bad("%s: payload of %d bytes, word_off[-1] = %d words" % (name, f["payload"].numel(), int(off[-1])))
        convs[name] = PackedConv(shape, f["qbits"], f["step"], f["mode"], f["base"], f["word_off"], f["payload"],
                                 int(off[-1]), qb)
    return PackedState(convs, tensors)


def load_packed(net, path, map_location="cpu"):
    """Read a save_packed file into ``net`` (restore_). The file is validated on the host before
    any kernel runs — format tag, cout and k of every conv, mode in 0..8, word_off starting at 0
    and advancing by each channel's word count, payload length = word_off[-1] — and a violation
    raises ValueError, with the net untouched. The file is always read into host memory (the
    validation reads every offset); ``map_location`` other than "cpu" is where the validated state
    is moved before restore_, which moves it on to the net's device if that is yet another.
    Returns {lnum: bits per channel} as load_checkpoint."""
    doc = torch.load(path, map_location="cpu", weights_only=True)
    st = _validate_packed(doc, net, path)
    if torch.device(map_location).type != "cpu":
        st = PackedState({n: pc.to(map_location) for n, pc in st.convs.items()},
                         {k: v.to(map_location) for k, v in st.tensors.items()})
    restore_(net, st)
    return bit_assignment(net)


def load_checkpoint(net, path, map_location="cpu", strict=True):
    """``net.load_state_dict(torch.load(path))`` with a safe loader, then restore the quantization
    metadata: exactly from a smpq-bits/2 sidecar (bits + fp32 steps), else recovered from the
    values (sidecar-guided when a smpq-bits/1 ``<path>.bits.json`` exists). Returns
    {lnum: bits per channel} after loading."""
    state = torch.load(path, map_location=map_location, weights_only=True)
    if strict:
        _strict_ok(net, state)
    net.load_state_dict(state, strict=False)
    side, side_steps = _read_sidecar_full(path)
    has_meta = any(k.endswith(".qbits") for k in state)
    for ln, conv in enumerate(addressable_convs(net), start=1):
        allowed = None
        if side is not None:
            allowed = side.get(ln)
            if allowed is None or not (allowed > 0).any():
                continue
            if len(allowed) != conv.out_channels:
                raise ValueError("sidecar lnum %d: %d channels, conv has %d"
                                 % (ln, len(allowed), conv.out_channels))
            if side_steps is not None and not has_meta:
                st = side_steps.get(ln)
                if st is None or len(st) != conv.out_channels:
                    raise ValueError("sidecar lnum %d: steps missing or of the wrong length" % ln)
                conv.clear_quant()
                conv.record_quant_all(np.asarray(allowed), torch.from_numpy(st.copy()))
                continue
        infer_quant_(conv, allowed)
    return bit_assignment(net)
