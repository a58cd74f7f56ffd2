"""Prefix activation cache, host side: which block inputs an evaluation could keep, what names
their content, and when a kept one may be replaced.

Almost every evaluation of a search differs from a state already evaluated in one semilayer only
(functions._make_semilayers: the pristine model with one semilayer quantized; the main loop: the
last accepted state with one). Everything upstream of that conv computes bit for bit what it
computed last time, so an evaluation could start at a block input ("boundary", ``layerL.B``) that
an earlier one kept. This module holds the parts of that plan that need no device:

  * ``boundary_keys``: the content key of a boundary — the set's ``(id, epoch)``, every upstream
    ``state_dict()`` tensor (name, dtype, shape, device fingerprint), bit-width mirror, module type
    and geometry, every setting of ``memo.settings()`` and every upstream static range (fp32 bits).
    It is ``memo.compose_key`` over the upstream part of what ``memo.state_key`` covers for the
    whole model; no id, data_ptr or _version of a model tensor enters;
  * ``boundary_shape`` / ``boundary_bytes`` / ``admit``: what a boundary costs and which ones a
    byte budget admits, deepest first (the deepest is the cheapest and saves the most);
  * ``Boundary``: the refill rule as a state machine.

Refill rule. A boundary whose stored key differs from this evaluation's is refilled during it only
if (1) this pass computes its content in full (the pass does not resume downstream of it) and
(2) the boundary is empty, or this evaluation's key was also this boundary's key in the previous
eligible evaluation. (2) keeps the one-off trial states of a sensitivity pass (A, B, A, C, A ...)
from ever overwriting the pristine prefix A, and lets an accepted state take over once it has been
seen twice: as the accepted trial, then as the base of the next trial (A, B, B refills during the
second B). A fill marks its boundary invalid first and valid only when the pass ran to its end; an
abandoned fill leaves the boundary empty, not holding what it held before.

Nothing here is consulted by an evaluation: the engine side (taps and a resume point in
``engine.forward_fused``, the per-batch slots, the switch in ``functions._run_eval``) is not part
of the package (DESIGN.md 5e says why).
"""
import re
import struct

from . import memo
from .qconv import QConv2d

DEFAULT_BLOCKS = ("layer3.0", "layer4.0")


def block_names(net):
    """``layerL.B`` of every block, in the order the forward runs them."""
    return ["layer%d.%d" % (li + 1, b) for li, layer in enumerate((net.layer1, net.layer2, net.layer3, net.layer4))
            for b in range(len(layer))]


def block_index(net, name):
    """Index of block ``layerL.B`` in forward order (ValueError if the net has none)."""
    if not re.fullmatch(r"layer[1-4]\.\d+", name) or name not in block_names(net):
        raise ValueError("smpq prefix: %r is not a block (layerL.B) of this net" % (name,))
    return block_names(net).index(name)


def upstream(net, j):
    """Module-name prefixes of everything the input of block ``j`` depends on: the stem and the
    blocks before it."""
    return ("conv1", "bn1", "relu", "maxpool") + tuple(block_names(net)[:j])


def _range_bits(r):
    try:
        return struct.pack("<f", r).hex()
    except OverflowError:  # beyond fp32: still one fixed spelling
        return struct.pack("<d", r).hex()


def boundary_keys(net, indices, ranges, set_key=None, digest=None):
    """{j: key} of the boundaries ``indices`` (block indices). ``ranges``: {id(conv): static range}
    as a calibration installs them (engine.set_calibration); ``set_key``: the evaluation set's
    ``(id, epoch)``; ``digest(net, named)``: one integer per (name, tensor) of ``state_dict()``
    (default: ``memo.device_digests``, one fingerprint launch and one host read for all keys)."""
    named = [(k, v.detach()) for k, v in net.state_dict().items()]
    digests = (digest or memo.device_digests)(net, named)
    bits = memo.bits_rows(net)
    convs = [(name, m) for name, m in net.named_modules() if isinstance(m, QConv2d)]
    names = block_names(net)
    knobs = memo.settings()
    out = {}
    for j in indices:
        ups = upstream(net, j)

        def up(name, ups=ups):
            return any(name == p or name.startswith(p + ".") for p in ups)
        sel = [i for i, (k, _) in enumerate(named) if up(k)]
        rng = tuple((name, _range_bits(ranges[id(m)]) if id(m) in ranges else None) for name, m in convs if up(name))
        out[j] = memo.compose_key([(named[i][0], str(named[i][1].dtype), tuple(named[i][1].shape)) for i in sel],
                                  [digests[i] for i in sel], [(n, b) for n, b in bits if up(n)],
                                  memo.structure(net, keep=lambda n, up=up: n == "" or up(n)),
                                  knobs + (("prefix_boundary", names[j]), ("set", set_key), ("ranges", rng)))
    return out


def boundary_shape(net, j, n, h, w, limbs):
    """Shape ``(limbs, n, h', w', c)`` of the int8 limb planes entering block ``j`` for ``n`` images
    of h x w pixels."""
    def down(d, s):
        return (d - 1) // s + 1
    h, w = down(down(h, 2), 2), down(down(w, 2), 2)  # stem 7x7/2 pad 3, max pool 3x3/2 pad 1
    blocks = [b for layer in (net.layer1, net.layer2, net.layer3, net.layer4) for b in layer]
    for blk in blocks[:j]:
        s = blk.conv2.stride[0] if hasattr(blk, "conv3") else blk.conv1.stride[0]
        h, w = down(h, s), down(w, s)
    return (int(limbs), int(n), h, w, blocks[j].conv1.in_channels)


def boundary_bytes(limbs, c, h, w, images):
    """Bytes of ``images`` images' limb planes at a boundary of c channels and h x w pixels."""
    return int(limbs) * int(c) * int(h) * int(w) * int(images)


def admit(sizes, budget):
    """``sizes``: [(block index, bytes)]. Deepest first, each admitted while it fits what is left
    of ``budget``; one that does not fit is refused, and the shallower ones are still tried.
    -> (admitted, refused), both deepest first."""
    left, admitted, refused = int(budget), [], []
    for j, nb in sorted(sizes, reverse=True):
        if nb <= left:
            admitted.append(j)
            left -= nb
        else:
            refused.append(j)
    return admitted, refused


class Boundary:
    """One boundary's record and the refill rule (module docstring) as a state machine over the
    keys of successive eligible evaluations."""
    __slots__ = ("name", "j", "key", "valid", "candidate")

    def __init__(self, name, j):
        self.name, self.j = name, j
        self.key = self.candidate = None
        self.valid = False

    def decide(self, new_key, in_full=True):
        """What an evaluation whose key here is ``new_key`` does with the boundary: "hit" (the kept
        planes are this evaluation's), "fill" or "skip". ``in_full``: the pass computes the
        boundary's content in full (it does not resume downstream of it)."""
        if self.valid and self.key == new_key:
            verdict = "hit"
        elif in_full and (not self.valid or self.candidate == new_key):
            verdict = "fill"
        else:
            verdict = "skip"
        self.candidate = new_key
        return verdict

    def begin_fill(self, key):
        self.valid, self.key = False, key

    def end_fill(self, ok):
        """``ok``: the pass ran to its end without an overflow or stale rerun, on the set epoch it
        started with."""
        self.valid = bool(ok)
        if not ok:
            self.key = None
