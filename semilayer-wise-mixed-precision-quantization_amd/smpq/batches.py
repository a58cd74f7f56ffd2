"""Host batches to the device for the evaluation loops (functions.evaluate_acc_loss_softmax /
evaluate_loss, smpq.dp.sharded_eval), with the copy of the next batch overlapping the evaluation of
the current one (the reference copies each batch on the compute stream, functions.py:109-111), and
ResidentSet: the set read from its loader once, kept on the device as uint8 and replayed bitwise."""
import sys
import threading

import torch


class DeviceBatches:
    """The batches of ``loader`` on ``dev``, with batch i+1's host-to-device copy in flight on a
    side stream while batch i is being evaluated (the reference copies each batch on the compute
    stream, functions.py:109-111, so copy and forward alternate). Host batches are copied from
    pinned memory: a pinned batch (the reference's DataLoader uses pin_memory=True) directly, any
    other one after a copy into one of two reusable pinned buffers, made on a worker thread while
    the GPU runs. Device batches pass through untouched."""

    def __init__(self, loader, dev):
        if isinstance(loader, ResidentSet):
            # this class asks for batch i+1 while batch i is in use; a resident batch lives only
            # until the next one is requested
            raise ValueError("smpq: a ResidentSet is iterated directly, not through DeviceBatches")
        self.loader, self.dev = loader, dev
        self.stream = torch.cuda.Stream(device=dev)
        self._pinned = {}    # (shape, dtype) -> [buffer 0, buffer 1]
        self._done = [None, None]  # copy-finished event of each pinned slot
        self._slot = 0

    def _pin(self, t):
        if t.is_pinned():
            return t, None
        key = (tuple(t.shape), t.dtype)
        bufs = self._pinned.get(key)
        if bufs is None:
            bufs = self._pinned[key] = [torch.empty(t.shape, dtype=t.dtype).pin_memory() for _ in range(2)]
        k = self._slot
        self._slot ^= 1
        if self._done[k] is not None:
            self._done[k].synchronize()  # the slot's previous copy has left the buffer
        bufs[k].copy_(t)
        return bufs[k], k

    def _stage(self, x, y):
        """(x, y) -> device tensors + the event that marks their copy done (None: nothing to wait)."""
        if x.is_cuda:
            return x, y, None
        xp, kx = self._pin(x)
        yp = y if (not torch.is_tensor(y) or y.is_pinned()) else y.pin_memory()
        with torch.cuda.stream(self.stream):
            xd = xp.to(self.dev, non_blocking=True)
            yd = yp.to(self.dev, non_blocking=True) if torch.is_tensor(yp) else yp
            ev = torch.cuda.Event()
            ev.record(self.stream)
        if kx is not None:
            self._done[kx] = ev
        return xd, yd, ev

    def __iter__(self):
        it = iter(self.loader)
        staged = [None]

        from .engine import CAPTURE_LOCK

        def fetch():
            try:
                x, y = next(it)  # the loader's own work (host only) runs beside anything
                # device work waits for a graph capture on the main thread to end (engine.CAPTURE_LOCK)
                with CAPTURE_LOCK, torch.cuda.device(self.dev):
                    staged[0] = self._stage(x, y)
            except StopIteration:
                staged[0] = StopIteration
            except BaseException as e:  # noqa: BLE001 -- re-raised in the consuming thread
                staged[0] = e
        fetch()
        while staged[0] is not StopIteration:
            if isinstance(staged[0], BaseException):
                raise staged[0]
            xd, yd, ev = staged[0]
            worker = threading.Thread(target=fetch)  # stage batch i+1 while batch i runs
            worker.start()
            main = torch.cuda.current_stream(self.dev)
            if ev is not None:
                main.wait_event(ev)
                xd.record_stream(main)  # allocated on the copy stream, used on this one
                if torch.is_tensor(yd):
                    yd.record_stream(main)
            try:
                yield xd, yd
            finally:
                worker.join()


class ResidentSet:
    """An evaluation set that is read from ``loader`` once and then served from the device, with
    batches that are bit for bit what the loader delivers. Iterating it yields ``(x, y)`` device
    tensors like ``DeviceBatches``.

    The first complete pass yields the loader's batches (through ``DeviceBatches``) unchanged and
    keeps a copy of each: as uint8 when every element lies on the grid of ``lut`` (fp32 [c, 256],
    default ``ops.u8lut_table()``: what ToTensor + Normalize make of a uint8 image; checked bit for
    bit by ``ops.u8lut_encode``), as the fp32 batch itself otherwise ("raw": still resident, still
    exact). Labels stay on the device. A pass the consumer abandons early caches nothing.

    Later passes never touch ``loader``. uint8 batches are decoded (``ops.u8lut_decode``) on a side
    stream into two staging buffers the set owns; a short batch is a leading view of the same
    buffer, so a pass shows at most two input addresses per batch shape and the static-range
    forward replays its per-address graphs without an input copy (engine.GRAPHS_PER_MODEL). Batch
    i + 1 is decoded while batch i is evaluated: when batch i is requested, the decode of batch
    i + 1 is enqueued behind everything the consumer has enqueued on its stream so far, into the
    buffer that held batch i - 1. A yielded ``x`` of a resident pass is therefore valid until the
    next batch is requested: work enqueued on the consumer's stream before that request is ordered
    before the overwrite; clone ``x`` to keep it longer. (With two buffers and the next batch in
    flight during the evaluation of this one, the batch before this one has no place left.) Raw
    batches are yielded as they are kept. Iterate the set directly, as functions._run_eval and
    dp.sharded_eval do: a wrapper that asks for batch i + 1 before batch i has been used (such as
    DeviceBatches, which refuses a ResidentSet) breaks that contract.

    ``max_bytes``: if the kept images would exceed it the cache is dropped, one line goes to
    stderr, and every pass is served from the loader through ``DeviceBatches``; an evaluation never
    fails for it. ``shard=(rank, world)``: only rows ``dp.shard_range(b, rank, world)`` of each
    batch are kept and yielded (``dp.sharded_eval`` takes such a set as it comes). ``device=None``
    binds to the current device at the first pass. There is no CPU form."""

    def __init__(self, loader, device=None, lut=None, max_bytes=None, shard=None):
        self.loader = loader
        self.max_bytes = None if max_bytes is None else int(max_bytes)
        if shard is not None:
            rank, world = (int(v) for v in shard)
            if not 0 <= rank < world:
                raise ValueError("smpq: ResidentSet shard %r is not (rank, world) with 0 <= rank < world" % (shard,))
            shard = (rank, world)
        self.shard = shard
        self.dev = None
        self._lut_arg = lut
        self._lut = None
        self._stream = None
        self._staging = None   # two flat fp32 buffers sized for the largest uint8-backed batch
        self._cache = None     # list of ("u8", u, y, shape) / ("raw", x, y, None) once a pass completed
        self._fallback = False
        self._epoch = 0        # moves whenever the content later passes serve may have changed
        self._counts = dict.fromkeys(("images", "u8_batches", "raw_batches", "resident_bytes", "fp32_bytes",
                                      "off_grid_elements"), 0)
        self._passes = {"loader_passes": 0, "resident_passes": 0}
        if device is not None:
            self.bind(device)

    def bind(self, device):
        """Fix the device (a second, different one is a ValueError)."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ValueError("smpq: ResidentSet needs a GPU device, got %s" % dev)
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if self.dev is not None and self.dev != dev:
            raise ValueError("smpq: ResidentSet is bound to %s, asked for %s" % (self.dev, dev))
        self.dev = dev
        return self

    def _setup(self):
        if self.dev is None:
            self.bind(torch.device("cuda", torch.cuda.current_device()))
        if self._lut is None:
            from . import ops
            lut = ops.u8lut_table() if self._lut_arg is None else self._lut_arg
            self._lut = lut.to(self.dev)
            ops._u8lut_check_table(self._lut)  # here, once: no sync left for the decodes
            self._stream = torch.cuda.Stream(device=self.dev)

    def _sharded(self):
        """The loader's batches, cut to this set's shard."""
        from .dp import shard_range
        for x, y in self.loader:
            if self.shard is not None:
                s, e = shard_range(x.shape[0], *self.shard)
                if e <= s:
                    raise ValueError("smpq: a batch of %d images leaves rank %d of %d none" % ((x.shape[0],) + self.shard))
                x, y = x[s:e], (y[s:e] if torch.is_tensor(y) else y)
            yield x, y

    def invalidate(self):
        """Drop the cache (and a max_bytes fallback): the next pass reads the loader again."""
        if self._stream is not None:
            self._stream.synchronize()  # a decode in flight still reads the cache and writes the staging
        self._cache = self._staging = None
        self._fallback = False
        self._epoch += 1
        for k in self._counts:
            self._counts[k] = 0

    def report(self):
        """images, batches kept as uint8 / raw, resident bytes of the kept images and the fp32
        bytes they stand for, off-grid elements seen, loader passes and resident passes served, and
        the epoch: a counter that moves whenever a cache is installed and in invalidate(), so
        (id(set), epoch) names one fixed content (smpq.memo keys on it)."""
        r = dict(self._counts)
        r.update(self._passes)
        r["resident"] = self._cache is not None
        r["fallback"] = self._fallback
        r["epoch"] = self._epoch
        return r

    def __iter__(self):
        self._setup()
        if self._cache is not None:
            return self._resident_pass()
        return self._loader_pass()

    def _keep(self, x, y, from_device):
        """One batch of the filling pass -> its cache entry (one host read of the off-grid count)."""
        from . import ops
        c = self._counts
        lut = self._lut
        entry = None
        if x.dtype == torch.float32 and x.dim() >= 2 and x.is_contiguous() and x.shape[1] == lut.shape[0] \
                and 0 < x.numel() < 2 ** 31:
            u, bad = ops.u8lut_encode(x, lut)
            bad = int(bad.item()) & 0xFFFFFFFF
            c["off_grid_elements"] += bad
            if bad == 0:
                entry = ("u8", u, y, tuple(x.shape))
                c["u8_batches"] += 1
                c["resident_bytes"] += u.numel()
        if entry is None:
            # a batch the loader itself keeps on the device may be overwritten by it later: copy
            entry = ("raw", x.clone(), y.clone() if torch.is_tensor(y) else y, None) if from_device else \
                ("raw", x, y, None)
            c["raw_batches"] += 1
            c["resident_bytes"] += x.numel() * x.element_size()
        c["images"] += int(x.shape[0])
        c["fp32_bytes"] += x.numel() * x.element_size()
        return entry

    def _loader_pass(self):
        entries = None if self._fallback else []
        on_device = []

        def source():
            for x, y in self._sharded():
                on_device.append(bool(x.is_cuda))
                yield x, y
        if entries is not None:
            for k in self._counts:
                self._counts[k] = 0
        try:
            for x, y in DeviceBatches(source(), self.dev):
                if entries is not None:
                    entries.append(self._keep(x, y, on_device[len(entries)]))
                    if self.max_bytes is not None and self._counts["resident_bytes"] > self.max_bytes:
                        print("smpq ResidentSet: the set exceeds max_bytes=%d after %d batches -> not kept, "
                              "every pass reads the loader" % (self.max_bytes, len(entries)), file=sys.stderr)
                        entries = None
                        self._fallback = True
                yield x, y
            # only a pass that ran to its end counts and caches
            self._passes["loader_passes"] += 1
            if entries is not None:
                need = max([e[1].numel() for e in entries if e[0] == "u8"], default=0)
                self._staging = [torch.empty(need, dtype=torch.float32, device=self.dev) for _ in range(2)] \
                    if need else None
                self._cache = entries
                self._epoch += 1
        finally:
            if self._cache is None:  # abandoned, failed or over max_bytes: nothing is kept
                for k in self._counts:
                    self._counts[k] = 0

    def _resident_pass(self):
        from . import ops
        cache, lut, side = self._cache, self._lut, self._stream
        main = torch.cuda.current_stream(self.dev)
        u8 = [i for i, e in enumerate(cache) if e[0] == "u8"]
        slot_of = {i: k & 1 for k, i in enumerate(u8)}
        ready = {}

        def decode(i):
            """Enqueue batch i's decode on the side stream, behind the consumer's work so far."""
            if i >= len(cache) or cache[i][0] != "u8":
                return
            _, u, _, shape = cache[i]
            x = self._staging[slot_of[i]][:u.numel()].view(shape)
            side.wait_stream(main)  # the buffer's previous batch: everything enqueued up to here
            with torch.cuda.stream(side):
                ops.u8lut_decode(u, lut, out=x)
                ev = torch.cuda.Event()
                ev.record(side)
            ready[i] = (x, ev)
        decode(0)
        for i, (kind, data, y, _) in enumerate(cache):
            decode(i + 1)
            if kind == "u8":
                x, ev = ready.pop(i)
                main.wait_event(ev)
            else:
                x = data
            if i == len(cache) - 1:
                self._passes["resident_passes"] += 1  # (the last batch handed out: the pass is served)
            yield x, y
            main = torch.cuda.current_stream(self.dev)
