"""Tensor-level wrappers over the libsmpq C-ABI (include/smpq.h).

Every function validates shapes/dtypes/devices on the host before launching, so a kernel
never sees an operand that disagrees with its grid (no device-side faults on bad input).
"""
import numbers
import os
from collections import namedtuple

import torch

from . import _lib

# activation code width in int8 limbs (1 = int8, 2 = int16, 3 = int24); see DESIGN.md
# Activation code width in int8 limbs: 3 (int24, the default) is the parity mode — logits within
# 2e-4 relative of the fp32 reference and identical top-1 labels; 2 (int16) is the fast mode
# (~1e-2 relative logit error, top-1 identical except at near-ties); 1 (int8) is for experiments.
_ACT_LIMBS = [int(os.environ.get("SMPQ_ACT_LIMBS", "3"))]
# optional launch observer (bench.py): object with begin() / end(work) around each conv
_CONV_HOOK = [None]
LIMB_QMAX = {1: 127.0, 2: 32512.0, 3: 8323072.0}


def set_act_limbs(limbs):
    if limbs not in (1, 2, 3):
        raise ValueError("act limbs must be 1, 2 or 3")
    _ACT_LIMBS[0] = int(limbs)


def get_act_limbs():
    return _ACT_LIMBS[0]


def _req(cond, msg):
    if not cond:
        raise ValueError("smpq: " + msg)


def _launch(dev, name, *args):
    """Call the C-ABI entry ``name`` with ``args`` (a tensor as its address, None as the null pointer:
    ctypes takes both for a pointer argument) + torch's current stream on ``dev``; raises
    _lib.SmpqError ("name failed (rc): ...") unless it returns SMPQ_OK."""
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), name)(*args, _lib.stream_ptr()), name)


def _launch_twin(t, name, *args):
    """_launch of ``name`` for a device tensor ``t``; for a host tensor its native host twin
    ``name``_host: the same arguments as host addresses, no device and no stream."""
    if t.is_cuda:
        return _launch(t.device, name, *args)
    args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    _lib.check(getattr(_lib.load(), name + "_host")(*args), name + "_host")


# bytes per plane the kernel's 32-bit buffer offsets address (csrc/conv_glds.hip glds_planes_ok)
PLANE_LIMIT = 0x7fffff00


def _image_chunks(n, per_img, what):
    """The (i0, i1) image ranges a batch of ``n`` runs in when a plane (``per_img`` bytes per image)
    would pass PLANE_LIMIT (every image is independent: the result of one launch), else None."""
    nchunk = PLANE_LIMIT // per_img
    _req(nchunk >= 1, "%s: one image's planes exceed 2 GiB" % what)
    return [(i0, min(n, i0 + nchunk)) for i0 in range(0, n, nchunk)] if n > nchunk else None


# Rounding semantics of functions.py:41 `t / scale` (include/smpq.h SMPQ_QSEM_*): torch on the CPU
# divides (IEEE fp32), torch on the GPU multiplies by fp32(1.0 / scale). "auto" follows the
# tensor's device, as the reference's own result does; SMPQ_QUANT_SEMANTICS overrides it.
QSEM = {"cpu": 0, "device": 1}
_QSEM_MODE = [os.environ.get("SMPQ_QUANT_SEMANTICS", "auto")]


def set_quant_semantics(mode):
    """'auto' (default: device tensors round like torch on the GPU, host tensors like torch on
    the CPU), 'cpu' or 'device' (every tensor rounds that way)."""
    if mode not in ("auto", "cpu", "device"):
        raise ValueError("quant semantics must be 'auto', 'cpu' or 'device'")
    _QSEM_MODE[0] = mode


def get_quant_semantics():
    return _QSEM_MODE[0]


def _qsem(semantics, is_cuda):
    mode = semantics or _QSEM_MODE[0]
    if mode == "auto":
        mode = "device" if is_cuda else "cpu"
    _req(mode in QSEM, "quant semantics must be 'auto', 'cpu' or 'device'")
    return QSEM[mode]


def quantize_channels_(w2d, bits, semantics=None):
    """In-place fake-quantization of the rows of ``w2d`` (functions.py:25-43 per channel).

    w2d: fp32 [cout, k] contiguous (CPU or GPU); bits: int sequence/tensor [cout], 0 = skip.
    semantics: None (the process setting, ``set_quant_semantics``), 'auto', 'cpu' or 'device'.
    Returns the fp32 step (fp32(scale)) per row (0 for skipped rows) on w2d's device.
    Raises ZeroDivisionError on a constant channel, like the reference (functions.py:40).
    """
    _req(w2d.dtype == torch.float32 and w2d.dim() == 2 and w2d.is_contiguous(),
         "quantize_channels_: need a contiguous fp32 [cout, k] tensor")
    cout, k = w2d.shape
    lib = _lib.load()
    sem = _qsem(semantics, w2d.is_cuda)
    bits_t = torch.as_tensor(bits, dtype=torch.int8).reshape(-1)
    _req(bits_t.numel() == cout, "quantize_channels_: bits length != cout")
    _req(bool((bits_t >= 0).all()) and bool((bits_t <= 16).all()), "bits outside [0, 16]")
    if w2d.is_cuda:
        bits_d = bits_t.to(w2d.device)
        step = torch.zeros(cout, dtype=torch.float32, device=w2d.device)
        status = torch.zeros(1, dtype=torch.int32, device=w2d.device)
        _launch(w2d.device, "smpq_quantize_channels_ex", w2d, cout, k, bits_d, step, status, sem)
        bad = int(status.item())  # one sync: the reference raises synchronously
        if bad:
            raise ZeroDivisionError("float division by zero (constant channel %d)" % (bad - 1))
        return step
    step = torch.zeros(cout, dtype=torch.float32)
    bits_c = bits_t.contiguous()
    rc = lib.smpq_quantize_channels_host_ex(_lib.ptr(w2d), cout, k, _lib.ptr(bits_c), _lib.ptr(step), sem)
    if rc == _lib.SMPQ_E_CONSTANT:
        raise ZeroDivisionError(_lib.last_error())
    _lib.check(rc, "smpq_quantize_channels_host_ex")
    return step


def pack_weights(w, step):
    """fp32 fake-quantized weight [cout, cin, kh, kw] -> (codes int8 [cout, kh*kw*cin], offset int32)."""
    _req(w.is_cuda and w.dtype == torch.float32 and w.dim() == 4, "pack_weights: need a CUDA fp32 4-D weight")
    w = w.contiguous()
    cout, cin, kh, kw = w.shape
    step = step.to(device=w.device, dtype=torch.float32).contiguous()
    _req(step.numel() == cout, "pack_weights: step length")
    codes = torch.empty(cout, kh * kw * cin, dtype=torch.int8, device=w.device)
    offset = torch.empty(cout, dtype=torch.int32, device=w.device)
    status = torch.zeros(2, dtype=torch.int32, device=w.device)
    _launch(w.device, "smpq_pack_weights", w, cout, cin, kh, kw, step, codes, offset, status)
    return codes, offset, status


def pack_weights_ex(w, step, wlimbs):
    """Weight codes for conv2d_q: (codes int8 [wlimbs, cout, K], offset int32 [cout] | None,
    wscale fp32 [cout], status int32 [3] (device)). See include/smpq.h smpq_pack_weights_ex."""
    _req(w.is_cuda and w.dtype == torch.float32 and w.dim() == 4, "pack_weights_ex: need a CUDA fp32 4-D weight")
    _req(wlimbs in (1, 2, 3), "pack_weights_ex: wlimbs")
    w = w.contiguous()
    cout, cin, kh, kw = w.shape
    _req(cin % 64 == 0, "pack_weights_ex: cin must be a multiple of 64 (the stem: pack_weights_s2d)")
    K = cin * kh * kw
    if step is not None:
        step = step.to(device=w.device, dtype=torch.float32).contiguous()
        _req(step.numel() == cout, "pack_weights_ex: step length")
    _req(wlimbs >= 2 or step is not None, "pack_weights_ex: wlimbs=1 needs step")
    codes = torch.empty(wlimbs, cout, K, dtype=torch.int8, device=w.device)
    offset = torch.zeros(cout, dtype=torch.int32, device=w.device)
    wscale = torch.empty(cout, dtype=torch.float32, device=w.device)
    status = torch.zeros(3, dtype=torch.int32, device=w.device)
    _launch(w.device, "smpq_pack_weights_ex", w, cout, cin, kh, kw, step, int(wlimbs), codes, offset, wscale, status)
    if KMAJOR[0]:
        # the K-major copy the LDS-DMA tiles stage their weight pieces from (whole cache lines);
        # it lives and dies with these codes
        codes._smpq_km = weights_kmajor(codes)
    return codes, offset, wscale, status


KMAJOR = [os.environ.get("SMPQ_KMAJOR", "1") != "0"]


def weights_kmajor(codes):
    """codes int8 [LW, cout, K] (K % 64 == 0) -> the K-major copy [LW, K/64, cout, 64]
    (smpq_weights_kmajor) that smpq_conv2d_fwd_q_km's LDS-DMA tiles read."""
    if codes.dim() == 2:
        codes = codes.unsqueeze(0)
    wl, cout, K = codes.shape
    _req(codes.is_cuda and codes.dtype == torch.int8 and codes.is_contiguous() and K % 64 == 0,
         "weights_kmajor: need contiguous int8 [LW, cout, K] with K % 64 == 0")
    out = torch.empty(wl, K // 64, cout, 64, dtype=torch.int8, device=codes.device)
    _launch(codes.device, "smpq_weights_kmajor", codes, int(wl), int(cout), int(K), out)
    return out


# ---- trial row patch (include/smpq.h): one channel of a packed operand, in place ------------------
TRIAL_MAX_K = 4608
TRIAL_SAVE_HEADER = 16


def trial_save_bytes(wlimbs, K):
    """Bytes of the save area of one trial row (header + the row's wlimbs * K code bytes)."""
    return TRIAL_SAVE_HEADER + int(wlimbs) * int(K)


def _trial_operand(what, codes, wscale, col_scale, save, channel, km, slots=1):
    _req(codes.dtype == torch.int8 and codes.dim() == 3 and codes.is_contiguous() and codes.shape[0] in (2, 3),
         "%s: codes must be contiguous int8 [LW, cout, K] with LW 2 or 3" % what)
    lw, cout, K = codes.shape
    dev = codes.device
    _req(K % 64 == 0 and K <= TRIAL_MAX_K, "%s: K must be a multiple of 64, at most %d" % (what, TRIAL_MAX_K))
    _req(0 <= int(channel) < cout, "%s: channel outside [0, cout)" % what)
    for name, t in (("wscale", wscale), ("col_scale", col_scale)):
        _req(t.dtype == torch.float32 and t.numel() == cout and t.is_contiguous() and t.device == dev,
             "%s: %s must be a contiguous fp32 [cout] tensor on the codes' device" % (what, name))
    _req(save.dtype == torch.int8 and save.dim() == 1 and save.is_contiguous() and save.device == dev
         and save.numel() >= slots * trial_save_bytes(lw, K) and save.data_ptr() % 4 == 0,
         "%s: save must be a contiguous, 4-byte aligned int8 tensor of at least %strial_save_bytes(LW, K)"
         % (what, "n * " if slots != 1 else ""))
    if km is not None:
        _req(dev.type == "cuda" and km.dtype == torch.int8 and km.shape == (lw, K // 64, cout, 64)
             and km.is_contiguous() and km.device == dev, "%s: K-major codes must be int8 [LW, K/64, cout, 64]" % what)
    return lw, cout, K


def trial_row_patch(w, channel, bits, bn_a, codes, wscale, col_scale, save, status, km=None, semantics=None):
    """Overwrite row ``channel`` of a packed operand (``codes`` int8 [LW, cout, K] with LW >= 2, its
    K-major copy ``km`` or None, ``wscale``, ``col_scale`` = wscale * ``bn_a``) with what quantizing
    that channel of the fp32 weight ``w`` [cout, cin, kh, kw] at ``bits`` and packing it would give;
    ``w`` is only read. The row's current bytes and scalars go to ``save`` (int8
    [trial_save_bytes(LW, K)]) first. ``status`` (int32 [1], caller-zeroed) is set to 1 for a
    constant channel, whose operand stays as it is. Device tensors: one launch on the current
    stream, no host sync; host tensors: the native twin (no K-major copy)."""
    _req(w.dtype == torch.float32 and w.dim() == 4 and w.is_contiguous(), "trial_row_patch: need a contiguous fp32 4-D weight")
    lw, cout, K = _trial_operand("trial_row_patch", codes, wscale, col_scale, save, channel, km)
    _req(w.device == codes.device and w.shape[0] == cout and w.shape[1] % 64 == 0
         and w.shape[1] * w.shape[2] * w.shape[3] == K, "trial_row_patch: weight and codes disagree")
    _req(1 <= int(bits) <= 16, "trial_row_patch: bits outside 1..16")
    _req(bn_a.dtype == torch.float32 and bn_a.numel() == cout and bn_a.is_contiguous() and bn_a.device == w.device,
         "trial_row_patch: bn_a must be a contiguous fp32 [cout] tensor on the weight's device")
    _req(status.dtype == torch.int32 and status.numel() >= 1 and status.device == w.device, "trial_row_patch: status")
    sem = _qsem(semantics, w.is_cuda)
    head = (w, cout, int(w.shape[1]), int(w.shape[2]), int(w.shape[3]), int(channel), int(bits), sem, lw, bn_a, codes)
    if w.is_cuda:
        _launch(w.device, "smpq_trial_row_patch", *head, km, wscale, col_scale, save, status)
    else:
        _launch_twin(w, "smpq_trial_row_patch", *head, wscale, col_scale, save, status)


def trial_row_restore(channel, codes, wscale, col_scale, save, km=None):
    """Put back what trial_row_patch saved: the row's code bytes (both layouts) and its two scalars."""
    lw, cout, K = _trial_operand("trial_row_restore", codes, wscale, col_scale, save, channel, km)
    if codes.is_cuda:
        _launch(codes.device, "smpq_trial_row_restore", cout, K, int(channel), lw, codes, km, wscale, col_scale, save)
    else:
        _launch_twin(codes, "smpq_trial_row_restore", cout, K, int(channel), lw, codes, wscale, col_scale, save)


# ---- trial rows patch (include/smpq.h): n channels of one packed operand, one launch ----------------
TrialRows = namedtuple("TrialRows", "channels bits n cout")


def trial_rows_save_bytes(wlimbs, K, n):
    """Bytes of the save area of ``n`` trial rows: n slots of trial_save_bytes(wlimbs, K)."""
    return int(n) * trial_save_bytes(wlimbs, K)


def trial_rows_lists(channels, bits, cout, device, what="trial_rows_patch", max_bits=16):
    """The validated pair of lists of one rows patch on ``device``: TrialRows(channels int32 [n],
    bits int32 [n], n, cout). ``channels``: a sequence or host tensor, non-empty, each in [0, cout),
    pairwise distinct; ``bits``: one int for every row or a sequence of the same length, each in
    1..``max_bits`` (8 for trial_rows_patch_x8). One upload each; a sweep makes the pairs of a conv up
    front and passes them back in."""
    ch = torch.as_tensor(channels).reshape(-1)
    _req(not ch.is_cuda and not ch.is_floating_point() and ch.dtype != torch.bool,
         "%s: channels must be an integer sequence or host tensor" % what)
    ch = ch.to(torch.int64)
    n = ch.numel()
    _req(n >= 1, "%s: the channel list is empty" % what)
    _req(n <= int(cout), "%s: more channels than cout" % what)
    _req(int(ch.min()) >= 0 and int(ch.max()) < int(cout), "%s: channel outside [0, cout)" % what)
    _req(torch.unique(ch).numel() == n, "%s: a channel is listed twice" % what)
    if isinstance(bits, numbers.Integral):
        b = torch.full((n,), int(bits), dtype=torch.int64)
    else:
        b = torch.as_tensor(bits).reshape(-1)
        _req(not b.is_cuda and not b.is_floating_point() and b.dtype != torch.bool,
             "%s: bits must be an int, an integer sequence or a host tensor" % what)
        b = b.to(torch.int64)
        _req(b.numel() == n, "%s: channels and bits differ in length" % what)
    _req(int(b.min()) >= 1 and int(b.max()) <= int(max_bits), "%s: bits outside 1..%d" % (what, max_bits))
    return TrialRows(ch.to(torch.int32).contiguous().to(device), b.to(torch.int32).contiguous().to(device), n, int(cout))


def _trial_rows(what, channels, bits, cout, device):
    if isinstance(channels, TrialRows):
        _req(channels.cout == cout and channels.channels.device == device,
             "%s: the uploaded lists belong to another operand" % what)
        return channels
    return trial_rows_lists(channels, 8 if bits is None else bits, cout, device, what)  # (a restore reads no bits)


def _trial_rows_operand(what, codes, wscale, col_scale, save, channels, bits, km):
    """_trial_operand's checks for the rows ``channels`` of ``codes``, the save size scaled by n."""
    _req(torch.is_tensor(codes) and codes.dim() == 3, "%s: codes must be contiguous int8 [LW, cout, K] with LW 2 or 3" % what)
    rows = _trial_rows(what, channels, bits, codes.shape[1], codes.device)
    lw, cout, K = _trial_operand(what, codes, wscale, col_scale, save, 0, km, slots=rows.n)
    return lw, cout, K, rows


def trial_rows_patch(w, channels, bits, bn_a, codes, wscale, col_scale, save, status, km=None, semantics=None):
    """trial_row_patch for the rows ``channels`` (distinct) of one operand in ONE launch, row i at
    ``bits[i]`` bits (or ``bits`` for all): ``save`` holds trial_rows_save_bytes(LW, K, n) bytes
    (slot i = row i's single-row save area), ``status`` int32 [n], caller-zeroed (1 = constant
    channel, left as it is). ``channels`` may be the TrialRows of trial_rows_lists (``bits`` is then
    ignored). Returns the TrialRows, for the restore."""
    what = "trial_rows_patch"
    _req(w.dtype == torch.float32 and w.dim() == 4 and w.is_contiguous(), "%s: need a contiguous fp32 4-D weight" % what)
    lw, cout, K, rows = _trial_rows_operand(what, codes, wscale, col_scale, save, channels, bits, km)
    _req(w.device == codes.device and w.shape[0] == cout and w.shape[1] % 64 == 0
         and w.shape[1] * w.shape[2] * w.shape[3] == K, "%s: weight and codes disagree" % what)
    _req(bn_a.dtype == torch.float32 and bn_a.numel() == cout and bn_a.is_contiguous() and bn_a.device == w.device,
         "%s: bn_a must be a contiguous fp32 [cout] tensor on the weight's device" % what)
    _req(status.dtype == torch.int32 and status.dim() == 1 and status.is_contiguous() and status.numel() >= rows.n
         and status.device == w.device, "%s: status must be a contiguous int32 [n] tensor on the weight's device" % what)
    sem = _qsem(semantics, w.is_cuda)
    head = (w, cout, int(w.shape[1]), int(w.shape[2]), int(w.shape[3]), rows.channels, rows.bits, rows.n, sem, lw,
            bn_a, codes)
    if w.is_cuda:
        _launch(w.device, "smpq_trial_rows_patch", *head, km, wscale, col_scale, save, status)
    else:
        _launch_twin(w, "smpq_trial_rows_patch", *head, wscale, col_scale, save, status)
    return rows


def trial_rows_restore(channels, codes, wscale, col_scale, save, km=None):
    """Put back what trial_rows_patch saved for the same ``channels`` (a sequence or its TrialRows)."""
    what = "trial_rows_restore"
    lw, cout, K, rows = _trial_rows_operand(what, codes, wscale, col_scale, save, channels, None, km)
    if codes.is_cuda:
        _launch(codes.device, "smpq_trial_rows_restore", cout, K, rows.channels, rows.n, lw, codes, km, wscale,
                col_scale, save)
    else:
        _launch_twin(codes, "smpq_trial_rows_restore", cout, K, rows.channels, rows.n, lw, codes, wscale, col_scale, save)


# ---- trial rows patch, exact8 operands (include/smpq.h): rows of a fully quantized conv's operand -----
def _trial_rows_x8_operand(what, codes, offset, wscale, col_scale, save, channels, bits, km):
    """The checks of an exact8 operand (codes int8 [1, cout, K], ``offset`` int32 [cout] or None) for
    the rows ``channels``: (cout, K, TrialRows)."""
    _req(torch.is_tensor(codes) and codes.dtype == torch.int8 and codes.dim() == 3 and codes.is_contiguous()
         and codes.shape[0] == 1, "%s: codes must be contiguous int8 [1, cout, K]" % what)
    _, cout, K = codes.shape
    dev = codes.device
    _req(K % 64 == 0 and K <= TRIAL_MAX_K, "%s: K must be a multiple of 64, at most %d" % (what, TRIAL_MAX_K))
    if isinstance(channels, TrialRows) or bits is None:  # (uploaded lists: made with max_bits=8 by the caller)
        rows = _trial_rows(what, channels, bits, cout, dev)
    else:
        rows = trial_rows_lists(channels, bits, cout, dev, what, max_bits=8)
    for name, t in (("wscale", wscale), ("col_scale", col_scale)):
        _req(torch.is_tensor(t) and t.dtype == torch.float32 and t.numel() == cout and t.is_contiguous()
             and t.device == dev, "%s: %s must be a contiguous fp32 [cout] tensor on the codes' device" % (what, name))
    _req(offset is None or (torch.is_tensor(offset) and offset.dtype == torch.int32 and offset.shape == (cout,)
                            and offset.is_contiguous() and offset.device == dev),
         "%s: offset must be None or a contiguous int32 [cout] tensor on the codes' device" % what)
    _req(torch.is_tensor(save) and save.dtype == torch.int8 and save.dim() == 1 and save.is_contiguous()
         and save.device == dev and save.numel() >= trial_rows_save_bytes(1, K, rows.n) and save.data_ptr() % 4 == 0,
         "%s: save must be a contiguous, 4-byte aligned int8 tensor of at least trial_rows_save_bytes(1, K, n)" % what)
    if km is not None:
        _req(dev.type == "cuda" and km.dtype == torch.int8 and km.shape == (1, K // 64, cout, 64)
             and km.is_contiguous() and km.device == dev, "%s: K-major codes must be int8 [1, K/64, cout, 64]" % what)
    return cout, K, rows


def trial_rows_patch_x8(w, channels, bits, bn_a, codes, offset, wscale, col_scale, save, status, km=None,
                        semantics=None):
    """trial_rows_patch for an 'exact8' operand (``codes`` int8 [1, cout, K], ``offset`` int32 [cout]
    or None, ``wscale`` = the steps): row i re-quantized at ``bits[i]`` <= 8 bits and coded as
    pack_weights_ex(..., 1) would, in ONE launch (uploaded lists: trial_rows_lists(..., max_bits=8)).
    ``status`` int32 [n], caller-zeroed: 1 constant row, 3 the row is off the grid or spans more than
    256 levels, 4 the row needs an offset and ``offset`` is None; such a row stays as it is. Returns
    the TrialRows, for the restore."""
    what = "trial_rows_patch_x8"
    _req(w.dtype == torch.float32 and w.dim() == 4 and w.is_contiguous(), "%s: need a contiguous fp32 4-D weight" % what)
    cout, K, rows = _trial_rows_x8_operand(what, codes, offset, wscale, col_scale, save, channels, bits, km)
    _req(w.device == codes.device and w.shape[0] == cout and w.shape[1] % 64 == 0
         and w.shape[1] * w.shape[2] * w.shape[3] == K, "%s: weight and codes disagree" % what)
    _req(bn_a.dtype == torch.float32 and bn_a.numel() == cout and bn_a.is_contiguous() and bn_a.device == w.device,
         "%s: bn_a must be a contiguous fp32 [cout] tensor on the weight's device" % what)
    _req(status.dtype == torch.int32 and status.dim() == 1 and status.is_contiguous() and status.numel() >= rows.n
         and status.device == w.device, "%s: status must be a contiguous int32 [n] tensor on the weight's device" % what)
    sem = _qsem(semantics, w.is_cuda)
    head = (w, cout, int(w.shape[1]), int(w.shape[2]), int(w.shape[3]), rows.channels, rows.bits, rows.n, sem, bn_a, codes)
    if w.is_cuda:
        _launch(w.device, "smpq_trial_rows_patch_x8", *head, km, offset, wscale, col_scale, save, status)
    else:
        _launch_twin(w, "smpq_trial_rows_patch_x8", *head, offset, wscale, col_scale, save, status)
    return rows


def trial_rows_restore_x8(channels, codes, offset, wscale, col_scale, save, km=None):
    """Put back what trial_rows_patch_x8 saved for the same ``channels`` (a sequence or its TrialRows)."""
    what = "trial_rows_restore_x8"
    cout, K, rows = _trial_rows_x8_operand(what, codes, offset, wscale, col_scale, save, channels, None, km)
    if codes.is_cuda:
        _launch(codes.device, "smpq_trial_rows_restore_x8", cout, K, rows.channels, rows.n, codes, km, offset, wscale,
                col_scale, save)
    else:
        _launch_twin(codes, "smpq_trial_rows_restore_x8", cout, K, rows.channels, rows.n, codes, offset, wscale,
                     col_scale, save)


# ---- trial rows conv (include/smpq.h): listed output channels of one conv into held limb planes -----
def trial_rows_conv_save_bytes(L, pixels, nrows):
    """Bytes of the save area of trial_rows_conv: ``nrows`` slots of L * pixels digit bytes."""
    return int(nrows) * int(L) * int(pixels)


def _trial_rows_conv_planes(what, yq, save, channels):
    """The checks of the held planes ``yq`` [L, n, ho, wo, cout], the save area and the list:
    (L, pixels, cout, TrialRows)."""
    _req(torch.is_tensor(yq) and yq.dtype == torch.int8 and yq.dim() == 5 and yq.is_contiguous()
         and yq.shape[0] in (2, 3), "%s: yq must be contiguous int8 [L, n, ho, wo, cout] with L 2 or 3" % what)
    L, n, ho, wo, cout = yq.shape
    rows = _trial_rows(what, channels, None, cout, yq.device)
    _req(torch.is_tensor(save) and save.dtype == torch.int8 and save.dim() == 1 and save.is_contiguous()
         and save.device == yq.device and save.numel() >= trial_rows_conv_save_bytes(L, n * ho * wo, rows.n),
         "%s: save must be a contiguous int8 tensor of at least trial_rows_conv_save_bytes(L, pixels, n)" % what)
    return L, n * ho * wo, cout, rows


def trial_rows_conv(xq, x_absmax, codes, kh, kw, stride, pad, col_scale, col_shift, channels, yq, emit_range,
                    overflow, save, residual_q=None, residual_range=None):
    """The output channels ``channels`` (distinct; a sequence or the TrialRows of trial_rows_lists) of
    conv2d_q(xq, x_absmax, codes, None, kh, kw, stride, pad, col_scale, col_shift, relu=True,
    emit_range=..., want_f32=False, residual_q=..., residual_range=...) written IN PLACE into the held
    output planes ``yq`` [L, n, h, w, cout], bit for bit what that launch would write there; every other
    byte of ``yq`` stays. The replaced digit bytes go to ``save`` (int8
    [trial_rows_conv_save_bytes(L, n*h*w, nrows)]) first; ``overflow`` (int32 [1]) is set exactly when
    the conv would set it for these channels. ``codes`` int8 [LW, cout, K] row-major with LW >= 2 (no
    offsets); 1x1 / stride 1 / pad 0 or 3x3 / stride 1 / pad 1, cin % 64 == 0, K <= TRIAL_MAX_K, L 2 or
    3. Device tensors: one launch on the current stream, no host sync; host tensors: the native twin.
    Returns the TrialRows, for the restore."""
    what = "trial_rows_conv"
    _req(torch.is_tensor(xq) and xq.dtype == torch.int8 and xq.dim() == 5 and xq.is_contiguous(),
         "%s: xq must be contiguous int8 [L, n, h, w, cin]" % what)
    L, pixels, cout, rows = _trial_rows_conv_planes(what, yq, save, channels)
    limbs, n, h, w, cin = xq.shape
    dev = xq.device
    _req(limbs == L and yq.shape[1:4] == (n, h, w) and yq.device == dev, "%s: xq and yq disagree" % what)
    _req((kh, kw, stride, pad) in ((1, 1, 1, 0), (3, 3, 1, 1)),
         "%s: only 1x1 / stride 1 / pad 0 and 3x3 / stride 1 / pad 1" % what)
    _req(torch.is_tensor(codes) and codes.dtype == torch.int8 and codes.dim() == 3 and codes.is_contiguous()
         and codes.shape[0] in (2, 3) and codes.device == dev and (codes.shape[0] < 3 or L == 3),
         "%s: codes must be contiguous int8 [LW, cout, K] with LW 2 or 3 (3 with L = 3 only)" % what)
    lw, cout_w, K = codes.shape
    _req(cout_w == cout and K == kh * kw * cin, "%s: codes and planes disagree" % what)
    _req(cin % 64 == 0 and K <= TRIAL_MAX_K and cout % 16 == 0,
         "%s: cin must be a multiple of 64, K at most %d, cout a multiple of 16" % (what, TRIAL_MAX_K))
    _req(xq.data_ptr() % 16 == 0 and codes.data_ptr() % 16 == 0, "%s: xq and codes must be 16-byte aligned" % what)
    _req(x_absmax.dtype == torch.float32 and x_absmax.numel() == n and x_absmax.is_contiguous()
         and x_absmax.device == dev, "%s: x_absmax" % what)
    for t in (col_scale, col_shift):
        _req(t.dtype == torch.float32 and t.numel() == cout and t.is_contiguous() and t.device == dev,
             "%s: col vectors" % what)
    _req(emit_range is not None and emit_range > 0, "%s: emit_range must be > 0" % what)
    _req(torch.is_tensor(overflow) and overflow.dtype == torch.int32 and overflow.numel() >= 1
         and overflow.device == dev, "%s: overflow" % what)
    if residual_q is not None:
        _req(residual_q.shape == yq.shape and residual_q.dtype == torch.int8 and residual_q.is_contiguous()
             and residual_q.device == dev and residual_range is not None and residual_range > 0,
             "%s: residual_q" % what)
    _launch_twin(xq, "smpq_trial_rows_conv_q", xq, x_absmax, n, h, w, cin, codes, int(lw), cout, kh, kw, stride, pad,
                 col_scale, col_shift, int(L), residual_q, float(residual_range or 0.0), rows.channels, rows.n, yq,
                 float(emit_range), overflow, save)
    return rows


def trial_rows_conv_restore(channels, yq, save):
    """Put back the digit bytes trial_rows_conv saved for the same ``channels`` and planes."""
    L, pixels, cout, rows = _trial_rows_conv_planes("trial_rows_conv_restore", yq, save, channels)
    _launch_twin(yq, "smpq_trial_rows_conv_restore", rows.channels, rows.n, int(L), int(pixels), cout, yq, save)


def image_quantize_s2d(x, x_absmax, limbs=None):
    """NCHW fp32 images (c <= 4, h, w >= 2) -> space-to-depth limb planes
    [limbs, n, ceil(h/2), ceil(w/2), 16] (channel (dy*2 + dx)*4 + c = pixel (2i+dy, 2j+dx), channel c;
    zero past an odd h or w): the stem's input (stem_conv_s2d)."""
    limbs = limbs or get_act_limbs()
    _req(x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous() and x.shape[1] <= 4,
         "image_quantize_s2d: need contiguous NCHW fp32 with <= 4 channels")
    n, c, h, w = x.shape
    _req(h >= 2 and w >= 2, "image_quantize_s2d: h and w must be >= 2")
    _req(x_absmax.numel() == n and x_absmax.dtype == torch.float32, "image_quantize_s2d: absmax")
    out = torch.empty(limbs, n, (h + 1) // 2, (w + 1) // 2, 16, dtype=torch.int8, device=x.device)
    _launch(x.device, "smpq_image_quantize_s2d", x, n, c, h, w, x_absmax, int(limbs), out)
    return out


def pack_weights_s2d(w, wlimbs, step=None):
    """7x7 stem weight fp32 [cout, c <= 4, 7, 7] -> (codes int8 [wlimbs, cout, 256] in the
    space-to-depth K order, wscale fp32 [cout]): channels with a recorded quantization step
    (``step`` [cout], 0 = never quantized) as exact codes, the others in per-channel fixed point
    (wlimbs 2 or 3: 16 / 24 bits), like pack_weights_ex."""
    _req(w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and tuple(w.shape[2:]) == (7, 7)
         and w.shape[1] <= 4, "pack_weights_s2d: need a CUDA fp32 [cout, <=4, 7, 7] weight")
    _req(wlimbs in (2, 3), "pack_weights_s2d: wlimbs must be 2 or 3")
    w = w.contiguous()
    cout, cin = w.shape[:2]
    codes = torch.empty(wlimbs, cout, 256, dtype=torch.int8, device=w.device)
    wscale = torch.empty(cout, dtype=torch.float32, device=w.device)
    status = torch.zeros(3, dtype=torch.int32, device=w.device)
    if step is not None:
        step = step.to(device=w.device, dtype=torch.float32).contiguous()
        _req(step.numel() == cout, "pack_weights_s2d: step length")
    _launch(w.device, "smpq_pack_weights_s2d_ex", w, cout, cin, step, int(wlimbs), codes, wscale, status)
    return codes, wscale


def stem_conv_s2d(xq, x_absmax, codes, h, w, col_scale, col_shift, relu=True, y_absmax=None, tile_cfg=-1,
                  emit_range=None, overflow=None, want_f32=True):
    """The stem conv (7x7/2/3 on the original h x w image) on space-to-depth planes from
    image_quantize_s2d with pack_weights_s2d codes -> NHWC fp32 y [n, h/2, w/2, cout] (and the
    next limb planes when emit_range is given: returns (y or None, yq) then)."""
    limbs, n, h2, w2, c16 = xq.shape
    _req(c16 == 16 and h2 == (h + 1) // 2 and w2 == (w + 1) // 2, "stem_conv_s2d: planes do not match h, w")
    wlimbs, cout, K = codes.shape
    _req(K == 256, "stem_conv_s2d: codes must come from pack_weights_s2d")
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if emit_range is None:
        want_f32 = True
    y = torch.empty(n, ho, wo, cout, dtype=torch.float32, device=xq.device) if want_f32 else None
    yq = None
    if emit_range is not None:
        _req(overflow is not None, "stem_conv_s2d: emit_range needs an overflow flag tensor")
        yq = torch.empty(limbs, n, ho, wo, cout, dtype=torch.int8, device=xq.device)
    per_img = max(limbs * h2 * w2 * 16, (4 if want_f32 else 0) * ho * wo * cout,
                  (limbs if yq is not None else 0) * ho * wo * cout)
    chunks = _image_chunks(n, per_img, "stem_conv_s2d")
    if chunks:
        # 32-bit plane offsets in the kernel: the images in chunks, as conv2d_q does
        for i0, i1 in chunks:
            r = stem_conv_s2d(xq[:, i0:i1].contiguous(), x_absmax[i0:i1], codes, h, w, col_scale, col_shift, relu,
                              None if y_absmax is None else y_absmax[i0:i1], tile_cfg, emit_range, overflow, want_f32)
            if emit_range is None:
                y[i0:i1].copy_(r)
            else:
                if y is not None:
                    y[i0:i1].copy_(r[0])
                yq[:, i0:i1].copy_(r[1])
        return y if emit_range is None else (y, yq)
    hook = _CONV_HOOK[0]
    if hook is not None:
        hook.begin()
    _launch(xq.device, "smpq_stem_conv_s2d_q", xq, x_absmax, n, h, w, codes, int(wlimbs), cout, col_scale, col_shift,
            1 if relu else 0, int(limbs), y, y_absmax, yq, float(emit_range or 0.0), overflow, int(tile_cfg))
    if hook is not None:
        hook.end(alg_work(n, h, w, 3, cout, 7, 7, ho, wo, limbs, wlimbs, y is not None, yq is not None, False, False))
    return y if emit_range is None else (y, yq)


def tuned_stem_conv_s2d(xq, x_absmax, codes, h, w, col_scale, col_shift, relu=True, y_absmax=None, **kw):
    """stem_conv_s2d on the tile the committed table (or the autotuner) picks for this shape
    (every tile gives bitwise-identical results)."""
    key = ("stem_s2d", tuple(xq.shape), tuple(codes.shape), h, w, y_absmax is not None,
           kw.get("emit_range") is not None, kw.get("want_f32", True))

    def run(c):
        stem_conv_s2d(xq, x_absmax, codes, h, w, col_scale, col_shift, relu, y_absmax, c, **kw)
    # (the stem's 16-channel pixels use 64-wide K steps)
    cfg = _choose_tile(key, run, [c for c in tile_configs() if tile_kind(c) == TILE_LDS_DMA])
    return stem_conv_s2d(xq, x_absmax, codes, h, w, col_scale, col_shift, relu, y_absmax,
                         -1 if cfg is None else cfg, **kw)


def stem_pool_supported(xq, codes, h, w):
    """True when stem_pool_s2d handles these planes / codes (cout 64, h and w multiples of 4,
    w <= 224, (limbs, wlimbs) in {(3, 3), (2, 2), (1, 2)})."""
    limbs, n = xq.shape[:2]
    wlimbs, cout = codes.shape[:2]
    return bool(_lib.load().smpq_stem_pool_supported(n, h, w, cout, int(limbs), int(wlimbs)))


def stem_pool_s2d(xq, x_absmax, codes, h, w, col_scale, col_shift, emit_range, overflow):
    """conv1 7x7/2/3 + BN + ReLU + maxpool 3x3/2/1 (resnet.py:143-147) in one launch, static range:
    the pooled output's limb planes [limbs, n, h/4, w/4, 64], bitwise identical to
    maxpool_limbs(stem_conv_s2d(..., relu=True, emit_range=emit_range)[1])."""
    limbs, n, h2, w2, c16 = xq.shape
    _req(c16 == 16 and h2 == (h + 1) // 2 and w2 == (w + 1) // 2, "stem_pool_s2d: planes do not match h, w")
    wlimbs, cout, K = codes.shape
    _req(K == 256, "stem_pool_s2d: codes must come from pack_weights_s2d")
    _req(overflow is not None and emit_range is not None, "stem_pool_s2d: needs an output range and an overflow flag")
    yq = torch.empty(limbs, n, h // 4, w // 4, cout, dtype=torch.int8, device=xq.device)
    hook = _CONV_HOOK[0]
    if hook is not None:
        hook.begin()
    _launch(xq.device, "smpq_stem_pool_s2d_q", xq, x_absmax, n, h, w, codes, int(wlimbs), cout, col_scale, col_shift,
            int(limbs), yq, float(emit_range), overflow)
    if hook is not None:
        work = alg_work(n, h, w, 3, cout, 7, 7, h // 2, w // 2, limbs, wlimbs, False, False, False, False)
        work["bytes"] += limbs * n * (h // 4) * (w // 4) * cout  # the pooled output, written once
        work["shape"] = "%4d->%4d k7 %3d->%3d pool" % (3, cout, h, h // 4)
        hook.end(work)
    return yq


def maxpool_limbs(xq):
    """3x3/2/1 max pool on limb planes [L, n, h, w, c] (c % 16 == 0) -> [L, n, ho, wo, c] (exact:
    the quantizer is monotone, so pooling the codes = quantizing the pooled values)."""
    limbs, n, h, w, c = xq.shape
    _req(xq.is_cuda and xq.dtype == torch.int8 and xq.is_contiguous() and c % 16 == 0, "maxpool_limbs: planes")
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = torch.empty(limbs, n, ho, wo, c, dtype=torch.int8, device=xq.device)
    _launch(xq.device, "smpq_maxpool_limbs", xq, n, h, w, c, int(limbs), out)
    return out


def maxpool_quantize(x_nhwc, x_absmax, limbs=None, want_f32=True):
    """MaxPool2d(3, 2, 1) on NHWC fp32 fused with the activation quantizer of its output.
    Returns (limb planes [limbs, n, ho, wo, c], fp32 NHWC pooled or None)."""
    limbs = limbs or get_act_limbs()
    _req(x_nhwc.is_cuda and x_nhwc.dtype == torch.float32 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous()
         and x_nhwc.shape[3] % 4 == 0, "maxpool_quantize: need contiguous NHWC fp32, c % 4 == 0")
    n, h, w, c = x_nhwc.shape
    _req(x_absmax.numel() == n and x_absmax.dtype == torch.float32, "maxpool_quantize: absmax")
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    q = torch.empty(limbs, n, ho, wo, c, dtype=torch.int8, device=x_nhwc.device)
    f = torch.empty(n, ho, wo, c, dtype=torch.float32, device=x_nhwc.device) if want_f32 else None
    _launch(x_nhwc.device, "smpq_maxpool_quantize", x_nhwc, n, h, w, c, x_absmax, int(limbs), q, f)
    return q, f


def act_absmax(x_nhwc, out=None):
    """Per-image max|x| of an NHWC (or any [n, ...]) fp32 CUDA tensor -> fp32 [n]."""
    _req(x_nhwc.is_cuda and x_nhwc.dtype == torch.float32 and x_nhwc.is_contiguous(),
         "act_absmax: need a contiguous CUDA fp32 tensor")
    n = x_nhwc.shape[0]
    if out is None:
        out = torch.zeros(n, dtype=torch.float32, device=x_nhwc.device)
    _req(out.numel() == n and out.dtype == torch.float32 and out.is_contiguous(), "act_absmax: out")
    per = x_nhwc.numel() // n
    _launch(x_nhwc.device, "smpq_act_absmax", x_nhwc, n, per, out)
    return out


def act_quantize(x, x_absmax, limbs=None, out=None):
    """fp32 [n, ...] -> int8 [limbs, n, ...] balanced digit planes (per-image range x_absmax)."""
    limbs = limbs or get_act_limbs()
    _req(x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(), "act_quantize: need contiguous CUDA fp32")
    n = x.shape[0]
    per = x.numel() // n
    _req(per % 8 == 0, "act_quantize: elements per image must be a multiple of 8")
    _req(x_absmax.dtype == torch.float32 and x_absmax.numel() == n and x_absmax.device == x.device, "act_quantize: absmax")
    if out is None:
        out = torch.empty((limbs,) + tuple(x.shape), dtype=torch.int8, device=x.device)
    _req(out.shape == (limbs,) + tuple(x.shape) and out.dtype == torch.int8 and out.is_contiguous(), "act_quantize: out")
    _launch(x.device, "smpq_act_quantize", x, n, per, x_absmax, int(limbs), out)
    return out


_TILES = {}


def tile_configs():
    """{cfg: (BM, BN, threads)} of the conv kernel's block tiles (BM output pixels x BN output
    channels; csrc/conv_glds_kernel.h kGlds)."""
    if not _TILES:
        lib = _lib.load()
        import ctypes
        for c in range(lib.smpq_conv2d_num_tile_configs()):
            bm, bn, nt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            _lib.check(lib.smpq_conv2d_tile_config(c, ctypes.byref(bm), ctypes.byref(bn), ctypes.byref(nt)),
                       "smpq_conv2d_tile_config")
            _TILES[c] = (bm.value, bn.value, nt.value)
            kind = lib.smpq_conv2d_tile_kind(c)
            if kind < 0:
                _lib.check(kind, "smpq_conv2d_tile_kind")
            _KINDS[c] = kind
    return _TILES


TILE_LDS_DMA, TILE_LDS_DMA_K128, TILE_HALO3X3, TILE_RESIDENT1X1 = 2, 3, 4, 5  # include/smpq.h SMPQ_TILE_*
TILE_RESIDENT1X1_W = 6
_KINDS = {}


def tile_kind(cfg):
    """Kernel family of a tile config (TILE_LDS_DMA / TILE_LDS_DMA_K128: 64- or 128-wide K steps;
    TILE_HALO3X3: the halo-patch 3x3 kernel, static-range limb-plane output only;
    TILE_RESIDENT1X1 / TILE_RESIDENT1X1_W: the weight-stationary 1x1 tiles)."""
    tile_configs()
    return _KINDS[cfg]


def conv2d_q(xq, x_absmax, codes, offset, kh, kw, stride, pad, col_scale, col_shift,
             residual=None, relu=False, y_absmax=None, out=None, tile_cfg=-1,
             emit_range=None, overflow=None, want_f32=True, residual_q=None, residual_range=None,
             weight_layout="auto"):
    """Quantized conv on int8 limb planes xq [L, n, h, w, cin] (from act_quantize / maxpool_quantize /
    stem_pool_s2d / a previous conv2d_q) and weight limb planes codes [LW, cout, K] (or
    [cout, K] for LW = 1): y = conv(x, w) * s_x * col_scale + col_shift (+res) (relu), NHWC fp32.
    With ``emit_range`` (static range of the output, float) the epilogue also writes the output's
    int8 limb planes [L, n, ho, wo, cout] and sets ``overflow`` (int32 [1]) if a value exceeded the
    range; returns (y or None, yq) then. ``residual_q`` (+ ``residual_range``): the residual as
    int8 limb planes [L, n, ho, wo, cout] instead of fp32 ``residual``. ``weight_layout``: "auto"
    lets the kernel read the K-major copy pack_weights_ex attached to ``codes`` (bitwise the same
    results; only while KMAJOR is on), "rowmajor" keeps it on ``codes`` itself. A batch whose
    planes would reach 2 GiB (the kernel's 32-bit buffer offsets) runs in image chunks."""
    _req(xq.is_cuda and xq.dtype == torch.int8 and xq.dim() == 5 and xq.is_contiguous(), "conv: xq must be [L,n,h,w,c] int8")
    limbs, n, h, w, cin = xq.shape
    _req(limbs in (1, 2, 3), "conv: limbs")
    km = getattr(codes, "_smpq_km", None) if (weight_layout == "auto" and KMAJOR[0]) else None
    if codes.dim() == 2:
        codes = codes.unsqueeze(0)
    wlimbs, cout, K = codes.shape
    _req(wlimbs in (1, 2, 3) and (wlimbs < 3 or limbs == 3), "conv: weight limbs")
    _req(codes.dtype == torch.int8 and K == kh * kw * cin and codes.is_contiguous() and codes.device == xq.device,
         "conv: codes shape")
    _req(cin % 64 == 0, "conv: cin must be a multiple of 64 (the <= 4-channel stem: stem_conv_s2d)")
    _req(cout % 16 == 0, "conv: cout must be a multiple of 16")
    _req(offset is None or (offset.dtype == torch.int32 and offset.numel() == cout), "conv: offset")
    _req(x_absmax.dtype == torch.float32 and x_absmax.numel() == n, "conv: x_absmax")
    for t in (col_scale, col_shift):
        _req(t.dtype == torch.float32 and t.numel() == cout and t.is_contiguous() and t.device == xq.device,
             "conv: col vectors")
    ho = (h + 2 * pad - kh) // stride + 1
    wo = (w + 2 * pad - kw) // stride + 1
    _req(ho > 0 and wo > 0, "conv: empty output")
    yq = None
    if emit_range is not None:
        _req(emit_range > 0 and cout % 4 == 0, "conv: emit_range must be > 0 and cout % 4 == 0")
        _req(overflow is not None and overflow.dtype == torch.int32 and overflow.device == xq.device, "conv: overflow")
        yq = torch.empty(limbs, n, ho, wo, cout, dtype=torch.int8, device=xq.device)
    else:
        want_f32 = True
    if out is None and want_f32:
        out = torch.empty(n, ho, wo, cout, dtype=torch.float32, device=xq.device)
    _req(out is None or (out.shape == (n, ho, wo, cout) and out.is_contiguous()), "conv: out shape")
    if residual is not None:
        _req(residual.shape == (n, ho, wo, cout) and residual.is_contiguous() and residual.dtype == torch.float32,
             "conv: residual shape")
    if residual_q is not None:
        _req(residual is None and residual_q.shape == (limbs, n, ho, wo, cout) and residual_q.dtype == torch.int8
             and residual_q.is_contiguous() and residual_range is not None and residual_range > 0
             and cout % 4 == 0, "conv: residual_q")
    if y_absmax is not None:
        _req(y_absmax.numel() == n and y_absmax.dtype == torch.float32, "conv: y_absmax")
    per_img = max(limbs * h * w * cin, (limbs if (yq is not None or residual_q is not None) else 0) * ho * wo * cout,
                  (4 if (out is not None or residual is not None) else 0) * ho * wo * cout)
    chunks = _image_chunks(n, per_img, "conv")
    if chunks:
        # the kernel addresses each plane with 32-bit offsets: run the images in chunks
        for i0, i1 in chunks:
            r = conv2d_q(xq[:, i0:i1].contiguous(), x_absmax[i0:i1], codes, offset, kh, kw, stride, pad,
                         col_scale, col_shift, residual=None if residual is None else residual[i0:i1], relu=relu,
                         y_absmax=None if y_absmax is None else y_absmax[i0:i1],
                         out=None if out is None else out[i0:i1], tile_cfg=tile_cfg, emit_range=emit_range,
                         overflow=overflow, want_f32=want_f32,
                         residual_q=None if residual_q is None else residual_q[:, i0:i1].contiguous(),
                         residual_range=residual_range, weight_layout=weight_layout)
            if yq is not None:
                yq[:, i0:i1].copy_(r[1])
        return (out, yq) if emit_range is not None else out
    hook = _CONV_HOOK[0]
    if hook is not None:
        hook.begin()
    if km is not None:
        _req(km.shape == (wlimbs, K // 64, cout, 64) and km.device == xq.device, "conv: K-major codes")
    _launch(xq.device, "smpq_conv2d_fwd_q_km", xq, x_absmax, n, h, w, cin, codes, km, int(wlimbs), offset, cout, kh, kw,
            stride, pad, col_scale, col_shift, residual, 1 if relu else 0, int(limbs), out, y_absmax, yq,
            float(emit_range or 0.0), overflow, residual_q, float(residual_range or 0.0), int(tile_cfg))
    if hook is not None:
        hook.end(alg_work(n, h, w, cin, cout, kh, kw, ho, wo, limbs, wlimbs, out is not None, yq is not None,
                          residual is not None, residual_q is not None))
    if emit_range is not None:
        return out, yq
    return out


def conv_pair_supported(cin, cout1, cout2, limbs=3):
    """Does smpq_conv2d_pair_fwd run this Bottleneck chain (conv3 cin -> cout1, next conv1 cout1 ->
    cout2)?"""
    return bool(_lib.load().smpq_conv2d_pair_supported(int(cin), int(cout1), int(cout2), int(limbs)))


def conv_chain_supported(cin, cout1, cout2=0, limbs=3):
    """Does smpq_conv2d_chain_fwd run a conv3 cin -> cout1 (+ a fused downsample) (-> next conv1
    cout1 -> cout2; 0: none)?"""
    return bool(_lib.load().smpq_conv2d_chain_supported(int(cin), int(cout1), int(cout2), int(limbs)))


def conv_chain_ds_supported(cin, cout1, ds_cin, ds_stride, limbs=3):
    """Does smpq_conv2d_chain_fwd run conv3 cin -> cout1 with a fused 1x1 downsample ds_cin ->
    cout1 of this stride (and no chained conv1)?"""
    return bool(_lib.load().smpq_conv2d_chain_ds_supported(int(cin), int(cout1), int(ds_cin), int(ds_stride),
                                                           int(limbs)))


def _one_limb(codes, what):
    _req(codes.dim() == 2 or codes.shape[0] == 1, "chain: %s needs exact codes (one weight limb)" % what)
    return codes[0] if codes.dim() == 3 else codes


# conv_chain_q's fused downsample: its input limb planes and their per-image range, its codes
# [3, cout1, ds_cin], folded scale and shift, static output range and stride; and its chained next
# conv1: codes, folded scale and shift, static output range
ChainDs = namedtuple("ChainDs", "xq x_absmax codes col_scale col_shift rng stride", defaults=(1,))
ChainNext = namedtuple("ChainNext", "codes col_scale col_shift rng")


def conv_chain_q(xq, x_absmax, codes1, offset1, col_scale1, col_shift1, emit_range1, y1_absmax, overflow,
                 residual_q=None, residual_range=None, ds=None, nxt=None):
    """A Bottleneck's conv3 (1x1 + folded BN + identity + ReLU, exact codes, optional weight offsets)
    in one launch with (csrc/conv_resident.hip, smpq_conv2d_chain_fwd):
      - its identity: ``residual_q`` limb planes (+ ``residual_range``), or ``ds`` (a ChainDs, or its
        fields as a plain tuple): the block's 1x1 downsample (stride 1 by default) over conv3's
        output pixels, computed in the same tiles (its output codes feed the residual; never written);
      - ``nxt`` (a ChainNext, or its fields as a plain tuple): the next block's conv1 (ReLU) on
        conv3's output tile.
    Returns (yq1, yq2 or None), bitwise what the separate launches write; ``overflow`` covers every
    output of the chain (the downsample's included)."""
    ds = None if ds is None else ChainDs(*ds)
    nxt = None if nxt is None else ChainNext(*nxt)
    _req(xq.is_cuda and xq.dtype == torch.int8 and xq.dim() == 5 and xq.is_contiguous(), "chain: xq")
    limbs, n, h, w, cin = xq.shape
    c1 = _one_limb(codes1, "conv3")
    cout1 = c1.shape[0]
    c2 = _one_limb(nxt.codes, "conv1") if nxt is not None else None
    cout2 = c2.shape[0] if c2 is not None else 0
    _req(c1.shape == (cout1, cin) and c1.is_contiguous() and c1.dtype == torch.int8, "chain: conv3 codes")
    _req(c2 is None or (c2.shape == (cout2, cout1) and c2.is_contiguous() and c2.dtype == torch.int8),
         "chain: conv1 codes")
    if ds is not None:
        _req(cout2 == 0 and conv_chain_ds_supported(cin, cout1, ds.xq.shape[-1], int(ds.stride), limbs),
             "chain: shape not built")
    else:
        _req(conv_chain_supported(cin, cout1, cout2, limbs), "chain: shape not built")
    _req((residual_q is None) != (ds is None), "chain: one identity source (residual_q or ds)")
    _req(offset1 is None or (offset1.dtype == torch.int32 and offset1.numel() == cout1), "chain: offset")
    if residual_q is not None:
        _req(residual_q.shape == (limbs, n, h, w, cout1) and residual_q.dtype == torch.int8
             and residual_q.is_contiguous() and residual_range is not None and residual_range > 0, "chain: residual_q")
    vecs = [(col_scale1, cout1), (col_shift1, cout1)]
    dh = dw = dcin = 0
    if ds is not None:
        dxq, ds_stride = ds.xq, int(ds.stride)
        _, _, dh, dw, dcin = dxq.shape
        _req(dxq.dim() == 5 and dxq.shape[:2] == (limbs, n) and (dh - 1) // ds_stride + 1 == h
             and (dw - 1) // ds_stride + 1 == w and dxq.dtype == torch.int8 and dxq.is_contiguous()
             and ds.x_absmax.numel() == n, "chain: downsample input (its output pixels must be conv3's)")
        _req(ds.codes.shape == (3, cout1, dcin) and ds.codes.dtype == torch.int8 and ds.codes.is_contiguous(),
             "chain: downsample codes [3, cout, ds_cin]")
        _req(ds.rng > 0, "chain: downsample range")
        vecs += [(ds.col_scale, cout1), (ds.col_shift, cout1)]
    if nxt is not None:
        vecs += [(nxt.col_scale, cout2), (nxt.col_shift, cout2)]
        _req(y1_absmax is not None and y1_absmax.numel() == n, "chain: y1_absmax")
    for t, c in vecs:
        _req(t.dtype == torch.float32 and t.numel() == c and t.is_contiguous() and t.device == xq.device,
             "chain: col vectors")
    _req(x_absmax.numel() == n and overflow is not None and overflow.dtype == torch.int32
         and overflow.device == xq.device, "chain: absmax / overflow")
    chunks = _image_chunks(n, limbs * max(h * w * max(cin, cout1), dh * dw * dcin), "chain")
    yq1 = torch.empty(limbs, n, h, w, cout1, dtype=torch.int8, device=xq.device)
    yq2 = torch.empty(limbs, n, h, w, cout2, dtype=torch.int8, device=xq.device) if nxt is not None else None
    if chunks:  # 32-bit buffer offsets: image chunks
        for i0, i1 in chunks:
            a, b = conv_chain_q(
                xq[:, i0:i1].contiguous(), x_absmax[i0:i1], codes1, offset1, col_scale1, col_shift1, emit_range1,
                None if y1_absmax is None else y1_absmax[i0:i1], overflow,
                residual_q=None if residual_q is None else residual_q[:, i0:i1].contiguous(),
                residual_range=residual_range,
                ds=None if ds is None else ds._replace(xq=dxq[:, i0:i1].contiguous(), x_absmax=ds.x_absmax[i0:i1]),
                nxt=nxt)
            yq1[:, i0:i1].copy_(a)
            if b is not None:
                yq2[:, i0:i1].copy_(b)
        return yq1, yq2
    hook = _CONV_HOOK[0]
    if hook is not None:
        hook.begin()
    # (an absent downsample / next conv: null pointers and zeros)
    d = ds or ChainDs(None, None, None, None, None, 0.0, 0)
    nx = nxt or ChainNext(None, None, None, 0.0)
    _launch(xq.device, "smpq_conv2d_chain_fwd", xq, x_absmax, n, h, w, cin, c1, offset1, cout1, col_scale1, col_shift1,
            residual_q, float(residual_range or 0.0),
            d.xq, d.x_absmax, dh, dw, dcin, int(d.stride), d.codes, 3 if ds else 0, d.col_scale, d.col_shift,
            float(d.rng), yq1, float(emit_range1), y1_absmax,
            c2, cout2, nx.col_scale, nx.col_shift, yq2, float(nx.rng), overflow)
    if hook is not None:
        # one launch doing every chained conv's work; the reads / writes it removes are not counted
        w1 = alg_work(n, h, w, cin, cout1, 1, 1, h, w, limbs, 1, False, True, False, residual_q is not None)
        ops_, nbytes, shape = w1["ops"], w1["bytes"], "%4d->%4d" % (cin, cout1)
        if ds is not None:
            wd = alg_work(n, dh, dw, dcin, cout1, 1, 1, h, w, limbs, 3, False, False, False, False)
            ops_ += wd["ops"]
            nbytes += wd["bytes"]  # the downsample's input and weights (its output never leaves the CU)
            shape += "+ds"
        if nxt is not None:
            w2 = alg_work(n, h, w, cout1, cout2, 1, 1, h, w, limbs, 1, False, True, False, False)
            ops_ += w2["ops"]
            nbytes += w2["bytes"] - limbs * n * h * w * cout1  # conv1 reads conv3's tile from LDS
            shape += "->%4d" % cout2
        hook.end({"ops": ops_, "bytes": nbytes, "passes": w1["passes"], "shape": "%s k1 %3d chain" % (shape, h)})
    return yq1, yq2


def conv_pair_q(xq, x_absmax, codes1, col_scale1, col_shift1, residual_q, residual_range, emit_range1,
                y1_absmax, codes2, col_scale2, col_shift2, emit_range2, overflow):
    """A Bottleneck's conv3 (1x1 + folded BN + limb-plane identity + ReLU) chained with the next
    block's conv1 (1x1 + folded BN + ReLU) in one launch: returns (yq1, yq2), bitwise

        _, yq1 = conv2d_q(xq, x_absmax, codes1, None, 1, 1, 1, 0, col_scale1, col_shift1, relu=True,
                          emit_range=emit_range1, overflow=overflow, want_f32=False,
                          residual_q=residual_q, residual_range=residual_range)
        _, yq2 = conv2d_q(yq1, y1_absmax, codes2, None, 1, 1, 1, 0, col_scale2, col_shift2, relu=True,
                          emit_range=emit_range2, overflow=overflow, want_f32=False)

    without reading yq1 back from HBM (conv_chain_q with the next conv and no downsample)."""
    c1, c2 = _one_limb(codes1, "conv3"), _one_limb(codes2, "conv1")
    _req(conv_pair_supported(xq.shape[-1], c1.shape[0], c2.shape[0], xq.shape[0]), "pair: shape not built")
    return conv_chain_q(xq, x_absmax, codes1, None, col_scale1, col_shift1, emit_range1, y1_absmax, overflow,
                        residual_q=residual_q, residual_range=residual_range,
                        nxt=(codes2, col_scale2, col_shift2, emit_range2))


# ---- per-shape tile choice (cf. cudnn.benchmark=True, resnet50_main.py:10) ---------------------
# Every tile configuration gives bitwise-identical results; only the time differs. A shape's tile
# comes from (1) this process's cache, (2) the committed table smpq/data/tiles_gfx950.json
# (tools/tune_tiles.py: medians of many timed launches on an MI355X, so a benchmark does not depend
# on a short timing race), or (3) the autotuner: TUNE_REPS timed launches per candidate after two
# warm-ups, the candidate with the smallest median wins. SMPQ_TILE_TABLE=<path> uses another table,
# SMPQ_TILE_TABLE=off none; SMPQ_AUTOTUNE=0 turns (3) off (the C-ABI default tile then).
AUTOTUNE = [os.environ.get("SMPQ_AUTOTUNE", "1") != "0"]
TUNE_REPS = [int(os.environ.get("SMPQ_TUNE_REPS", "10"))]
# diagnostics (A/B of tile families on one box): tile configs the autotuner never tries
TILES_EXCLUDED = {int(c) for c in os.environ.get("SMPQ_TILES_EXCLUDE", "").split(",") if c.strip()}
# SMPQ_RESIDENT_W=1: the TILE_RESIDENT1X1_W configurations are candidates for the 1x1 convs they run (3
# weight limbs + ReLU: a model under search); 0: the candidates are those without the kind. On by the
# rule and the measurement in DESIGN §5l (the pristine ResNet-50 forward: 7.80 against 8.64 ms per batch).
RESIDENT_W = [os.environ.get("SMPQ_RESIDENT_W", "1") != "0"]
# tools/tune_tiles.py --concurrent: time each candidate as TUNE_CONCURRENT copies launched together on
# their own streams (the timed forward runs its batch slices concurrently, and a tile's isolated time
# does not predict how it shares the GPU with the other slice's kernels); TUNE_LOG keeps every
# candidate's median per key
TUNE_CONCURRENT = [1]
TUNE_LOG = {}
_TUNED = {}
TILE_TABLE_DEFAULT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "tiles_gfx950.json")
_TABLE = {"path": None, "sha16": None, "entries": {}, "hits": 0, "tuned": 0}


def key_str(key):
    """The table's text form of a tile key (the tuple tuned_conv2d_q / tuned_stem_conv_s2d use)."""
    def f(v):
        if isinstance(v, tuple):
            return "x".join(f(u) for u in v)
        return str(int(v)) if isinstance(v, bool) else str(v)
    return "|".join(f(v) for v in key)


def load_tile_table(path=None):
    """(Re)load the committed tile table (None: SMPQ_TILE_TABLE or the default; "off": none)."""
    import hashlib
    import json
    path = path or os.environ.get("SMPQ_TILE_TABLE", TILE_TABLE_DEFAULT)
    _TABLE.update(path=None, sha16=None, entries={}, hits=0, tuned=0, loaded=True)
    if path in ("off", "0", "") or not os.path.exists(path):
        return _TABLE
    raw = open(path, "rb").read()
    doc = json.loads(raw)
    _TABLE.update(path=path, sha16=hashlib.sha256(raw).hexdigest()[:16],
                  entries={k: int(v) for k, v in doc.get("tiles", {}).items()})
    return _TABLE


def tile_table_info():
    """What the bench reports: table file, content hash, entries, table hits / autotuned shapes."""
    return {"path": None if _TABLE["path"] is None else os.path.relpath(_TABLE["path"], os.path.dirname(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
            "sha16": _TABLE["sha16"], "entries": len(_TABLE["entries"]), "hits": _TABLE["hits"],
            "autotuned": _TABLE["tuned"]}


def _choose_tile(key, run, cands, variant=None):
    """The tile for ``key``: cached, from the table, or autotuned (None: the C-ABI default).
    ``variant`` separates calls of one key whose candidate sets differ (the cache only)."""
    ckey = key if variant is None else (key, variant)
    cfg = _TUNED.get(ckey)
    if cfg is not None:
        return cfg
    if not _TABLE.get("loaded"):
        load_tile_table()
    t = _TABLE["entries"].get(key_str(key))
    if t is not None and t in cands:
        _TUNED[ckey] = t
        _TABLE["hits"] += 1
        return t
    if not AUTOTUNE[0] or torch.cuda.is_current_stream_capturing():
        return None
    best = None
    nconc = TUNE_CONCURRENT[0]
    side = [torch.cuda.Stream() for _ in range(nconc)] if nconc > 1 else []

    def once(c):
        if not side:
            run(c)
            return
        main = torch.cuda.current_stream()
        for st in side:  # the copies write the same outputs: identical values, timing only
            st.wait_stream(main)
            with torch.cuda.stream(st):
                run(c)
        for st in side:
            main.wait_stream(st)
    log = TUNE_LOG.setdefault(key_str(key) + ("" if variant is None else "|" + str(variant)), {})
    for c in cands:
        if c in TILES_EXCLUDED:
            continue
        try:
            once(c)
            once(c)
            evs = []
            for _ in range(TUNE_REPS[0]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                once(c)
                e1.record()
                evs.append((e0, e1))
        except _lib.SmpqError:
            continue  # the configuration does not take this shape
        torch.cuda.synchronize()
        ts = sorted(a.elapsed_time(b) for a, b in evs)
        t_med = ts[len(ts) // 2]
        log[c] = round(t_med * 1e3, 2)
        if best is None or t_med < best[0]:
            best = (t_med, c)
    if best is None:
        return None
    _TUNED[ckey] = best[1]
    _TABLE["tuned"] += 1
    return best[1]


def _tile_fits(cfg, limbs, wlimbs=1, cout=None, cin=None, k=1):
    """Can tile config ``cfg`` run this conv (libsmpq's own launch rules)? ``cin``/``cout`` default
    to a shape every configuration takes."""
    cin = cin if cin is not None else 128
    cout = cout if cout is not None else 64
    return bool(_lib.load().smpq_conv2d_tile_supported(int(cfg), int(cin), int(cout), int(k), int(k),
                                                         int(limbs), int(wlimbs)))


def tuned_conv2d_q(xq, x_absmax, codes, offset, kh, kw, stride, pad, col_scale, col_shift,
                   residual=None, relu=False, y_absmax=None, out=None, emit_range=None, overflow=None,
                   want_f32=True, residual_q=None, residual_range=None):
    """conv2d_q on the tile the committed table (or the autotuner) picks for this shape. Every
    tile gives bitwise-identical results (exact integer accumulation, same epilogue)."""
    limbs, n, h, w, cin = xq.shape
    wlimbs = codes.shape[0] if codes.dim() == 3 else 1
    cout = codes.shape[-2]
    key = (n, h, w, cin, cout, kh, kw, stride, pad, limbs, wlimbs, residual is not None, emit_range is not None,
           want_f32, residual_q is not None)

    args = (xq, x_absmax, codes, offset, kh, kw, stride, pad, col_scale, col_shift)
    kwargs = dict(residual=residual, relu=relu, y_absmax=y_absmax, out=out, emit_range=emit_range, overflow=overflow,
               want_f32=want_f32, residual_q=residual_q, residual_range=residual_range)

    def run(c):
        conv2d_q(*args, tile_cfg=c, **kwargs)
    gates = _conv_tile_gates(kh, kw, stride, pad, wlimbs, offset, residual, relu, y_absmax, out, emit_range,
                             want_f32, residual_q)
    variant = _conv_tile_variant(gates)
    # this process's cache first: the candidate list (one smpq_conv2d_tile_supported call per tile
    # configuration) is built only for a key's first call
    cfg = _TUNED.get(key if variant is None else (key, variant))
    if cfg is None:
        cfg = _choose_tile(key, run, _conv_tile_candidates(limbs, wlimbs, cout, cin, kh, gates), variant=variant)
    return conv2d_q(*args, tile_cfg=-1 if cfg is None else cfg, **kwargs)


def _conv_tile_gates(kh, kw, stride, pad, wlimbs, offset, residual, relu, y_absmax, out, emit_range, want_f32,
                     residual_q):
    """(halo_ok, res_ok, resw_ok): which lean-epilogue tile kinds may run this tuned_conv2d_q call.
    The key does not carry relu / y_absmax / offset, so other calls of a key never see them."""
    lean = emit_range is not None and not want_f32 and residual is None and y_absmax is None and out is None
    # the halo tiles run only the static-range limb-plane epilogue with ReLU, optionally with a
    # limb-plane residual (stride 1 / pad 1 for now)
    halo_ok = bool(lean and relu and kh == 3 and kw == 3 and stride == 1 and pad == 1)
    # the weight-stationary 1x1 tiles: the static-range limb-plane epilogue, built for the
    # downsamples (3 weight limbs, no ReLU or residual) and for exact-code convs with ReLU + a
    # limb-plane residual, ReLU only (both also with weight offsets), or neither
    # (smpq_conv2d_tile_supported checks the shape)
    res_ok = bool(lean and kh == 1 and kw == 1 and pad == 0
                  and (offset is None or (wlimbs == 1 and relu))
                  and (not (relu or residual_q is not None) if wlimbs == 3 else (relu or residual_q is None)))
    # the same with 3 weight limbs + ReLU (with or without a limb-plane residual, stride 1): the
    # 1x1 convs of a model under search, whose operand is fixed point while a channel is free
    resw_ok = bool(RESIDENT_W[0] and lean and relu and offset is None and kh == 1 and kw == 1 and pad == 0
                   and stride == 1 and wlimbs == 3)
    return halo_ok, res_ok, resw_ok


def _conv_tile_variant(gates):
    """The cache variant of a call: separates calls of one key whose candidate sets differ."""
    halo_ok, res_ok, resw_ok = gates
    return "resw" if resw_ok else (None if (halo_ok or res_ok) else "nohalo")


def _conv_tile_candidates(limbs, wlimbs, cout, cin, kh, gates):
    """The tile configurations tuned_conv2d_q may choose from for a call with these gates."""
    halo_ok, res_ok, resw_ok = gates
    return [c for c in tile_configs() if _tile_fits(c, limbs, wlimbs, cout, cin, kh)
            and (halo_ok or tile_kind(c) != TILE_HALO3X3) and (res_ok or tile_kind(c) != TILE_RESIDENT1X1)
            and (resw_ok or tile_kind(c) != TILE_RESIDENT1X1_W)]


def conv2d_nhwc(x, x_absmax, codes, offset, kh, kw, stride, pad, col_scale, col_shift,
                residual=None, relu=False, limbs=None, y_absmax=None, out=None):
    """act_quantize + (autotuned) conv2d_q on an NHWC fp32 input."""
    xq = act_quantize(x, x_absmax, limbs)
    return tuned_conv2d_q(xq, x_absmax, codes, offset, kh, kw, stride, pad, col_scale, col_shift,
                          residual=residual, relu=relu, y_absmax=y_absmax, out=out)


def set_conv_hook(hook):
    """hook.begin() / hook.end(work) around every quantized-conv launch (bench.py's timer);
    work = alg_work(...) of the launch."""
    _CONV_HOOK[0] = hook


def alg_work(n, h, w, cin, cout, kh, kw, ho, wo, limbs, wlimbs, y_f32, y_q, res_f32, res_q):
    """Algorithmic work of one quantized-conv launch: ops = 2 * MACs; bytes =
    each input activation code read once (limbs bytes per element: the int8/16/24 code), the
    weight codes once, and every output element written once (limbs bytes for the next conv's
    limb planes, 4 for fp32) plus its residual read once (limbs or 4 bytes). Halo re-reads of
    3x3 windows and zero padding are not counted: they are the kernel's overhead."""
    macs = n * ho * wo * cout * kh * kw * cin
    out_elems = n * ho * wo * cout
    per_out = (4 if y_f32 else 0) + (limbs if y_q else 0) + (4 if res_f32 else 0) + (limbs if res_q else 0)
    # a strided 1x1 conv reads only the pixels it samples (1/stride^2 of its input)
    in_elems = n * ho * wo * cin if (kh == 1 and kw == 1) else n * h * w * cin
    nbytes = limbs * in_elems + wlimbs * cout * kh * kw * cin + out_elems * per_out
    return {"ops": 2 * macs, "bytes": nbytes, "passes": limbs * wlimbs - _skipped_passes(limbs, wlimbs),
            "shape": "%4d->%4d k%d %3d->%3d %s%s" % (cin, cout, kh, h, ho, "f" if y_f32 else "-",
                                                    "r" if (res_f32 or res_q) else "-")}


def _skipped_passes(limbs, wlimbs):
    smin = max(0, limbs + wlimbs - 4)  # low-digit products skipped by the kernels (conv.hip)
    return sum(1 for la in range(limbs) for lw in range(wlimbs) if la + lw < smin)


def debug_mfma_i8(a, b):
    """One v_mfma_i32_16x16x64_i8 with the kernel's fragment mapping: a[16,64] @ b[16,64]^T."""
    _req(a.is_cuda and a.dtype == torch.int8 and a.shape == (16, 64), "debug_mfma: a")
    _req(b.is_cuda and b.dtype == torch.int8 and b.shape == (16, 64), "debug_mfma: b")
    c = torch.empty(16, 16, dtype=torch.int32, device=a.device)
    _launch(a.device, "smpq_debug_mfma_i8", a.contiguous(), b.contiguous(), c)
    return c


# ---- evaluation reductions (functions.py:84-149) on device -----------------------------------
def softmax_xent(logits, labels, stats, want_probs=True):
    """One batch of functions.evaluate_acc_loss_softmax (functions.py:113-121) in one kernel:
    returns the softmax [B, C] fp32 (or None) and accumulates into ``stats`` (float64 [4], on the
    logits' device): [0] += batch-mean cross entropy, [1] += correct top-1, [2] += rows, [3] += 1."""
    _req(logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous(),
         "softmax_xent: logits must be a contiguous fp32 [B, C] device tensor")
    rows, cols = logits.shape
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    _req(labels.numel() == rows, "softmax_xent: labels")
    _req(stats.dtype == torch.float64 and stats.numel() >= 4 and stats.device == logits.device, "softmax_xent: stats")
    probs = torch.empty_like(logits) if want_probs else None
    ws = torch.empty(2 * max(rows, 1), dtype=torch.float32, device=logits.device)
    _launch(logits.device, "smpq_softmax_xent", logits, labels, rows, cols, probs, stats, ws)
    return probs


def kl_rows(p_ref, p, stats):
    """functions.KLdiv (functions.py:131-149) for one batch pair: stats (float64 [2]) +=
    (sum over images of sum_c p_ref * log(p_ref / p), images)."""
    for t in (p_ref, p):
        _req(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2, "kl_rows: fp32 [B, C] device tensors")
    _req(p_ref.shape == p.shape and p_ref.device == p.device, "kl_rows: shapes")
    p_ref, p = p_ref.contiguous(), p.contiguous()
    _req(stats.dtype == torch.float64 and stats.numel() >= 2 and stats.device == p.device, "kl_rows: stats")
    rows, cols = p.shape
    ws = torch.empty(max(rows, 1), dtype=torch.float32, device=p.device)
    _launch(p.device, "smpq_kl_rows", p_ref, p, rows, cols, stats, ws)


def avgpool_fc(x_nhwc, weight, bias, out=None):
    """AdaptiveAvgPool2d(1) + flatten + Linear (resnet.py:216-218) on the last block's NHWC fp32
    output [n, h, w, c] -> logits [n, nout] fp32 (into ``out`` when given: a contiguous [n, nout]
    fp32 tensor, e.g. a batch slice's rows of the whole batch's logits). Each logit is summed in an
    order fixed by c alone (smpq_avgpool_fc), so an image's logits are the same bits in any batch
    or data-parallel shard."""
    _req(x_nhwc.is_cuda and x_nhwc.dtype == torch.float32 and x_nhwc.dim() == 4 and x_nhwc.is_contiguous(),
         "avgpool_fc: need contiguous NHWC fp32 on the GPU")
    n, h, w, c = x_nhwc.shape
    _req(c % 4 == 0, "avgpool_fc: channels must be a multiple of 4")
    wt = weight.detach().float().contiguous()
    _req(wt.dim() == 2 and wt.shape[1] == c and wt.device == x_nhwc.device, "avgpool_fc: weight shape")
    nout = wt.shape[0]
    b = None if bias is None else bias.detach().float().contiguous()
    _req(b is None or (b.numel() == nout and b.device == x_nhwc.device), "avgpool_fc: bias")
    pooled = torch.empty(n, c, dtype=torch.float32, device=x_nhwc.device)
    if out is None:
        out = torch.empty(n, nout, dtype=torch.float32, device=x_nhwc.device)
    _req(out.shape == (n, nout) and out.dtype == torch.float32 and out.is_contiguous() and out.device == x_nhwc.device,
         "avgpool_fc: out must be a contiguous [n, nout] fp32 tensor on the input's device")
    _launch(x_nhwc.device, "smpq_avgpool_fc", x_nhwc, n, h * w, c, wt, b, nout, pooled, out)
    return out


# ---- bit-packed weight store, format smpq-packed/1 (include/smpq.h) ----------------------------
# Every function takes the weight's device from its tensors: the HIP kernels for device tensors,
# the native host twins for host tensors. Outputs are allocated here as int8 (byte) buffers.
BITPACK_MAX_K = 1 << 26


def _bp_meta(cout, dev, **named):
    """The per-channel arrays of one weight: dtype, length, device, contiguity."""
    want = {"qbits": torch.int8, "mode": torch.int8, "base": torch.int32, "step": torch.float32}
    for name, t in named.items():
        if name == "word_off":
            _req(t.dtype == torch.int64 and t.numel() == cout + 1 and t.device == dev and t.is_contiguous(),
                 "bitpack: word_off must be a contiguous int64 [cout + 1] tensor on the weight's device")
        else:
            _req(t.dtype == want[name] and t.numel() == cout and t.device == dev and t.is_contiguous(),
                 "bitpack: %s must be a contiguous %s [cout] tensor on the weight's device" % (name, want[name]))


def _bp_weight(w2d, what):
    _req(w2d.dtype == torch.float32 and w2d.dim() == 2 and w2d.is_contiguous() and w2d.numel() > 0,
         "%s: need a contiguous fp32 [cout, k] tensor" % what)
    _req(w2d.shape[1] <= BITPACK_MAX_K, "%s: k above 2^26" % what)
    return int(w2d.shape[0]), int(w2d.shape[1])


def bitpack_plan(w2d, qbits, step):
    """Which channels of ``w2d`` (fp32 [cout, k]) pack at their recorded bit-width (the six
    conditions of include/smpq.h): (mode int8 [cout], base int32 [cout], words int32 [cout] = each
    channel's payload word count), on w2d's device."""
    cout, k = _bp_weight(w2d, "bitpack_plan")
    dev = w2d.device
    _bp_meta(cout, dev, qbits=qbits, step=step)
    mode = torch.empty(cout, dtype=torch.int8, device=dev)
    base = torch.empty(4 * cout, dtype=torch.int8, device=dev).view(torch.int32)
    words = torch.empty(4 * cout, dtype=torch.int8, device=dev).view(torch.int32)
    _launch_twin(w2d, "smpq_bitpack_plan", w2d, cout, k, qbits, step, mode, base, words)
    return mode, base, words


def bitpack_offsets(words):
    """word_off int64 [cout + 1]: the exclusive prefix sum of the per-channel word counts (no host
    sync); word_off[-1] is the payload's length in words."""
    off = torch.zeros(words.numel() + 1, dtype=torch.int64, device=words.device)
    torch.cumsum(words, 0, dtype=torch.int64, out=off[1:])
    return off


def bitpack_store(w2d, mode, base, step, word_off, total_words=None):
    """The payload of ``w2d`` under a plan: int8 [4 * total_words] (the byte view of the 32-bit
    words). ``total_words`` = word_off[-1] when the caller already has it on the host (one host
    sync here otherwise)."""
    cout, k = _bp_weight(w2d, "bitpack_store")
    dev = w2d.device
    _bp_meta(cout, dev, mode=mode, base=base, step=step, word_off=word_off)
    total = int(word_off[-1].item()) if total_words is None else int(total_words)
    _req(cout <= total <= cout * k, "bitpack_store: total_words outside [cout, cout * k]")
    payload = torch.empty(4 * total, dtype=torch.int8, device=dev)
    _req(payload.data_ptr() % 4 == 0, "bitpack_store: payload not word aligned")
    _launch_twin(w2d, "smpq_bitpack_store", w2d, cout, k, mode, base, step, word_off, payload)
    return payload


def bitpack_load(payload, cout, k, mode, base, step, word_off, out=None):
    """Unpack a payload (int8 bytes of the 32-bit words) into fp32 [cout, k]: a new tensor on the
    payload's device, or ``out`` (a contiguous fp32 tensor of cout * k elements there, e.g. a conv
    weight, written in place). The caller vouches for mode / word_off (checkpoint.load_packed
    validates files); no host sync."""
    cout, k = int(cout), int(k)
    dev = payload.device
    _req(payload.dtype == torch.int8 and payload.dim() == 1 and payload.is_contiguous()
         and payload.numel() % 4 == 0 and payload.data_ptr() % 4 == 0,
         "bitpack_load: payload must be a contiguous, word-aligned int8 tensor of whole words")
    _req(cout > 0 and 0 < k <= BITPACK_MAX_K and 4 * cout <= payload.numel() <= 4 * cout * k,
         "bitpack_load: payload length does not fit [cout, k]")
    _bp_meta(cout, dev, mode=mode, base=base, step=step, word_off=word_off)
    if out is None:
        out = torch.empty(cout, k, dtype=torch.float32, device=dev)
    _req(out.dtype == torch.float32 and out.numel() == cout * k and out.is_contiguous() and out.device == dev,
         "bitpack_load: out must be a contiguous fp32 tensor of cout * k elements on the payload's device")
    _launch_twin(payload, "smpq_bitpack_load", payload, cout, k, mode, base, step, word_off, out)
    return out


# ---- uint8 images through a per-channel table (include/smpq.h) ----------------------------------
# After Resize / CenterCrop / ToTensor / Normalize a pixel is one of 256 fp32 values per channel:
# an fp32 batch that lies on that grid is kept as uint8 and decoded back bit for bit.
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
U8LUT_MAX_C = 4


def u8lut_table(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The fp32 [c, 256] table of ToTensor then Normalize on a uint8 pixel, computed by torch's own
    fp32 CPU operators in their order: u / 255, minus mean_c, divided by std_c, each rounded to
    fp32 (a fused restatement differs in most entries). Defaults: torchvision's ImageNet constants."""
    m = torch.as_tensor(mean, dtype=torch.float32).reshape(-1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).reshape(-1, 1)
    _req(m.numel() == s.numel() and 1 <= m.numel() <= U8LUT_MAX_C, "u8lut_table: need 1 to 4 means and as many stds")
    t = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    lut = t.repeat(m.numel(), 1).sub_(m).div_(s)
    _u8lut_check_table(lut)
    return lut


def _u8lut_check_table(lut):
    """Validate a table on the host (one copy of 1 - 4 KB for a device table), once per tensor and
    version: fp32 [c, 256], contiguous, every row finite and strictly increasing."""
    _req(torch.is_tensor(lut) and lut.dtype == torch.float32 and lut.dim() == 2 and lut.shape[1] == 256
         and 1 <= lut.shape[0] <= U8LUT_MAX_C and lut.is_contiguous(),
         "u8lut: the table must be a contiguous fp32 [c, 256] tensor with 1 <= c <= 4")
    if getattr(lut, "_smpq_u8lut_ok", None) == lut._version:  # set below, on the tensor itself
        return
    h = lut.detach().cpu()
    _req(bool(torch.isfinite(h).all()) and bool((h[:, 1:] > h[:, :-1]).all()),
         "u8lut: every table row must be finite and strictly increasing")
    lut._smpq_u8lut_ok = lut._version


def _u8lut_images(t, dtype, lut, what):
    """(n, c, hw) of a contiguous [n, c, ...] image tensor of ``dtype`` on the table's device."""
    _req(torch.is_tensor(t) and t.dtype == dtype and t.dim() >= 2 and t.is_contiguous() and t.numel() > 0,
         "%s: need a non-empty contiguous %s [n, c, ...] tensor" % (what, dtype))
    _req(t.device == lut.device, "%s: images and table on different devices" % what)
    _req(t.shape[1] == lut.shape[0], "%s: %d channels against a table of %d rows" % (what, t.shape[1], lut.shape[0]))
    _req(t.numel() < 2 ** 31, "%s: 2^31 elements or more" % what)
    n, c = int(t.shape[0]), int(t.shape[1])
    return n, c, t.numel() // (n * c)


def u8lut_encode(x, lut, out=None):
    """fp32 images [n, c, ...] -> (u, bad): u uint8 of x's shape with u = the largest v with
    lut[c][v] <= x (0 when there is none or x is NaN), and bad = a uint32 count (an int32 [1]
    tensor on x's device, so reading it is the caller's sync) of the elements whose bit pattern is
    not lut[c][u]'s. ``out``: a contiguous uint8 tensor of x's shape to write u into."""
    _u8lut_check_table(lut)
    n, c, hw = _u8lut_images(x, torch.float32, lut, "u8lut_encode")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _req(torch.is_tensor(out) and out.dtype == torch.uint8 and out.shape == x.shape and out.is_contiguous()
         and out.device == x.device, "u8lut_encode: out must be a contiguous uint8 tensor of x's shape on its device")
    bad = torch.zeros(1, dtype=torch.int32, device=x.device)
    _launch_twin(x, "smpq_u8lut_encode", x, n, c, hw, lut, out, bad)
    return out, bad


def u8lut_decode(u, lut, out=None):
    """uint8 images [n, c, ...] -> fp32 x of the same shape, x = lut[c][u]. ``out``: a contiguous
    fp32 tensor of u's shape to write into (e.g. a view of a staging buffer); nothing outside it
    is written. No host sync for a table already validated."""
    _u8lut_check_table(lut)
    n, c, hw = _u8lut_images(u, torch.uint8, lut, "u8lut_decode")
    if out is None:
        out = torch.empty(u.shape, dtype=torch.float32, device=u.device)
    _req(torch.is_tensor(out) and out.dtype == torch.float32 and out.shape == u.shape and out.is_contiguous()
         and out.device == u.device and out.data_ptr() % 4 == 0,
         "u8lut_decode: out must be a contiguous fp32 tensor of u's shape on its device")
    _launch_twin(u, "smpq_u8lut_decode", u, n, c, hw, lut, out)
    return out
