"""libsmpq on the host: ABI exports, the native host quantizer vs the reference's KAT vectors,
and the drop-in functions API on CPU tensors (no GPU needed)."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, REPO
from test_oracle_golden import device_kat_cases, kat_cases


def header_symbols():
    src = open(REPO + "/include/smpq.h").read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[\w\*\s]+?\b(smpq_\w+)\s*\(", src, re.M)))


def test_library_exports_every_header_symbol(built_lib):
    syms = header_symbols()
    assert len(syms) >= 9
    from smpq import _lib
    for s in syms:
        assert hasattr(built_lib, s), s
        assert s in _lib.EXPORTED_SYMBOLS, s
    assert built_lib.smpq_abi_version() == 7


def test_loaded_library_matches_the_sources(built_lib):
    """Content-addressed build: the loaded libsmpq.so carries the SHA-256 of exactly the sources,
    headers and flags in this tree (a stale binary cannot pass as current)."""
    import __graft_entry__ as ge
    stamp = ge.source_stamp()
    assert re.fullmatch(r"[0-9a-f]{64}", stamp)
    assert built_lib.smpq_build_stamp().decode() == stamp
    assert ge.library_stamp() == stamp


def test_source_stamp_tracks_content(tmp_path, monkeypatch):
    """The stamp changes with any byte of a source or with the flags, and not with mtimes."""
    import shutil
    import __graft_entry__ as ge
    base = ge.source_stamp()
    csrc = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, csrc)
    (tmp_path / "include").mkdir()
    shutil.copy(ge.PUBLIC_HEADER, tmp_path / "include" / "smpq.h")
    monkeypatch.setattr(ge, "CSRC", str(csrc))
    monkeypatch.setattr(ge, "PUBLIC_HEADER", str(tmp_path / "include" / "smpq.h"))
    monkeypatch.setattr(ge, "REPO", str(tmp_path))
    same = ge.source_stamp()
    os.utime(csrc / "eval.hip", (0, 0))
    assert ge.source_stamp() == same
    with open(csrc / "eval.hip", "a") as f:
        f.write("\n")
    assert ge.source_stamp() != same
    monkeypatch.setattr(ge, "FLAGS", ge.FLAGS + ["-DX"])
    assert ge.source_stamp() != same
    assert base  # (the tree's own stamp is unaffected: the copy lives in tmp_path)


def test_host_quantizer_bitexact_vs_reference(built_lib):
    from smpq import ops
    for kind, chain, x, y in kat_cases():
        w = torch.from_numpy(x.copy()).reshape(1, -1)
        for b in chain:
            ops.quantize_channels_(w, [b])
        assert np.array_equal(w.numpy().ravel().view(np.uint32), y.view(np.uint32)), (kind, chain)


def test_host_quantizer_device_semantics_vs_torch_gpu(built_lib):
    # the host twin with SMPQ_QSEM_DEVICE reproduces what torch computes on the GPU
    from smpq import ops
    for kind, chain, x, y in device_kat_cases():
        w = torch.from_numpy(x.copy()).reshape(1, -1)
        for b in chain:
            ops.quantize_channels_(w, [b], semantics="device")
        assert np.array_equal(w.numpy().ravel().view(np.uint32), y.view(np.uint32)), (kind, chain)


def test_quant_semantics_setting(built_lib):
    from smpq import ops
    assert ops._qsem(None, False) == 0 and ops._qsem(None, True) == 1  # auto follows the device
    try:
        ops.set_quant_semantics("cpu")
        assert ops._qsem(None, True) == 0
        ops.set_quant_semantics("device")
        assert ops._qsem(None, False) == 1
    finally:
        ops.set_quant_semantics("auto")
    with pytest.raises(ValueError):
        ops.set_quant_semantics("fast")


def test_host_quantizer_constant_channel(built_lib):
    from smpq import ops
    w = torch.full((1, 9), 0.25)
    with pytest.raises(ZeroDivisionError):
        ops.quantize_channels_(w, [8])


def test_dropin_functions_record_metadata(built_lib):
    import functions
    import resnet
    torch.manual_seed(0)
    net = resnet.resnet18()
    conv = net.layer1[0].conv1
    before = conv.weight.data[3].clone()
    ret = functions.channel_wise_quantizationperchan(conv.weight.data, 6, 3)
    assert ret.data_ptr() == conv.weight.data_ptr()
    from oracle import quant_ref
    exp = quant_ref.quantize_wgt(before.numpy(), 6)
    assert np.array_equal(conv.weight.data[3].numpy().view(np.uint32), exp.view(np.uint32))
    assert int(conv.qbits[3]) == 6 and float(conv.qstep[3]) > 0 and conv._bits_host[3] == 6
    assert int(conv.qbits[2]) == 0
    # quantize_wgt returns a new tensor and records nothing
    t = conv.weight.data[5].clone()
    q = functions.quantize_wgt(t, 4)
    assert q.data_ptr() != t.data_ptr() and int(conv.qbits[5]) == 0
    # metadata survives state_dict round trip (resnet50_main.py:212,233-234)
    sd = net.state_dict()
    net2 = resnet.resnet18()
    net2.load_state_dict(sd)
    assert int(net2.layer1[0].conv1.qbits[3]) == 6 and net2.layer1[0].conv1._bits_host[3] == 6


def test_dropin_semilayer_split_and_order():
    import functions
    params = [[0, 0, 1, c, 8, 0, 32, c + 1] for c in range(4)] + [[0, 0, 2, c, 8, 0, 32, 5 + c] for c in range(3)]
    d = [[0, 0, 0, 0, v] for v in (-1, 2, 0, 3, 5, -2, -1)]
    minus, plus = functions.make_divide_minusplusmodels(params, d, 4)
    assert [r[3] for r in minus] == [0, 2, 1, 2] and [r[5] for r in minus] == [0, 0, -1, -1]
    assert [r[3] for r in plus] == [1, 3, 0] and [r[5] for r in plus] == [1, 1, 2]
    sem = [[params[0]], [params[1], params[3]], [params[4]]]
    flat = functions.make_quantizedlists(sem, [[0, 0.5], [1, 0.1], [2, 0.3]])
    assert [r[3] for r in flat[:-1]] == [1, 3, 0, 0] and flat[-1][2] == 100


def test_dropin_kldiv_has_no_cpu_fallback():
    # functions.KLdiv runs on the HIP kernel (smpq_kl_rows) only: CPU tensors are refused loudly
    import functions
    p = [torch.softmax(torch.randn(5, 10), 1)]
    with pytest.raises(ValueError):
        functions.KLdiv(p, p)


def test_dropin_grouping_matches_reference_golden():
    """functions.make_divide_minusplusmodels / make_quantizedlists vs the reference's own outputs
    (tests/golden/grouping_golden.npz, make_golden.py grouping), including the postponing phase's
    subset-vs-full-Δloss index misalignment (resnet50_main.py:417) kept bug-compatible."""
    import functions
    z = np.load(os.path.join(GOLDEN, "grouping_golden.npz"), allow_pickle=False)
    params = z["params"].tolist()
    d = z["d"].tolist()
    sub = [r for r in params if r[6] == 32]
    for name, rows in (("full", params), ("subset", sub)):
        for index in (4, 5, 6, 7):
            mi, pl = functions.make_divide_minusplusmodels([list(r) for r in rows], d, index)
            np.testing.assert_array_equal(np.array(mi, dtype=np.int64).reshape(-1, 8), z["%s_%d_minus" % (name, index)])
            np.testing.assert_array_equal(np.array(pl, dtype=np.int64).reshape(-1, 8), z["%s_%d_plus" % (name, index)])
    nl = int(z["params"][:, 2].max())
    sem = [[list(r) for r in params if r[2] == ln] for ln in range(1, nl + 1)]
    orders = [[int(o[0]), float(o[1])] for o in z["orders"]]
    got = functions.make_quantizedlists(sem, orders)
    np.testing.assert_array_equal(np.array(got, dtype=np.int64), z["quantizedlist"])


def test_imagenet_synthetic_is_opt_in(monkeypatch):
    # a missing dataset raises like the reference (imagenet.py:11-40); synthetic only on SMPQ_SYNTHETIC=1
    import importlib
    import sys
    sys.modules.pop("imagenet", None)
    monkeypatch.delenv("SMPQ_SYNTHETIC", raising=False)
    monkeypatch.setenv("SMPQ_IMAGENET_ROOT", "/nonexistent-imagenet")
    with pytest.raises(Exception):
        importlib.import_module("imagenet")
    sys.modules.pop("imagenet", None)
    monkeypatch.setenv("SMPQ_SYNTHETIC", "1")
    monkeypatch.setenv("SMPQ_SYNTH_IMAGES", "6")
    mod = importlib.import_module("imagenet")
    batches = list(mod.val_loader)
    assert [b[0].shape[0] for b in batches] == [6] and batches[0][0].shape[1:] == (3, 224, 224)
    sys.modules.pop("imagenet", None)


def test_host_fingerprint_formula(built_lib):
    # smpq_fingerprint_host = sum_i H(w_i, i) mod 2^64 (the device kernel's formula, include/smpq.h)
    # (the plain-integer formula lives in tests/tail_ref.py, next to the vectorised reference)
    from smpq.fingerprint import host_fingerprint
    from tail_ref import fingerprint_scalar

    t = torch.randn(1000, generator=torch.Generator().manual_seed(3))
    exp = fingerprint_scalar(t.numpy().view(np.uint32).tolist())
    assert host_fingerprint(t) == exp
    t2 = t.clone()
    t2[999] = torch.nextafter(t2[999], torch.tensor(1e9))
    assert host_fingerprint(t2) != exp
    # structured change the old odd-multiplier sum missed: a BN variance of ones scaled by 4
    ones = torch.ones(128)
    assert host_fingerprint(ones) != host_fingerprint(ones * 4.0)
