"""The whole-image device API (fourmc_gpu_image_*) without a GPU: declared, exported, reachable from Python, and refused loudly."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import helpers

ROOT = helpers.ROOT
NAMES = ("fourmc_gpu_image_bound", "fourmc_gpu_image_compress", "fourmc_gpu_image_decompress", "fourmc_gpu_image_reason_text",
         "fourmc_gpu_image_parse_stats")


def test_symbols_are_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(raw, name) is not None, name
        assert name in p.exported_symbols(), name
    assert C.sizeof(p.ImageStatus) == 40


def test_python_entry_points_exist():
    p = helpers.pkg()
    for name in ("compress_image", "decompress_image", "image_bound", "image_parse_stats"):
        assert callable(getattr(p, name)), name


def test_bound_and_reason_texts():
    p = helpers.pkg()
    L = p.lib()
    B = p.BLOCKSIZE
    assert p.image_bound(0) == 44                                 # header + end mark + empty footer: the CLI's image of an empty file
    assert p.image_bound(1) == 12 + 12 + 1 + 12 + 24
    assert p.image_bound(2 * B + 1) == 12 + 3 * 12 + 2 * B + 1 + 12 + 20 + 12
    # the messages fourmc_file.c prints, one per verdict
    src = open(os.path.join(ROOT, "4mc_amd", "csrc", "fourmc_file.c")).read()
    assert L.fourmc_gpu_image_reason_text(0) == b""
    for r in range(1, 16):
        t = L.fourmc_gpu_image_reason_text(r).decode()
        assert t and '"%s' % t in src, (r, t)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_both_calls_fail_with_enodev():
    p = helpers.pkg()
    L = p.lib()
    out = C.c_uint64(12345)
    src = np.zeros(64, np.uint8)
    img = np.zeros(4096, np.uint8)
    rc = L.fourmc_gpu_image_compress(src.ctypes.data, 64, img.ctypes.data, 4096, C.byref(out), p.MAGIC_4MC, 1, None)
    assert rc == -1 and out.value == 12345, rc                   # FOURMC_ENODEV, nothing reported as a result
    st = p.ImageStatus()
    st.exit_code = 77
    rc = L.fourmc_gpu_image_decompress(img.ctypes.data, 44, img.ctypes.data, 4096, p.MAGIC_4MC, C.byref(st), None)
    assert rc == -1 and st.exit_code == 77, rc
    assert L.fourmc_gpu_last_error()
    # the Python entry points refuse a tensor that is not in device memory before any call
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_image(torch.zeros(16, dtype=torch.uint8), torch.zeros(4096, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.decompress_image(torch.zeros(44, dtype=torch.uint8), None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_the_python_entry_points_raise_the_engines_enodev(monkeypatch):
    """No CUDA tensor can exist here, so the tensor check is bypassed with host pointers: what has to surface is the library's
    FOURMC_ENODEV (-1) as an EngineError, not a status."""
    p = helpers.pkg()
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_compress failed \(-1\)"):
        p.compress_image(torch.zeros(16, dtype=torch.uint8), torch.zeros(4096, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_decompress failed \(-1\)"):
        p.decompress_image(torch.zeros(44, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_decompress failed \(-1\)"):
        p.decompress_image(torch.zeros(44, dtype=torch.uint8), None)
    assert p.image_parse_stats() == (0, 0)                   # nothing was parsed
