"""The streaming image writer (fourmc_gpu_image_writer_*) without a GPU: declared, exported, reachable from Python, argument checks
before the device check, and refused loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import helpers

ROOT = helpers.ROOT
NAMES = ("fourmc_gpu_image_writer_begin", "fourmc_gpu_image_writer_append", "fourmc_gpu_image_writer_finish",
         "fourmc_gpu_image_writer_abort")
EINVAL, ENODEV = -3, -1


def test_symbols_are_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(raw, name) is not None, name
        assert name in p.exported_symbols(), name
    assert re.search(r"typedef struct fourmc_image_writer fourmc_image_writer;", text)


def test_python_entry_point_exists_and_refuses_host_tensors():
    p = helpers.pkg()
    assert callable(p.ImageWriter)
    for name in ("append", "finish", "abort", "__enter__", "__exit__"):
        assert hasattr(p.ImageWriter, name), name
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.ImageWriter(torch.zeros(64, dtype=torch.uint8))


def test_a_writer_refuses_host_chunks():
    """append's tensor check comes before any call into the library: a writer built without begin shows it."""
    p = helpers.pkg()
    w = p.ImageWriter.__new__(p.ImageWriter)
    w._h, w._stream = 1, None                      # never reaches C: the chunk is refused first
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        w.append(torch.zeros(16, dtype=torch.uint8))
    w._h = None
    with pytest.raises(p.EngineError, match="finished or aborted"):
        w.append(torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="finished or aborted"):
        w.finish()


def test_null_handles_and_argument_checks():
    p = helpers.pkg()
    L = p.lib()
    img = np.zeros(64, np.uint8)
    h = C.c_void_p(1234)
    # bad magic, null image, capacity below the empty image's 44 bytes: EINVAL, *w NULL, before any device check
    assert L.fourmc_gpu_image_writer_begin(C.byref(h), img.ctypes.data, 64, 0x12345678, 1, 0, None) == EINVAL
    assert h.value is None
    h = C.c_void_p(1234)
    assert L.fourmc_gpu_image_writer_begin(C.byref(h), None, 64, p.MAGIC_4MC, 1, 0, None) == EINVAL
    assert h.value is None
    h = C.c_void_p(1234)
    assert L.fourmc_gpu_image_writer_begin(C.byref(h), img.ctypes.data, 43, p.MAGIC_4MZ, 1, 0, None) == EINVAL
    assert h.value is None and b"capacity" in L.fourmc_gpu_last_error()
    assert L.fourmc_gpu_image_writer_begin(None, img.ctypes.data, 64, p.MAGIC_4MC, 1, 0, None) == EINVAL
    # null writers
    n = C.c_uint64(7)
    assert L.fourmc_gpu_image_writer_append(None, img.ctypes.data, 4) == EINVAL
    assert L.fourmc_gpu_image_writer_finish(None, C.byref(n)) == EINVAL
    assert n.value == 7
    L.fourmc_gpu_image_writer_abort(None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_begin_returns_enodev_and_leaves_the_writer_null():
    p = helpers.pkg()
    L = p.lib()
    img = np.zeros(4096, np.uint8)
    for magic in (p.MAGIC_4MC, p.MAGIC_4MZ):
        h = C.c_void_p(1234)
        assert L.fourmc_gpu_image_writer_begin(C.byref(h), img.ctypes.data, img.nbytes, magic, 1, 0, None) == ENODEV
        assert h.value is None


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_the_python_writer_raises_the_engines_enodev(monkeypatch):
    import importlib
    p = helpers.pkg()
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_writer_begin failed \(-1\)"):
        p.ImageWriter(torch.zeros(4096, dtype=torch.uint8), stream=object())
