"""The streaming image reader (fourmc_gpu_image_reader_*) without a GPU: declared, exported, reachable from Python, argument checks
before the device check, and refused loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import helpers

ROOT = helpers.ROOT
NAMES = ("fourmc_gpu_image_reader_begin", "fourmc_gpu_image_reader_append", "fourmc_gpu_image_reader_finish",
         "fourmc_gpu_image_reader_abort")
EINVAL, ENODEV = -3, -1


def test_symbols_are_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(raw, name) is not None, name
        assert name in p.exported_symbols(), name
    assert re.search(r"typedef struct fourmc_image_reader fourmc_image_reader;", text)


def test_python_entry_point_exists_and_refuses_host_tensors():
    p = helpers.pkg()
    assert callable(p.ImageReader)
    for name in ("append", "finish", "abort", "__enter__", "__exit__"):
        assert hasattr(p.ImageReader, name), name
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.ImageReader(torch.zeros(64, dtype=torch.uint8))


def test_a_reader_refuses_host_chunks():
    """append's tensor check comes before any call into the library: a reader built without begin shows it."""
    p = helpers.pkg()
    r = p.ImageReader.__new__(p.ImageReader)
    r._h, r._stream = 1, None                      # never reaches C: the chunk is refused first
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        r.append(torch.zeros(16, dtype=torch.uint8))
    r._h = None
    with pytest.raises(p.EngineError, match="finished or aborted"):
        r.append(torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="finished or aborted"):
        r.finish()
    with pytest.raises(p.EngineError, match="finished or aborted"):
        r.abort()


def test_null_handles_and_argument_checks():
    p = helpers.pkg()
    L = p.lib()
    dst = np.zeros(64, np.uint8)
    # bad magic, null destination: EINVAL, *r NULL, before any device check
    for args in ((dst.ctypes.data, 64, 0x12345678), (dst.ctypes.data, 64, 0), (None, 64, p.MAGIC_4MC), (None, 0, p.MAGIC_4MZ)):
        h = C.c_void_p(1234)
        assert L.fourmc_gpu_image_reader_begin(C.byref(h), *args, 0, None) == EINVAL, args
        assert h.value is None, args
    assert L.fourmc_gpu_image_reader_begin(None, dst.ctypes.data, 64, p.MAGIC_4MC, 0, None) == EINVAL
    # null readers
    st = p.ImageStatus()
    st.reason = 7
    assert L.fourmc_gpu_image_reader_append(None, dst.ctypes.data, 4) == EINVAL
    assert L.fourmc_gpu_image_reader_finish(None, C.byref(st)) == EINVAL
    assert st.reason == 7
    L.fourmc_gpu_image_reader_abort(None)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_begin_returns_enodev_and_leaves_the_reader_null():
    p = helpers.pkg()
    L = p.lib()
    dst = np.zeros(4096, np.uint8)
    for magic in (p.MAGIC_4MC, p.MAGIC_4MZ):
        for batch in (0, 1, 64):
            h = C.c_void_p(1234)
            assert L.fourmc_gpu_image_reader_begin(C.byref(h), dst.ctypes.data, dst.nbytes, magic, batch, None) == ENODEV
            assert h.value is None


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_the_python_reader_raises_the_engines_enodev(monkeypatch):
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
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_reader_begin failed \(-1\)"):
        p.ImageReader(torch.zeros(4096, dtype=torch.uint8), stream=object())
