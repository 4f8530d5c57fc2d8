"""Random access into device images (fourmc_gpu_image_index / _decode_blocks / _read) without a GPU: declared, exported,
reachable from Python, argument checks before the device check, and refused loudly."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import helpers

ROOT = helpers.ROOT
NAMES = ("fourmc_gpu_image_index", "fourmc_gpu_image_decode_blocks", "fourmc_gpu_image_read")


def test_symbols_are_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(raw, name) is not None, name
        assert name in p.exported_symbols(), name
    for struct in ("fourmc_image_entry", "fourmc_image_index_info", "fourmc_image_range"):
        assert re.search(r"typedef struct %s\b" % struct, text), struct


def test_structures_are_32_bytes():
    p = helpers.pkg()
    assert C.sizeof(p.ImageEntry) == 32 and C.sizeof(p.ImageRange) == 32 and C.sizeof(p.ImageIndexInfo) == 32
    assert p.IMAGE_ENTRY_DTYPE.itemsize == 32
    assert [f for f, _ in p.ImageEntry._fields_] == list(p.IMAGE_ENTRY_DTYPE.names)


def test_python_entry_points_exist_and_refuse_host_tensors():
    p = helpers.pkg()
    img = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.image_index(img)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.image_decode_blocks(img, 0, 1, torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.image_read(img, [(0, 1, 0)], torch.zeros(64, dtype=torch.uint8))


def test_overlapping_destinations_are_refused_before_the_device_check():
    p = helpers.pkg()
    L = p.lib()
    img = np.zeros(64, np.uint8)
    dst = np.zeros(64, np.uint8)

    def call(triples):
        arr = (p.ImageRange * len(triples))()
        for i, (o, ln, d) in enumerate(triples):
            arr[i].offset, arr[i].length, arr[i].dst_off, arr[i].result = o, ln, d, 77
        rc = L.fourmc_gpu_image_read(img.ctypes.data, 64, C.cast(arr, C.c_void_p), len(triples), dst.ctypes.data, 64, None)
        return rc, [arr[i].result for i in range(len(triples))]
    for bad in ([(0, 10, 0), (20, 10, 5)], [(0, 1, 63), (0, 64, 0)], [(0, 8, 8), (0, 1, 0), (0, 4, 14)]):
        rc, res = call(bad)
        assert rc == -3, (bad, rc)                                  # FOURMC_EINVAL, nothing reported
        assert res == [77] * len(bad)
        assert b"overlap" in L.fourmc_gpu_last_error()
    # touching destinations and empty ranges are no overlap: these reach the device check
    if not torch.cuda.is_available():
        rc, res = call([(0, 10, 0), (5, 10, 10), (3, 0, 5)])
        assert rc == -1, rc
    # null pointers
    res = C.c_int64(5)
    assert L.fourmc_gpu_image_decode_blocks(img.ctypes.data, 64, 0, 1, dst.ctypes.data, 64, None, None) == -3
    assert L.fourmc_gpu_image_decode_blocks(None, 64, 0, 1, dst.ctypes.data, 64, C.byref(res), None) == -3
    assert L.fourmc_gpu_image_index(img.ctypes.data, 64, None, 0, None, None) == -3
    assert L.fourmc_gpu_image_read(img.ctypes.data, 64, None, 3, dst.ctypes.data, 64, None) == -3
    assert res.value == 5


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_the_python_entry_points_raise_the_engines_enodev(monkeypatch):
    """No CUDA tensor can exist here, so the tensor check is bypassed with host pointers: what has to surface is the library's
    FOURMC_ENODEV (-1) as an EngineError, not a result."""
    p = helpers.pkg()
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    img, dst = torch.zeros(44, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_index failed \(-1\)"):
        p.image_index(img)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_decode_blocks failed \(-1\)"):
        p.image_decode_blocks(img, 0, 1, dst)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_read failed \(-1\)"):
        p.image_read(img, [(0, 4, 0), (4, 4, 8)], dst)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_read failed \(-3\)"):      # overlap: refused before the device
        p.image_read(img, [(0, 4, 0), (4, 4, 2)], dst)
