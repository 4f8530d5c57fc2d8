"""Many images with one call (fourmc_gpu_images_decompress) without a GPU: declared, exported, reachable from Python, and every
argument error refused before a device is looked for, with the items left as they came."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import helpers

ROOT = helpers.ROOT
NAME = "fourmc_gpu_images_decompress"
OK, ENODEV, EINVAL = 0, -1, -3
IMAGES, DST = 1000, 4096                 # bytes of the two (host) buffers the items point into


def test_symbol_is_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert getattr(raw, NAME) is not None
    assert NAME in p.exported_symbols()
    assert C.sizeof(p.ImageItem) == 72
    assert p.ImageItem.status.offset == 32 and p.ImageItem.status.size == C.sizeof(p.ImageStatus)
    assert callable(p.decompress_images)


def _items(p, rows):
    """host items with every status field preset, so that a call that touches one shows"""
    arr = (p.ImageItem * max(len(rows), 1))()
    for i, (io, ib, do, dc) in enumerate(rows):
        arr[i].image_off, arr[i].image_bytes, arr[i].dst_off, arr[i].dst_cap = io, ib, do, dc
        st = arr[i].status
        st.decoded_bytes, st.total_bytes, st.fail_offset = 11 + i, 22 + i, 33 + i
        st.streams, st.blocks, st.exit_code, st.reason = 44, 55, 77, 66
    return arr


def _untouched(arr, rows):
    for i, row in enumerate(rows):
        st = arr[i].status
        assert (arr[i].image_off, arr[i].image_bytes, arr[i].dst_off, arr[i].dst_cap) == tuple(row), i
        assert (st.decoded_bytes, st.total_bytes, st.fail_offset, st.streams, st.blocks, st.exit_code, st.reason) == \
            (11 + i, 22 + i, 33 + i, 44, 55, 77, 66), i


GOOD = [(0, 44, 0, 100), (44, 500, 100, 1000), (44, 500, 2000, 0), (1000, 0, 1100, 2996)]
EINVAL_CASES = {
    # name: (rows, magic is good, images pointer given, destination pointer given)
    "magic": (GOOD, False, True, True),
    "magic, size query": (GOOD, False, True, False),
    "null images": (GOOD, True, False, True),
    "null images, size query": ([(0, 0, 0, 0), (0, 1, 0, 0)], True, False, False),
    "image starts beyond the buffer": ([(0, 44, 0, 10), (IMAGES + 1, 0, 10, 10)], True, True, True),
    "image ends beyond the buffer": ([(0, 44, 0, 10), (IMAGES - 43, 44, 10, 10)], True, True, True),
    "image ends beyond the buffer, size query": ([(IMAGES - 43, 44, 0, 0)], True, True, False),
    "image_off + image_bytes wraps": ([(8, 2 ** 64 - 4, 0, 10)], True, True, True),
    "region starts beyond the destination": ([(0, 44, DST + 1, 0)], True, True, True),
    "region ends beyond the destination": ([(0, 44, 0, 10), (44, 44, DST - 9, 10)], True, True, True),
    "dst_off + dst_cap wraps": ([(0, 44, 16, 2 ** 64 - 8)], True, True, True),
    "regions overlap by one byte": ([(0, 44, 100, 50), (44, 44, 0, 101)], True, True, True),
    "one region inside another": ([(0, 44, 0, 1000), (44, 44, 3000, 10), (88, 44, 500, 1)], True, True, True),
    "the same region twice": ([(0, 44, 64, 64), (0, 44, 64, 64)], True, True, True),
}


@pytest.mark.parametrize("name", list(EINVAL_CASES))
def test_argument_errors_are_einval_before_any_device(name):
    """no skip with a GPU present: these return before the device is looked at, so the host pointers are never used"""
    p = helpers.pkg()
    L = p.lib()
    rows, good_magic, have_images, have_dst = EINVAL_CASES[name]
    images = np.zeros(IMAGES + 64, np.uint8)
    dst = np.zeros(DST, np.uint8)
    arr = _items(p, rows)
    rc = L.fourmc_gpu_images_decompress(images.ctypes.data if have_images else None, IMAGES, dst.ctypes.data if have_dst else None, DST,
                                        p.MAGIC_4MC if good_magic else 0x12345678, C.cast(arr, C.c_void_p), len(rows), None)
    assert rc == EINVAL, (name, rc)
    assert L.fourmc_gpu_last_error()
    _untouched(arr, rows)
    assert not dst.any()


def test_null_items_is_einval_and_no_items_is_ok():
    p = helpers.pkg()
    L = p.lib()
    images = np.zeros(IMAGES + 64, np.uint8)
    dst = np.zeros(DST, np.uint8)
    assert L.fourmc_gpu_images_decompress(images.ctypes.data, IMAGES, dst.ctypes.data, DST, p.MAGIC_4MC, None, 3, None) == EINVAL
    for items in (None, C.cast(_items(p, GOOD), C.c_void_p)):
        for magic in (p.MAGIC_4MC, p.MAGIC_4MZ):
            assert L.fourmc_gpu_images_decompress(images.ctypes.data, IMAGES, dst.ctypes.data, DST, magic, items, 0, None) == OK
            assert L.fourmc_gpu_images_decompress(None, 0, None, 0, magic, items, 0, None) == OK
    assert L.fourmc_gpu_images_decompress(None, 0, None, 0, 7, None, 0, None) == EINVAL        # the magic is checked first


@pytest.mark.skipif(torch.cuda.is_available(), reason="a well-formed call would run on the device with host pointers")
def test_regions_that_touch_or_are_empty_do_not_overlap():
    """accepted by the argument checks: what comes back is the device's answer (here: there is none)"""
    p = helpers.pkg()
    L = p.lib()
    images = np.zeros(IMAGES + 64, np.uint8)
    dst = np.zeros(DST, np.uint8)
    rows = [(0, 44, 0, 100), (0, 44, 100, 100), (44, 44, 50, 0), (44, 44, 150, 0), (88, 0, DST, 0), (IMAGES, 0, 200, DST - 200)]
    arr = _items(p, rows)
    rc = L.fourmc_gpu_images_decompress(images.ctypes.data, IMAGES, dst.ctypes.data, DST, p.MAGIC_4MC, C.cast(arr, C.c_void_p), len(rows), None)
    assert rc == ENODEV, rc
    _untouched(arr, rows)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_a_well_formed_call_fails_with_enodev(monkeypatch):
    import importlib
    p = helpers.pkg()
    L = p.lib()
    images = np.zeros(IMAGES + 64, np.uint8)
    dst = np.zeros(DST, np.uint8)
    for have_dst in (True, False):
        arr = _items(p, GOOD)
        rc = L.fourmc_gpu_images_decompress(images.ctypes.data, IMAGES, dst.ctypes.data if have_dst else None, DST, p.MAGIC_4MZ,
                                            C.cast(arr, C.c_void_p), len(GOOD), None)
        assert rc == ENODEV, rc
        assert L.fourmc_gpu_last_error()
        _untouched(arr, GOOD)
    # the overlapping regions of a size query are nobody's business: it gets as far as the device
    rows = [(0, 44, 0, 100), (0, 44, 0, 100)]
    arr = _items(p, rows)
    assert L.fourmc_gpu_images_decompress(images.ctypes.data, IMAGES, None, 0, p.MAGIC_4MC, C.cast(arr, C.c_void_p), 2, None) == ENODEV
    _untouched(arr, rows)
    # the Python entry point: host tensors are refused before any call; with the check bypassed the library's ENODEV surfaces
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.decompress_images(torch.zeros(64, dtype=torch.uint8), [(0, 44, 0, 10)], None)
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    for d_dst in (torch.zeros(DST, dtype=torch.uint8), None):
        with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_decompress failed \(-1\)"):
            p.decompress_images(torch.zeros(IMAGES, dtype=torch.uint8), GOOD, d_dst)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_decompress failed \(-3\)"):
        p.decompress_images(torch.zeros(IMAGES, dtype=torch.uint8), [(0, 44, 0, 10), (44, 44, 5, 10)], torch.zeros(DST, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="beyond the tensor"):
        p.decompress_images(torch.zeros(IMAGES, dtype=torch.uint8), GOOD, None, images_bytes=IMAGES + 1)
    assert p.image_parse_stats() == (0, 0)
