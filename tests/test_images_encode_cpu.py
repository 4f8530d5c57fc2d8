"""Many images encoded with one call (fourmc_gpu_images_compress) without a GPU: declared, exported, reachable from Python, and
every argument error refused before a device is looked for, with the items and the image buffer left as they came."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import helpers

ROOT = helpers.ROOT
NAME = "fourmc_gpu_images_compress"
OK, ENODEV, EINVAL = 0, -1, -3
SRC, IMAGES = 1000, 4096                 # bytes of the two (host) buffers the items point into
B = helpers.B
CANARY = 0xC3


def bound(n):
    """fourmc_gpu_image_bound: header + 12 per block + the bytes + end mark + footer"""
    k = (n + B - 1) // B
    return 12 + 12 * k + n + 12 + 20 + 4 * k


def test_symbol_is_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert getattr(raw, NAME) is not None
    assert NAME in p.exported_symbols()
    assert C.sizeof(p.ImageEncItem) == 40
    assert [f[0] for f in p.ImageEncItem._fields_] == ["src_off", "src_bytes", "image_off", "image_cap", "image_bytes"]
    assert p.ImageEncItem.image_bytes.offset == 32
    assert callable(p.compress_images)
    assert bound(0) == 44 == p.lib().fourmc_gpu_image_bound(0) and bound(B + 1) == p.lib().fourmc_gpu_image_bound(B + 1)
    # the decode's header comment no longer lists the batched encode as missing
    assert "Not reproduced: a batched encode" not in text


def _items(p, rows):
    """host items with image_bytes preset, so that a call that touches one shows"""
    arr = (p.ImageEncItem * max(len(rows), 1))()
    for i, (so, sb, io, ic) in enumerate(rows):
        arr[i].src_off, arr[i].src_bytes, arr[i].image_off, arr[i].image_cap, arr[i].image_bytes = so, sb, io, ic, 7700 + i
    return arr


def _untouched(arr, rows):
    for i, row in enumerate(rows):
        assert (arr[i].src_off, arr[i].src_bytes, arr[i].image_off, arr[i].image_cap) == tuple(row), i
        assert arr[i].image_bytes == 7700 + i, i


GOOD = [(0, 100, 0, bound(100)), (100, 900, 200, 2000), (50, 200, 2200, bound(200)), (1000, 0, 4052, 44)]
HUGE = 0x3FFFFFFF * B + 1                # one block more than an item may have
EINVAL_CASES = {
    # name: (rows, magic is good, source pointer given, images pointer given, src_total)
    "magic": (GOOD, False, True, True, SRC),
    "null source": (GOOD, True, False, True, SRC),
    "null images": (GOOD, True, True, False, SRC),
    "null images, empty sources only": ([(0, 0, 0, 44)], True, True, False, SRC),
    "source starts beyond the buffer": ([(0, 10, 0, 100), (SRC + 1, 0, 100, 100)], True, True, True, SRC),
    "source ends beyond the buffer": ([(0, 10, 0, 100), (SRC - 9, 10, 100, 100)], True, True, True, SRC),
    "src_off + src_bytes wraps": ([(8, 2 ** 64 - 4, 0, IMAGES)], True, True, True, SRC),
    "region starts beyond the images": ([(0, 0, IMAGES + 1, 0)], True, True, True, SRC),
    "region ends beyond the images": ([(0, 10, 0, 100), (10, 10, IMAGES - 99, 100)], True, True, True, SRC),
    "image_off + image_cap wraps": ([(0, 10, 16, 2 ** 64 - 8)], True, True, True, SRC),
    "image_cap one below the bound": ([(0, 10, 0, 100), (10, 300, 100, bound(300) - 1)], True, True, True, SRC),
    "image_cap below the 44 bytes of an empty image": ([(0, 0, 0, 43)], True, True, True, SRC),
    "an item of more than 0x3FFFFFFF blocks": ([(0, HUGE, 0, IMAGES)], True, True, True, 2 ** 63),
    "regions overlap by one byte": ([(0, 10, 100, 100), (10, 10, 0, 101)], True, True, True, SRC),
    "one region inside another": ([(0, 10, 0, 1000), (10, 10, 3000, 100), (20, 10, 500, 60)], True, True, True, SRC),
    "the same region twice": ([(0, 10, 64, 64), (0, 10, 64, 64)], True, True, True, SRC),
    "the same region twice, empty sources": ([(0, 0, 64, 44), (0, 0, 64, 44)], True, True, True, SRC),
}


@pytest.mark.parametrize("name", list(EINVAL_CASES))
def test_argument_errors_are_einval_before_any_device(name):
    """no skip with a GPU present: these return before the device is looked at, so the host pointers are never used"""
    p = helpers.pkg()
    L = p.lib()
    rows, good_magic, have_src, have_images, src_total = EINVAL_CASES[name]
    src = np.zeros(SRC + 64, np.uint8)
    images = np.full(IMAGES, CANARY, np.uint8)
    arr = _items(p, rows)
    for level in (1, 3):
        rc = L.fourmc_gpu_images_compress(src.ctypes.data if have_src else None, src_total, images.ctypes.data if have_images else None,
                                          IMAGES, p.MAGIC_4MC if good_magic else 0x12345678, level, C.cast(arr, C.c_void_p), len(rows), None)
        assert rc == EINVAL, (name, rc)
        assert L.fourmc_gpu_last_error()
        _untouched(arr, rows)
        assert (images == CANARY).all()


def test_null_items_is_einval_no_items_is_ok_and_the_magic_comes_first():
    p = helpers.pkg()
    L = p.lib()
    src = np.zeros(SRC + 64, np.uint8)
    images = np.full(IMAGES, CANARY, np.uint8)
    assert L.fourmc_gpu_images_compress(src.ctypes.data, SRC, images.ctypes.data, IMAGES, p.MAGIC_4MC, 1, None, 3, None) == EINVAL
    for items in (None, C.cast(_items(p, GOOD), C.c_void_p)):
        for magic in (p.MAGIC_4MC, p.MAGIC_4MZ):
            assert L.fourmc_gpu_images_compress(src.ctypes.data, SRC, images.ctypes.data, IMAGES, magic, 1, items, 0, None) == OK
            assert L.fourmc_gpu_images_compress(None, 0, None, 0, magic, 1, items, 0, None) == OK       # nothing else is looked at
    assert L.fourmc_gpu_images_compress(None, 0, None, 0, 7, 1, None, 0, None) == EINVAL                # the magic is checked first
    assert b"magic" in L.fourmc_gpu_last_error()
    # ... before the items of a call that has every other error too
    arr = _items(p, [(SRC, 10, IMAGES, 1)])
    assert L.fourmc_gpu_images_compress(None, SRC, None, IMAGES, 7, 1, C.cast(arr, C.c_void_p), 1, None) == EINVAL
    assert b"magic" in L.fourmc_gpu_last_error()
    assert (images == CANARY).all()


@pytest.mark.skipif(torch.cuda.is_available(), reason="a well-formed call would run on the device with host pointers")
def test_regions_that_touch_and_sources_that_overlap_pass_the_checks():
    """accepted by the argument checks: what comes back is the device's answer (here: there is none)"""
    p = helpers.pkg()
    L = p.lib()
    src = np.zeros(SRC + 64, np.uint8)
    images = np.full(IMAGES, CANARY, np.uint8)
    rows = [(0, 100, 0, bound(100)), (0, 100, bound(100), bound(100)),            # the same source; regions touch at the bound
            (50, 100, 2 * bound(100), bound(100)), (SRC, 0, IMAGES - 44, 44),     # an overlapping source; an empty one at the very end
            (0, SRC, 3 * bound(100), bound(SRC))]
    assert 3 * bound(100) + bound(SRC) <= IMAGES - 44
    arr = _items(p, rows)
    for magic in (p.MAGIC_4MC, p.MAGIC_4MZ):
        rc = L.fourmc_gpu_images_compress(src.ctypes.data, SRC, images.ctypes.data, IMAGES, magic, 1, C.cast(arr, C.c_void_p), len(rows), None)
        assert rc == ENODEV, rc
        _untouched(arr, rows)
    assert (images == CANARY).all()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_a_well_formed_call_fails_with_enodev(monkeypatch):
    import importlib
    p = helpers.pkg()
    L = p.lib()
    src = np.zeros(SRC + 64, np.uint8)
    images = np.full(IMAGES, CANARY, np.uint8)
    for magic, level in ((p.MAGIC_4MC, 1), (p.MAGIC_4MZ, 4)):
        arr = _items(p, GOOD)
        rc = L.fourmc_gpu_images_compress(src.ctypes.data, SRC, images.ctypes.data, IMAGES, magic, level, C.cast(arr, C.c_void_p), len(GOOD), None)
        assert rc == ENODEV, rc
        assert L.fourmc_gpu_last_error()
        _untouched(arr, GOOD)
    # a NULL source is fine as long as every source is empty
    rows = [(0, 0, 0, 44), (0, 0, 44, 44)]
    arr = _items(p, rows)
    assert L.fourmc_gpu_images_compress(None, 0, images.ctypes.data, IMAGES, p.MAGIC_4MC, 1, C.cast(arr, C.c_void_p), 2, None) == ENODEV
    _untouched(arr, rows)
    assert (images == CANARY).all()
    # the Python entry point: host tensors are refused before any call; with the check bypassed the library's ENODEV surfaces
    host_src, host_img = torch.zeros(SRC, dtype=torch.uint8), torch.zeros(IMAGES, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_images(host_src, [(0, 10, 0, 100)], host_img)
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_compress failed \(-1\)"):
        p.compress_images(host_src, GOOD, host_img)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_compress failed \(-3\)"):
        p.compress_images(host_src, [(0, 10, 0, 100), (10, 10, 99, 100)], host_img)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_compress failed \(-3\)"):
        p.compress_images(host_src, GOOD, host_img, src_bytes=SRC - 1)              # GOOD's last source starts at SRC
    with pytest.raises(p.EngineError, match="src_bytes beyond the tensor"):
        p.compress_images(host_src, GOOD, host_img, src_bytes=SRC + 1)
    with pytest.raises(p.EngineError, match="images_bytes beyond the tensor"):
        p.compress_images(host_src, GOOD, host_img, images_bytes=IMAGES + 1)
    assert p.compress_images(host_src, [], host_img) == []
    assert not host_img.any()
