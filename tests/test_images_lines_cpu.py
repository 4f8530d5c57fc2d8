"""The lines of the splits of many images with one call (fourmc_gpu_images_read_lines, fourmc_gpu_images_align_slices) without a
GPU: declared, exported, reachable from Python, the structs laid out as the header says, and every argument error refused before
a device is looked for, with the items and slices left byte for byte as they came."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import helpers

ROOT = helpers.ROOT
READ, STATS, ALIGN = "fourmc_gpu_images_read_lines", "fourmc_gpu_images_lines_stats", "fourmc_gpu_images_align_slices"
OK, ENODEV, EINVAL = 0, -1, -3
BUF, DST, TABLE = 256, 4096, 256         # bytes of the (host) image buffer and destination, entries of the two (host) tables
MAX = 0x7FFFFFFF
IMAGES = [(0, 64), (64, 100), (164, 0), (164, 92)]         # (image_off, image_bytes): abutting, one empty, the last ends the buffer


def _fields_in_header(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s*[,;]", body)


def test_symbols_are_declared_exported_and_bound():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in (READ, STATS, ALIGN):
        assert re.search(r"\b%s\s*\(" % name, text)
        assert getattr(raw, name) is not None
        assert name in p.exported_symbols()
    assert C.sizeof(p.ImageRef) == 16 and C.sizeof(p.ImagesSplitItem) == 96 and C.sizeof(p.ImagesSlice) == 56
    assert [f[0] for f in p.ImageRef._fields_] == _fields_in_header(text, "fourmc_image_ref") == ["image_off", "image_bytes"]
    assert [f[0] for f in p.ImagesSplitItem._fields_] == _fields_in_header(text, "fourmc_images_split_item") == \
        ["image", "pad", "split_start", "split_end", "dst_off", "dst_cap", "table_off", "lines_cap", "out"]
    assert [f[0] for f in p.ImagesSlice._fields_] == _fields_in_header(text, "fourmc_images_slice") == ["image", "pad", "s"]
    assert p.ImagesSplitItem.split_start.offset == 8 and p.ImagesSplitItem.out.offset == 56 and p.ImagesSlice.s.offset == 8
    assert callable(p.images_read_lines) and callable(p.images_align_slices) and callable(p.images_lines_stats)
    # neither header comment lists the call as missing any more
    assert "Not reproduced: several images in one call" not in text
    assert "Not reproduced.** Several images in one call" not in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def _refs(p, images):
    arr = (p.ImageRef * max(len(images), 1))()
    for k, (o, b) in enumerate(images):
        arr[k].image_off, arr[k].image_bytes = o, b
    return arr


def _items(p, rows):
    """host items, every byte of `out` and of the padding set, and the bytes as they are now"""
    arr = (p.ImagesSplitItem * max(len(rows), 1))()
    C.memset(arr, 0xA7, C.sizeof(arr))
    for i, row in enumerate(rows):
        (arr[i].image, arr[i].split_start, arr[i].split_end, arr[i].dst_off, arr[i].dst_cap, arr[i].table_off, arr[i].lines_cap) = row
    return arr, bytes(arr)


def _slices(p, rows):
    arr = (p.ImagesSlice * max(len(rows), 1))()
    C.memset(arr, 0xA7, C.sizeof(arr))
    for i, (im, a, z) in enumerate(rows):
        arr[i].image, arr[i].s.start, arr[i].s.end = im, a, z
    return arr, bytes(arr)


class Buffers:
    def __init__(self):
        self.img = np.zeros(BUF, np.uint8)
        self.dst = np.full(DST, 0xC3, np.uint8)
        self.st = np.full(TABLE, 0x1111, np.uint64)
        self.tl = np.full(TABLE, 0x2222, np.uint32)

    def clean(self):
        return bool((self.dst == 0xC3).all() and (self.st == 0x1111).all() and (self.tl == 0x2222).all())


def _call(p, buf, rows, arr=None, image=True, dst=True, starts=True, tlen=True, max_len=MAX, n=None, dst_bytes=DST, entries=TABLE,
          images=IMAGES, refs=True, nimages=None, images_bytes=BUF):
    """-> (return code, the items, whether the items are byte for byte as they came)"""
    before = None
    if arr is None:
        arr, before = _items(p, rows)
    r = _refs(p, images)
    rc = p.lib().fourmc_gpu_images_read_lines(
        buf.img.ctypes.data if image else None, images_bytes, C.cast(r, C.c_void_p) if refs else None,
        len(images) if nimages is None else nimages, max_len, buf.dst.ctypes.data if dst else None, dst_bytes,
        buf.st.ctypes.data if starts else None, buf.tl.ctypes.data if tlen else None, entries,
        C.cast(arr, C.c_void_p) if arr is not False else None, len(rows) if n is None else n, None)
    return rc, arr, before is None or bytes(arr) == before


# (image, split_start, split_end, dst_off, dst_cap, table_off, lines_cap)
GOOD = [(0, 0, 64, 0, 100, 0, 10), (1, 0, 100, 100, 900, 10, 20), (3, 12, 92, 1000, 96, 30, 0), (2, 0, 0, 4096, 0, 256, 0), (1, 12, 50, 2000, 7, 40, 3)]
EINVAL_CASES = {
    # name: (rows, keyword arguments of _call)
    "null images buffer": (GOOD, dict(image=False)),
    "null destination": (GOOD, dict(dst=False)),
    "null destination, size queries only": ([(0, 0, 64, 0, 0, 0, 4)], dict(dst=False)),
    "starts without text_len": (GOOD, dict(tlen=False)),
    "text_len without starts": (GOOD, dict(starts=False)),
    "max_line_len 0x80000000": (GOOD, dict(max_len=0x80000000)),
    "max_line_len 0xFFFFFFFF, count only": (GOOD, dict(max_len=0xFFFFFFFF, starts=False, tlen=False)),
    "region starts beyond the destination": ([(0, 0, 64, DST + 1, 0, 0, 4)], {}),
    "region ends beyond the destination": ([(0, 0, 64, 0, 100, 0, 4), (1, 0, 64, DST - 99, 100, 4, 4)], {}),
    "dst_off + dst_cap wraps": ([(0, 0, 64, 16, 2 ** 64 - 8, 0, 4)], {}),
    "regions of two images overlap by one byte": ([(0, 0, 64, 100, 100, 0, 4), (1, 0, 64, 0, 101, 4, 4)], {}),
    "regions overlap by one byte, count only": ([(0, 0, 64, 100, 100, 0, 0), (3, 0, 64, 0, 101, 0, 0)], dict(starts=False, tlen=False)),
    "the same region twice": ([(0, 0, 64, 64, 64, 0, 4), (0, 0, 64, 64, 64, 4, 4)], {}),
    "table region starts beyond the tables": ([(0, 0, 64, 0, 100, TABLE + 1, 0)], {}),
    "table region ends beyond the tables": ([(0, 0, 64, 0, 100, 0, 4), (1, 0, 64, 100, 100, TABLE - 3, 4)], {}),
    "table_off + lines_cap wraps": ([(0, 0, 64, 0, 100, 8, 2 ** 64 - 4)], {}),
    "table regions of two images overlap by one entry": ([(0, 0, 64, 0, 100, 10, 10), (1, 0, 64, 100, 100, 0, 11)], {}),
    "the same table region twice": ([(0, 0, 64, 0, 100, 16, 8), (0, 0, 64, 100, 100, 16, 8)], {}),
    # only with several images
    "null images with nimages > 0": (GOOD, dict(refs=False)),
    "image == nimages": ([(0, 0, 64, 0, 100, 0, 10), (4, 0, 64, 100, 100, 10, 10)], {}),
    "image 0xFFFFFFFF": ([(0xFFFFFFFF, 0, 64, 0, 100, 0, 10)], {}),
    "an image, and no images": ([(0, 0, 64, 0, 100, 0, 10)], dict(images=[], refs=False)),
    "an image starts beyond the buffer": (GOOD, dict(images=IMAGES + [(BUF + 1, 0)])),
    "an image ends one byte beyond the buffer": (GOOD, dict(images=[(0, 64), (64, 100), (164, 0), (164, 93)])),
    "an image nobody names ends beyond the buffer": ([(0, 0, 64, 0, 100, 0, 10)], dict(images=[(0, 64), (200, 57)])),
    "image_off + image_bytes wraps": (GOOD, dict(images=[(0, 64), (64, 100), (164, 0), (16, 2 ** 64 - 8)])),
    "images in an empty buffer": (GOOD, dict(images_bytes=0)),
}


@pytest.mark.parametrize("name", list(EINVAL_CASES))
def test_argument_errors_are_einval_before_any_device(name):
    """no skip with a GPU present: these return before the device is looked at, so the host pointers are never used"""
    p = helpers.pkg()
    L = p.lib()
    rows, kw = EINVAL_CASES[name]
    buf = Buffers()
    rc, _, same = _call(p, buf, rows, **kw)
    assert rc == EINVAL, (name, rc)
    assert b"images_read_lines" in L.fourmc_gpu_last_error(), L.fourmc_gpu_last_error()
    assert same, "the items changed"
    assert buf.clean()


def test_null_items_is_einval_and_no_items_is_ok():
    p = helpers.pkg()
    L = p.lib()
    buf = Buffers()
    rc, _, _ = _call(p, buf, GOOD, arr=False, n=3)
    assert rc == EINVAL and b"images_read_lines" in L.fourmc_gpu_last_error()
    arr, before = _items(p, GOOD)
    for a in (False, arr):
        assert _call(p, buf, GOOD, arr=a, n=0)[0] == OK
        # nothing else is looked at
        assert _call(p, buf, GOOD, arr=a, n=0, image=False, dst=False, tlen=False, max_len=0xFFFFFFFF, refs=False, images_bytes=0)[0] == OK
    assert bytes(arr) == before and buf.clean()


@pytest.mark.skipif(torch.cuda.is_available(), reason="a well-formed call would run on the device with host pointers")
def test_what_the_checks_accept_ends_at_the_device_check():
    p = helpers.pkg()
    L = p.lib()
    buf = Buffers()
    rc, _, same = _call(p, buf, GOOD)
    assert rc == ENODEV and same and L.fourmc_gpu_last_error()
    # regions that touch, the same image twice in `images`, overlapping images, the same split twice, images nobody names
    twice = [(0, 64), (0, 64), (32, 100), (BUF, 0)]
    rows = [(0, 0, 64, 0, 100, 0, 10), (1, 0, 64, 100, 33, 10, 1), (2, 12, 64, 133, DST - 133, 11, TABLE - 11), (0, 0, 64, 50, 0, 5, 0)]
    rc, _, same = _call(p, buf, rows, images=twice)
    assert rc == ENODEV and same
    # table regions are looked at only when tables are given; max_line_len 0
    for rows in ([(0, 0, 64, 0, 100, 10, 10), (1, 0, 64, 100, 100, 0, 11)], [(0, 0, 64, 0, 100, TABLE + 1, 2 ** 64 - 1)]):
        rc, _, same = _call(p, buf, rows, starts=False, tlen=False, entries=0, max_len=0)
        assert rc == ENODEV and same, (rows, rc)
        assert _call(p, buf, rows)[0] == EINVAL
    assert buf.clean()


# ---- align ------------------------------------------------------------------------------------------------------------------
def _align(p, buf, rows, arr=None, image=True, images=IMAGES, refs=True, n=None, images_bytes=BUF):
    before = None
    if arr is None:
        arr, before = _slices(p, rows)
    r = _refs(p, images)
    rc = p.lib().fourmc_gpu_images_align_slices(buf.img.ctypes.data if image else None, images_bytes, C.cast(r, C.c_void_p) if refs else None,
                                                len(images), C.cast(arr, C.c_void_p) if arr is not False else None,
                                                len(rows) if n is None else n, None)
    return rc, before is None or bytes(arr) == before


SLICES = [(0, 0, 64), (1, 5, 50), (3, 0, 12), (2, 0, 0)]
ALIGN_EINVAL = {
    "null images buffer": (SLICES, dict(image=False)),
    "null images with nimages > 0": (SLICES, dict(refs=False)),
    "image == nimages": ([(0, 0, 64), (4, 0, 64)], {}),
    "an image ends one byte beyond the buffer": (SLICES, dict(images=[(0, 64), (64, 100), (164, 0), (164, 93)])),
    "image_off + image_bytes wraps": (SLICES, dict(images=[(0, 64), (64, 100), (164, 0), (16, 2 ** 64 - 8)])),
}


@pytest.mark.parametrize("name", list(ALIGN_EINVAL))
def test_align_argument_errors_are_einval_before_any_device(name):
    p = helpers.pkg()
    rows, kw = ALIGN_EINVAL[name]
    rc, same = _align(p, Buffers(), rows, **kw)
    assert rc == EINVAL, (name, rc)
    assert b"images_align_slices" in p.lib().fourmc_gpu_last_error()
    assert same, "the slices changed"


def test_align_null_slices_is_einval_and_no_slices_is_ok():
    p = helpers.pkg()
    buf = Buffers()
    assert _align(p, buf, SLICES, arr=False, n=2)[0] == EINVAL
    arr, before = _slices(p, SLICES)
    for a in (False, arr):
        assert _align(p, buf, SLICES, arr=a, n=0)[0] == OK
        assert _align(p, buf, SLICES, arr=a, n=0, image=False, refs=False, images_bytes=0)[0] == OK
    assert bytes(arr) == before


@pytest.mark.skipif(torch.cuda.is_available(), reason="a well-formed call would run on the device with host pointers")
def test_align_with_valid_arguments_ends_at_the_device_check():
    p = helpers.pkg()
    rc, same = _align(p, Buffers(), SLICES)
    assert rc == ENODEV and same


# ---- Python -----------------------------------------------------------------------------------------------------------------
def test_python_entry_points_validate_their_tensors():
    p = helpers.pkg()
    img, dst = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.images_read_lines(img, [(0, 64)], [(0, 0, 64, 0, 64, 0, 0)], dst)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.images_align_slices(img, [(0, 64)], [(0, 0, 64)])


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_the_python_entry_points_raise_the_engines_enodev(monkeypatch):
    p = helpers.pkg()
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    img, dst = torch.zeros(88, dtype=torch.uint8), torch.full((64,), 7, dtype=torch.uint8)
    images = [(0, 44), (44, 44)]
    rows = [(0, 0, 44, 0, 32, 0, 2), (1, 0, 44, 32, 32, 2, 2)]
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_read_lines failed \(-1\)"):
        p.images_read_lines(img, images, rows, dst)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_read_lines failed \(-3\)"):
        p.images_read_lines(img, images, [(2, 0, 44, 0, 32, 0, 0)], dst)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_read_lines failed \(-3\)"):
        p.images_read_lines(img, [(0, 44), (44, 45)], rows, dst)
    with pytest.raises(p.EngineError, match="go together"):
        p.images_read_lines(img, images, rows, dst, starts=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(p.EngineError, match="max_line_len"):
        p.images_read_lines(img, images, rows, dst, max_line_len=0x80000000)
    with pytest.raises(p.EngineError, match="splits"):
        p.images_read_lines(img, images, [(0, 44, 0, 32, 0, 0)], dst)
    with pytest.raises(p.EngineError, match="images"):
        p.images_read_lines(img, [(0, 44, 1)], rows, dst)
    assert p.images_read_lines(img, images, [], dst) == []
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_align_slices failed \(-1\)"):
        p.images_align_slices(img, images, [(0, 0, 44), (1, 3, 40)])
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_align_slices failed \(-3\)"):
        p.images_align_slices(img, images, [(2, 0, 44)])
    assert p.images_align_slices(img, images, []) == []
    assert bool((dst == 7).all())
    assert p.images_lines_stats() == (0, 0, 0, 0)
