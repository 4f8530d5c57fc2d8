"""The lines of many splits with one call (fourmc_gpu_image_read_lines_batch) without a GPU: declared, exported, reachable from
Python, and every argument error refused before a device is looked for, with the items left as they came."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import helpers

ROOT = helpers.ROOT
NAME, STATS = "fourmc_gpu_image_read_lines_batch", "fourmc_gpu_image_lines_batch_stats"
OK, ENODEV, EINVAL = 0, -1, -3
IMG, DST, TABLE = 64, 4096, 256          # bytes of the (host) image and destination, entries of the two (host) tables
CANARY = 0x5EEDC0DE00 + 7
MAX = 0x7FFFFFFF


def test_symbols_are_declared_exported_and_bound():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in (NAME, STATS):
        assert re.search(r"\b%s\s*\(" % name, text)
        assert getattr(raw, name) is not None
        assert name in p.exported_symbols()
    assert re.search(r"typedef struct fourmc_image_split_item\b", text)
    assert C.sizeof(p.ImageSplitItem) == 88
    assert [f[0] for f in p.ImageSplitItem._fields_] == ["split_start", "split_end", "dst_off", "dst_cap", "table_off", "lines_cap", "out"]
    assert p.ImageSplitItem.out.offset == 48
    body = re.search(r"typedef struct fourmc_image_split_item \{(.*?)\} fourmc_image_split_item;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == [f[0] for f in p.ImageSplitItem._fields_]
    assert callable(p.image_read_lines_batch) and callable(p.image_lines_batch_stats)
    # the single call's header comment no longer lists the batch as missing
    assert "batching of splits" not in text


def _items(p, rows):
    """host items with a canary in every field of `out`, so that a call that touches one shows"""
    arr = (p.ImageSplitItem * max(len(rows), 1))()
    for i, row in enumerate(rows):
        (arr[i].split_start, arr[i].split_end, arr[i].dst_off, arr[i].dst_cap, arr[i].table_off, arr[i].lines_cap) = row
        for k, (f, _) in enumerate(p.ImageLines._fields_):
            setattr(arr[i].out, f, CANARY + 10 * i + k)
    return arr


def _untouched(p, arr, rows):
    for i, row in enumerate(rows):
        got = (arr[i].split_start, arr[i].split_end, arr[i].dst_off, arr[i].dst_cap, arr[i].table_off, arr[i].lines_cap)
        assert got == tuple(row), i
        for k, (f, _) in enumerate(p.ImageLines._fields_):
            assert getattr(arr[i].out, f) == CANARY + 10 * i + k, (i, f)


class Buffers:
    def __init__(self):
        self.img = np.zeros(IMG, np.uint8)
        self.dst = np.full(DST, 0xC3, np.uint8)
        self.st = np.full(TABLE, 0x1111, np.uint64)
        self.tl = np.full(TABLE, 0x2222, np.uint32)

    def clean(self):
        return bool((self.dst == 0xC3).all() and (self.st == 0x1111).all() and (self.tl == 0x2222).all())


def _call(p, buf, rows, arr=None, image=True, dst=True, starts=True, tlen=True, max_len=MAX, n=None, dst_bytes=DST, entries=TABLE):
    arr = _items(p, rows) if arr is None else arr
    rc = p.lib().fourmc_gpu_image_read_lines_batch(
        buf.img.ctypes.data if image else None, IMG, max_len, buf.dst.ctypes.data if dst else None, dst_bytes,
        buf.st.ctypes.data if starts else None, buf.tl.ctypes.data if tlen else None, entries,
        C.cast(arr, C.c_void_p) if arr is not False else None, len(rows) if n is None else n, None)
    return rc, arr


# (split_start, split_end, dst_off, dst_cap, table_off, lines_cap)
GOOD = [(0, 64, 0, 100, 0, 10), (0, 64, 100, 900, 10, 20), (12, 64, 1000, 96, 30, 0), (0, 64, 4096, 0, 256, 0)]
EINVAL_CASES = {
    # name: (rows, keyword arguments of _call)
    "null image": (GOOD, dict(image=False)),
    "null destination": (GOOD, dict(dst=False)),
    "null destination, size queries only": ([(0, 64, 0, 0, 0, 4)], dict(dst=False)),
    "starts without text_len": (GOOD, dict(tlen=False)),
    "text_len without starts": (GOOD, dict(starts=False)),
    "max_line_len 0x80000000": (GOOD, dict(max_len=0x80000000)),
    "max_line_len 0xFFFFFFFF, count only": (GOOD, dict(max_len=0xFFFFFFFF, starts=False, tlen=False)),
    "region starts beyond the destination": ([(0, 64, DST + 1, 0, 0, 4)], {}),
    "region ends beyond the destination": ([(0, 64, 0, 100, 0, 4), (0, 64, DST - 99, 100, 4, 4)], {}),
    "dst_off + dst_cap wraps": ([(0, 64, 16, 2 ** 64 - 8, 0, 4)], {}),
    "dst_off + dst_cap wraps, count only": ([(0, 64, 16, 2 ** 64 - 8, 0, 4)], dict(starts=False, tlen=False)),
    "regions overlap by one byte": ([(0, 64, 100, 100, 0, 4), (0, 64, 0, 101, 4, 4)], {}),
    "regions overlap by one byte, count only": ([(0, 64, 100, 100, 0, 0), (0, 64, 0, 101, 0, 0)], dict(starts=False, tlen=False)),
    "one region inside another": ([(0, 64, 0, 1000, 0, 4), (0, 64, 3000, 100, 4, 4), (0, 64, 500, 60, 8, 4)], {}),
    "the same region twice": ([(0, 64, 64, 64, 0, 4), (0, 64, 64, 64, 4, 4)], {}),
    "table region starts beyond the tables": ([(0, 64, 0, 100, TABLE + 1, 0)], {}),
    "table region ends beyond the tables": ([(0, 64, 0, 100, 0, 4), (0, 64, 100, 100, TABLE - 3, 4)], {}),
    "table_off + lines_cap wraps": ([(0, 64, 0, 100, 8, 2 ** 64 - 4)], {}),
    "table regions overlap by one entry": ([(0, 64, 0, 100, 10, 10), (0, 64, 100, 100, 0, 11)], {}),
    "one table region inside another": ([(0, 64, 0, 100, 0, 100), (0, 64, 100, 100, 200, 10), (0, 64, 200, 100, 50, 6)], {}),
    "the same table region twice": ([(0, 64, 0, 100, 16, 8), (0, 64, 100, 100, 16, 8)], {}),
}


@pytest.mark.parametrize("name", list(EINVAL_CASES))
def test_argument_errors_are_einval_before_any_device(name):
    """no skip with a GPU present: these return before the device is looked at, so the host pointers are never used"""
    p = helpers.pkg()
    L = p.lib()
    rows, kw = EINVAL_CASES[name]
    buf = Buffers()
    rc, arr = _call(p, buf, rows, **kw)
    assert rc == EINVAL, (name, rc)
    assert b"image_read_lines_batch" in L.fourmc_gpu_last_error(), L.fourmc_gpu_last_error()
    _untouched(p, arr, rows)
    assert buf.clean()


def test_null_items_is_einval_and_no_items_is_ok():
    p = helpers.pkg()
    L = p.lib()
    buf = Buffers()
    rc, _ = _call(p, buf, GOOD, arr=False, n=3)
    assert rc == EINVAL and b"image_read_lines_batch" in L.fourmc_gpu_last_error()
    for arr in (False, _items(p, GOOD)):
        assert _call(p, buf, GOOD, arr=arr, n=0)[0] == OK
        assert _call(p, buf, GOOD, arr=arr, n=0, image=False, dst=False, tlen=False, max_len=0xFFFFFFFF)[0] == OK   # nothing else is looked at
        if arr is not False:
            _untouched(p, arr, GOOD)
    assert buf.clean()


@pytest.mark.skipif(torch.cuda.is_available(), reason="a well-formed call would run on the device with host pointers")
def test_what_the_checks_accept_ends_at_the_device_check():
    """regions that touch, table overlaps in a count-only call, empty regions anywhere inside: the answer is the device's (none)"""
    p = helpers.pkg()
    L = p.lib()
    buf = Buffers()
    touching = [(0, 64, 0, 100, 0, 10), (0, 64, 100, 33, 10, 1), (0, 64, 133, DST - 133, 11, TABLE - 11), (0, 64, 50, 0, 5, 0), (0, 64, DST, 0, TABLE, 0)]
    rc, arr = _call(p, buf, touching)
    assert rc == ENODEV, rc
    assert L.fourmc_gpu_last_error()
    _untouched(p, arr, touching)
    rc, arr = _call(p, buf, GOOD)
    assert rc == ENODEV
    _untouched(p, arr, GOOD)
    # overlapping and out-of-range table regions are an error only when tables are given
    for rows in ([(0, 64, 0, 100, 10, 10), (0, 64, 100, 100, 0, 11)], [(0, 64, 0, 100, TABLE + 1, 2 ** 64 - 1)], [(0, 64, 0, 100, 16, 8), (0, 64, 100, 100, 16, 8)]):
        rc, arr = _call(p, buf, rows, starts=False, tlen=False, entries=0)
        assert rc == ENODEV, (rows, rc)
        _untouched(p, arr, rows)
        assert _call(p, buf, rows)[0] == EINVAL
    # the same split twice, max_line_len 0
    same = [(12, 64, 0, 100, 0, 10), (12, 64, 100, 100, 10, 10)]
    assert _call(p, buf, same, max_len=0)[0] == ENODEV
    assert buf.clean()


def test_python_entry_point_validates_its_tensors():
    p = helpers.pkg()
    img, dst = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.image_read_lines_batch(img, [(0, 64, 0, 64, 0, 0)], dst)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_the_python_entry_point_raises_the_engines_enodev(monkeypatch):
    p = helpers.pkg()
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    img, dst = torch.zeros(44, dtype=torch.uint8), torch.full((64,), 7, dtype=torch.uint8)
    rows = [(0, 44, 0, 32, 0, 2), {"split_start": 0, "split_end": 44, "dst_off": 32, "dst_cap": 32}]
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_read_lines_batch failed \(-1\)"):
        p.image_read_lines_batch(img, rows, dst)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_read_lines_batch failed \(-3\)"):
        p.image_read_lines_batch(img, [(0, 44, 0, 33, 0, 0), (0, 44, 32, 32, 0, 0)], dst)
    with pytest.raises(p.EngineError, match="go together"):
        p.image_read_lines_batch(img, rows, dst, starts=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(p.EngineError, match="go together"):
        p.image_read_lines_batch(img, rows, dst, text_len=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(p.EngineError, match="int64 CUDA tensor"):
        p.image_read_lines_batch(img, rows, dst, starts=torch.zeros(4, dtype=torch.int64), text_len=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(p.EngineError, match="max_line_len"):
        p.image_read_lines_batch(img, rows, dst, max_line_len=0x80000000)
    with pytest.raises(p.EngineError, match="splits"):
        p.image_read_lines_batch(img, [(0, 44, 0, 32)], dst)
    assert p.image_read_lines_batch(img, [], dst) == []
    assert bool((dst == 7).all())
    assert p.image_lines_batch_stats() == (0, 0, 0)
