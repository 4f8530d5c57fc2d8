"""What the many-item entry points of the engine refuse, and in which words: every argument check of fourmc_gpu_images_compress,
_images_decompress, _bstreams_compress, _images_compress_writes, _bstreams_decompress, _zsts_compress, _zsts_decompress, _image_read,
_image_read_lines_batch and _images_read_lines, as (return code, fourmc_gpu_last_error()) against
tests/golden/engine_arg_messages.json.

The golden was recorded from the builds in which every entry point still carried its own copy of the span and overlap checks (run
this module as a script to write it); it is not written again from code that shares them.  Every refused call returns before a
device is looked for, so these cases need none and behave the same with one."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import helpers

GOLDEN = os.path.join(helpers.ROOT, "tests", "golden", "engine_arg_messages.json")
OK, ENODEV, EINVAL, EUNSUP = 0, -1, -3, -5
SRC, IMG, DST, TABLE, WRITES = 4096, 8192, 4096, 256, 64      # bytes of sources, images and destination; entries of the tables
MAGIC, LZ4, ZSTD = 0x344D4300, 0, 3
W = 2 ** 64
MAXLEN = 0x7FFFFFFF


class Buffers:
    """host memory behind every pointer: no case gets as far as reading or writing it"""
    def __init__(self):
        self.src = np.zeros(SRC + 64, np.uint8)
        self.img = np.zeros(IMG, np.uint8)
        self.dst = np.zeros(DST, np.uint8)
        self.writes = np.zeros(WRITES, np.uint32)
        self.starts = np.zeros(TABLE, np.uint64)
        self.tlen = np.zeros(TABLE, np.uint32)


BUF = Buffers()


def _ptr(a, given=True):
    return a.ctypes.data if given else None


def _fill(cls, fields, rows):
    arr = (cls * max(len(rows), 1))()
    for i, row in enumerate(rows):
        for f, v in zip(fields, row):
            setattr(arr[i], f, v)
    return arr


def _items(arr, given=True):
    return C.cast(arr, C.c_void_p) if given else None


def _n(rows, n):
    return len(rows) if n is None else n


# rows: (src_off, src_bytes, image_off, image_cap); fourmc_gpu_image_bound(100) is 160
def images_compress(p, rows, items=True, src=True, images=True, magic=MAGIC, n=None):
    arr = _fill(p.ImageEncItem, ("src_off", "src_bytes", "image_off", "image_cap"), rows)
    return p.lib().fourmc_gpu_images_compress(_ptr(BUF.src, src), SRC, _ptr(BUF.img, images), IMG, magic, 1, _items(arr, items), _n(rows, n), None)


DEC_FIELDS = ("image_off", "image_bytes", "dst_off", "dst_cap")


# rows: (image_off, image_bytes, dst_off, dst_cap)
def images_decompress(p, rows, items=True, images=True, dst=True, magic=MAGIC, n=None):
    arr = _fill(p.ImageItem, DEC_FIELDS, rows)
    return p.lib().fourmc_gpu_images_decompress(_ptr(BUF.img, images), IMG, _ptr(BUF.dst, dst), DST, magic, _items(arr, items), _n(rows, n), None)


def bstreams_decompress(p, rows, items=True, images=True, dst=True, codec=LZ4, n=None):
    arr = _fill(p.BstreamItem, DEC_FIELDS, rows)
    return p.lib().fourmc_gpu_bstreams_decompress(_ptr(BUF.img, images), IMG, _ptr(BUF.dst, dst), DST, codec, _items(arr, items), _n(rows, n), None)


def zsts_decompress(p, rows, items=True, images=True, dst=True, n=None):
    arr = _fill(p.ZstItem, DEC_FIELDS, rows)
    return p.lib().fourmc_gpu_zsts_decompress(_ptr(BUF.img, images), IMG, _ptr(BUF.dst, dst), DST, _items(arr, items), _n(rows, n), None)


# rows: (src_off, src_bytes, image_off, image_cap, writes_off, n_writes)
def bstreams_compress(p, rows, items=True, src=True, writes=True, images=True, codec=LZ4, level=1, n=None):
    arr = _fill(p.BstreamEncItem, ("src_off", "src_bytes", "image_off", "image_cap", "writes_off", "n_writes"), rows)
    return p.lib().fourmc_gpu_bstreams_compress(_ptr(BUF.src, src), SRC, _ptr(BUF.writes, writes), WRITES, _ptr(BUF.img, images), IMG, codec, level,
                                                _items(arr, items), _n(rows, n), None)


# rows: (src_off, src_bytes, image_off, image_cap, writes_off, n_writes)
def images_compress_writes(p, rows, items=True, src=True, writes=True, images=True, magic=MAGIC, level=1, n=None):
    arr = _fill(p.ImageWrItem, ("src_off", "src_bytes", "image_off", "image_cap", "writes_off", "n_writes"), rows)
    return p.lib().fourmc_gpu_images_compress_writes(_ptr(BUF.src, src), SRC, _ptr(BUF.writes, writes), WRITES, _ptr(BUF.img, images), IMG, magic, level,
                                                     _items(arr, items), _n(rows, n), None)


# rows: (src_off, src_bytes, image_off, image_cap, level)
def zsts_compress(p, rows, items=True, src=True, images=True, n=None):
    arr = _fill(p.ZstwItem, ("src_off", "src_bytes", "image_off", "image_cap", "level"), rows)
    return p.lib().fourmc_gpu_zsts_compress(_ptr(BUF.src, src), SRC, _ptr(BUF.img, images), IMG, _items(arr, items), _n(rows, n), None)


# rows: (offset, length, dst_off)
def image_read(p, rows, ranges=True, image=True, dst=True, image_bytes=IMG, n=None):
    arr = _fill(p.ImageRange, ("offset", "length", "dst_off"), rows)
    return p.lib().fourmc_gpu_image_read(_ptr(BUF.img, image), image_bytes, _items(arr, ranges), _n(rows, n), _ptr(BUF.dst, dst), DST, None)


# rows: (split_start, split_end, dst_off, dst_cap, table_off, lines_cap)
def lines_batch(p, rows, items=True, image=True, dst=True, starts=True, tlen=True, max_len=MAXLEN, n=None):
    arr = _fill(p.ImageSplitItem, ("split_start", "split_end", "dst_off", "dst_cap", "table_off", "lines_cap"), rows)
    return p.lib().fourmc_gpu_image_read_lines_batch(_ptr(BUF.img, image), IMG, max_len, _ptr(BUF.dst, dst), DST, _ptr(BUF.starts, starts),
                                                     _ptr(BUF.tlen, tlen), TABLE, _items(arr, items), _n(rows, n), None)


# rows: (image, split_start, split_end, dst_off, dst_cap, table_off, lines_cap); refs: (image_off, image_bytes)
def images_lines(p, rows, items=True, image=True, dst=True, starts=True, tlen=True, max_len=MAXLEN, n=None, refs=((0, 64), (64, 100)), refs_given=True):
    arr = _fill(p.ImagesSplitItem, ("image", "split_start", "split_end", "dst_off", "dst_cap", "table_off", "lines_cap"), rows)
    r = _fill(p.ImageRef, ("image_off", "image_bytes"), refs)
    return p.lib().fourmc_gpu_images_read_lines(_ptr(BUF.img, image), IMG, _items(r, refs_given), len(refs), max_len, _ptr(BUF.dst, dst), DST,
                                                _ptr(BUF.starts, starts), _ptr(BUF.tlen, tlen), TABLE, _items(arr, items), _n(rows, n), None)


def _decode_cases(name, call, noun, **first):
    """the cases the three decode validators share; `first`: what the call checks before its items (a bad magic or codec)"""
    ok = (0, 100, 0, 200)
    cases = [
        (f"{name}: null items", call, [ok], dict(items=False)),
        (f"{name}: null {noun}s with a non-empty {noun}", call, [(0, 0, 0, 200), ok], dict(images=False)),
        (f"{name}: {noun} starts beyond the buffer", call, [ok, (IMG + 1, 0, 200, 200)], {}),
        (f"{name}: {noun} ends beyond the buffer", call, [(IMG - 4, 8, 0, 200)], {}),
        (f"{name}: image_off + image_bytes wraps", call, [(8, W - 4, 0, 200)], {}),
        (f"{name}: region starts beyond the destination", call, [(0, 100, DST + 1, 0)], {}),
        (f"{name}: region ends beyond the destination", call, [ok, (100, 100, DST - 100, 101)], {}),
        (f"{name}: dst_off + dst_cap wraps", call, [(0, 100, 16, W - 8)], {}),
        (f"{name}: regions overlap by one byte", call, [(0, 100, 200, 200), (100, 100, 1, 200)], {}),
        (f"{name}: the same region twice", call, [(0, 100, 64, 64), (100, 100, 64, 64)], {}),
        (f"{name}: one region inside another", call, [(0, 100, 0, 1000), (100, 100, 2000, 100), (200, 100, 300, 200)], {}),
        (f"{name}: two faults, the {noun} and its region", call, [(IMG + 1, 0, DST + 1, 0)], {}),
        (f"{name}: two faults, an overlap and a later region", call, [(0, 100, 0, 200), (0, 100, 100, 200), (0, 100, DST, 1)], {}),
        (f"{name}: two faults, a region and a later null {noun}s", call, [(0, 0, DST + 1, 0), ok], dict(images=False)),
    ]
    for key, bad in first.items():
        cases.append((f"{name}: two faults, {key} and null items", call, [ok], dict(items=False, **{key: bad})))
    return cases


LINE = (0, 64, 0, 100, 0, 10)


def _lines_cases(name, call, pre):
    """`pre`: the leading columns of a row of this call (the image number of images_read_lines)"""
    def R(*rows): return [pre + r for r in rows]
    return [
        (f"{name}: null items", call, R(LINE), dict(items=False)),
        (f"{name}: null image", call, R(LINE), dict(image=False)),
        (f"{name}: null destination", call, R(LINE), dict(dst=False)),
        (f"{name}: starts without text_len", call, R(LINE), dict(tlen=False)),
        (f"{name}: max_line_len 0x80000000", call, R(LINE), dict(max_len=0x80000000)),
        (f"{name}: region starts beyond the destination", call, R((0, 64, DST + 1, 0, 0, 4)), {}),
        (f"{name}: region ends beyond the destination", call, R(LINE, (0, 64, DST - 99, 100, 10, 4)), {}),
        (f"{name}: dst_off + dst_cap wraps", call, R((0, 64, 16, W - 8, 0, 4)), {}),
        (f"{name}: regions overlap by one byte", call, R((0, 64, 100, 100, 0, 4), (0, 64, 0, 101, 4, 4)), {}),
        (f"{name}: regions overlap by one byte, count only", call, R((0, 64, 100, 100, 0, 0), (0, 64, 0, 101, 0, 0)), dict(starts=False, tlen=False)),
        (f"{name}: the same region twice", call, R((0, 64, 64, 64, 0, 4), (0, 64, 64, 64, 4, 4)), {}),
        (f"{name}: one region inside another", call, R((0, 64, 0, 1000, 0, 4), (0, 64, 2000, 100, 4, 4), (0, 64, 300, 200, 8, 4)), {}),
        (f"{name}: table region starts beyond the tables", call, R((0, 64, 0, 100, TABLE + 1, 0)), {}),
        (f"{name}: table region ends beyond the tables", call, R(LINE, (0, 64, 100, 100, TABLE - 3, 4)), {}),
        (f"{name}: table_off + lines_cap wraps", call, R((0, 64, 0, 100, 8, W - 4)), {}),
        (f"{name}: table regions overlap by one entry", call, R((0, 64, 0, 100, 10, 10), (0, 64, 100, 100, 0, 11)), {}),
        (f"{name}: the same table region twice", call, R((0, 64, 0, 100, 16, 8), (0, 64, 100, 100, 16, 8)), {}),
        (f"{name}: one table region inside another", call, R((0, 64, 0, 100, 0, 100), (0, 64, 100, 100, 200, 8), (0, 64, 200, 100, 30, 20)), {}),
        (f"{name}: two faults, a table region and a later output region", call, R((0, 64, 0, 100, TABLE + 1, 0), (0, 64, DST + 1, 0, 0, 4)), {}),
        (f"{name}: two faults, output overlap and a later table region", call, R((0, 64, 0, 100, 0, 4), (0, 64, 50, 100, TABLE, 1)), {}),
        (f"{name}: two faults, output overlap and table overlap", call, R((0, 64, 0, 100, 0, 4), (0, 64, 99, 100, 3, 4)), {}),
        (f"{name}: two faults, max_line_len and a region", call, R((0, 64, DST + 1, 0, 0, 4)), dict(max_len=0xFFFFFFFF)),
    ]


ENC = (0, 100, 0, 200)                   # images_compress: a source of 100 bytes needs 160
BSW = (0, 100, 0, 200, 0, 2)
ZSW = (0, 100, 0, 200, 1)
REFUSED = (
    [
        ("images_compress: null items", images_compress, [ENC], dict(items=False)),
        ("images_compress: null images", images_compress, [ENC], dict(images=False)),
        ("images_compress: null source with a non-empty image", images_compress, [(0, 0, 0, 200), (0, 100, 200, 200)], dict(src=False)),
        ("images_compress: source starts beyond the buffer", images_compress, [ENC, (SRC + 1, 0, 200, 200)], {}),
        ("images_compress: source ends beyond the buffer", images_compress, [(SRC - 4, 8, 0, 200)], {}),
        ("images_compress: src_off + src_bytes wraps", images_compress, [(8, W - 4, 0, 200)], {}),
        ("images_compress: region starts beyond the images", images_compress, [(0, 100, IMG + 1, 0)], {}),
        ("images_compress: region ends beyond the images", images_compress, [ENC, (0, 100, IMG - 199, 200)], {}),
        ("images_compress: image_off + image_cap wraps", images_compress, [(0, 100, 8, W - 4)], {}),
        ("images_compress: capacity one below the bound", images_compress, [ENC, (0, 100, 200, 159)], {}),
        ("images_compress: capacity 0", images_compress, [(0, 0, 100, 0)], {}),
        ("images_compress: regions overlap by one byte", images_compress, [(0, 100, 200, 200), (0, 100, 1, 200)], {}),
        ("images_compress: the same region twice", images_compress, [ENC, ENC], {}),
        ("images_compress: one region inside another", images_compress, [(0, 100, 0, 1000), (0, 100, 2000, 200), (0, 100, 300, 200)], {}),
        ("images_compress: two faults, a source and its region", images_compress, [(SRC + 1, 0, IMG + 1, 0)], {}),
        ("images_compress: two faults, a region and its capacity", images_compress, [(0, 100, IMG - 10, 11)], {}),
        ("images_compress: two faults, an overlap and a later capacity", images_compress, [ENC, (0, 100, 100, 200), (0, 100, 400, 100)], {}),
        ("images_compress: two faults, magic and null items", images_compress, [ENC], dict(items=False, magic=0x12345678)),
    ]
    + _decode_cases("images_decompress", images_decompress, "image", magic=0x12345678)
    + _decode_cases("bstreams_decompress", bstreams_decompress, "stream", codec=9)
    + _decode_cases("zsts_decompress", zsts_decompress, "stream")
    + [
        ("bstreams_compress: null items", bstreams_compress, [BSW], dict(items=False)),
        ("bstreams_compress: null source with a non-empty stream", bstreams_compress, [(0, 0, 0, 200, 0, 0), (0, 100, 200, 200, 0, 2)], dict(src=False)),
        ("bstreams_compress: null write table with writes", bstreams_compress, [(0, 100, 0, 200, 0, 0), (0, 100, 200, 200, 0, 2)], dict(writes=False)),
        ("bstreams_compress: source starts beyond the buffer", bstreams_compress, [BSW, (SRC + 1, 0, 200, 200, 0, 0)], {}),
        ("bstreams_compress: source ends beyond the buffer", bstreams_compress, [(SRC - 4, 8, 0, 200, 0, 2)], {}),
        ("bstreams_compress: src_off + src_bytes wraps", bstreams_compress, [(8, W - 4, 0, 200, 0, 2)], {}),
        ("bstreams_compress: write sizes start beyond the table", bstreams_compress, [(0, 100, 0, 200, WRITES + 1, 0)], {}),
        ("bstreams_compress: write sizes end beyond the table", bstreams_compress, [BSW, (0, 100, 200, 200, WRITES - 3, 4)], {}),
        ("bstreams_compress: writes_off + n_writes wraps", bstreams_compress, [(0, 100, 0, 200, 8, W - 4)], {}),
        ("bstreams_compress: region starts beyond the images", bstreams_compress, [(0, 100, IMG + 1, 0, 0, 2)], {}),
        ("bstreams_compress: region ends beyond the images", bstreams_compress, [BSW, (0, 100, IMG - 199, 200, 2, 2)], {}),
        ("bstreams_compress: image_off + image_cap wraps", bstreams_compress, [(0, 100, 8, W - 4, 0, 2)], {}),
        ("bstreams_compress: regions overlap by one byte", bstreams_compress, [(0, 100, 200, 200, 0, 2), (0, 100, 1, 200, 2, 2)], {}),
        ("bstreams_compress: the same region twice", bstreams_compress, [BSW, BSW], {}),
        ("bstreams_compress: one region inside another", bstreams_compress, [(0, 100, 0, 1000, 0, 2), (0, 100, 2000, 200, 0, 2), (0, 100, 300, 200, 0, 2)], {}),
        ("bstreams_compress: a zstd level not on the device", bstreams_compress, [BSW], dict(codec=ZSTD, level=13)),
        ("bstreams_compress: two faults, a source and its write sizes", bstreams_compress, [(SRC + 1, 0, 0, 200, WRITES + 1, 0)], {}),
        ("bstreams_compress: two faults, write sizes and the region", bstreams_compress, [(0, 100, IMG + 1, 0, WRITES + 1, 0)], {}),
        ("bstreams_compress: two faults, an overlap and a later region", bstreams_compress, [BSW, (0, 100, 100, 200, 0, 2), (0, 100, IMG, 1, 0, 2)], {}),
        ("bstreams_compress: two faults, an overlap and the level", bstreams_compress, [BSW, (0, 100, 100, 200, 0, 2)], dict(codec=ZSTD, level=13)),
        ("bstreams_compress: two faults, codec and null items", bstreams_compress, [BSW], dict(items=False, codec=9)),

        # bstreams_compress's rows, one for one, but for the level: this call refuses none
        ("images_compress_writes: null items", images_compress_writes, [BSW], dict(items=False)),
        ("images_compress_writes: null source with a non-empty stream", images_compress_writes, [(0, 0, 0, 200, 0, 0), (0, 100, 200, 200, 0, 2)], dict(src=False)),
        ("images_compress_writes: null write table with writes", images_compress_writes, [(0, 100, 0, 200, 0, 0), (0, 100, 200, 200, 0, 2)], dict(writes=False)),
        ("images_compress_writes: source starts beyond the buffer", images_compress_writes, [BSW, (SRC + 1, 0, 200, 200, 0, 0)], {}),
        ("images_compress_writes: source ends beyond the buffer", images_compress_writes, [(SRC - 4, 8, 0, 200, 0, 2)], {}),
        ("images_compress_writes: src_off + src_bytes wraps", images_compress_writes, [(8, W - 4, 0, 200, 0, 2)], {}),
        ("images_compress_writes: write sizes start beyond the table", images_compress_writes, [(0, 100, 0, 200, WRITES + 1, 0)], {}),
        ("images_compress_writes: write sizes end beyond the table", images_compress_writes, [BSW, (0, 100, 200, 200, WRITES - 3, 4)], {}),
        ("images_compress_writes: writes_off + n_writes wraps", images_compress_writes, [(0, 100, 0, 200, 8, W - 4)], {}),
        ("images_compress_writes: region starts beyond the images", images_compress_writes, [(0, 100, IMG + 1, 0, 0, 2)], {}),
        ("images_compress_writes: region ends beyond the images", images_compress_writes, [BSW, (0, 100, IMG - 199, 200, 2, 2)], {}),
        ("images_compress_writes: image_off + image_cap wraps", images_compress_writes, [(0, 100, 8, W - 4, 0, 2)], {}),
        ("images_compress_writes: regions overlap by one byte", images_compress_writes, [(0, 100, 200, 200, 0, 2), (0, 100, 1, 200, 2, 2)], {}),
        ("images_compress_writes: the same region twice", images_compress_writes, [BSW, BSW], {}),
        ("images_compress_writes: one region inside another", images_compress_writes,
         [(0, 100, 0, 1000, 0, 2), (0, 100, 2000, 200, 0, 2), (0, 100, 300, 200, 0, 2)], {}),
        ("images_compress_writes: two faults, a source and its write sizes", images_compress_writes, [(SRC + 1, 0, 0, 200, WRITES + 1, 0)], {}),
        ("images_compress_writes: two faults, write sizes and the region", images_compress_writes, [(0, 100, IMG + 1, 0, WRITES + 1, 0)], {}),
        ("images_compress_writes: two faults, an overlap and a later region", images_compress_writes, [BSW, (0, 100, 100, 200, 0, 2), (0, 100, IMG, 1, 0, 2)], {}),
        ("images_compress_writes: two faults, magic and null items", images_compress_writes, [BSW], dict(items=False, magic=0x12345678)),

        ("zsts_compress: null items", zsts_compress, [ZSW], dict(items=False)),
        ("zsts_compress: null source with a non-empty stream", zsts_compress, [(0, 0, 0, 200, 1), (0, 100, 200, 200, 1)], dict(src=False)),
        ("zsts_compress: null images with a non-empty region", zsts_compress, [(0, 100, 0, 0, 1), (0, 100, 200, 200, 1)], dict(images=False)),
        ("zsts_compress: source starts beyond the buffer", zsts_compress, [ZSW, (SRC + 1, 0, 200, 200, 1)], {}),
        ("zsts_compress: source ends beyond the buffer", zsts_compress, [(SRC - 4, 8, 0, 200, 1)], {}),
        ("zsts_compress: region starts beyond the images", zsts_compress, [(0, 100, IMG + 1, 0, 1)], {}),
        ("zsts_compress: region ends beyond the images", zsts_compress, [ZSW, (0, 100, IMG - 199, 200, 1)], {}),
        ("zsts_compress: image_off + image_cap wraps", zsts_compress, [(0, 100, 8, W - 4, 1)], {}),
        ("zsts_compress: regions overlap by one byte", zsts_compress, [(0, 100, 200, 200, 1), (0, 100, 1, 200, 3)], {}),
        ("zsts_compress: the same region twice", zsts_compress, [ZSW, ZSW], {}),
        ("zsts_compress: one region inside another", zsts_compress, [(0, 100, 0, 1000, 1), (0, 100, 2000, 200, 1), (0, 100, 300, 200, 1)], {}),
        ("zsts_compress: a source beyond 3 GiB is not read, its region is", zsts_compress, [(SRC + 1, 0xC0000001, IMG + 1, 0, 1)], {}),
        ("zsts_compress: two faults, a source and its region", zsts_compress, [(SRC + 1, 0, IMG + 1, 0, 1)], {}),
        ("zsts_compress: two faults, an overlap and a later region", zsts_compress, [ZSW, (0, 100, 100, 200, 1), (0, 100, IMG, 1, 1)], {}),
        ("zsts_compress: two faults, a region and a later null source", zsts_compress, [(0, 0, IMG + 1, 0, 1), ZSW], dict(src=False)),

        ("image_read: null ranges", image_read, [(0, 10, 0)], dict(ranges=False)),
        ("image_read: null image", image_read, [(0, 10, 0)], dict(image=False)),
        ("image_read: more than 2^30 ranges", image_read, [(0, 10, 0)], dict(n=(1 << 30) + 1)),
        ("image_read: null destination with a non-empty range", image_read, [(0, 0, 0), (0, 10, 0)], dict(dst=False)),
        ("image_read: destinations overlap by one byte", image_read, [(0, 100, 100), (0, 101, 0)], {}),
        ("image_read: the same destination twice", image_read, [(0, 64, 64), (64, 64, 64)], {}),
        ("image_read: one destination inside another", image_read, [(0, 1000, 0), (0, 100, 2000), (0, 200, 300)], {}),
        ("image_read: dst_off + length wraps into another", image_read, [(0, 100, W - 8), (0, 4, W - 4)], {}),
        ("image_read: two faults, an overlap and a null destination", image_read, [(0, 100, 0), (0, 100, 50)], dict(dst=False)),
        ("image_read: two faults, null image and an overlap", image_read, [(0, 100, 0), (0, 100, 50)], dict(image=False)),
    ]
    + _lines_cases("image_read_lines_batch", lines_batch, ())
    + _lines_cases("images_read_lines", images_lines, (0,))
    + [
        ("images_read_lines: two faults, table overlap and an image beyond the buffer", images_lines,
         [(0, 0, 64, 0, 100, 0, 4), (1, 0, 64, 100, 100, 3, 4)], dict(refs=((0, 64), (IMG, 1)))),
        ("images_read_lines: two faults, an image beyond the buffer and a split of no image", images_lines,
         [(2, 0, 64, 0, 100, 0, 4)], dict(refs=((0, 64), (IMG, 1)))),
    ]
)
# what the checks let through: regions that touch, empty regions wherever they lie, and what a size query does not look at
ACCEPTED = [
    ("images_compress: regions that touch", images_compress, [ENC, (0, 100, 200, 200), (100, 0, 400, 44), (SRC, 0, IMG - 44, 44)], {}),
    ("images_decompress: regions that touch, empty regions", images_decompress, [(0, 100, 0, 200), (100, 100, 200, 200), (200, 0, 100, 0), (IMG, 0, DST, 0)], {}),
    ("images_decompress: the size query looks at no destination", images_decompress, [(0, 100, 0, 200), (100, 100, 100, 200), (0, 100, DST + 1, W - 1)], dict(dst=False)),
    ("bstreams_decompress: regions that touch, empty regions", bstreams_decompress, [(0, 100, 0, 200), (100, 100, 200, 200), (200, 0, 100, 0), (IMG, 0, DST, 0)], {}),
    ("bstreams_decompress: the size query looks at no destination", bstreams_decompress, [(0, 100, 0, 200), (100, 100, 100, 200), (0, 100, DST + 1, W - 1)], dict(dst=False)),
    ("zsts_decompress: regions that touch, empty regions", zsts_decompress, [(0, 100, 0, 200), (100, 100, 200, 200), (200, 0, 100, 0), (IMG, 0, DST, 0)], {}),
    ("zsts_decompress: the size query looks at no destination", zsts_decompress, [(0, 100, 0, 200), (100, 100, 100, 200), (0, 100, DST + 1, W - 1)], dict(dst=False)),
    ("bstreams_compress: regions that touch, empty regions", bstreams_compress, [BSW, (0, 100, 200, 200, 2, 2), (0, 100, 100, 0, 0, 0), (SRC, 0, IMG, 0, WRITES, 0)], {}),
    ("bstreams_compress: the size query looks at no region", bstreams_compress, [BSW, (0, 100, 100, 200, 0, 2), (0, 100, IMG + 1, W - 1, 0, 2)], dict(images=False)),
    ("images_compress_writes: regions that touch, empty regions", images_compress_writes,
     [BSW, (0, 100, 200, 200, 2, 2), (0, 100, 100, 0, 0, 0), (SRC, 0, IMG, 0, WRITES, 0)], {}),
    ("images_compress_writes: the size query looks at no region", images_compress_writes,
     [BSW, (0, 100, 100, 200, 0, 2), (0, 100, IMG + 1, W - 1, 0, 2)], dict(images=False)),
    ("images_compress_writes: every level is taken", images_compress_writes, [BSW], dict(level=99)),
    ("zsts_compress: regions that touch, empty regions", zsts_compress,[ZSW, (0, 100, 200, 200, 3), (50, 0, 100, 0, 2), (SRC, 0, IMG, 0, 4)], {}),
    ("image_read: destinations that touch, empty ranges", image_read, [(0, 100, 0), (0, 100, 100), (0, 0, 50), (0, 0, W - 1)], {}),
    ("image_read: a null destination of empty ranges", image_read, [(0, 0, 0), (0, 0, 0)], dict(dst=False)),
    ("image_read_lines_batch: regions that touch, empty regions", lines_batch,
     [(0, 64, 0, 100, 0, 10), (0, 64, 100, 100, 10, 10), (0, 64, 50, 0, 5, 0), (0, 64, DST, 0, TABLE, 0)], {}),
    ("image_read_lines_batch: count only looks at no table", lines_batch,
     [(0, 64, 0, 100, 0, 10), (0, 64, 100, 100, 5, 10), (0, 64, 200, 100, TABLE + 1, W - 1)], dict(starts=False, tlen=False)),
    ("images_read_lines: regions that touch, empty regions", images_lines,
     [(0, 0, 64, 0, 100, 0, 10), (1, 0, 64, 100, 100, 10, 10), (0, 0, 64, 50, 0, 5, 0), (1, 0, 64, DST, 0, TABLE, 0)], {}),
    ("images_read_lines: count only looks at no table", images_lines,
     [(0, 0, 64, 0, 100, 0, 10), (1, 0, 64, 100, 100, 5, 10), (0, 0, 64, 200, 100, TABLE + 1, W - 1)], dict(starts=False, tlen=False)),
]
REFUSED_BY_NAME = {c[0]: c for c in REFUSED}
assert len(REFUSED_BY_NAME) == len(REFUSED), "two cases of one name"


def _run(case):
    _, call, rows, kw = case
    p = helpers.pkg()
    rc = call(p, rows, **kw)
    return rc, p.lib().fourmc_gpu_last_error().decode()


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_golden_has_exactly_the_cases():
    assert list(_golden()) == [c[0] for c in REFUSED]


@pytest.mark.parametrize("name", list(REFUSED_BY_NAME))
def test_refused_call_keeps_its_code_and_message(name):
    rc, msg = _run(REFUSED_BY_NAME[name])
    assert rc in (EINVAL, EUNSUP), (name, rc, msg)
    assert [rc, msg] == _golden()[name]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a well-formed call would run on the device with host pointers")
@pytest.mark.parametrize("name", [c[0] for c in ACCEPTED])
def test_what_the_checks_accept_ends_at_the_device_check(name):
    rc, msg = _run(next(c for c in ACCEPTED if c[0] == name))
    assert rc == ENODEV, (name, rc, msg)


if __name__ == "__main__":
    out = {}
    for case in REFUSED:
        rc, msg = _run(case)
        assert rc in (EINVAL, EUNSUP), (case[0], rc, msg)
        out[case[0]] = [rc, msg]
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=0)
        f.write("\n")
    print(f"{len(out)} cases -> {GOLDEN}")
