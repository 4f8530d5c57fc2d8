"""Hadoop block streams (fourmc_gpu_bstream_*) without a GPU: the constants, the bound, the Python model of the writer and the
reader (tests/bstream_model.py), the symbols, and every argument error refused before a device is looked for.

No file written by a JVM is available (BlockCompressorStream is Hadoop's class, and there is no JVM where these tests are built), so
tests/golden holds no fixture for this format: the model restates the writer from the reference's Lz4Compressor.java and from
knowledge of Hadoop's class, and include/fourmc_gpu.h states the format as the contract."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bstream_model as bm
import helpers

ROOT = helpers.ROOT
OK, ENODEV, EINVAL, EUNSUP = 0, -1, -3, -5
NAMES = ["fourmc_gpu_bstream_max_input", "fourmc_gpu_bstream_bound", "fourmc_gpu_bstream_compress", "fourmc_gpu_bstream_decompress",
         "fourmc_gpu_bstreams_decompress", "fourmc_gpu_bstream_reason_text"]
LZ4, ZSTD = 0, 3
M_LZ4, M_ZSTD = 4177840, 4177920
_MEMO = {}


def data():
    if "data" not in _MEMO:
        _MEMO["data"] = helpers.corpus(2 * M_ZSTD + 4096).tobytes()
    return _MEMO["data"]


# ---- the constants and the bound ----------------------------------------------------------------------------------------------
def test_max_input_is_the_buffer_less_the_codec_overhead():
    p = helpers.pkg()
    L = p.lib()
    B = p.BLOCKSIZE
    assert L.fourmc_LZ4_compressBound(B) == 4210768 and L.fourmc_ZSTD_compressBound(B) == 4210688
    for codec in (p.CODEC_LZ4_FAST, p.CODEC_LZ4_MC, p.CODEC_LZ4_HC):
        assert p.bstream_max_input(codec) == M_LZ4 == B - (L.fourmc_LZ4_compressBound(B) - B) == bm.max_input(False)
    assert p.bstream_max_input(p.CODEC_ZSTD) == M_ZSTD == B - (L.fourmc_ZSTD_compressBound(B) - B) == bm.max_input(True)
    for codec in (-1, 4, 99):
        assert p.bstream_max_input(codec) == 0 and p.bstream_bound(1000, codec, 0) == 0


def model_bound(n, zstd, G):
    """4 for the empty stream, else 8 + the codec's bound per group"""
    if n == 0:
        return 4
    total = 0
    for at in range(0, n, G):
        total += 8 + bm.block_bound(min(G, n - at), zstd)
    return total


@pytest.mark.parametrize("zstd", [False, True], ids=["lz4", "zstd"])
def test_bound_against_the_model(zstd):
    p = helpers.pkg()
    codec = ZSTD if zstd else LZ4
    M = bm.max_input(zstd)
    for G in (1, 1000, M):
        for n in (0, 1, G - 1, G, G + 1, 3 * G):
            if G == 1 and n > 64:
                continue
            assert p.bstream_bound(n, codec, G) == model_bound(n, zstd, G), (G, n)
            if G == M:
                assert p.bstream_bound(n, codec, 0) == model_bound(n, zstd, M), n
    assert p.bstream_bound(5, codec, M + 1) == 0                 # no such group
    # the library's bound twins are what the model's formulas say, on the sizes a group can have
    L = p.lib()
    for n in (0, 1, 255, 256, 1000, (128 << 10) - 1, 128 << 10, M, 4 << 20):
        assert L.fourmc_LZ4_compressBound(n) == bm.lz4_bound(n) and L.fourmc_ZSTD_compressBound(n) == helpers.zstd_bound(n), n


# ---- the model ------------------------------------------------------------------------------------------------------------------
def patterns(M):
    return {"1-byte writes": [1] * 3000, "64 KiB writes": [65536] * 70, "one write of M": [M], "one write of M + 1": [M + 1],
            "2M + 5 after a small write": [100, 2 * M + 5], "nothing": [], "M then 1": [M, 1], "three whole chunks": [3 * M]}


def fake_compressor(b):
    """a stand-in the shape tests can afford on 12 MiB: the length and a few bytes (the shape does not depend on the codec)"""
    return len(b).to_bytes(4, "little") + b[:3]


@pytest.mark.parametrize("zstd", [False, True], ids=["lz4", "zstd"])
def test_model_writer_obeys_the_shape_invariant(zstd):
    M = bm.max_input(zstd)
    zero = b"\x55" * (3 * M)                                    # a payload never ends with a zero
    for name, pat in patterns(M).items():
        n = sum(pat)
        img = bm.write_stream(zero[:n], pat, fake_compressor, zstd)
        # chase the headers with the fake payloads' own lengths: every group of rawlen R has ceil(R / M) chunks, all but the last of M
        p, seen, groups = 0, 0, []
        while len(img) - p >= 4:
            R = int.from_bytes(img[p:p + 4], "big")
            p += 4
            if R == 0:
                break
            got = []
            while sum(got) < R:
                clen = int.from_bytes(img[p:p + 4], "big")
                assert clen == 4 + min(3, int.from_bytes(img[p + 4:p + 8], "little")), name
                got.append(int.from_bytes(img[p + 4:p + 8], "little"))
                p += 4 + clen
            assert sum(got) == R and len(got) == -(-R // M) and all(g == M for g in got[:-1]) and 0 < got[-1] <= M, (name, R, got)
            groups.append(R)
            seen += R
        assert seen == n and p == len(img), name
        long_last = bool(pat) and pat[-1] > M
        assert img.endswith(b"\0\0\0\0") == (long_last or not pat), name           # the trailing zero of the long-write path
        if not pat:
            assert img == b"\0\0\0\0"
        if name == "1-byte writes":
            assert groups == [3000]                                                # small writes accumulate into one group
        if name == "64 KiB writes":
            k = M // 65536
            assert groups == [k * 65536, (70 - k) * 65536]                         # until the next one would pass M
        if name == "M then 1":
            assert groups == [M, 1]
        if name == "2M + 5 after a small write":
            assert groups == [100, 2 * M + 5]


@pytest.mark.parametrize("zstd", [False, True], ids=["lz4", "zstd"])
def test_model_reader_round_trips_the_writer(zstd):
    M = bm.max_input(zstd)
    cb = bm.oracle_compressor(ZSTD if zstd else LZ4, 1)
    memo = {}

    def compress(b):                                             # the same 4 MiB pieces come again and again
        if b not in memo:
            memo[b] = cb(b)
        return memo[b]
    for name, pat in patterns(M).items():
        if name == "three whole chunks":
            continue                                             # the shape test's; 12 MiB through the oracle is not quick
        n = sum(pat)
        src = data()[:n]
        img = bm.write_stream(src, pat, compress, zstd)
        st, out = bm.read_stream(img, zstd)
        assert out == src, name
        assert st["reason"] == bm.OK and st["decoded_bytes"] == st["total_bytes"] == n and st["fail_offset"] == len(img), (name, st)
        groups, end = bm.shape(img, zstd)
        assert st["groups"] == len(groups) and st["chunks"] == sum(len(c) for _, c in groups)
        assert end in (len(img), len(img) - 4) or not pat
        q, _ = bm.read_stream(img, zstd, "query")
        assert q == dict(st, decoded_bytes=0)
        if n:
            small, nothing = bm.read_stream(img, zstd, n - 1)
            assert small["reason"] == bm.DST_SMALL and small["total_bytes"] == n and nothing == b""
        # trailing bytes at a group boundary, and anything after a zero rawlen
        for tail in (b"\x01", b"\x01\x02", b"\x01\x02\x03", b"\0\0\0\0" + bytes(range(1, 30))):
            st2, out2 = bm.read_stream(img + tail, zstd)
            assert out2 == src and st2["reason"] == bm.OK and st2["fail_offset"] == len(img) + len(tail), (name, tail)


def test_model_reader_verdicts():
    """the reader rule's errors on hand-made streams (the GPU tests compare the device with this model)"""
    raw = data()[:3000]
    comp = bm.oracle_compressor(LZ4, 0)(raw)
    g = bm.be32(3000) + bm.be32(len(comp)) + comp
    n = len(g)

    def verdict(img, **kw):
        st, out = bm.read_stream(img, False, **kw)
        assert out == raw * (st["decoded_bytes"] // 3000)
        return st["reason"], st["fail_offset"], st["groups"], st["chunks"], st["decoded_bytes"]
    assert verdict(g + g) == (bm.OK, 2 * n, 2, 2, 6000)
    assert verdict(g + b"\x80\0\0\0" + g[4:]) == (bm.BAD_RAWLEN, n, 1, 1, 3000)
    for cut in range(4):
        assert verdict(g + g[:4 + cut]) == (bm.CLEN_UNREADABLE, n + 4, 1, 1, 3000)
    assert verdict(g + g[:4] + bm.be32(0) + comp) == (bm.BAD_CLEN, n + 4, 1, 1, 3000)
    assert verdict(g + g[:4] + bm.be32((4 << 20) + 1) + comp) == (bm.BAD_CLEN, n + 4, 1, 1, 3000)
    assert verdict(g + g[:-1]) == (bm.DATA_UNREADABLE, n + 4, 1, 1, 3000)
    short = bm.oracle_compressor(LZ4, 0)(raw[:2999])
    assert verdict(g + bm.be32(3000) + bm.be32(len(short)) + short + g) == (bm.SHAPE, n + 4, 1, 1, 3000)
    longer = bm.oracle_compressor(LZ4, 0)(raw + b"x")
    assert verdict(g + bm.be32(3000) + bm.be32(len(longer)) + longer + g) == (bm.CORRUPT, n + 4, 1, 1, 3000)
    # a multi-chunk group cut short counts for nothing: its leading chunks are not decoded
    M = bm.max_input(False)
    assert verdict(g + bm.be32(M + 1) + bm.be32(len(comp)) + comp) == (bm.CLEN_UNREADABLE, 2 * n, 1, 1, 3000)


# ---- the symbols ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(raw, name) is not None, name
        assert name in p.exported_symbols(), name
    assert C.sizeof(p.BstreamStatus) == 40 and C.sizeof(p.BstreamItem) == 72 and p.BstreamItem.status.offset == 32
    for k, name in enumerate(p.BSTREAM_REASONS):
        assert re.search(r"FOURMC_BS_%s\s*=\s*%d\b" % (name, k), text), name
        msg = p.lib().fourmc_gpu_bstream_reason_text(k).decode()
        assert (msg == "") == (k == 0), (k, msg)
    assert p.lib().fourmc_gpu_bstream_reason_text(77).decode() == "unknown"
    assert [getattr(bm, n) for n in p.BSTREAM_REASONS] == list(range(8))
    for f in (p.bstream_max_input, p.bstream_bound, p.compress_bstream, p.decompress_bstream, p.decompress_bstreams, p.bstream_codec):
        assert callable(f)
    assert "bstream.hip" in open(os.path.join(ROOT, "4mc_amd", "csrc", "Makefile")).read()


def test_extensions_map_to_the_compressor_classes_levels():
    p = helpers.pkg()
    want = {".lz4_fast": (p.CODEC_LZ4_FAST, 0), ".lz4_mc": (p.CODEC_LZ4_MC, 0), ".lz4_hc": (p.CODEC_LZ4_HC, 4), ".lz4_uc": (p.CODEC_LZ4_HC, 8),
            ".zstd_fast": (p.CODEC_ZSTD, 1), ".zstd_mc": (p.CODEC_ZSTD, 3), ".zstd_hc": (p.CODEC_ZSTD, 6), ".zstd_uc": (p.CODEC_ZSTD, 12)}
    for ext, cl in want.items():
        assert p.bstream_codec(ext) == cl and p.bstream_codec("part-r-00000" + ext) == cl and p.bstream_codec(ext[1:]) == cl
    for bad in (".4mc", ".zst", "", ".lz4"):
        with pytest.raises(p.EngineError):
            p.bstream_codec(bad)


# ---- arguments ------------------------------------------------------------------------------------------------------------------
SRC, CAP = 5000, 8192


def _compress(L, codec=LZ4, src=True, src_bytes=SRC, image=True, cap=CAP, out=True, level=1, G=1000):
    s = np.zeros(SRC, np.uint8)
    img = np.full(CAP, 0xC3, np.uint8)
    n = C.c_uint64(777)
    rc = L.fourmc_gpu_bstream_compress(s.ctypes.data if src else None, src_bytes, img.ctypes.data if image else None, cap,
                                       C.byref(n) if out else None, codec, level, G, None)
    assert n.value == 777 and (img == 0xC3).all()
    return rc


COMPRESS_EINVAL = {
    "codec": dict(codec=4), "codec, everything else wrong too": dict(codec=-1, src=False, image=False, out=False, G=2 ** 31),
    "null source": dict(src=False), "null image": dict(image=False), "null image_bytes": dict(out=False),
    "group_bytes M + 1": dict(G=M_LZ4 + 1), "group_bytes M + 1, zstd": dict(codec=ZSTD, G=M_ZSTD + 1),
    "group_bytes of the other family's M": dict(codec=LZ4, G=M_ZSTD), "group_bytes 0xFFFFFFFF": dict(G=0xFFFFFFFF),
    "capacity one below the bound": dict(cap=5 * (8 + bm.lz4_bound(1000)) - 1),
    "capacity one below the bound, zstd": dict(codec=ZSTD, cap=5 * (8 + helpers.zstd_bound(1000)) - 1),
    "capacity below 4 for nothing": dict(src_bytes=0, cap=3),
}


@pytest.mark.parametrize("name", list(COMPRESS_EINVAL))
def test_compress_argument_errors_are_einval_before_any_device(name):
    L = helpers.pkg().lib()
    assert _compress(L, **COMPRESS_EINVAL[name]) == EINVAL, name
    assert L.fourmc_gpu_last_error()


def test_compress_level_outside_the_device_is_eunsup():
    L = helpers.pkg().lib()
    for level in (0, 13, -1, 22):
        assert _compress(L, codec=ZSTD, level=level) == EUNSUP, level
    assert _compress(L, codec=4, level=13) == EINVAL             # the codec is checked first


def _items(p, rows):
    arr = (p.BstreamItem * max(len(rows), 1))()
    for i, (io, ib, do, dc) in enumerate(rows):
        arr[i].image_off, arr[i].image_bytes, arr[i].dst_off, arr[i].dst_cap = io, ib, do, dc
        st = arr[i].status
        st.decoded_bytes, st.total_bytes, st.fail_offset, st.groups, st.chunks, st.reason, st.pad = 11 + i, 22 + i, 33 + i, 44, 55, 66, 77
    return arr


def _untouched(arr, rows):
    for i, row in enumerate(rows):
        st = arr[i].status
        assert (arr[i].image_off, arr[i].image_bytes, arr[i].dst_off, arr[i].dst_cap) == tuple(row), i
        assert (st.decoded_bytes, st.total_bytes, st.fail_offset, st.groups, st.chunks, st.reason, st.pad) == (11 + i, 22 + i, 33 + i, 44, 55, 66, 77), i


IMAGES, DST = 1000, 4096
GOOD = [(0, 44, 0, 100), (44, 500, 100, 1000), (44, 500, 2000, 0), (1000, 0, 1100, 2996)]
MANY_EINVAL = {
    # name: (rows, codec, images pointer given, destination pointer given)
    "codec": (GOOD, 4, True, True), "codec, size query": (GOOD, -1, True, False),
    "null images": (GOOD, LZ4, False, True), "null images, size query": ([(0, 0, 0, 0), (0, 1, 0, 0)], ZSTD, False, False),
    "stream starts beyond the buffer": ([(0, 44, 0, 10), (IMAGES + 1, 0, 10, 10)], LZ4, True, True),
    "stream ends beyond the buffer": ([(0, 44, 0, 10), (IMAGES - 43, 44, 10, 10)], ZSTD, True, True),
    "stream ends beyond the buffer, size query": ([(IMAGES - 43, 44, 0, 0)], LZ4, True, False),
    "image_off + image_bytes wraps": ([(8, 2 ** 64 - 4, 0, 10)], LZ4, True, True),
    "region starts beyond the destination": ([(0, 44, DST + 1, 0)], LZ4, True, True),
    "region ends beyond the destination": ([(0, 44, 0, 10), (44, 44, DST - 9, 10)], LZ4, True, True),
    "dst_off + dst_cap wraps": ([(0, 44, 16, 2 ** 64 - 8)], ZSTD, True, True),
    "regions overlap by one byte": ([(0, 44, 100, 50), (44, 44, 0, 101)], LZ4, True, True),
    "one region inside another": ([(0, 44, 0, 1000), (44, 44, 3000, 10), (88, 44, 500, 1)], LZ4, True, True),
    "the same region twice": ([(0, 44, 64, 64), (0, 44, 64, 64)], ZSTD, True, True),
}


@pytest.mark.parametrize("name", list(MANY_EINVAL))
def test_many_streams_argument_errors_are_einval_before_any_device(name):
    p = helpers.pkg()
    L = p.lib()
    rows, codec, have_images, have_dst = MANY_EINVAL[name]
    images = np.zeros(IMAGES + 64, np.uint8)
    dst = np.zeros(DST, np.uint8)
    arr = _items(p, rows)
    rc = L.fourmc_gpu_bstreams_decompress(images.ctypes.data if have_images else None, IMAGES, dst.ctypes.data if have_dst else None, DST,
                                          codec, C.cast(arr, C.c_void_p), len(rows), None)
    assert rc == EINVAL, (name, rc)
    assert L.fourmc_gpu_last_error()
    _untouched(arr, rows)
    assert not dst.any()


def test_null_items_is_einval_and_no_items_is_ok():
    p = helpers.pkg()
    L = p.lib()
    images = np.zeros(IMAGES + 64, np.uint8)
    dst = np.zeros(DST, np.uint8)
    assert L.fourmc_gpu_bstreams_decompress(images.ctypes.data, IMAGES, dst.ctypes.data, DST, LZ4, None, 3, None) == EINVAL
    for items in (None, C.cast(_items(p, GOOD), C.c_void_p)):
        for codec in (0, 1, 2, 3):
            assert L.fourmc_gpu_bstreams_decompress(images.ctypes.data, IMAGES, dst.ctypes.data, DST, codec, items, 0, None) == OK
            assert L.fourmc_gpu_bstreams_decompress(None, 0, None, 0, codec, items, 0, None) == OK
    assert L.fourmc_gpu_bstreams_decompress(None, 0, None, 0, 7, None, 0, None) == EINVAL        # the codec is checked first


def test_single_decompress_argument_errors_are_einval_before_any_device():
    p = helpers.pkg()
    L = p.lib()
    img = np.zeros(64, np.uint8)
    dst = np.zeros(64, np.uint8)
    st = p.BstreamStatus()
    st.reason = 66
    for codec, image, n, status in ((4, True, 64, True), (-1, False, 64, False), (LZ4, False, 64, True), (ZSTD, True, 64, False),
                                    (LZ4, False, 0, False)):
        rc = L.fourmc_gpu_bstream_decompress(img.ctypes.data if image else None, n, dst.ctypes.data, 64, codec,
                                             C.byref(st) if status else None, None)
        assert rc == EINVAL, (codec, image, n, status)
        assert st.reason == 66 and not dst.any()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_well_formed_calls_fail_with_enodev(monkeypatch):
    import importlib
    p = helpers.pkg()
    L = p.lib()
    for codec, level in ((0, 0), (1, 0), (2, 4), (2, 99), (3, 1), (3, 12)):
        for G in (0, 1, 1000, p.bstream_max_input(codec)):
            cap = CAP if G != 1 else 400000
            s = np.zeros(SRC, np.uint8)
            img = np.full(cap, 0xC3, np.uint8)
            n = C.c_uint64(777)
            assert L.fourmc_gpu_bstream_compress(s.ctypes.data, SRC, img.ctypes.data, cap, C.byref(n), codec, level, G, None) == ENODEV
            assert n.value == 777 and (img == 0xC3).all() and L.fourmc_gpu_last_error()
    assert _compress(L, src=False, src_bytes=0, cap=4) == ENODEV                   # nothing to read: no source is needed
    images = np.zeros(IMAGES + 64, np.uint8)
    dst = np.zeros(DST, np.uint8)
    for have_dst in (True, False):
        for codec in (LZ4, ZSTD):
            arr = _items(p, GOOD)
            rc = L.fourmc_gpu_bstreams_decompress(images.ctypes.data, IMAGES, dst.ctypes.data if have_dst else None, DST, codec,
                                                  C.cast(arr, C.c_void_p), len(GOOD), None)
            assert rc == ENODEV, rc
            _untouched(arr, GOOD)
            st = p.BstreamStatus()
            st.reason = 66
            assert L.fourmc_gpu_bstream_decompress(images.ctypes.data, IMAGES, dst.ctypes.data if have_dst else None, DST, codec,
                                                   C.byref(st), None) == ENODEV
            assert st.reason == 66
    # regions that touch or are empty do not overlap; the overlapping regions of a size query are nobody's business
    for rows, have_dst in (([(0, 44, 0, 100), (0, 44, 100, 100), (44, 44, 50, 0), (88, 0, DST, 0)], True), ([(0, 44, 0, 100)] * 2, False)):
        arr = _items(p, rows)
        assert L.fourmc_gpu_bstreams_decompress(images.ctypes.data, IMAGES, dst.ctypes.data if have_dst else None, DST, LZ4,
                                                C.cast(arr, C.c_void_p), len(rows), None) == ENODEV
        _untouched(arr, rows)
    # the Python entry points: host tensors are refused before any call; with the check bypassed the library's codes surface
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.decompress_bstreams(torch.zeros(64, dtype=torch.uint8), [(0, 44, 0, 10)], None)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_bstream(torch.zeros(64, dtype=torch.uint8), torch.zeros(4096, dtype=torch.uint8))
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    big = torch.zeros(CAP, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstream_compress failed \(-1\)"):
        p.compress_bstream(torch.zeros(SRC, dtype=torch.uint8), big, *p.bstream_codec(".zstd_uc"), group_bytes=1000)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstream_compress failed \(-3\)"):
        p.compress_bstream(torch.zeros(SRC, dtype=torch.uint8), big[:100], group_bytes=1000)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstream_decompress failed \(-1\)"):
        p.decompress_bstream(big, torch.zeros(DST, dtype=torch.uint8), p.CODEC_ZSTD)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstreams_decompress failed \(-1\)"):
        p.decompress_bstreams(torch.zeros(IMAGES, dtype=torch.uint8), GOOD, torch.zeros(DST, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstreams_decompress failed \(-3\)"):
        p.decompress_bstreams(torch.zeros(IMAGES, dtype=torch.uint8), [(0, 44, 0, 10), (44, 44, 5, 10)], torch.zeros(DST, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="beyond the tensor"):
        p.decompress_bstreams(torch.zeros(IMAGES, dtype=torch.uint8), GOOD, None, images_bytes=IMAGES + 1)
