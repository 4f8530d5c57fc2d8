"""The write side of .zst streams without a GPU: the inputs of tests/zst_write_model.py reach what they are there for on the
reference, the committed fixture is what the reference writes, the reference's bytes do not depend on how its input is cut, and the
host side of fourmc_gpu_zsts_compress (bound, level mapping, exports, argument errors)."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
import zst_model as zm
import zst_write_model as wm

OK, EINVAL, ENODEV = 0, -3, -1
needs_ref = pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref is not built (no reference tree)")


# ---------------------------------------------------------------------------------------------- model and reference
def test_every_required_input_exists():
    assert set(wm.REQUIRED) == set(wm.inputs()) and len(set(wm.REQUIRED)) == len(wm.REQUIRED)
    assert set(wm.fixture()) == set(wm.REQUIRED)


@needs_ref
@pytest.mark.parametrize("name", wm.REQUIRED)
def test_reference_reaches_what_the_input_is_for(name):
    assert wm.reached(name, wm.reference()[name]), name


@needs_ref
def test_fixture_is_what_the_reference_writes_now():
    assert wm.fixture() == wm.fixture_build()


@needs_ref
@pytest.mark.parametrize("level", (1, 3))
@pytest.mark.parametrize("which", ("G", "P"))
def test_reference_bytes_do_not_depend_on_the_pieces(which, level):
    src = wm.inputs()[f"G:l{level}:R+B" if which == "G" and level == 1 else "G:l3:2R+B+5" if which == "G" else f"P:l{level}:b"][0]
    if which == "G": src = src[:wm.ring(level) + wm.B]
    want = zm.zstcodec(src, level)
    for pieces in ((131072,), (131071, 131073), (4093,)):        # Java's iBuffSize; one byte off either way; small pieces
        assert wm.chunked(src, level, pieces) == want, pieces


@needs_ref
@pytest.mark.parametrize("name", wm.REQUIRED)
def test_reference_image_decodes_to_its_source(name):
    src = wm.inputs()[name][0]
    r, out = zm.ref_decode(wm.reference()[name], len(src))
    assert r == len(src) and out == src.tobytes()


def test_modes_against_a_direct_statement():
    B = wm.B
    for level, m in ((1, 5), (2, 9), (3, 17), (4, 17)):
        assert wm.ring(level) == m * B
        for n in (0, 1, B, m * B - 1, m * B, m * B + 1, m * B + B, 2 * m * B + 1, 2 * m * B + B + 5, 3 * m * B + 7):
            want = [k >= m and k % m != m - 1 for k in range(-(-n // B))]
            assert wm.modes(n, level) == want, (level, n)
    got = wm.modes(2 * wm.ring(1) + 1, 1)
    assert got[:5] == [False] * 5 and got[5] and got == [False] * 5 + [True] * 4 + [False, True]
    for name, count in wm.EXT_BLOCKS.items():
        src, level = wm.inputs()[name]
        assert sum(wm.modes(len(src), level)) == count, name


@needs_ref
def test_geometry_constants_are_the_reference_rows():
    class CParams(C.Structure):
        _fields_ = [(n, C.c_uint) for n in ("windowLog", "chainLog", "hashLog", "searchLog", "minMatch", "targetLength", "strategy")]
    f = helpers.ref().ZSTD_getCParams
    f.restype, f.argtypes = CParams, [C.c_int, C.c_ulonglong, C.c_size_t]
    for level, strat in ((1, 1), (2, 1), (3, 2), (4, 2)):
        cp = f(level, 0, 0)
        assert (1 << cp.windowLog, cp.strategy) == (wm.WINDOW[level], strat), level


# ---------------------------------------------------------------------------------------------- the C ABI
NEW_SYMBOLS = ("fourmc_gpu_zst_bound", "fourmc_zst_codec_level", "fourmc_gpu_zst_compress", "fourmc_gpu_zsts_compress", "fourmc_gpu_zstw_reason_text")


def test_new_symbols_are_exported_by_both_libraries():
    p = helpers.pkg()
    for path in (p.lib_path(), p.research_lib_path()):
        L = C.CDLL(path)
        for s in NEW_SYMBOLS: assert hasattr(L, s), (path, s)
    for s in NEW_SYMBOLS: assert s in p.exported_symbols(), s
    assert p.ZSTW_REASONS == ("OK", "DST_SMALL", "LEVEL", "TOO_LONG")
    L = p.lib()
    assert [L.fourmc_gpu_zstw_reason_text(i) for i in range(5)] == [b"", b"Destination buffer too small", b"zstd : level not written on the device (1 to 4 are)",
                                                                    b"zstd : source beyond 3 GiB", b"unknown"]
    assert C.sizeof(p.ZstwStatus) == 24 and C.sizeof(p.ZstwItem) == 64
    for name in ("compress_zst", "compress_zsts", "zst_bound", "zst_codec_level", "ZSTW_REASONS"): assert hasattr(p, name), name


def test_bound_and_codec_level():
    p = helpers.pkg()
    B = wm.B
    for n in (0, 1, B - 1, B, B + 1, 5 * B, 0xC0000000):
        assert p.zst_bound(n) == 6 + n + 3 * (n // B + 1), n
    assert [p.zst_codec_level(v) for v in (0, -5, 1, 22, 23, 100)] == [3, 3, 1, 22, 3, 3]
    assert [p.zst_codec_level(v) for v in range(1, 23)] == list(range(1, 23))


@needs_ref
def test_bound_holds_the_reference_images():
    p = helpers.pkg()
    for name, img in wm.reference().items():
        assert len(img) <= p.zst_bound(len(wm.inputs()[name][0])), name
    bg = wm.background()
    assert len(zm.zstcodec(bg, 1)) == p.zst_bound(len(bg))           # every block raw: the bound is exact


SRC, IMAGES = 4096, 8192
BAD_ROWS = {
    "source beyond the buffer": [(0, 100, 0, 200, 1), (SRC - 10, 11, 200, 200, 1)],
    "source offset beyond the buffer": [(SRC + 1, 0, 0, 200, 1)],
    "source ends beyond the buffer": [(SRC - 4, 8, 0, 200, 1)],
    "region beyond the images": [(0, 100, IMAGES - 10, 11, 1)],
    "region offset beyond the images": [(0, 100, IMAGES + 1, 0, 1)],
    "region length wraps": [(0, 100, 8, 2 ** 64 - 4, 1)],
    "regions overlap": [(0, 100, 0, 200, 1), (100, 100, 199, 200, 3)],
    "regions overlap, given out of order": [(0, 100, 500, 100, 1), (0, 100, 0, 100, 2), (0, 100, 450, 51, 4)],
    "a refused item's region still counts": [(0, 100, 0, 200, 7), (0, 100, 100, 200, 1)],
}


def _items(p, rows):
    arr = (p.ZstwItem * max(len(rows), 1))()
    for i, (so, sb, io, ic, lv) in enumerate(rows):
        arr[i].src_off, arr[i].src_bytes, arr[i].image_off, arr[i].image_cap, arr[i].level = so, sb, io, ic, lv
        arr[i].status.reason = 66
    return arr


@pytest.mark.parametrize("name", sorted(BAD_ROWS))
def test_many_streams_argument_errors_are_einval_before_any_device(name):
    p = helpers.pkg()
    L = p.lib()
    src, images = np.zeros(SRC + 64, np.uint8), np.zeros(IMAGES, np.uint8)
    rows = BAD_ROWS[name]
    arr = _items(p, rows)
    rc = L.fourmc_gpu_zsts_compress(src.ctypes.data, SRC, images.ctypes.data, IMAGES, C.cast(arr, C.c_void_p), len(rows), None)
    assert rc == EINVAL, (name, rc)
    assert L.fourmc_gpu_last_error()
    assert all(arr[i].status.reason == 66 for i in range(len(rows))) and not images.any()


def test_null_pointers_are_einval_and_no_items_is_ok():
    p = helpers.pkg()
    L = p.lib()
    src, images = np.zeros(SRC + 64, np.uint8), np.zeros(IMAGES, np.uint8)
    assert L.fourmc_gpu_zsts_compress(src.ctypes.data, SRC, images.ctypes.data, IMAGES, None, 3, None) == EINVAL
    arr = _items(p, [(0, 100, 0, 200, 1)])
    assert L.fourmc_gpu_zsts_compress(None, SRC, images.ctypes.data, IMAGES, C.cast(arr, C.c_void_p), 1, None) == EINVAL
    assert L.fourmc_gpu_zsts_compress(src.ctypes.data, SRC, None, IMAGES, C.cast(arr, C.c_void_p), 1, None) == EINVAL
    assert arr[0].status.reason == 66
    assert L.fourmc_gpu_zsts_compress(None, 0, None, 0, None, 0, None) == OK
    assert L.fourmc_gpu_zsts_compress(src.ctypes.data, SRC, images.ctypes.data, IMAGES, C.cast(arr, C.c_void_p), 0, None) == OK
    assert L.fourmc_gpu_zst_compress(src.ctypes.data, 64, images.ctypes.data, 200, 1, None, None) == EINVAL
    st = p.ZstwStatus()
    st.reason = 66
    assert L.fourmc_gpu_zst_compress(None, 64, images.ctypes.data, 200, 1, C.byref(st), None) == EINVAL
    assert st.reason == 66 and not images.any()


def test_refused_items_need_no_device():
    """A level outside 1 .. 4 and a source beyond 3 GiB are decided on the host: a call of nothing else never looks for a device, and
    the over-long source is only a descriptor."""
    p = helpers.pkg()
    L = p.lib()
    src, images = np.zeros(SRC + 64, np.uint8), np.zeros(IMAGES, np.uint8)
    rows = [(0, 100, 0, 200, 5), (0, 100, 200, 200, 0), (0, 100, 400, 200, 22), (0, 0xC0000001, 600, 200, 1), (0, 100, 800, 200, -1)]
    arr = _items(p, rows)
    assert L.fourmc_gpu_zsts_compress(src.ctypes.data, SRC, images.ctypes.data, IMAGES, C.cast(arr, C.c_void_p), len(rows), None) == OK
    assert [arr[i].status.reason for i in range(5)] == [2, 2, 2, 3, 2]
    assert all(arr[i].status.image_bytes == 0 and arr[i].status.codec_result == 0 for i in range(5)) and not images.any()
    st = p.ZstwStatus()
    assert L.fourmc_gpu_zst_compress(src.ctypes.data, 100, images.ctypes.data, 200, 12, C.byref(st), None) == OK and st.reason == 2


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_well_formed_calls_fail_with_enodev():
    p = helpers.pkg()
    L = p.lib()
    src, images = np.zeros(SRC + 64, np.uint8), np.zeros(IMAGES, np.uint8)
    # regions that touch or are empty do not overlap; two items may name the same source bytes; a source exactly at the limit is read
    rows = [(0, 100, 0, 200, 1), (0, 100, 200, 200, 3), (50, 0, 100, 0, 2), (SRC, 0, IMAGES, 0, 4), (0, 100, 400, 200, 9)]
    arr = _items(p, rows)
    assert L.fourmc_gpu_zsts_compress(src.ctypes.data, SRC, images.ctypes.data, IMAGES, C.cast(arr, C.c_void_p), len(rows), None) == ENODEV
    assert all(arr[i].status.reason == 66 for i in range(len(rows))) and not images.any()
    st = p.ZstwStatus()
    st.reason = 66
    assert L.fourmc_gpu_zst_compress(src.ctypes.data, 100, images.ctypes.data, 200, 1, C.byref(st), None) == ENODEV and st.reason == 66
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_zst(torch.zeros(64, dtype=torch.uint8), torch.zeros(200, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_zsts(torch.zeros(64, dtype=torch.uint8), [(0, 44, 0, 100, 1)], torch.zeros(200, dtype=torch.uint8))
