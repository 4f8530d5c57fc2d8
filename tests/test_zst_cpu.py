""".zst streams, host side: the shapes of the GPU test's inputs (tests/zst_model.py) as the inspector sees them, the model's walk
against the reference's own frame walk and decoder, the argument checks of both calls without a device, the exported symbols."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers
import zst_model as zm
import zstd_shapes as zs

needs_ref = pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not present")
OK, EINVAL, ENODEV = 0, -3, -1
LONG1, LONG3 = f"A:l1:{zm.A_SIZES[-1]}", f"A:l3:{zm.A_SIZES[-1]}"


@needs_ref
def test_ledger_of_the_input_shapes():
    """What each input is there for, read back from its bytes: if the reference (or the corpus) changed what it writes, this
    fails before the GPU test runs on inputs that no longer have their shape."""
    I = zm.inputs()
    W = {k: zm.walk(v[0]) for k, v in I.items()}
    R = {k: zm.reach(v[0]) for k, v in I.items()}
    L = {k: zs.inspect(v[0])[0] for k, v in I.items()}
    assert all(w["ok"] for w in W.values())
    # A: one frame, no content size, no checksum, not single-segment; the windowLog of the level; full blocks closed by an empty
    # raw last block; the empty stream is the 9-byte frame
    for k in I:
        if not k.startswith("A:"): continue
        img = I[k][0]
        assert (W[k]["frames"], W[k]["skippable"]) == (1, 0), k
        assert img[4] == 0, (k, img[4])                                  # Frame_Header_Descriptor: nothing set
        assert L[k]["hdr:fcs:0"] == 1 and L[k]["hdr:single:0"] == 1 and not L[k]["hdr:checksum"], k
    assert len(I["A:l1:0"][0]) == 9 and W["A:l1:0"]["blocks"] == 1
    assert (I[LONG1][0][5] >> 3) + 10 == 19 and (I[LONG3][0][5] >> 3) + 10 == 21
    assert W["A:l1:131072"]["blocks"] == 2 and W["A:l1:131073"]["blocks"] == 2
    for k in (LONG1, LONG3):
        tab = zm.block_table(I[k][0])
        assert len(tab) == 71 and tab[70]["type"] == 0 and tab[70]["size"] == 0, k
        assert all(e["type"] == 2 for e in tab[:70]), k
    assert R[LONG1]["treeless_all"] == 53 and R[LONG1]["treeless"] == 6         # 6 treeless blocks read a table of the first group of 64
    assert R[LONG3]["treeless_all"] == 10
    # B: 200 blocks in one frame, one Huffman table for all of them
    assert W["B:flush1300"]["blocks"] == 200 and R["B:flush1300"]["treeless_all"] == 199 and R["B:flush1300"]["treeless"] == 136
    # C: many small blocks; Repeat-mode tables of each kind and treeless blocks reach across a group of 64
    assert W["C:pledged"]["blocks"] == 274 and W["C:streamed"]["blocks"] == 275
    for k in ("C:pledged", "C:streamed"):
        assert R[k] == {"treeless": 210, "ll": 48, "of": 48, "ml": 48, "treeless_all": 272}, (k, R[k])
    assert L["C:pledged"]["hdr:fcs:0"] == 0 and L["C:streamed"]["hdr:fcs:0"] == 1
    # D: matches 4.75 MiB back, beyond 22 bits; 38 raw blocks among the 40; once with a checksum
    for k in ("D:far", "D:far:checksum"):
        assert W[k]["blocks"] == 40 and L[k]["block:raw"] == 38, k
    assert L["D:far:checksum"]["hdr:checksum"] == 1 and not L["D:far"]["hdr:checksum"]
    assert len(I["D:far"][1]) - (256 << 10) > 1 << 22
    # E: A's long frame, a skippable frame, a one-shot frame with a content size, a checksum frame, the empty frame
    assert (W["E:concat"]["frames"], W["E:concat"]["skippable"], W["E:concat"]["blocks"]) == (4, 1, 77)
    assert len(zm.e_parts()) == 6 and L["E:concat"]["hdr:checksum"] == 1 and L["E:concat"]["multiframe"] == 1
    # F: RLE blocks
    assert L["F:rle"]["block:rle"] == 22 and W["F:rle"]["blocks"] == 23
    # B and C cross rounds of 64 and of 100 entries inside their frame
    assert W["B:flush1300"]["blocks"] > 100 and W["C:streamed"]["blocks"] > 100


@needs_ref
def test_model_walk_equals_the_reference():
    """Frame by frame the walk ends where ZSTD_findFrameCompressedSize says, and the sizes are ZSTD_decompress's."""
    for k, (img, src) in zm.inputs().items():
        w = zm.walk(img)
        at, frames, skips = 0, 0, 0
        while at < len(img):
            n = zm.find_frame_size(img, at)
            assert n > 0, (k, at)
            if int.from_bytes(img[at:at + 4], "little") & 0xFFFFFFF0 == 0x184D2A50: skips += 1
            else:
                assert w["spans"][frames][:2] == (at, at + n), (k, frames)
                frames += 1
            at += n
        assert (frames, skips, at) == (w["frames"], w["skippable"], len(img)) and w["fail_offset"] == len(img), k
        r, out = zm.ref_decode(img, len(src))
        assert r == len(src) and out == src, k
        e = zm.expect(img, len(src))
        assert e["ok"] and e["decoded"] == len(src) and e["data"] == src, k


@needs_ref
def test_every_damage_class_has_a_case_the_reference_rejects():
    I = zm.inputs()
    seen = {}
    for cls, label, img, base in zm.damaged():
        cap = len(I[base][1])
        r, _ = zm.ref_decode(img, cap)
        e = zm.expect(img, cap)
        assert e["ok"] == (r >= 0), label                                # the frame-by-frame model agrees with the whole-file call
        if r >= 0: assert e["decoded"] == r, label
        seen.setdefault(cls, []).append(r < 0)
    assert set(seen) == {"trunc_frame", "trunc_block", "magic", "block_type", "huffman", "sequences", "cut_block0", "checksum", "trailing"}
    assert all(any(v) for v in seen.values()), seen
    assert all(seen["trunc_block"]) and all(seen["trailing"]) and all(seen["checksum"])


@needs_ref
def test_committed_fixture_is_what_the_reference_writes():
    built, have = zm.fixture_build(), zm.fixture()
    for n in zm.FIXTURES:
        assert have[n][0] == built[n], n
        r, out = zm.ref_decode(have[n][0], len(have[n][1]))
        assert r == len(have[n][1]) and out == have[n][1], n


def test_committed_fixture_shapes():
    """Without the reference: the committed files have the shapes the GPU test relies on."""
    F = zm.fixture()
    for n in zm.FIXTURES: assert os.path.getsize(os.path.join(zs.HERE, "golden", n)) < (1 << 20)
    w = zm.walk(F["zst_small.zst"][0])
    assert (w["ok"], w["frames"], w["skippable"], w["blocks"]) == (True, 3, 1, 203)
    assert zm.reach(F["zst_small.zst"][0])["treeless"] == 136
    w = zm.walk(F["zst_blocks.zst"][0])
    assert (w["ok"], w["frames"], w["blocks"]) == (True, 1, 275)
    assert zm.reach(F["zst_blocks.zst"][0]) == {"treeless": 210, "ll": 48, "of": 48, "ml": 48, "treeless_all": 272}


def test_model_walk_on_damage_without_the_reference():
    img = zm.fixture()["zst_small.zst"][0]
    spans = zm.walk(img)["spans"]
    for k, (start, end, b0, nb, sk) in enumerate(spans):
        for cut in (start + 1, start + 8, end - 1):
            w = zm.walk(img[:cut])
            assert (w["ok"], w["fail_offset"], w["frames"], w["blocks"], w["skippable"]) == (False, start, k, b0, sk), (k, cut)
    assert zm.walk(img + b"\0")["fail_offset"] == len(img) and zm.walk(b"")["ok"]


# ---------------------------------------------------------------------------------------------- the C ABI
NEW_SYMBOLS = ("fourmc_gpu_zst_decompress", "fourmc_gpu_zsts_decompress", "fourmc_gpu_zst_reason_text", "fourmc_gpu_zst_stats",
               "fourmc_gpu_set_zst_round_blocks", "fourmc_gpu_get_zst_round_blocks")


def test_new_symbols_are_exported_by_both_libraries():
    p = helpers.pkg()
    for path in (p.lib_path(), p.research_lib_path()):
        L = C.CDLL(path)
        for s in NEW_SYMBOLS: assert hasattr(L, s), (path, s)
    assert p.ZST_REASONS == ("OK", "FRAME", "DST_SMALL")
    L = p.lib()
    assert [L.fourmc_gpu_zst_reason_text(i) for i in range(4)] == [b"", b"zstd : frame decoding failed", b"Destination buffer too small", b"unknown"]
    assert C.sizeof(p.ZstStatus) == 48 and C.sizeof(p.ZstItem) == 80


IMAGES, DST = 4096, 8192
BAD_ROWS = {
    "image beyond the buffer": [(0, 100, 0, 100), (IMAGES - 10, 11, 200, 100)],
    "image offset beyond the buffer": [(IMAGES + 1, 0, 0, 100)],
    "image length wraps": [(8, 2 ** 64 - 4, 0, 100)],
    "region beyond the destination": [(0, 100, DST - 10, 11)],
    "region offset beyond the destination": [(0, 100, DST + 1, 0)],
    "regions overlap": [(0, 100, 0, 100), (100, 100, 99, 100)],
    "regions overlap, given out of order": [(0, 100, 500, 100), (0, 100, 0, 100), (0, 100, 450, 51)],
}


def _items(p, rows):
    arr = (p.ZstItem * max(len(rows), 1))()
    for i, (io, ib, do, dc) in enumerate(rows):
        arr[i].image_off, arr[i].image_bytes, arr[i].dst_off, arr[i].dst_cap = io, ib, do, dc
        arr[i].status.reason = 66
    return arr


@pytest.mark.parametrize("name", sorted(BAD_ROWS))
def test_many_streams_argument_errors_are_einval_before_any_device(name):
    p = helpers.pkg()
    L = p.lib()
    images, dst = np.zeros(IMAGES + 64, np.uint8), np.zeros(DST, np.uint8)
    rows = BAD_ROWS[name]
    arr = _items(p, rows)
    rc = L.fourmc_gpu_zsts_decompress(images.ctypes.data, IMAGES, dst.ctypes.data, DST, C.cast(arr, C.c_void_p), len(rows), None)
    assert rc == EINVAL, (name, rc)
    assert L.fourmc_gpu_last_error()
    assert all(arr[i].status.reason == 66 for i in range(len(rows))) and not dst.any()


def test_null_pointers_are_einval_and_no_items_is_ok():
    p = helpers.pkg()
    L = p.lib()
    images, dst = np.zeros(IMAGES + 64, np.uint8), np.zeros(DST, np.uint8)
    assert L.fourmc_gpu_zsts_decompress(images.ctypes.data, IMAGES, dst.ctypes.data, DST, None, 3, None) == EINVAL
    arr = _items(p, [(0, 100, 0, 100)])
    assert L.fourmc_gpu_zsts_decompress(None, IMAGES, dst.ctypes.data, DST, C.cast(arr, C.c_void_p), 1, None) == EINVAL
    assert arr[0].status.reason == 66
    assert L.fourmc_gpu_zsts_decompress(None, 0, None, 0, None, 0, None) == OK
    assert L.fourmc_gpu_zsts_decompress(images.ctypes.data, IMAGES, dst.ctypes.data, DST, C.cast(arr, C.c_void_p), 0, None) == OK
    st = p.ZstStatus()
    st.reason = 66
    assert L.fourmc_gpu_zst_decompress(images.ctypes.data, 64, dst.ctypes.data, 64, None, None) == EINVAL
    assert L.fourmc_gpu_zst_decompress(None, 64, dst.ctypes.data, 64, C.byref(st), None) == EINVAL
    assert st.reason == 66 and not dst.any()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_well_formed_calls_fail_with_enodev():
    p = helpers.pkg()
    L = p.lib()
    images, dst = np.zeros(IMAGES + 64, np.uint8), np.zeros(DST, np.uint8)
    # regions that touch or are empty do not overlap; two items may name the same image bytes; a size query looks at no region
    for rows, have_dst in (([(0, 44, 0, 100), (0, 44, 100, 100), (44, 44, 50, 0), (88, 0, DST, 0)], True), ([(0, 44, 0, 100)] * 2, False)):
        arr = _items(p, rows)
        rc = L.fourmc_gpu_zsts_decompress(images.ctypes.data, IMAGES, dst.ctypes.data if have_dst else None, DST, C.cast(arr, C.c_void_p), len(rows), None)
        assert rc == ENODEV, rc
        assert all(arr[i].status.reason == 66 for i in range(len(rows)))
    st = p.ZstStatus()
    st.reason = 66
    assert L.fourmc_gpu_zst_decompress(images.ctypes.data, IMAGES, dst.ctypes.data, DST, C.byref(st), None) == ENODEV
    assert L.fourmc_gpu_zst_decompress(None, 0, None, 0, C.byref(st), None) == ENODEV
    assert st.reason == 66 and not dst.any()
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.decompress_zst(torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.decompress_zsts(torch.zeros(64, dtype=torch.uint8), [(0, 44, 0, 10)], None)
