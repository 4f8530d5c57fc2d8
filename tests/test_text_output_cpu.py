"""CPU: the writer rule of the line writers (tests/text_output_model.py) held against the stream models, and every argument the
three entry points refuse on the host - fourmc_gpu_lines_pack, _images_write_lines, _bstreams_write_lines - through ctypes with host
memory behind the pointers: every refused call returns before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import fourmc_stream_model as fm
import helpers
import lines_model as lm
import text_output_model as tm

M = tm.M
OK, ENODEV, EINVAL, EUNSUP = 0, -1, -3, -5
NAMES = ("fourmc_gpu_lines_pack", "fourmc_gpu_images_write_lines", "fourmc_gpu_bstreams_write_lines")
_MEMO = {}


def case(name):
    """(texts, data, write sizes, the closed-form image with its block offsets and lengths) of a cut case, .4mc level 1"""
    if name not in _MEMO:
        texts = tm.lines_of(tm.cut_lengths()[name])
        data, sizes = tm.schedule(texts)
        _MEMO[name] = (texts, data, sizes, tm.image(texts, fm.compressor(fm.MAGIC_4MC, 1), fm.MAGIC_4MC))
    return _MEMO[name]


CUTS = list(tm.cut_lengths())


# ---- the rule -------------------------------------------------------------------------------------------------------------------
def test_schedule_is_text_then_newline():
    data, sizes = tm.schedule([b"ab", b"", b"c\rd"])
    assert data == b"ab\n\nc\rd\n" and sizes == [2, 1, 0, 1, 3, 1]
    assert tm.schedule([]) == (b"", [])
    for name in CUTS:
        texts, data, sizes, _ = case(name)
        assert len(sizes) == 2 * len(texts) and sum(sizes) == len(data) == sum(len(t) for t in texts) + len(texts)
        assert not texts or data.endswith(b"\n")


def test_block_cuts_of_the_cut_cases():
    want = {"[M-1]": [M], "[M]": [M, 1], "[M+1]": [M, 1, 1], "[M-2, 5]": [M - 1, 6], "[0, 0, 3, 0]": [7], "no line": []}
    for name, blocks in want.items():
        assert fm.cuts(case(name)[2]) == blocks, name
    many = fm.cuts(case("70000 lines")[2])
    assert len(many) == 2 and many[0] <= M and sum(many) == len(case("70000 lines")[1])
    assert case("[M]")[3][0][case("[M]")[3][1][1] + 12:][:1] == b"\n"           # the second block of [M] is stored: "\n"


@pytest.mark.parametrize("name", CUTS)
def test_stream_fed_write_by_write_gives_the_closed_form(name):
    texts, data, sizes, (img, offs, lens, stored) = case(name)
    assert fm.write_image(data, sizes, fm.compressor(fm.MAGIC_4MC, 1), fm.MAGIC_4MC) == img
    if not texts:
        assert len(img) == 44


@pytest.mark.parametrize("name", CUTS)
def test_parsed_blocks_decode_to_the_data(name):
    texts, data, sizes, (img, offs, lens, stored) = case(name)
    got = b""
    for (p, u, c, x), off, k, st in zip(fm.parse(img), offs, lens, stored):
        assert (p, u) == (off, k) and (c == u) == st
        payload = np.frombuffer(img[p + 12:p + 12 + c], np.uint8)
        if st:
            got += payload.tobytes()
        else:
            r, back = helpers.orc_decompress(payload, u)
            assert r == u
            got += back[:u].tobytes()
    assert got == data


@pytest.mark.parametrize("name", CUTS)
def test_lines_model_reads_back_the_written_lines(name):
    texts, data, sizes, (img, offs, lens, stored) = case(name)
    n = len(img)
    model = lm.Model(np.frombuffer(data, np.uint8), offs, lens, n - 12 - 20 - 4 * len(offs))
    w = model.lines(0, n)
    assert w["result"] == len(texts) and w["data_bytes"] == len(data)
    assert list(w["text_len"]) == [len(t) for t in texts]
    assert list(w["starts"]) == list(np.concatenate([[0], np.cumsum([len(t) + 1 for t in texts])]).astype(np.int64))


def test_verdicts_from_lists():
    tl, st = [3, 0, 5, 0x80000000, 4], [0, 3, 3, 0, 6]
    assert tm.verdict(10, tl, st, 0, [0, 1, 2]) == (tm.OK, 11)
    assert tm.verdict(10, tl, st, 0, [4]) == (tm.OK, 5) and tm.verdict(9, tl, st, 0, [4]) == (tm.LINE, 0)
    assert tm.verdict(10, tl, st, 0, [0, 5]) == (tm.LINE, 0) and tm.verdict(10, tl, st, 0, [5, 3]) == (tm.WRITE, 0)
    assert tm.verdict(10, tl, st, 0, [2, 2, 0], cap=15) == (tm.CAP, 16) and tm.verdict(10, tl, st, 0, [2, 2, 0], cap=16) == (tm.OK, 16)
    assert tm.verdict(48, [24, 25], None, 24, [0]) == (tm.OK, 25) and tm.verdict(48, [24, 25], None, 24, [1]) == (tm.LINE, 0)
    assert tm.verdict(0, [], None, 0, []) == (tm.OK, 0)


# ---- the symbols ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(helpers.ROOT, "include", "fourmc_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(raw, name) is not None, name
        assert name in p.exported_symbols(), name
    assert p.BSTREAM_WRITE_REASONS[4] == "LINE" and re.search(r"FOURMC_BSW_LINE\s*=\s*4\b", text)
    assert C.sizeof(p.LinesSrc) == 64 and C.sizeof(p.LinesPackItem) == 56 and C.sizeof(p.LinesWrItem) == 72
    assert p.LinesPackItem.reason.offset == 40 and p.LinesPackItem.packed_bytes.offset == 48
    assert p.LinesWrItem.reason.offset == 32 and p.LinesWrItem.text_bytes.offset == 40 and p.LinesWrItem.stored_blocks.offset == 64
    for f in (p.pack_lines, p.write_lines_images, p.write_lines_bstreams, p.LinesSource):
        assert callable(f)
    for part in ("Makefile", "kernels.h"):
        assert "lines_pack" in open(os.path.join(helpers.ROOT, "4mc_amd", "csrc", part)).read(), part


# ---- arguments ------------------------------------------------------------------------------------------------------------------
TEXT, LINES, PICKS, PACKED, WRITES, IMG = 4096, 64, 32, 8192, 256, 8192
MAGIC, LZ4, ZSTD = 0x344D4300, 0, 3
W = 2 ** 64


class Buffers:
    """host memory behind every pointer: no case gets as far as reading or writing it"""
    def __init__(self):
        self.text = np.zeros(TEXT, np.uint8)
        self.starts = np.zeros(LINES, np.uint64)
        self.tlen = np.zeros(LINES, np.uint32)
        self.pick = np.zeros(PICKS, np.uint64)
        self.packed = np.zeros(PACKED, np.uint8)
        self.writes = np.zeros(WRITES, np.uint32)
        self.img = np.zeros(IMG, np.uint8)


BUF = Buffers()


def _src(p, text=True, starts=True, tlen=True, pick=False, text_bytes=TEXT, row_bytes=0, table_lines=LINES, pick_total=PICKS):
    at = lambda a, given: a.ctypes.data if given else None
    return p.LinesSrc(at(BUF.text, text), text_bytes, at(BUF.starts, starts), row_bytes, at(BUF.tlen, tlen), table_lines,
                      at(BUF.pick, pick), pick_total)


PACK_FIELDS = ("line_off", "n_lines", "packed_off", "packed_cap", "writes_off")
WR_FIELDS = ("line_off", "n_lines", "image_off", "image_cap")
SENTINEL = 0x5A


def _call(p, which, rows, src=True, items=True, out=True, writes=True, n=None, kind=None, level=1, **src_kw):
    """(return code, message, the items' bytes before, after) of one call of `which` (0 pack, 1 images, 2 bstreams)"""
    cls, fields = (p.LinesPackItem, PACK_FIELDS) if which == 0 else (p.LinesWrItem, WR_FIELDS)
    arr = (cls * max(len(rows), 1))()
    C.memset(arr, SENTINEL, C.sizeof(arr))
    for i, row in enumerate(rows):
        for f, v in zip(fields, row):
            setattr(arr[i], f, v)
    before = bytes(arr)
    s = _src(p, **src_kw)
    sp = C.byref(s) if src else None
    ip = C.cast(arr, C.c_void_p) if items else None
    cnt = len(rows) if n is None else n
    L = p.lib()
    if which == 0:
        rc = L.fourmc_gpu_lines_pack(sp, BUF.packed.ctypes.data if out else None, PACKED, BUF.writes.ctypes.data if writes else None, WRITES, ip, cnt, None)
    elif which == 1:
        rc = L.fourmc_gpu_images_write_lines(sp, BUF.img.ctypes.data if out else None, IMG, MAGIC if kind is None else kind, level, ip, cnt, None)
    else:
        rc = L.fourmc_gpu_bstreams_write_lines(sp, BUF.img.ctypes.data if out else None, IMG, LZ4 if kind is None else kind, level, ip, cnt, None)
    return rc, L.fourmc_gpu_last_error().decode(), before, bytes(arr)


CALLS = ("lines_pack", "images_write_lines", "bstreams_write_lines")


def _row(which, line_off, n_lines, off, cap, writes_off=0):
    return (line_off, n_lines, off, cap, writes_off) if which == 0 else (line_off, n_lines, off, cap)


# (name, rows(which), keywords, the item the message names or None)
def _refusals(which):
    R = lambda *a, **k: _row(which, *a, **k)
    good = R(0, 4, 0, 1000)
    cases = [
        ("null lines description", [good], dict(src=False), None),
        ("null items", [good], dict(items=False), None),
        ("null text with text_bytes", [good], dict(text=False), None),
        ("null text_len with table lines", [good], dict(tlen=False), None),
        ("neither starts nor row_bytes", [good], dict(starts=False, row_bytes=0), None),
        ("rows beyond the text", [good], dict(starts=False, row_bytes=65), None),
        ("rows times stride overflows", [good], dict(starts=False, row_bytes=0xFFFFFFFF, table_lines=1 << 40), None),
        ("lines start beyond the tables", [good, R(LINES + 1, 0, 1000, 10)], {}, 1),
        ("lines end beyond the tables", [good, R(LINES - 3, 4, 1000, 10, 8)], {}, 1),
        ("line_off + n_lines wraps", [R(8, W - 4, 0, 1000)], {}, 0),
        ("lines beyond the pick, inside the tables", [good, R(PICKS - 1, 2, 1000, 10, 8)], dict(pick=True), 1),
        ("a pick of no entries", [R(0, 1, 0, 1000)], dict(pick=True, pick_total=0), 0),
        ("region starts beyond the buffer", [R(0, 4, PACKED + 1, 0)], {}, 0),
        ("region ends beyond the buffer", [good, R(4, 4, PACKED - 99, 100, 8)], {}, 1),
        ("off + cap wraps", [R(0, 4, 16, W - 8)], {}, 0),
        ("regions overlap by one byte", [R(0, 4, 100, 100), R(4, 4, 0, 101, 8)], {}, None),
        ("the same region twice", [R(0, 4, 64, 64), R(4, 4, 64, 64, 8)], {}, None),
        ("one region inside another", [R(0, 4, 0, 1000), R(4, 4, 2000, 100, 8), R(8, 4, 300, 200, 16)], {}, None),
    ]
    if which == 0:
        cases += [
            ("null write table", [good], dict(writes=False), 0),
            ("write slice starts beyond the table", [R(0, 0, 0, 10, WRITES + 1)], {}, 0),
            ("write slice ends beyond the table", [good, R(4, 4, 1000, 10, WRITES - 7)], {}, 1),
            ("writes_off + 2 n_lines wraps", [R(0, 4, 0, 10, W - 4)], {}, 0),
            ("write slices overlap by one entry", [R(0, 4, 0, 100, 0), R(4, 4, 100, 100, 7)], {}, None),
        ]
    elif which == 1:
        cases += [("a magic that is neither", [good], dict(kind=0x12345678), None),
                  ("two faults, the magic and null items", [good], dict(kind=0x12345678, items=False), None)]
    else:
        cases += [("a codec that is none", [good], dict(kind=9), None),
                  ("two faults, the codec and null items", [good], dict(kind=9, items=False), None)]
    return cases


REFUSED = [(which, *c) for which in range(3) for c in _refusals(which)]


@pytest.mark.parametrize("which,name,rows,kw,item", REFUSED, ids=["%s: %s" % (CALLS[c[0]], c[1]) for c in REFUSED])
def test_refused_on_the_host_with_items_untouched(which, name, rows, kw, item):
    rc, msg, before, after = _call(helpers.pkg(), which, rows, **kw)
    assert rc == EINVAL, (rc, msg)
    assert after == before, "items were written"
    assert msg.startswith(CALLS[which] + ": "), msg
    if item is not None:
        assert re.search(r"\b(item|stream) %d\b" % item, msg), msg


def test_zstd_level_not_on_the_device_is_unsupported():
    rc, msg, before, after = _call(helpers.pkg(), 2, [(0, 4, 0, 1000)], kind=ZSTD, level=13)
    assert rc == EUNSUP and "level 13" in msg and after == before


@pytest.mark.parametrize("which", range(3), ids=CALLS)
def test_nothing_to_do_is_ok_whatever_else_is_null(which):
    rc, msg, before, after = _call(helpers.pkg(), which, [], src=False, items=False, out=False, writes=False, n=0)
    assert rc == OK and after == before


ACCEPTED = [
    ("regions that touch, empty regions anywhere", lambda R: [R(0, 4, 0, 100), R(4, 4, 100, 100, 8), R(8, 0, 50, 0, 16), R(LINES, 0, PACKED, 0, WRITES)], {}),
    ("the size query looks at no region and no write slice", lambda R: [R(0, 4, 0, 100), R(4, 4, 50, 100, 0), R(8, 4, PACKED + 1, W - 1, WRITES + 1)], dict(out=False, writes=False)),
    ("the row layout up to the last byte", lambda R: [R(0, LINES, 0, 4000)], dict(starts=False, row_bytes=64)),
    ("lines through a pick, up to its last entry",lambda R: [R(PICKS - 4, 4, 0, 1000)], dict(pick=True)),
    ("no text at all and no line", lambda R: [R(0, 0, 0, 0)], dict(text=False, tlen=False, starts=False, text_bytes=0, table_lines=0)),
]


@pytest.mark.skipif(torch.cuda.is_available(), reason="a well-formed call would run on the device with host pointers")
@pytest.mark.parametrize("which", range(3), ids=CALLS)
@pytest.mark.parametrize("name,rows,kw", ACCEPTED, ids=[c[0] for c in ACCEPTED])
def test_what_the_checks_accept_ends_at_the_device_check(which, name, rows, kw):
    rc, msg, before, after = _call(helpers.pkg(), which, rows(lambda *a, **k: _row(which, *a, **k)), **kw)
    assert rc == ENODEV and after == before, (rc, msg)
