"""Lines by number (fourmc_gpu_image_line_index / _image_read_lines_at) without a GPU: the model the GPU tests compare with
(line_index_model.py) stated twice and held against lines_model.Model; the symbols declared, exported and bound; the struct sizes;
every argument check before the device check; FOURMC_ENODEV where there is no device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import helpers
import line_index_model as lim
import lines_model as lm

ROOT = helpers.ROOT
NAMES = ("fourmc_gpu_image_line_index", "fourmc_gpu_image_read_lines_at", "fourmc_gpu_image_lines_at_stats")
EINVAL, ENODEV = -3, -1


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _families(B, seed):
    rng = np.random.default_rng(seed)

    def text(n):
        return rng.choice(np.frombuffer(b"abc \n", np.uint8), n, p=[0.25, 0.25, 0.2, 0.1, 0.2]).copy()

    def noise(n):
        return rng.integers(0, 256, n, dtype=np.uint8)
    return lm.families(B, text, noise)


def _cuts(T, B, rng):
    """usizes: blocks of B bytes with a short last one, and random cuts with blocks of no bytes among them"""
    yield [B] * (T // B) + ([T % B] if T % B else [])
    cuts = sorted(int(c) for c in rng.integers(0, T + 1, int(rng.integers(1, 9)))) if T else [0, 0]
    edges = [0] + cuts + [T]
    yield [b - a for a, b in zip(edges, edges[1:])]


def _cases():
    rng = np.random.default_rng(11)
    for B in (16, 64, 4096):
        for name, data in _families(B, 100 + B).items():
            for us in _cuts(len(data), B, rng):
                yield "%s/%d" % (name, B), data, us
    alphabet = np.frombuffer(b"\r\na", np.uint8)
    for i in range(1500):                                   # every seam shape at sizes where every byte is a seam
        T = int(rng.integers(0, 40))
        data = rng.choice(alphabet, T, p=rng.dirichlet([1, 1, 1])).copy()
        for us in _cuts(T, int(rng.integers(1, 9)), rng):
            yield "random%d" % i, data, us


def test_the_two_statements_of_the_index_agree():
    n = 0
    seen = set()
    for name, data, us in _cases():
        a, la = lim.index(data, us)
        b, lb = lim.index_loop(data, us)
        assert la == lb and np.array_equal(a, b), (name, us, a, b)
        assert int(a["ends"].sum()) == int(a["ends_before"][-1]) == len(lm.line_ends(data)), name
        seen.update(int(f) & 3 for f in a["flags"])
        n += 1
    assert n > 3000 and seen == {0, 1, 2, 3}


def test_every_family_is_covered():
    assert set(_families(16, 1)) == {"crlf_text", "cr_only", "lf_only", "mixed", "all_cr", "all_lf", "alternating_crlf", "alternating_lfcr",
                                     "no_terminator", "zero_blocks", "one_block", "stored_block", "cr_at_block_end", "ends_with_crlf",
                                     "ends_with_cr", "tail_only_cr_last", "tail_only_cr_last_lf", "three_blocks"}


def test_lines_at_equals_slicing_by_the_split_model():
    rng = np.random.default_rng(12)
    checked = 0
    for name, data, us in _cases():
        if len(data) > 400:
            continue
        off, end_mark, _ = lm.layout(us, [1] * len(us))
        m = lm.Model(data, off, us, end_mark)
        starts = m.file_lines()
        lines = len(starts) - 1 if m.T else 0
        assert lines == lim.index(data, us)[1] == lim.count_lines(data), name
        ks = list(range(lines + 2)) + [int(k) for k in rng.integers(0, lines + 1, 5)] + [1 << 40]
        for row_bytes, mx, pad in ((1, lm.DEFAULT_MAX, 0), (5, lm.DEFAULT_MAX, 0x20), (64, 3, 0xEE), (7, 0, 1)):
            rows, tl, st = lim.lines_at(data, ks, row_bytes, mx, pad)
            for i, k in enumerate(ks):
                if k >= lines:
                    assert st[i] == -3 and tl[i] == 0 and (rows[i] == pad).all(), (name, k)
                    continue
                s, e = int(starts[k]), int(starts[k + 1])
                text = min(e - s - m.term_len(s, e), mx)
                c = min(text, row_bytes)
                assert st[i] == 1 and tl[i] == text, (name, k)
                assert rows[i, :c].tobytes() == data[s:s + c].tobytes() and (rows[i, c:] == pad).all(), (name, k)
                checked += 1
    assert checked > 50000


def test_needed_blocks_of_a_line_over_three_blocks():
    B = 64
    data = _families(B, 3)["three_blocks"]
    us = [B, B, B, len(data) - 3 * B]
    P = lm.line_ends(data)
    k = int(np.searchsorted(P, B // 2))                     # the line that runs from block 0 into block 2
    assert P[k] >= 2 * B and (k == 0 or P[k - 1] < B)
    s = 0 if k == 0 else int(P[k - 1]) + 1
    assert lim.needed_blocks(data, us, [k], B - s) == [0, 2]                # its first bytes end with block 0: block 1 is not staged
    assert lim.needed_blocks(data, us, [k], B - s + 1) == [0, 1, 2]
    assert lim.needed_blocks(data, us, [k], 4 * B, max_line_len=1) == [0, 2]
    assert lim.needed_blocks(data, us, [1 << 50], 8) == []


# ---- the ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    research = re.search(r"#ifdef FOURMC_RESEARCH(.*?)#endif", text, re.S).group(1)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text) and name not in research
        assert getattr(raw, name) is not None
        assert name in p.exported_symbols()
        assert "debug" not in name
    assert callable(p.image_line_index) and callable(p.image_read_lines_at) and callable(p.image_lines_at_stats)
    assert p.image_lines_at_stats() == (0, 0, 0) or torch.cuda.is_available()


def test_struct_sizes():
    p = helpers.pkg()
    assert C.sizeof(p.ImageLineEntry) == 16 and C.sizeof(p.ImageLineInfo) == 40 and C.sizeof(p.ImageLinesAt) == 32
    assert p.IMAGE_LINE_ENTRY_DTYPE.itemsize == 16 and lim.ENTRY == p.IMAGE_LINE_ENTRY_DTYPE
    assert [f for f, _ in p.ImageLineEntry._fields_] == ["ends_before", "ends", "flags"]
    assert [f for f, _ in p.ImageLineInfo._fields_] == ["result", "lines", "ends", "total_bytes", "nblocks", "pad"]
    assert [f for f, _ in p.ImageLinesAt._fields_] == ["result", "served", "blocks_staged", "rounds"]
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for s in ("fourmc_image_line_entry", "fourmc_image_line_info", "fourmc_image_lines_at"):
        assert re.search(r"typedef struct %s\b" % s, text)


class Args:
    """valid host stand-ins for every argument: the checks under test come before anything is dereferenced"""

    def __init__(self, p):
        self.img, self.index = np.zeros(64, np.uint8), np.zeros(4, lim.ENTRY)
        self.lines, self.rows = np.zeros(4, np.uint64), np.zeros(64, np.uint8)
        self.tl, self.st = np.full(4, 0x5A5A5A5A, np.uint32), np.full(4, 0x5A5A5A5A, np.int32)
        self.info, self.out = p.ImageLineInfo(), p.ImageLinesAt()
        self.info.result = self.out.result = 77
        self.L = p.lib()

    def index_call(self, **kw):
        a = dict(image=self.img.ctypes.data, index=self.index.ctypes.data, cap=4, info=C.byref(self.info))
        a.update(kw)
        return self.L.fourmc_gpu_image_line_index(a["image"], 64, a["index"], a["cap"], a["info"], None)

    def read_call(self, **kw):
        a = dict(image=self.img.ctypes.data, index=self.index.ctypes.data, lines=self.lines.ctypes.data, n=4, mx=0x7FFFFFFF,
                 rows=self.rows.ctypes.data, row_bytes=16, tl=self.tl.ctypes.data, st=self.st.ctypes.data, out=C.byref(self.out))
        a.update(kw)
        return self.L.fourmc_gpu_image_read_lines_at(a["image"], 64, a["index"], 4, a["lines"], a["n"], a["mx"], a["rows"], a["row_bytes"], 0,
                                                     a["tl"], a["st"], a["out"], None)

    def untouched(self):
        return (self.info.result == 77 and self.out.result == 77 and (self.tl == 0x5A5A5A5A).all() and (self.st == 0x5A5A5A5A).all()
                and not self.rows.any())


def test_argument_checks_come_before_the_device_check():
    p = helpers.pkg()
    a = Args(p)
    for kw in (dict(image=None), dict(info=None)):
        assert a.index_call(**kw) == EINVAL, kw
        assert b"image_line_index" in a.L.fourmc_gpu_last_error()
    for kw in (dict(image=None), dict(out=None), dict(index=None), dict(lines=None), dict(rows=None), dict(tl=None), dict(st=None),
               dict(row_bytes=0), dict(mx=0x80000000), dict(mx=0xFFFFFFFF), dict(n=0, row_bytes=0), dict(n=0, index=None)):
        assert a.read_call(**kw) == EINVAL, kw
        assert b"image_read_lines_at" in a.L.fourmc_gpu_last_error()
    assert a.untouched()
    # n * row_bytes: both are 32-bit in this ABI, so no pair of values overflows 64 bits; the largest pair passes the check
    if not torch.cuda.is_available():
        assert a.read_call(n=0xFFFFFFFF, row_bytes=0xFFFFFFFF) == ENODEV
    # no requests: nothing to do, whatever the request pointers are, and no device is looked for
    assert a.read_call(n=0, lines=None, rows=None, tl=None, st=None) == 0 and a.out.result == 0
    a.L.fourmc_gpu_image_lines_at_stats(None, None, None)    # every pointer is optional


def test_without_a_gpu_valid_arguments_meet_enodev():
    if torch.cuda.is_available():
        return
    p = helpers.pkg()
    a = Args(p)
    assert a.index_call() == ENODEV and a.index_call(index=None, cap=0) == ENODEV
    assert a.read_call() == ENODEV and a.read_call(mx=0) == ENODEV
    assert a.untouched()


def test_python_entry_points_validate_their_tensors(monkeypatch):
    p = helpers.pkg()
    img = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.image_line_index(img)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.image_read_lines_at(img, torch.zeros((2, 2), dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 16)
    if torch.cuda.is_available():
        return
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what):
        keep.append(t.numpy())
        return keep[-1].ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_index failed \(-1\)"):
        p.image_line_index(img)
    idx, ks = torch.zeros((2, 2), dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(p.EngineError, match="index"):
        p.image_read_lines_at(img, idx, ks, 16)
    with pytest.raises(p.EngineError, match="index"):
        p.image_read_lines_at(img, torch.zeros(4, dtype=torch.int64), ks, 16)
