"""The lines of a split by Hadoop's default rule (fourmc_gpu_image_read_lines) without a GPU: declared, exported, reachable from
Python, argument checks before the device check - and the model the GPU tests compare with (lines_model.py): its closed form held
against LineReader's loop stated by brute force, and against the property the format exists for: however a file is cut into raw
slices, every line is read exactly once."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import helpers
import lines_model as lm

ROOT = helpers.ROOT
NAME = "fourmc_gpu_image_read_lines"
EINVAL = -3


def test_symbol_is_declared_exported_and_bound():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    assert re.search(r"\b%s\s*\(" % NAME, text)
    assert getattr(raw, NAME) is not None
    assert NAME in p.exported_symbols()
    assert re.search(r"typedef struct fourmc_image_lines\b", text)
    assert C.sizeof(p.ImageLines) == 40
    assert [f for f, _ in p.ImageLines._fields_] == ["result", "base", "data_off", "data_bytes", "reserved"]
    assert callable(p.image_read_lines)
    # the scan alone is a debug export: declared under FOURMC_RESEARCH, in the research library only
    block = re.search(r"#ifdef FOURMC_RESEARCH(.*?)#endif", text, re.S).group(1)
    assert "fourmc_gpu_debug_lines_scan" in block and "fourmc_gpu_debug_lines_scan" not in p.exported_symbols()
    assert not hasattr(raw, "fourmc_gpu_debug_lines_scan")
    assert getattr(C.CDLL(p.research_lib_path()), "fourmc_gpu_debug_lines_scan") is not None


def _call(L, img, dst, starts, tlen, out, max_len=0x7FFFFFFF, cap=4):
    return L.fourmc_gpu_image_read_lines(img, 64, 0, 64, max_len, dst, 64, starts, tlen, cap, out, None)


def test_argument_checks_come_before_the_device_check():
    p = helpers.pkg()
    L = p.lib()
    img, dst = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    st, tl = np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    out = p.ImageLines()
    out.result = 77
    ref = C.byref(out)
    bad = [(None, dst.ctypes.data, None, None, ref, 0x7FFFFFFF),                         # no image
           (img.ctypes.data, dst.ctypes.data, None, None, None, 0x7FFFFFFF),             # no result
           (img.ctypes.data, None, None, None, ref, 0x7FFFFFFF),                         # no destination
           (img.ctypes.data, dst.ctypes.data, st.ctypes.data, None, ref, 0x7FFFFFFF),    # one table without the other
           (img.ctypes.data, dst.ctypes.data, None, tl.ctypes.data, ref, 0x7FFFFFFF),
           (img.ctypes.data, dst.ctypes.data, st.ctypes.data, tl.ctypes.data, ref, 0x80000000),
           (img.ctypes.data, dst.ctypes.data, None, None, ref, 0xFFFFFFFF)]
    for image, d, s, t, o, mx in bad:
        assert _call(L, image, d, s, t, o, mx) == EINVAL, (image, d, s, t, mx)
        assert b"image_read_lines" in L.fourmc_gpu_last_error()
    assert out.result == 77
    if not torch.cuda.is_available():                       # valid arguments: the engine's FOURMC_ENODEV, never a result
        assert _call(L, img.ctypes.data, dst.ctypes.data, None, None, ref) == -1
        assert _call(L, img.ctypes.data, dst.ctypes.data, st.ctypes.data, tl.ctypes.data, ref, 0) == -1


def test_python_entry_point_validates_its_tensors():
    p = helpers.pkg()
    img, dst = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.image_read_lines(img, 0, 64, dst)


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
    img, dst = torch.zeros(44, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_read_lines failed \(-1\)"):
        p.image_read_lines(img, 0, 44, dst)
    with pytest.raises(p.EngineError, match="go together"):
        p.image_read_lines(img, 0, 44, dst, starts=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(p.EngineError, match="go together"):
        p.image_read_lines(img, 0, 44, dst, text_len=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(p.EngineError, match="int64 CUDA tensor"):
        p.image_read_lines(img, 0, 44, dst, starts=torch.zeros(4, dtype=torch.int64), text_len=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(p.EngineError, match="max_line_len"):
        p.image_read_lines(img, 0, 44, dst, max_line_len=0x80000000)


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def test_line_ends_of_the_small_cases():
    def ends(b):
        return lm.line_ends(np.frombuffer(b, np.uint8)).tolist()
    assert ends(b"a\nb") == [1] and ends(b"a\rb") == [1] and ends(b"a\r\nb") == [2]
    assert ends(b"\r\r") == [0, 1] and ends(b"\n\r") == [0, 1] and ends(b"\r\n\r\n") == [1, 3] and ends(b"\n\n") == [0, 1]
    assert ends(b"ab\r") == [2] and ends(b"ab") == [] and ends(b"") == [] and ends(b"\r\r\n") == [0, 2]
    m = lm.Model(np.frombuffer(b"ab\r\ncd\re\n\nlast", np.uint8), [12], [14], 12 + 12 + 5)
    r = m.lines(0, 1000)
    assert r["result"] == 5 and r["starts"].tolist() == [0, 4, 7, 9, 10, 14] and r["text_len"].tolist() == [2, 2, 1, 0, 4]
    m.max_line_len = 1
    assert m.lines(0, 1000)["text_len"].tolist() == [1, 1, 1, 0, 1]
    m.max_line_len = 0
    assert m.lines(0, 1000)["text_len"].tolist() == [0] * 5 and m.lines(0, 1000)["starts"].tolist() == r["starts"].tolist()


def _cpu_families(B, seed):
    rng = np.random.default_rng(seed)

    def text(n):
        return rng.choice(np.frombuffer(b"abc \n", np.uint8), n, p=[0.25, 0.25, 0.2, 0.1, 0.2]).copy()

    def noise(n):
        return rng.integers(0, 256, n, dtype=np.uint8)
    return lm.families(B, text, noise)


def _blocks(T, B, rng=None):
    """usizes: blocks of B bytes, the last one short, or random cuts (Hadoop's writer flushes: any sizes)"""
    if rng is None:
        return [B] * (T // B) + ([T % B] if T % B else [])
    cuts = sorted(set(int(c) for c in rng.integers(1, T, int(rng.integers(0, 7))))) if T > 1 else []
    edges = [0] + cuts + [T]
    return [b - a for a, b in zip(edges, edges[1:]) if b > a]


MAXES = (0, 1, 3, 0x7FFFFFFF)


def _family_models(seed=5):
    rng = np.random.default_rng(seed)
    for B in (16, 24):
        for name, data in _cpu_families(B, seed + B).items():
            for cut in (None, rng):
                us = _blocks(len(data), B, cut)
                off, end_mark, size = lm.layout(us, rng.integers(1, 30, len(us)))
                # the reader's buffer smaller than a block, so that refills (and prevCharCR across them) happen in these sizes too
                yield name, lm.Model(data, off, us, end_mark, MAXES[int(rng.integers(0, 4))], buffer=int(rng.choice([7, 16, 65536]))), size


def _random_models(count, seed=6):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"\r\na", np.uint8)
    for i in range(count):
        T = int(rng.integers(1, 60))
        data = rng.choice(alphabet, T, p=rng.dirichlet([1, 1, 1])).copy()
        us = _blocks(T, 0, rng)
        off, end_mark, size = lm.layout(us, rng.integers(1, 30, len(us)))
        yield "random%d" % i, lm.Model(data, off, us, end_mark, MAXES[int(rng.integers(0, 4))], buffer=int(rng.choice([1, 2, 5, 65536]))), size


def _check_closed_form_against_the_loop(name, m, size):
    checked = 0
    heads = m.offsets + [m.end_mark, size]
    for s in [0] + m.offsets:
        for e in heads:
            if e < s:
                assert m.lines(s, e)["result"] == -3
                continue
            r = m.lines(s, e)
            want = m.brute(s, e)
            ds, _ = m.resolve(s, e)
            key = (name, s, e, m.max_line_len, m.buffer)
            assert r["result"] == len(want) and r["base"] == ds, key
            assert (r["base"] + r["starts"][:len(want)]).tolist() == [a for a, _ in want], key
            assert r["text_len"].tolist() == [t for _, t in want], key
            if want:
                assert r["data_off"] == want[0][0] - ds and r["starts"][-1] == r["data_bytes"], key
            else:
                assert r["data_off"] == r["data_bytes"] == 0 and r["starts"].tolist() == [0], key
            checked += 1
    return checked


def test_every_family_is_covered():
    names = {name for name, _, _ in _family_models()}
    assert names == {"crlf_text", "cr_only", "lf_only", "mixed", "all_cr", "all_lf", "alternating_crlf", "alternating_lfcr",
                     "no_terminator", "zero_blocks", "one_block", "stored_block", "cr_at_block_end", "ends_with_crlf", "ends_with_cr",
                     "tail_only_cr_last", "tail_only_cr_last_lf", "three_blocks"}


def test_closed_form_equals_the_readers_loop_on_every_family():
    assert sum(_check_closed_form_against_the_loop(*x) for x in _family_models()) > 500


def test_closed_form_equals_the_readers_loop_on_random_contents():
    models = list(_random_models(3000))
    assert sum(_check_closed_form_against_the_loop(*x) for x in models) > 10000
    assert {m.max_line_len for _, m, _ in models} == set(MAXES)


def _partition_reads(m, size, cuts):
    edges = [0] + list(cuts) + [size]
    got = []
    for a, z in zip(edges, edges[1:]):
        sl = lm.align_slice(m.offsets, a, z, size)
        if not sl["result"]:
            continue
        r = m.lines(sl["split_start"], sl["split_end"])
        assert r["result"] >= 0, (a, z, sl, r)
        got.extend((r["base"] + r["starts"][:r["result"]]).tolist())
    return got


def test_every_partition_reads_every_line_exactly_once():
    rng = np.random.default_rng(78)
    parts = 0
    for name, m, size in list(_family_models(seed=7)) + list(_random_models(3000, seed=8)):
        want = m.file_lines()[:-1].tolist() if m.T else []
        if not m.offsets:                                   # an empty index leaves the default splits: one reader of everything
            assert m.lines(0, size)["result"] == 0
            continue
        for n in range(1, 7):                               # n raw slices: n - 1 cuts anywhere in the file
            cuts = sorted(set(int(c) for c in rng.integers(1, size, n - 1)))
            assert _partition_reads(m, size, cuts) == want, (name, cuts)
            heads = sorted(set(int(c) + int(rng.integers(0, 2)) for c in rng.choice(m.offsets, min(n - 1, len(m.offsets)), replace=False)))
            assert _partition_reads(m, size, [c for c in heads if 0 < c < size]) == want, (name, heads)
            parts += 2
    assert parts > 30000


def test_truncation_changes_lengths_only_and_capacity_codes_of_the_model():
    for name, m, size in _family_models(seed=9):
        if not m.offsets:
            continue
        m.max_line_len = 0x7FFFFFFF
        r = m.lines(0, size)
        for mx in MAXES:
            m.max_line_len = mx
            q = m.lines(0, size)
            assert q["starts"].tolist() == r["starts"].tolist() and q["result"] == r["result"]
            assert q["text_len"].tolist() == np.minimum(r["text_len"], mx).tolist()
        short = m.lines(0, size, dst_cap=len(m.data) - 1)
        assert (short["result"], short["data_bytes"]) == (-5, len(m.data))
        few = m.lines(0, size, lines_cap=r["result"])
        assert (few["result"], few["reserved"], few["data_bytes"], few["text_len"]) == (-5, r["result"], len(m.data), None)
        assert m.lines(0, size, dst_cap=len(m.data), lines_cap=r["result"] + 1)["result"] == r["result"]
