"""The line records of a split (fourmc_gpu_image_align_slices / fourmc_gpu_image_read_records) without a GPU: declared, exported,
reachable from Python, argument checks before the device check - and the model the GPU tests compare with (records_model.py) held
against the host's index functions, against the reader's loop stated by brute force, and against the property the format exists
for: however a file is cut into raw slices, every record is read exactly once."""
import ctypes as C
import importlib
import itertools
import os
import re

import numpy as np
import pytest
import torch

import helpers
import records_model as rm

ROOT = helpers.ROOT
NAMES = ("fourmc_gpu_image_align_slices", "fourmc_gpu_image_read_records")


def test_symbols_are_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(raw, name) is not None, name
        assert name in p.exported_symbols(), name
    for struct in ("fourmc_image_slice", "fourmc_image_records"):
        assert re.search(r"typedef struct %s\b" % struct, text), struct
    assert C.sizeof(p.ImageSlice) == 48 and C.sizeof(p.ImageRecords) == 40
    assert [f for f, _ in p.ImageSlice._fields_] == ["start", "end", "split_start", "split_end", "first_block", "block_count", "result"]
    assert [f for f, _ in p.ImageRecords._fields_] == ["result", "base", "data_off", "data_bytes", "reserved"]
    assert callable(p.image_align_slices) and callable(p.image_read_records)


def test_argument_checks_come_before_the_device_check():
    p = helpers.pkg()
    L = p.lib()
    img, dst = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    out = p.ImageRecords()
    out.result = 77
    sl = (p.ImageSlice * 2)()
    EINVAL = -3
    assert L.fourmc_gpu_image_read_records(None, 64, 0, 64, 10, dst.ctypes.data, 64, None, 0, C.byref(out), None) == EINVAL
    assert L.fourmc_gpu_image_read_records(img.ctypes.data, 64, 0, 64, 10, dst.ctypes.data, 64, None, 0, None, None) == EINVAL
    assert L.fourmc_gpu_image_read_records(img.ctypes.data, 64, 0, 64, 10, None, 64, None, 0, C.byref(out), None) == EINVAL
    assert b"image_read_records" in L.fourmc_gpu_last_error()
    assert L.fourmc_gpu_image_align_slices(None, 64, C.cast(sl, C.c_void_p), 2, None) == EINVAL
    assert L.fourmc_gpu_image_align_slices(img.ctypes.data, 64, None, 2, None) == EINVAL
    assert out.result == 77
    if not torch.cuda.is_available():                       # valid arguments: the engine's FOURMC_ENODEV, never a result
        assert L.fourmc_gpu_image_read_records(img.ctypes.data, 64, 0, 64, 10, dst.ctypes.data, 64, None, 0, C.byref(out), None) == -1
        assert L.fourmc_gpu_image_align_slices(img.ctypes.data, 64, C.cast(sl, C.c_void_p), 2, None) == -1
        assert L.fourmc_gpu_image_align_slices(img.ctypes.data, 64, None, 0, None) == -1


def test_python_entry_points_refuse_host_tensors():
    p = helpers.pkg()
    img, dst = torch.zeros(64, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.image_align_slices(img, [(0, 64)])
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.image_read_records(img, 0, 64, dst)


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
    img, dst = torch.zeros(44, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_align_slices failed \(-1\)"):
        p.image_align_slices(img, [(0, 10), (10, 44)])
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_image_read_records failed \(-1\)"):
        p.image_read_records(img, 0, 44, dst)
    with pytest.raises(p.EngineError, match="int64 CUDA tensor"):
        p.image_read_records(img, 0, 44, dst, starts=torch.zeros(4, dtype=torch.int64))


# ---- alignment: the model against the host's index functions ---------------------------------------------------------------
def _host_align(L, offsets, start, end, file_size):
    a = np.asarray(offsets, dtype=np.uint64)
    ptr = a.ctypes.data if len(a) else None
    return (L.fourmc_index_align_start(ptr, len(a), start, end), L.fourmc_index_align_end(ptr, len(a), end, file_size))


def test_the_reference_unit_tests_index():
    """TestFourMcBlockIndex.testAlignSlice: blocks at 100, 200, 300, 400"""
    L = helpers.pkg().lib()
    off = [100, 200, 300, 400]
    for (start, end, size), want in (((0, 350, 550), (0, 400)), ((100, 350, 550), (100, 400)), ((100, 250, 550), (100, 300))):
        got = rm.align_slice(off, start, end, size)
        assert (got["split_start"], got["split_end"]) == want == _host_align(L, off, start, end, size)
    # a start that finds no block before the end is dropped; an end behind the last block is the file's size
    assert rm.align_slice(off, 310, 390, 550)["result"] == 0 and _host_align(L, off, 310, 390, 550)[0] == rm.NOT_FOUND
    assert rm.align_slice(off, 401, 550, 550)["result"] == 0
    got = rm.align_slice(off, 150, 520, 550)
    assert (got["split_start"], got["split_end"], got["first_block"], got["block_count"], got["result"]) == (200, 550, 1, 3, 1)
    got = rm.align_slice(off, 0, 12, 550)                    # [0, e <= 12): kept with zero blocks
    assert (got["split_start"], got["split_end"], got["first_block"], got["block_count"], got["result"]) == (0, 100, 0, 0, 1)


def test_model_alignment_equals_the_host_functions():
    L = helpers.pkg().lib()
    rng = np.random.default_rng(41)
    for _ in range(300):
        n = int(rng.integers(1, 40))
        off, end_mark, size = rm.layout([1] * n, rng.integers(1, 50, n))
        for _ in range(40):
            a, z = sorted(int(v) for v in rng.integers(0, size + 2, 2))
            got = rm.align_slice(off, a, z, size)
            hs, he = _host_align(L, off, a, z, size)
            assert (got["split_start"], got["split_end"]) == (hs, he), (off, a, z)
            assert got["result"] == (0 if hs == rm.NOT_FOUND else 1)
            if got["result"]:
                inside = [i for i, o in enumerate(off) if hs <= o < he]
                assert got["block_count"] == len(inside) and (not inside or got["first_block"] == inside[0])


# ---- the ownership rule -----------------------------------------------------------------------------------------------------
def _cpu_families(B, seed):
    rng = np.random.default_rng(seed)

    def text(n):
        return rng.choice(np.frombuffer(b"abc \n", np.uint8), n, p=[0.25, 0.25, 0.2, 0.1, 0.2]).copy()

    def noise(n):
        return rng.integers(0, 256, n, dtype=np.uint8)
    return rm.families(B, text, noise)


def _blocks(T, B, rng=None):
    """usizes: blocks of B bytes, the last one short (the CLI's cut), or random cuts (Hadoop's writer flushes: any sizes)"""
    if rng is None:
        return [B] * (T // B) + ([T % B] if T % B else [])
    cuts = sorted(set(int(c) for c in rng.integers(1, T, int(rng.integers(0, 7))))) if T > 1 else []
    edges = [0] + cuts + [T]
    return [b - a for a, b in zip(edges, edges[1:]) if b > a]


def _models(seed=5):
    rng = np.random.default_rng(seed)
    for B in (16, 24):
        for name, (data, delim) in _cpu_families(B, seed + B).items():
            for cut in (None, rng, rng):
                us = _blocks(len(data), B, cut)
                off, end_mark, size = rm.layout(us, rng.integers(1, 30, len(us)))
                yield name, rm.Model(data, off, us, end_mark, delim), size


def _cut_points(m, size):
    """One raw cut position per class the alignment can tell apart: it depends on a position only through the first block header
    at or after it, so both sides of every header, the file's first byte and the end mark stand for every byte of the file."""
    pts = {1, m.end_mark, size - 1}
    for o in m.offsets:
        pts.update((o, o + 1))
    return sorted(x for x in pts if 0 < x < size)


def _partition_reads(m, size, cuts):
    edges = [0] + list(cuts) + [size]
    got = []
    for a, z in zip(edges, edges[1:]):
        sl = rm.align_slice(m.offsets, a, z, size)
        if not sl["result"]:
            continue
        r = m.records(sl["split_start"], sl["split_end"])
        assert r["result"] >= 0, (a, z, sl, r)
        got.extend((r["base"] + r["starts"][:r["result"]]).tolist())
    return got


def test_every_family_is_covered():
    names = {name for name, _, _ in _models()}
    assert names == {"block_edges", "three_blocks", "long_tail", "empty_records", "no_trailing_delimiter", "no_delimiter",
                     "all_delimiters", "stored_block", "zero_blocks", "one_block", "delimiter_0"}


def test_closed_form_equals_the_readers_loop():
    checked = 0
    for name, m, size in _models():
        heads = m.offsets + [m.end_mark, size]
        for s in [0] + m.offsets:
            for e in heads:
                if e < s:
                    assert m.records(s, e)["result"] == -3
                    continue
                r = m.records(s, e)
                want = m.brute(s, e)
                ds, _ = m.resolve(s, e)
                assert r["result"] == len(want) and r["base"] == ds, (name, s, e)
                assert (r["base"] + r["starts"][:len(want)]).tolist() == want, (name, s, e)
                if want:                                     # contiguous: lengths are differences, the last record ends the data
                    assert r["data_off"] == want[0] - ds and r["starts"][-1] == r["data_bytes"]
                    assert ds + r["data_bytes"] == len(m.data) or m.data[ds + r["data_bytes"] - 1] == m.delim
                else:
                    assert r["data_off"] == r["data_bytes"] == 0 and r["starts"].tolist() == [0]
                checked += 1
        # offsets that are no block header are refused
        for bad in (5, 13, m.end_mark - 1):
            if bad not in m.offsets and 0 < bad < m.end_mark:
                assert m.records(bad, size)["result"] == -3 and m.records(0, bad)["result"] == -3
    assert checked > 500


def test_every_partition_reads_every_record_exactly_once():
    rng = np.random.default_rng(77)
    exhaustive = sampled = 0
    for name, m, size in _models():
        want = m.file_records()[:-1].tolist() if m.T else []
        if not m.offsets:                                   # an empty index leaves the default splits: one reader of everything
            assert rm.align_slice([], 5, 20, size)["split_start"] == 5
            assert m.records(0, size)["result"] == 0
            continue
        pts = _cut_points(m, size)
        if len(m.offsets) <= 4:                             # every way to cut the file into 1..6 slices, up to equivalence
            for k in range(0, 6):
                for cuts in itertools.combinations(pts, k):
                    assert _partition_reads(m, size, cuts) == want, (name, cuts)
                    exhaustive += 1
        else:
            for _ in range(300):
                k = int(rng.integers(0, 6))
                cuts = sorted(set(int(c) for c in rng.choice(pts, min(k, len(pts)), replace=False)))
                assert _partition_reads(m, size, cuts) == want, (name, cuts)
                sampled += 1
        for _ in range(100):                                # and raw byte positions anywhere in the file
            cuts = sorted(set(int(c) for c in rng.integers(1, size, int(rng.integers(0, 6)))))
            assert _partition_reads(m, size, cuts) == want, (name, cuts)
    assert exhaustive > 5000 and sampled > 500


def test_capacity_codes_of_the_model():
    for name, m, size in _models(seed=9):
        if not m.offsets:
            continue
        r = m.records(0, size)
        short = m.records(0, size, dst_cap=len(m.data) - 1)
        assert (short["result"], short["data_bytes"]) == (-5, len(m.data))
        few = m.records(0, size, starts_cap=r["result"])
        assert (few["result"], few["reserved"], few["data_bytes"]) == (-5, r["result"], len(m.data))
        assert m.records(0, size, dst_cap=len(m.data), starts_cap=r["result"] + 1)["result"] == r["result"]
