"""fourmc_gpu_bstreams_compress / fourmc_gpu_bstream_writes_bound without a GPU: the grouping rule restated
(tests/bstream_writes_model.py) against the model writer (tests/bstream_model.py), the bound against every schedule, the symbols, and
every argument error refused before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bstream_model as bm
import bstream_writes_model as wm
import helpers

ROOT = helpers.ROOT
OK, ENODEV, EINVAL, EUNSUP = 0, -1, -3, -5
LZ4, ZSTD = 0, 3
NAMES = ["fourmc_gpu_bstreams_compress", "fourmc_gpu_bstream_writes_bound"]


def schedules(M):
    """the schedules the issue names: every branch of the rule, and a table deep enough for a three-level search"""
    return [(), (0,), (0, 0), (5,), (0, 5, 0), (M,), (M, 1), (1, M), (M + 1,), (1, M + 1), (M + 1, 1), (0, M + 1), (M + 1, 0, 0), (2 * M,),
            (2 * M + 5,), (M - 1, 1, 1), (1, M + 1) * 3, (60,) * 70000]


def fake_compressor(b):
    """the length and a few bytes: the shape does not depend on the codec, and a payload never ends with a zero"""
    return len(b).to_bytes(4, "little") + b[:3] + b"\x01"


# ---- the model of the rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zstd", [False, True], ids=["lz4", "zstd"])
def test_the_rule_restated_equals_the_model_writer(zstd):
    M = bm.max_input(zstd)
    data = b"\x55" * (3 * M + 16)
    for pat in schedules(M):
        n = sum(pat)
        img = bm.write_stream(data[:n], list(pat), fake_compressor, zstd)
        want, trailer = wm.plan(list(pat), M)
        got, end = bm.shape(img, zstd)
        assert got == want, pat[:4]
        # the trailer actually written: behind the last whole group there is BE32(0) or nothing
        assert img[end:] == (b"\0\0\0\0" if trailer else b""), pat[:4]
        assert len(img) <= wm.worst_case(list(pat), M, lambda k: 8)               # the fake payload is at most 8 bytes
    assert wm.plan([60] * 70000, M)[0] == [((M // 60) * 60, [(M // 60) * 60]), (70000 * 60 - (M // 60) * 60, [70000 * 60 - (M // 60) * 60])]
    assert wm.plan([2 * M + 5], M) == ([(2 * M + 5, [M, M, 5])], True)
    assert wm.plan([M + 1, 0, 0], M) == ([(M + 1, [M, 1])], True) and wm.plan([0, 5, 0], M) == ([(5, [5])], False)
    assert wm.plan([], M) == ([], True) and wm.plan([0, 0], M) == ([], True)


def test_uniform_schedules_are_what_group_bytes_cuts():
    """n_writes == 0: writes of w bytes accumulate into groups of floor(M / w) * w, which is bstream_compress's correspondence"""
    M = bm.max_input(False)
    for S, w in ((0, 0), (0, 7), (5, 0), (2500, 1000), (3 * M + 5, 1 << 20), (2 * M + 5, 0), (3 * M, M + 1), (10, 100)):
        pat = wm.uniform(S, w)
        assert sum(pat) == S and all(pat)
        groups, trailer = wm.plan(pat, M)
        if w and w <= M:
            G = (M // w) * w
            assert [r for r, _ in groups] == [min(G, S - at) for at in range(0, S, G)] and trailer == (S == 0)


# ---- the bound ------------------------------------------------------------------------------------------------------------------
def test_max_chunks_and_groups_by_exhaustive_enumeration():
    """every schedule of up to 6 writes of 0 .. 2M + 2 bytes at M = 3, 4, 5, through the writer's own state machine (a write that no
    longer fits closes the open group; a long write is a group of its own) on all schedules at once"""
    for M in (3, 4, 5):
        V = 2 * M + 3
        for k in range(7):
            grid = np.indices((V,) * k, dtype=np.int16).reshape(k, -1) if k else np.zeros((0, 1), np.int16)
            N = grid.shape[1]
            acc, groups, chunks = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
            for w in grid:
                flush = (acc + w > M) & (acc > 0)
                groups += flush
                chunks += flush
                acc[flush] = 0
                long = w > M
                groups += long
                chunks += np.where(long, -(-w // M), 0)
                acc += np.where(long, 0, w)
            groups += acc > 0
            chunks += acc > 0
            S = grid.sum(axis=0, dtype=np.int32)
            cmax = 3 * (S // (M + 2)) + np.minimum(S % (M + 2), 2)
            gmax = 2 * (S // (M + 1)) + np.minimum(S % (M + 1), 1)
            assert (chunks <= cmax).all() and (groups <= gmax).all(), (M, k)
            # the state machine is the rule: a sample of the schedules through the restatement
            for col in range(0, N, max(1, N // 200)):
                g, _ = wm.plan([int(v) for v in grid[:, col]], M)
                assert (len(g), sum(len(c) for _, c in g)) == (groups[col], chunks[col]), (M, grid[:, col])
        for S in range(0, 8 * M):
            assert wm.max_chunks(S, M) == 3 * (S // (M + 2)) + min(S % (M + 2), 2) and wm.max_groups(S, M) == 2 * (S // (M + 1)) + min(S % (M + 1), 1)
        # the two adversarial patterns reach the counts
        assert sum(len(c) for _, c in wm.plan([1, M + 1] * 5, M)[0]) == 15 == wm.max_chunks(5 * (M + 2), M)
        assert len(wm.plan([1, M] * 5, M)[0]) == 10 == wm.max_groups(5 * (M + 1), M)


@pytest.mark.parametrize("zstd", [False, True], ids=["lz4", "zstd"])
def test_writes_bound_holds_for_every_schedule(zstd):
    p = helpers.pkg()
    codec = ZSTD if zstd else LZ4
    M = bm.max_input(zstd)
    assert p.bstream_max_input(codec) == M

    def bound(k):
        return bm.block_bound(k, zstd)
    pats = [list(s) for s in schedules(M)]
    for reps in (1, 2, 3):
        pats += [[1, M + 1] * reps, [1, M] * reps, [1, M] * reps + [1], [M + 1, 1] * reps, [1, M + 1] * reps + [1]]
    pats = [q for q in pats if sum(q) <= 3 * M + 16]
    pats += [wm.uniform(S, w) for S, w in ((3 * M, 0), (3 * M, M + 1), (3 * M, M), (2500, 1000), (3 * M, 1 << 20))]
    for pat in pats:
        S = sum(pat)
        got = p.bstream_writes_bound(S, codec)
        assert got == wm.writes_bound(S, M, zstd) if S else got == 4, pat[:4]
        assert got >= wm.worst_case(pat, M, bound), (pat[:4], S)
    # the codec's overhead splits as the header says: bound(n) - n <= V(n) + K with V additive
    for n in (1, 2, 255, 256, 1000, (128 << 10) - 1, 128 << 10, M - 1, M):
        assert bound(n) - n <= (n // 256 + 64 if zstd else n // 255 + 16), n
    for bad in (-1, 4, 99):
        assert p.bstream_writes_bound(1000, bad) == 0
    for c in ((1, 2) if not zstd else ()):
        assert p.bstream_writes_bound(12345, c) == p.bstream_writes_bound(12345, LZ4)


# ---- the symbols ----------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported():
    p = helpers.pkg()
    raw = C.CDLL(p.lib_path())
    text = open(os.path.join(ROOT, "include", "fourmc_gpu.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert getattr(raw, name) is not None, name
        assert name in p.exported_symbols(), name
    assert C.sizeof(p.BstreamEncItem) == 72 and p.BstreamEncItem.reason.offset == 52 and p.BstreamEncItem.image_bytes.offset == 56
    for k, name in enumerate(p.BSTREAM_WRITE_REASONS):
        assert re.search(r"FOURMC_BSW_%s\s*=\s*%d\b" % (name, k), text), name
    for f in (p.compress_bstreams, p.bstream_writes_bound):
        assert callable(f)
    for gone in ("Multi-chunk groups on the", "A many-streams encode"):
        assert gone not in text


# ---- arguments ------------------------------------------------------------------------------------------------------------------
SRC, TAB, IMAGES = 5000, 100, 16384
FIELDS = ("src_off", "src_bytes", "image_off", "image_cap", "writes_off", "n_writes", "write_bytes")
GOOD = [(0, 2500, 0, 4000, 0, 0, 1000), (2500, 0, 4000, 4, 0, 0, 0), (2500, 2500, 4004, 4000, 10, 5, 0), (0, 5000, 9000, 0, 0, 0, 0)]


def _items(p, rows):
    arr = (p.BstreamEncItem * max(len(rows), 1))()
    for i, row in enumerate(rows):
        for f, v in zip(FIELDS, row):
            setattr(arr[i], f, v)
        arr[i].reason, arr[i].image_bytes, arr[i].groups, arr[i].chunks = 66, 77 + i, 88, 99
    return arr


def _untouched(arr, rows):
    for i, row in enumerate(rows):
        assert tuple(getattr(arr[i], f) for f in FIELDS) == tuple(row), i
        assert (arr[i].reason, arr[i].image_bytes, arr[i].groups, arr[i].chunks) == (66, 77 + i, 88, 99), i


def _call(p, rows, codec=LZ4, level=1, src=True, tab=True, images=True, n=None, items=True):
    L = p.lib()
    s = np.zeros(SRC, np.uint8)
    t = np.full(TAB, 500, np.uint32)
    img = np.full(IMAGES, 0xC3, np.uint8)
    arr = _items(p, rows)
    rc = L.fourmc_gpu_bstreams_compress(s.ctypes.data if src else None, SRC, t.ctypes.data if tab else None, TAB,
                                        img.ctypes.data if images else None, IMAGES, codec, level,
                                        C.cast(arr, C.c_void_p) if items else None, len(rows) if n is None else n, None)
    _untouched(arr, rows)
    assert (img == 0xC3).all()
    return rc


MANY_EINVAL = {
    # name: (rows, keywords)
    "codec": (GOOD, dict(codec=4)), "codec, everything else wrong too": (GOOD, dict(codec=-1, src=False, tab=False, items=False)),
    "codec, size query": (GOOD, dict(codec=7, images=False)),
    "null items": (GOOD, dict(items=False)), "null source": (GOOD, dict(src=False)), "null table": (GOOD, dict(tab=False)),
    "null table, size query": (GOOD, dict(tab=False, images=False)),
    "source starts beyond the buffer": ([(SRC + 1, 0, 0, 100, 0, 0, 0)], {}),
    "source ends beyond the buffer": ([(SRC - 9, 10, 0, 100, 0, 0, 0)], {}),
    "source ends beyond the buffer, size query": ([(SRC - 9, 10, 0, 100, 0, 0, 0)], dict(images=False)),
    "src_off + src_bytes wraps": ([(8, 2 ** 64 - 4, 0, 100, 0, 0, 0)], {}),
    "table range starts beyond the table": ([(0, 0, 0, 100, TAB + 1, 0, 0)], {}),
    "table range ends beyond the table": ([(0, 500, 0, 1000, TAB - 4, 5, 0)], {}),
    "table range ends beyond the table, size query": ([(0, 500, 0, 1000, TAB - 4, 5, 0)], dict(images=False)),
    "writes_off + n_writes wraps": ([(0, 500, 0, 1000, 8, 2 ** 64 - 4, 0)], {}),
    "region starts beyond the images": ([(0, 10, IMAGES + 1, 0, 0, 0, 0)], {}),
    "region ends beyond the images": ([(0, 10, 0, 100, 0, 0, 0), (0, 10, IMAGES - 99, 100, 0, 0, 0)], {}),
    "image_off + image_cap wraps": ([(0, 10, 16, 2 ** 64 - 8, 0, 0, 0)], {}),
    "regions overlap by one byte": ([(0, 10, 100, 50, 0, 0, 0), (0, 10, 0, 101, 0, 0, 0)], {}),
    "one region inside another": ([(0, 10, 0, 1000, 0, 0, 0), (0, 10, 3000, 10, 0, 0, 0), (0, 10, 500, 1, 0, 0, 0)], {}),
    "the same region twice": ([(0, 10, 64, 64, 0, 0, 0)] * 2, {}),
}


@pytest.mark.parametrize("name", list(MANY_EINVAL))
def test_argument_errors_are_einval_before_any_device(name):
    p = helpers.pkg()
    rows, kw = MANY_EINVAL[name]
    assert _call(p, rows, **kw) == EINVAL, name
    assert p.lib().fourmc_gpu_last_error()


def test_level_outside_the_device_is_eunsup_and_no_items_is_ok():
    p = helpers.pkg()
    for level in (0, 13, -1, 22):
        assert _call(p, GOOD, codec=ZSTD, level=level) == EUNSUP, level
        assert _call(p, GOOD, codec=ZSTD, level=level, images=False) == EUNSUP, level
    assert _call(p, GOOD, codec=4, level=13) == EINVAL                                       # the codec is checked first
    assert _call(p, [(SRC + 1, 0, 0, 100, 0, 0, 0)], codec=ZSTD, level=13) == EINVAL         # and the arguments before the level
    for codec in (0, 1, 2, 3):
        assert _call(p, GOOD, codec=codec, n=0) == OK and _call(p, GOOD, codec=codec, n=0, items=False, src=False, tab=False, images=False) == OK
    assert _call(p, GOOD, codec=9, n=0) == EINVAL


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the behaviour without a device")
def test_without_a_gpu_well_formed_calls_fail_with_enodev(monkeypatch):
    import importlib
    p = helpers.pkg()
    for codec, level in ((0, 0), (1, 0), (2, 4), (3, 1), (3, 12)):
        for images in (True, False):
            assert _call(p, GOOD, codec=codec, level=level, images=images) == ENODEV
            assert p.lib().fourmc_gpu_last_error()
    # regions that touch or are empty do not overlap; the regions of a size query are nobody's business; no table is needed without entries
    assert _call(p, [(0, 10, 0, 100, 0, 0, 0), (0, 10, 100, 100, 0, 0, 0), (0, 10, 50, 0, 0, 0, 0), (0, 0, IMAGES, 0, TAB, 0, 0)], tab=False) == ENODEV
    assert _call(p, [(0, 10, 0, 100, 0, 0, 0)] * 2 + [(0, 10, IMAGES + 5, 7, 0, 0, 0)], images=False) == ENODEV
    assert _call(p, [(0, 0, 0, 4, 0, 0, 0)], src=False, tab=False) == ENODEV
    # the Python entry point: host tensors are refused before any call; with the check bypassed the library's codes surface
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_bstreams(torch.zeros(64, dtype=torch.uint8), [(0, 64, 0, 200, 0, 0, 0)], torch.zeros(4096, dtype=torch.uint8))
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_bstreams(None, [], None, d_writes=torch.zeros(4, dtype=torch.int32))
    eng = importlib.import_module("4mc_amd.engine")
    keep = []

    def host_ptr(t, what=None):
        a = t.numpy()
        keep.append(a)
        return a.ctypes.data
    monkeypatch.setattr(eng, "_dev_ptr", host_ptr)
    monkeypatch.setattr(eng, "_writes_ptr", host_ptr)
    monkeypatch.setattr(eng, "_stream_ptr", lambda stream: 0)
    src, img, tab = torch.zeros(SRC, dtype=torch.uint8), torch.zeros(IMAGES, dtype=torch.uint8), torch.full((TAB,), 500, dtype=torch.int32)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstreams_compress failed \(-1\)"):
        p.compress_bstreams(src, GOOD, img, *p.bstream_codec(".zstd_uc"), d_writes=tab)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstreams_compress failed \(-1\)"):
        p.compress_bstreams(src, GOOD, None, d_writes=tab)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstreams_compress failed \(-3\)"):
        p.compress_bstreams(src, [(0, 10, 64, 64, 0, 0, 0)] * 2, img)
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstreams_compress failed \(-5\)"):
        p.compress_bstreams(src, GOOD, img, p.CODEC_ZSTD, 13, d_writes=tab)
    with pytest.raises(p.EngineError, match="beyond the tensor"):
        p.compress_bstreams(src, GOOD, img, images_bytes=IMAGES + 1)
    assert p.compress_bstreams(src, [], img) == [] and p.compress_bstreams(None, [], None) == []
