"""Block streams written from a job's write() sizes, many per call (fourmc_gpu_bstreams_compress / compress_bstreams).

The device is compared byte for byte with the model writer of tests/bstream_model.py fed the same write() sizes, the oracle as block
compressor.  Chunk payloads are memoized by content, in the memo test_gpu_bstream.py keeps: the schedules are cut so that the 4 MB
chunks are the pieces [0, M) and [M, 2M) of one corpus wherever the shape allows it.  Every image region is its queried size, lies
between guard bytes of one value, and everything outside the written streams must still hold that value afterwards."""
import os

import numpy as np
import pytest
import torch

import bstream_model as bm
import bstream_writes_model as wm
import test_gpu_bstream as T

pytestmark = pytest.mark.gpu

CANARY = T.CANARY
GUARD = 64
PAIRS = T.PAIRS
FAST = [PAIRS[0], PAIRS[4]]
_MEMO = {}


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


def d_text():
    if "d_text" not in _MEMO:
        _MEMO["d_text"] = T.up(T.text(), 64)
    return _MEMO["d_text"]


def compressor(codec, level):
    """bytes -> bytes by the oracle, memoized by content (LZ4 fast and zstd 1 share test_gpu_bstream's memo)"""
    if (codec, level) in ((0, 0), (3, 1)):
        return lambda b: T.block(codec == 3, b)
    cb = bm.oracle_compressor(codec, level)

    def f(b):
        key = (codec, level, b)
        if key not in _MEMO:
            _MEMO[key] = cb(b)
        return _MEMO[key]
    return f


def model(codec, level, off, pattern):
    """(the model writer's stream, its source bytes) for write() calls of these sizes over the corpus from `off` on"""
    key = ("model", codec, level, off, tuple(pattern))
    if key not in _MEMO:
        src = T.text()[off:off + sum(pattern)]
        _MEMO[key] = (bm.write_stream(src, list(pattern), compressor(codec, level), codec == 3), src)
    return _MEMO[key]


def stream(off, pattern, uniform=None):
    """one stream of a call: its source starts `off` bytes into the corpus; `pattern` is what the writer is fed; uniform None: the
    pattern goes into the table, else it is the item's write_bytes and the pattern is what that means"""
    return {"off": off, "pattern": tuple(pattern), "uniform": uniform}


def uniform(off, src_bytes, w):
    return stream(off, wm.uniform(src_bytes, w), w)


def run(p, codec, level, streams, caps=None, table_edit=None, pad=3):
    """One compress_bstreams over `streams`, all tables in one d_writes (with `pad` foreign entries in front and between).  Returns
    (results, the written bytes per item or None for an item with a verdict, the query's results).  caps: {item: image_cap} instead
    of the queried size; table_edit: {item: pattern} written into the table in place of the item's own."""
    tab, rows = [7] * pad, []
    for i, s in enumerate(streams):
        pat = (table_edit or {}).get(i, s["pattern"])
        if s["uniform"] is None:
            rows.append([s["off"], sum(s["pattern"]), 0, 0, len(tab), len(pat), 0])
            tab += list(pat) + [9] * pad
        else:
            rows.append([s["off"], sum(s["pattern"]), 0, 0, 0, 0, s["uniform"]])
    d_writes = torch.from_numpy(np.array(tab, np.uint32).view(np.int32)).cuda()
    query = p.compress_bstreams(d_text(), [tuple(r) for r in rows], None, codec, level, d_writes=d_writes)
    at = GUARD
    for i, r in enumerate(rows):
        r[2], r[3] = at, (caps or {}).get(i, query[i]["image_bytes"])
        at += r[3] + GUARD
    d_images = torch.full((at + T.SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    res = p.compress_bstreams(d_text(), [tuple(r) for r in rows], d_images, codec, level, d_writes=d_writes, images_bytes=at)
    out = d_images.cpu().numpy()
    covered = np.zeros(len(out), bool)
    got = []
    for r, st in zip(rows, res):
        assert st["name"] == p.BSTREAM_WRITE_REASONS[st["reason"]]
        if st["reason"] == 0:
            assert st["image_bytes"] <= r[3], st
            covered[r[2]:r[2] + st["image_bytes"]] = True
            got.append(out[r[2]:r[2] + st["image_bytes"]].tobytes())
        else:
            got.append(None)
    assert (out[~covered] == CANARY).all(), "bytes written outside the streams"
    _MEMO["last"] = (d_images, rows)
    return res, got, query


def check(p, codec, level, streams, **kw):
    """run, and every stream equals the model writer's; the counts and the query agree with the rule; then the round trip"""
    zstd = codec == 3
    M = bm.max_input(zstd)
    res, got, query = run(p, codec, level, streams, **kw)
    for i, (s, st, q, g) in enumerate(zip(streams, res, query, got)):
        want, src = model(codec, level, s["off"], s["pattern"])
        groups, trailer = wm.plan(list(s["pattern"]), M)
        assert st["reason"] == 0 == q["reason"], (i, st, q)
        assert g == want, (i, s["pattern"][:4], len(g), len(want))
        assert st["groups"] == len(groups) == q["groups"] and st["chunks"] == sum(len(c) for _, c in groups) == q["chunks"], (i, st, q)
        assert q["image_bytes"] == wm.worst_case(list(s["pattern"]), M, lambda k: bm.block_bound(k, zstd)), (i, q)
        assert len(g) == st["image_bytes"] <= q["image_bytes"] <= p.bstream_writes_bound(len(src), codec), (i, st, q)
        assert g.endswith(b"\0\0\0\0") or not trailer
    round_trip(p, codec, streams, res)
    return res, got


def round_trip(p, codec, streams, res):
    """decompress_bstreams over the images the last run wrote: FOURMC_BS_OK, the sources' bytes, the writer's groups and chunks"""
    d_images, rows = _MEMO["last"]
    caps = [max(r[1], 1) for r in rows]
    dst_off = np.concatenate([[0], np.cumsum(caps)])
    d_dst = torch.empty(int(dst_off[-1]) + 64, dtype=torch.uint8, device="cuda")
    items = [(r[2], st["image_bytes"], int(dst_off[i]), r[1]) for i, (r, st) in enumerate(zip(rows, res))]
    back = p.decompress_bstreams(d_images, items, d_dst, codec)
    out = d_dst.cpu().numpy()
    for i, (s, st, b, r) in enumerate(zip(streams, res, back, rows)):
        assert b["reason"] == bm.OK and b["decoded_bytes"] == r[1] == b["total_bytes"], (i, b)
        assert (b["groups"], b["chunks"]) == (st["groups"], st["chunks"]), (i, b, st)
        assert out[dst_off[i]:dst_off[i] + r[1]].tobytes() == T.text()[s["off"]:s["off"] + r[1]], i


# ---- all eight codecs -----------------------------------------------------------------------------------------------------------
def five_small():
    return [stream(777, (1000, 0, 1000, 500)), stream(5000, (0, 0)), uniform(9000, 3000, 1000), uniform(13000, 1, 0), stream(15000, (333,) * 3)]


@pytest.mark.parametrize("ext,codec,level", PAIRS, ids=[e for e, _, _ in PAIRS])
def test_five_small_streams(p, ext, codec, level):
    res, got = check(p, codec, level, five_small())
    assert got[1] == b"\0\0\0\0" and [st["groups"] for st in res] == [1, 0, 1, 1, 1]
    assert p.compress_bstreams(d_text(), [], None, codec, level) == []


@pytest.mark.parametrize("ext,codec,level", PAIRS, ids=[e for e, _, _ in PAIRS])
def test_uniform_writes_equal_compress_bstream_at_their_group_bytes(p, ext, codec, level):
    """device against device, no oracle: writes of w bytes are groups of floor(M / w) * w bytes"""
    M = p.bstream_max_input(codec)
    cases = [(2999, 1000)] + ([(5 << 20, 1 << 20), ((3 << 20) + 5, 3 << 20)] if (ext, codec, level) in FAST else [])
    for n, w in cases:
        G = (M // w) * w
        src = T.text()[:n]
        want, _ = T.encode(p, src, codec, level, G)
        res, got, _ = run(p, codec, level, [uniform(0, n, w)])
        assert got[0] == want and res[0]["groups"] == res[0]["chunks"] == -(-n // G), (n, w, res)


# ---- where grouping can go wrong: LZ4 fast and zstd 1 -----------------------------------------------------------------------------
def shapes(M):
    """source offsets chosen so that every 4 MB chunk is [0, M) or [M, 2M) of the corpus"""
    return [stream(0, (2 * M + 5,)), stream(0, (M, 1)), stream(M - 1, (1, M)), stream(0, (M + 1,)), stream(M - 1, (1, M + 1)),
            stream(0, (M + 1, 1)), stream(0, (0, M + 1)), stream(0, (M + 1, 0, 0)), uniform(0, 2 * M + 5, 0)]


@pytest.mark.parametrize("ext,codec,level", FAST, ids=["lz4_fast", "zstd_fast"])
def test_grouping_shapes(p, ext, codec, level):
    M = p.bstream_max_input(codec)
    res, got = check(p, codec, level, shapes(M))
    assert [(st["groups"], st["chunks"]) for st in res] == [(1, 3), (2, 2), (2, 2), (1, 2), (2, 3), (2, 3), (1, 2), (1, 2), (1, 3)]
    assert [g.endswith(b"\0\0\0\0") for g in got] == [True, False, False, True, True, False, True, True, True]
    assert got[0] == got[8] and got[3] == got[6] == got[7]


@pytest.mark.parametrize("ext,codec,level", FAST, ids=["lz4_fast", "zstd_fast"])
def test_long_tables(p, ext, codec, level):
    """70 000 writes of 60 bytes: more than 64 * 64 entries, so the search for the group boundary goes three levels deep, and the
    boundary (entry 69 630 or so) falls inside a tile; 5 000 writes of random sizes in 0 .. 3000"""
    M = p.bstream_max_input(codec)
    rng = np.random.default_rng(20240611)
    rand = tuple(int(v) for v in rng.integers(0, 3001, 5000))
    assert sum(rand) > M and (codec == 3 or (M // 60) % 64 != 0)                 # (zstd's M puts the boundary on a tile's edge)
    res, got = check(p, codec, level, [stream(0, (60,) * 70000), stream(0, rand)])
    assert res[0]["groups"] == 2 and res[1]["groups"] == len(wm.plan(list(rand), M)[0]) >= 2


@pytest.mark.parametrize("ext,codec,level", FAST, ids=["lz4_fast", "zstd_fast"])
def test_six_streams_share_one_table_and_two_are_refused(p, ext, codec, level):
    good = [stream(100, (700, 0, 300)), stream(0, ()), stream(4000, (1,) * 130), uniform(2000, 2500, 1000)]
    streams = [good[0], stream(8000, (500, 500, 24)), good[1], good[2], stream(9000, (40,) * 70), good[3]]
    single = [run(p, codec, level, [s]) for s in good]
    worst = run(p, codec, level, [streams[4]])[2][0]["image_bytes"]
    # item 1's table sums to src_bytes - 1, item 4's region is one byte short of its queried size
    res, got, query = run(p, codec, level, streams, caps={4: worst - 1}, table_edit={1: (500, 500, 23)})
    assert [st["name"] for st in res] == ["OK", "SUM", "OK", "OK", "CAP", "OK"] and [q["name"] for q in query] == ["OK", "SUM", "OK", "OK", "OK", "OK"]
    assert got[1] is None and got[4] is None                     # (run checked that their regions still hold the guard value)
    assert (res[1]["image_bytes"], res[1]["groups"], res[1]["chunks"]) == (0, 0, 0) and res[4]["image_bytes"] == worst == query[4]["image_bytes"]
    for i, (sres, sgot, squery) in zip((0, 2, 3, 5), single):
        assert got[i] == sgot[0] and res[i] == sres[0] and query[i] == squery[0], i
        want, src = model(codec, level, streams[i]["off"], streams[i]["pattern"])
        assert got[i] == want
        assert len(got[i]) <= query[i]["image_bytes"] <= p.bstream_writes_bound(len(src), codec)
    # an entry above 0x7FFFFFFF wins over the sum it spoils
    res, got, _ = run(p, codec, level, [good[0], stream(8000, (500, 500, 24))], table_edit={1: (500, 0x80000000, 24)})
    assert [st["name"] for st in res] == ["OK", "WRITE"] and got[0] == single[0][1][0]


@pytest.mark.parametrize("ext,codec,level", FAST, ids=["lz4_fast", "zstd_fast"])
def test_rounds_end_inside_a_long_group(p, ext, codec, level):
    """FOURMC_BSW_ROUND=2 (read at every call): the third chunk of the long group falls into the second round, with the first small
    stream; the bytes are the default run's"""
    M = p.bstream_max_input(codec)
    streams = [stream(0, (2 * M + 5,)), stream(777, (1000, 0, 1000, 500)), uniform(9000, 3000, 1000), stream(15000, (333,) * 3)]
    res, got = check(p, codec, level, streams)
    assert "FOURMC_BSW_ROUND" not in os.environ
    os.environ["FOURMC_BSW_ROUND"] = "2"
    try:
        res2, got2, _ = run(p, codec, level, streams)
        round_trip(p, codec, streams, res2)
    finally:
        del os.environ["FOURMC_BSW_ROUND"]
    assert got2 == got and res2 == res and res[0]["chunks"] == 3 and sum(st["chunks"] for st in res) == 6


def test_under_the_parallel_lz4_encoder(p):
    """the payloads are the tolerant encoder's, so the framing is checked by the model reader and the round trip, not byte equality"""
    M = p.bstream_max_input(0)
    streams = [stream(M - 1, (1, M + 1)), stream(777, (1000, 0, 1000, 500)), stream(0, ())]
    L = p.lib()
    L.fourmc_gpu_set_lz4_encode_mode(1)
    try:
        res, got, query = run(p, 0, 0, streams)
        round_trip(p, 0, streams, res)
    finally:
        L.fourmc_gpu_set_lz4_encode_mode(0)
    for s, st, g, q in zip(streams, res, got, query):
        groups, trailer = wm.plan(list(s["pattern"]), M)
        assert st["reason"] == 0 and len(g) <= q["image_bytes"]
        assert bm.shape(g, False)[0] == groups and g.endswith(b"\0\0\0\0") == trailer
        rd, back = bm.read_stream(g, False)
        assert rd["reason"] == bm.OK and back == T.text()[s["off"]:s["off"] + sum(s["pattern"])]
        assert (rd["groups"], rd["chunks"]) == (st["groups"], st["chunks"])


def test_argument_errors_on_the_device(p):
    d_img = torch.full((8192,), CANARY, dtype=torch.uint8, device="cuda")
    tab = torch.full((8,), 100, dtype=torch.int32, device="cuda")
    for items, kw in (([(0, 800, 0, 4000, 0, 9, 0)], {}), ([(0, 800, 0, 4000, 0, 8, 0)], dict(codec=7)),
                      ([(0, 800, 0, 4000, 0, 8, 0)], dict(codec=3, level=13)), ([(0, 800, 0, 100, 0, 8, 0), (0, 10, 99, 100, 0, 0, 0)], {})):
        with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstreams_compress failed \(-[35]\)"):
            p.compress_bstreams(d_text(), items, d_img, d_writes=tab, **kw)
    torch.cuda.synchronize()
    assert bool((d_img == CANARY).all())
