""".4mc / .4mz images written as Hadoop's FourMcOutputStream cuts them, many per call (fourmc_gpu_images_compress_writes /
compress_images_writes).

The device is compared byte for byte with the closed form of tests/fourmc_stream_model.py (which tests/test_fourmc_stream_cpu.py
holds against the stream restated buffer by buffer), the oracle as block compressor.  The catalogue of tests/fourmc_stream_cases.py
is encoded with ONE call per (magic, level): level 1 of both formats runs all of it, levels 2 to 4 the reduced one, whose blocks stay
below 256 KiB.  Every image region is its queried size, lies between guard bytes of one value, and everything outside the written
images must still hold that value afterwards.  Then the images are read back by the existing readers, on block sizes they have not
seen in a test before."""
import os

import numpy as np
import pytest
import torch

import bstream_model as bm
import bstream_writes_model as wm
import fourmc_stream_cases as cases
import fourmc_stream_model as fm
import helpers
import line_index_model as lim
import lines_model as lm

pytestmark = pytest.mark.gpu

M = fm.M4
MC, MZ = fm.MAGIC_4MC, fm.MAGIC_4MZ
CANARY, GUARD, SLACK = 0xA7, 64, 4096
KINDS = [(MC, 1), (MZ, 1)] + [(m, lv) for lv in (2, 3, 4) for m in (MC, MZ)]
IDS = ["%s-%d" % ("4mc" if m == MC else "4mz", lv) for m, lv in KINDS]
_MEMO = {}


@pytest.fixture(scope="module")
def p(gpu):
    yield gpu
    _MEMO.clear()
    gpu.release_workspaces()
    torch.cuda.empty_cache()


def catalogue(level):
    return cases.full() if level == 1 else cases.reduced()


def want(magic, level, c):
    """(image, block offsets, block lengths, stored flags) of one case by the model, the oracle's compressor memoized by content"""
    key = ("want", magic, level, c.name, len(c.data))
    if key not in _MEMO:
        cb = fm.compressor(magic, level)

        def comp(b):
            k = ("blk", magic, level, b)
            if k not in _MEMO:
                _MEMO[k] = cb(b)
            return _MEMO[k]
        _MEMO[key] = fm.image(c.data, c.sizes, comp, magic)
    return _MEMO[key]


def sources(cs):
    """all sources in one device buffer, each at an odd distance from the one before; all tables in one, foreign entries between"""
    key = ("src", tuple(c.name for c in cs))
    if key not in _MEMO:
        buf, offs, tab, toffs = bytearray(b"\x55" * 3), [], [7] * 3, []
        for c in cs:
            offs.append(len(buf))
            buf += c.data + b"\x55" * (3 if len(buf) % 2 else 5)
            toffs.append(len(tab))
            if not c.uniform:
                tab += c.sizes + [9] * 3
        _MEMO[key] = (torch.from_numpy(np.frombuffer(bytes(buf), np.uint8).copy()).cuda(), offs, tab, toffs)
    return _MEMO[key]


def run(p, cs, magic, level, caps=None, table_edit=None):
    """One compress_images_writes over the cases.  Returns (results, the written bytes per item or None for one with a verdict, the
    query's results, the rows, the image buffer).  caps: {item: image_cap} instead of the queried size; table_edit: {item: sizes}
    written into the table in place of the item's own (same count)."""
    d_src, offs, tab, toffs = sources(cs)
    tab = list(tab)
    rows = []
    for i, c in enumerate(cs):
        if c.uniform:
            rows.append([offs[i], len(c.data), 0, 0, 0, 0, c.write_bytes])
        else:
            ed = (table_edit or {}).get(i, c.sizes)
            assert len(ed) == len(c.sizes)
            tab[toffs[i]:toffs[i] + len(ed)] = ed
            rows.append([offs[i], len(c.data), 0, 0, toffs[i], len(c.sizes), 0])
    d_writes = torch.from_numpy(np.array(tab, np.uint32).view(np.int32)).cuda()
    query = p.compress_images_writes(d_src, [tuple(r) for r in rows], None, magic, level, d_writes=d_writes)
    at = GUARD
    for i, (r, c) in enumerate(zip(rows, cs)):
        r[2], r[3] = at, (caps or {}).get(i, fm.worst_case(c.sizes))
        at += r[3] + GUARD
    d_images = torch.full((at + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
    res = p.compress_images_writes(d_src, [tuple(r) for r in rows], d_images, magic, level, d_writes=d_writes, images_bytes=at)
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
    assert (out[~covered] == CANARY).all(), "bytes written outside the images"
    return res, got, query, rows, d_images


def the_run(p, magic, level):
    """the ONE call of a (magic, level) over its catalogue, shared by the tests"""
    key = ("run", magic, level)
    if key not in _MEMO:
        _MEMO[key] = run(p, catalogue(level), magic, level)
    return _MEMO[key]


# ---- the bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("magic,level", KINDS, ids=IDS)
def test_images_counts_and_query_equal_the_model(p, magic, level):
    cs = catalogue(level)
    res, got, query, rows, _ = the_run(p, magic, level)
    for i, (c, st, q, g) in enumerate(zip(cs, res, query, got)):
        img, offs, lens, stored = want(magic, level, c)
        assert st["reason"] == 0 == q["reason"], (c.name, st, q)
        assert (st["blocks"], st["stored_blocks"]) == (len(lens), sum(stored)), (c.name, st, lens, stored)
        assert g is not None and len(g) == st["image_bytes"] == len(img), (c.name, st, len(img))
        assert [o for o, _, _, _ in fm.parse(g)] == offs and [(u, k) for _, u, k, _ in fm.parse(g)] == [(u, k) for _, u, k, _ in fm.parse(img)], c.name
        assert g == img, (c.name, next(k for k in range(len(img)) if g[k] != img[k]))
        assert q == dict(st, image_bytes=fm.worst_case(c.sizes), stored_blocks=0), (c.name, q)
        assert st["image_bytes"] <= q["image_bytes"] <= p.image_writes_bound(len(c.data)), c.name
        if not c.data:
            assert len(g) == 44
    by = {c.name: st for c, st in zip(cs, res)}
    assert by["[1]"]["stored_blocks"] == 1 == by["[1]"]["blocks"] and by["noise [70000]"]["stored_blocks"] == 1
    if level == 1:
        assert [by[n]["blocks"] for n in ("[M/2, M/2, 1]", "[M-1, 2]", "[M-1, 1, 1]", "[M+1, 5]", "[1, M+1]", "[2M]", "uniform M+1")] == [2, 2, 2, 3, 3, 2, 3]
        assert by["noise [M]"]["stored_blocks"] == 1 and by["text then noise"]["stored_blocks"] == 1 and by["[2M]"]["stored_blocks"] == 0
        assert by["70000 writes of 100 with zeros"]["blocks"] == 2
    else:
        assert got[2] == got[3]                          # 3000 writes of 100 bytes: the table and write_bytes = 100 say the same


def test_nothing_to_do(p):
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    assert p.compress_images_writes(d, [], d, MC, 1) == [] and p.compress_images_writes(None, [], None, MZ, 3) == []


# ---- verdicts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
def test_cap_sum_and_write_items_between_good_ones(p, magic):
    cs = cases.reduced()
    table = cs[2].sizes
    worst = fm.worst_case(cs[4].sizes)
    short = list(table); short[-1] -= 1
    res, got, query, rows, _ = run(p, cs, magic, 1, caps={4: worst - 1}, table_edit={2: short})
    assert [st["name"] for st in res] == ["OK", "OK", "SUM", "OK", "CAP", "OK"] and [q["name"] for q in query] == ["OK", "OK", "SUM", "OK", "OK", "OK"]
    assert got[2] is None and got[4] is None             # (run checked that their regions still hold the guard value)
    assert (res[2]["image_bytes"], res[2]["blocks"], res[2]["stored_blocks"]) == (0, 0, 0)
    assert (res[4]["image_bytes"], res[4]["blocks"], res[4]["stored_blocks"]) == (worst, 1, 0) and query[4]["image_bytes"] == worst
    for i in (0, 1, 3, 5):
        assert got[i] == want(magic, 1, cs[i])[0], cs[i].name
    # an entry above 0x7FFFFFFF wins over the sum it spoils; the capacity of exactly the worst case is enough
    big = list(table); big[5] = 0x80000000
    res, got, _, _, _ = run(p, cs, magic, 1, table_edit={2: big})
    assert [st["name"] for st in res] == ["OK", "OK", "WRITE", "OK", "OK", "OK"] and (res[2]["image_bytes"], res[2]["blocks"]) == (0, 0)
    for i in (0, 1, 3, 4, 5):
        assert got[i] == want(magic, 1, cs[i])[0], cs[i].name


# ---- rounds ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
def test_rounds_of_three_blocks_end_inside_streams_and_inside_a_long_write(p, magic):
    """FOURMC_BSW_ROUND=3 (read at every call) over streams of 1, 1, 2, 3, 1, 3, 1 blocks: the second block of the write of 2M falls
    into the second round, the rounds end inside [1, M+1] and [M+1, 5]; the bytes are the model's, as the default run's are"""
    by = {c.name: c for c in cases.full()}
    cs = [by[n] for n in ("[0, 3, 0, 0, 5, 0]", "[1]", "[2M]", "[1, M+1]", "noise [70000]", "[M+1, 5]", "uniform 1000")]
    assert "FOURMC_BSW_ROUND" not in os.environ
    os.environ["FOURMC_BSW_ROUND"] = "3"
    try:
        res, got, _, _, _ = run(p, cs, magic, 1)
    finally:
        del os.environ["FOURMC_BSW_ROUND"]
    assert [st["blocks"] for st in res] == [1, 1, 2, 3, 1, 3, 1]
    for c, st, g in zip(cs, res, got):
        img, _, lens, stored = want(magic, 1, c)
        assert g == img and st["stored_blocks"] == sum(stored), c.name


# ---- next to the block streams --------------------------------------------------------------------------------------------------
def test_streams_and_images_take_turns_on_one_stream_and_keep_their_bytes(p):
    """compress_bstreams and compress_images_writes run through one host path and lease the same two workspace registries.  On one
    stream, with rounds of three chunks: block streams (LZ4 fast), .4mc images (level 1), block streams again, each over a source of
    0 bytes, one of 5 000 bytes written 7 at a time from the table and one of 12 000 bytes as uniform writes of 4 096; then the same
    with twice the items, so that both leases grow between the calls.  Every byte is the model's, and the streams come out the same
    before and after the images."""
    text = helpers.corpus(40000).tobytes()
    lz4, blk = bm.oracle_compressor(0, 0), fm.compressor(MC, 1)
    sevens = [7] * (5000 // 7) + [5000 % 7]
    d_src = torch.from_numpy(np.frombuffer(text + b"\0" * 64, np.uint8).copy()).cuda()
    d_writes = torch.from_numpy(np.array([9] * 3 + sevens, np.int32)).cuda()
    assert "FOURMC_BSW_ROUND" not in os.environ
    os.environ["FOURMC_BSW_ROUND"] = "3"
    try:
        for copies in (1, 2):
            srcs = [(off, k, sizes, tab) for c in range(copies)
                    for off, k, sizes, tab in ((11 + 17001 * c, 0, [], False), (11 + 17001 * c, 5000, sevens, True),
                                               (5011 + 17001 * c, 12000, wm.uniform(12000, 4096), False))]
            rows = [[off, k, 0, 0, 3 if tab else 0, len(sizes) if tab else 0, 0 if tab else 4096] for off, k, sizes, tab in srcs]
            want_s = [bm.write_stream(text[off:off + k], sizes, lz4, False) for off, k, sizes, _ in srcs]
            want_i = [fm.image(text[off:off + k], sizes, blk, MC)[0] for off, k, sizes, _ in srcs]

            def call(fn, caps, *args):
                at = GUARD
                for r, cap in zip(rows, caps):
                    r[2], r[3] = at, cap
                    at += cap + GUARD
                d_images = torch.full((at + SLACK,), CANARY, dtype=torch.uint8, device="cuda")
                res = fn(d_src, [tuple(r) for r in rows], d_images, *args, d_writes=d_writes, images_bytes=at)
                out = d_images.cpu().numpy()
                got = [out[r[2]:r[2] + st["image_bytes"]].tobytes() for r, st in zip(rows, res)]
                for r, st in zip(rows, res):
                    assert st["reason"] == 0 and st["image_bytes"] <= r[3], st
                    out[r[2]:r[2] + st["image_bytes"]] = CANARY
                assert (out == CANARY).all(), "bytes written outside the regions"
                return res, got
            s_caps = [p.bstream_writes_bound(k, 0) for _, k, _, _ in srcs]
            i_caps = [fm.worst_case(sizes) for _, _, sizes, _ in srcs]
            first = call(p.compress_bstreams, s_caps, 0, 0)
            images = call(p.compress_images_writes, i_caps, MC, 1)
            again = call(p.compress_bstreams, s_caps, 0, 0)
            assert first[1] == want_s and images[1] == want_i
            assert again == first
    finally:
        del os.environ["FOURMC_BSW_ROUND"]


# ---- the readers on uneven blocks -----------------------------------------------------------------------------------------------
UNEVEN = ("[1, M+1]", "[M+1, 5]", "[M-1, 2]", "70000 writes of 100 with zeros", "text then noise", "uniform M+1", "[0, 3, 0, 0, 5, 0]")


@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
def test_decompress_images_gives_the_data(p, magic):
    cs = cases.full()
    res, got, _, rows, d_images = the_run(p, magic, 1)
    caps = [len(c.data) for c in cs]
    dst_off = np.concatenate([[0], np.cumsum([k + 7 for k in caps])])
    d_dst = torch.full((int(dst_off[-1]) + 64,), CANARY, dtype=torch.uint8, device="cuda")
    back = p.decompress_images(d_images, [(r[2], st["image_bytes"], int(dst_off[i]), caps[i]) for i, (r, st) in enumerate(zip(rows, res))], d_dst, magic)
    out = d_dst.cpu().numpy()
    for i, (c, b, st) in enumerate(zip(cs, back, res)):
        assert b["exit_code"] == 0 and b["reason"] == 0 and b["total_bytes"] == len(c.data) and b["blocks"] == st["blocks"], (c.name, b)
        assert out[dst_off[i]:dst_off[i] + caps[i]].tobytes() == c.data, c.name
        assert (out[dst_off[i] + caps[i]:dst_off[i + 1]] == CANARY).all(), c.name


def _image(p, magic, name):
    """(case, a device copy of its image from the shared run, its size, the model's block offsets and lengths)"""
    cs = cases.full()
    i = next(k for k, c in enumerate(cs) if c.name == name)
    res, got, _, rows, d_images = the_run(p, magic, 1)
    _, offs, lens, _ = want(magic, 1, cs[i])
    n = res[i]["image_bytes"]
    d_img = torch.empty(n + 64, dtype=torch.uint8, device="cuda")
    d_img[:n] = d_images[rows[i][2]:rows[i][2] + n]
    return cs[i], d_img, n, offs, lens


@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
def test_align_slices_land_on_the_models_block_offsets(p, magic):
    for name in UNEVEN:
        c, d_img, n, offs, lens = _image(p, magic, name)
        cuts = sorted({0, 1, 12, 13, n // 3, n // 2, n - 45, n - 1, n} | {o + d for o in offs for d in (-1, 0, 1, 12)})
        cuts = [k for k in cuts if 0 <= k <= n]
        slices = [(a, z) for a, z in zip(cuts[:-1], cuts[1:])] + [(0, n), (n // 2, n), (offs[-1] + 1, n)]
        got = p.image_align_slices(d_img, slices, image_bytes=n)
        for (a, z), g in zip(slices, got):
            assert g == lm.align_slice(offs, a, z, n), (name, a, z, g)
        kept = [g for g in got[:len(cuts) - 1] if g["result"] == 1]
        assert sum(g["block_count"] for g in kept) == len(offs), name      # the raw cuts partition the file: every block once


@pytest.mark.parametrize("magic", [MC, MZ], ids=["4mc", "4mz"])
def test_lines_of_the_whole_image_and_lines_by_number(p, magic):
    for name in UNEVEN:
        c, d_img, n, offs, lens = _image(p, magic, name)
        data = np.frombuffer(c.data, np.uint8)
        end_mark = n - 12 - 20 - 4 * len(offs)
        model = lm.Model(data, offs, lens, end_mark)
        w = model.lines(0, n)
        k = w["result"]
        d_dst = torch.full((w["need"] + 100 + 64,), CANARY, dtype=torch.uint8, device="cuda")
        d_st = torch.full((k + 4,), -7, dtype=torch.int64, device="cuda")
        d_tl = torch.full((k + 4,), -9, dtype=torch.int32, device="cuda")
        r = p.image_read_lines(d_img, 0, n, d_dst[:w["need"] + 100], d_st, d_tl, image_bytes=n)
        torch.cuda.synchronize()
        assert (int(r.result), int(r.data_bytes)) == (k, w["data_bytes"]), (name, int(r.result), k)
        assert d_dst[:w["data_bytes"]].cpu().numpy().tobytes() == c.data[w["base"]:w["base"] + w["data_bytes"]], name
        assert np.array_equal(d_st.cpu().numpy()[:k + 1], w["starts"]) and np.array_equal(d_tl.cpu().numpy()[:k], w["text_len"]), name
        assert bool((d_dst[w["need"] + 100:] == CANARY).all()) and bool((d_st[k + 1:] == -7).all()) and bool((d_tl[k:] == -9).all()), name
        # a split that starts at the second block, where there is one
        if len(offs) > 1:
            w2 = model.lines(offs[1], n)
            r2 = p.image_read_lines(d_img, offs[1], n, d_dst[:w["need"] + 100], d_st, d_tl, image_bytes=n)
            torch.cuda.synchronize()
            assert int(r2.result) == w2["result"] and np.array_equal(d_st.cpu().numpy()[:w2["result"] + 1], w2["starts"]), name
        index, info = p.image_line_index(d_img, image_bytes=n)
        ent, lines = lim.index(data, lens)
        assert info == {"result": 0, "lines": lines, "ends": int(ent[-1]["ends_before"]), "total_bytes": len(data), "nblocks": len(lens)}, (name, info)
        assert np.array_equal(index.cpu().numpy().view(np.uint8).reshape(-1).view(lim.ENTRY), ent), name
        ks = np.array(sorted({0, 1, lines // 2, max(lines - 2, 0), max(lines - 1, 0), lines, lines + 5} |
                             {int(e["ends_before"]) + d for e in ent for d in (-1, 0, 1) if int(e["ends_before"]) + d >= 0}), np.int64)
        got = p.image_read_lines_at(d_img, index, torch.from_numpy(ks).cuda(), 96, pad=0x2E, image_bytes=n)
        torch.cuda.synchronize()
        rows_w, tl_w, st_w = lim.lines_at(data, ks, 96, pad=0x2E)
        assert np.array_equal(got["status"].cpu().numpy(), st_w) and np.array_equal(got["text_len"].cpu().numpy(), tl_w), name
        assert np.array_equal(got["rows"].cpu().numpy(), rows_w), name


# ---- arguments on the device ----------------------------------------------------------------------------------------------------
def test_argument_errors_on_the_device(p):
    d_src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    d_img = torch.full((8192,), CANARY, dtype=torch.uint8, device="cuda")
    tab = torch.full((8,), 100, dtype=torch.int32, device="cuda")
    for items, kw in (([(0, 800, 0, 4000, 0, 9, 0)], {}), ([(0, 800, 0, 4000, 0, 8, 0)], dict(magic=7)),
                      ([(0, 800, 0, 1000, 0, 8, 0), (0, 10, 999, 100, 0, 0, 0)], {}), ([(4000, 97, 0, 1000, 0, 0, 0)], {})):
        with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_compress_writes failed \(-3\)"):
            p.compress_images_writes(d_src, items, d_img, d_writes=tab, **kw)
    torch.cuda.synchronize()
    assert bool((d_img == CANARY).all())
