"""The lines of many splits with one call on the device (fourmc_gpu_image_read_lines_batch): every item against the model of
tests/lines_model.py and against fourmc_gpu_image_read_lines on the same image, on the images and splits of
tests/test_gpu_image_lines.py, with sentinel bytes around every region and every table region.  The comparisons run on the
device: a call's destination is a hundred megabytes, and only the verdicts cross to the host."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import helpers
import lines_model as lm
import test_gpu_image_lines as one

pytestmark = pytest.mark.gpu

B = helpers.B
SENT, SSENT, TSENT = one.SENT, one.SSENT, one.TSENT
FIELDS = one.FIELDS
LF, CR = 10, 13
UNTOUCHED = {"result": -3, "base": 0, "data_off": 0, "data_bytes": 0, "reserved": 0}


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


@pytest.fixture(scope="module")
def cases(p):
    out = {}
    for name, data in one._families().items():
        for tag, z in one.KINDS:
            c = one.Case(p, name, z, data)
            c.d_data = torch.from_numpy(data.copy()).cuda() if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")
            out[(name, tag)] = c
    yield out
    out.clear()
    p.release_workspaces()
    torch.cuda.empty_cache()


def _want(c, s, e, **kw):
    c.model.max_line_len = kw.pop("max_line_len", lm.DEFAULT_MAX)
    return c.model.lines(s, e, **kw)


class Batch:
    """One call: the regions packed into one destination and one pair of tables, and what came back.
    rows: (split_start, split_end, dst_cap, lines_cap).  guards: sentinel bytes in front of every region, with region i at an
    offset of residue phase + i mod 16 (and table region i behind 1 + i % 5 sentinel entries); without, the regions abut."""

    def __init__(self, p, d_img, nbytes, rows, guards=True, count_only=False, stream=None, max_line_len=lm.DEFAULT_MAX, tdtype=torch.int32,
                 phase=0):
        self.rows, self.count_only = rows, count_only
        off, toff, self.items = 0, 0, []
        for i, (s, e, cap, lcap) in enumerate(rows):
            if guards:
                off += 16
                off += (phase + i - off) % 16
                toff += 1 + i % 5
            self.items.append((s, e, off, cap, toff, lcap))
            off += cap
            toff += lcap
        self.dst_bytes, self.entries = off + 64, toff + 8
        self.d_dst = torch.full((self.dst_bytes,), SENT, dtype=torch.uint8, device="cuda")
        self.d_st = torch.full((self.entries,), SSENT, dtype=torch.int64, device="cuda")
        self.d_tl = torch.full((self.entries,), TSENT, dtype=torch.int32, device="cuda")
        # what the call may have written: regions are entered as their items are checked
        self.may = torch.zeros(self.dst_bytes, dtype=torch.bool, device="cuda")
        self.tmay = torch.zeros(self.entries, dtype=torch.bool, device="cuda")
        if stream is not None:
            torch.cuda.synchronize()
        self.out = p.image_read_lines_batch(d_img, self.items, self.d_dst, None if count_only else self.d_st,
                                            None if count_only else self.d_tl.view(tdtype), max_line_len=max_line_len,
                                            image_bytes=nbytes, stream=stream)
        torch.cuda.synchronize()

    def region(self, i):
        _, _, off, cap, _, _ = self.items[i]
        return self.d_dst[off:off + cap]

    def tables(self, i):
        _, _, _, _, toff, lcap = self.items[i]
        return self.d_st[toff:toff + lcap], self.d_tl[toff:toff + lcap]

    def check(self, i, want, content, key):
        """item i against the model's `want`: the fields; the content (a device tensor of data_bytes bytes or more) for a
        result >= 0 and for the -5 of lines_cap; the tables in full mode.  Only then is the item's region entered as writable:
        -3 and the -5 of dst_cap (the model's need exceeds the region) leave it to the sentinel check."""
        _, _, off, cap, toff, lcap = self.items[i]
        res = self.out[i]
        assert {f: res[f] for f in FIELDS} == {f: want[f] for f in FIELDS}, (key, i, res, {f: want[f] for f in FIELDS})
        if res["result"] >= 0 or (res["result"] == -5 and want["need"] <= cap):
            self.may[off:off + cap] = True
            nb = res["data_bytes"]
            if content is not None and nb:
                assert torch.equal(self.d_dst[off:off + nb], content[:nb]), (key, i, "content")
        if self.count_only:
            return
        st, tl = self.tables(i)
        k = res["result"]
        if k >= 0:
            self.tmay[toff:toff + k + 1] = True
            assert torch.equal(st[:k + 1], torch.from_numpy(np.asarray(want["starts"], np.int64)).cuda()), (key, i, "starts")
            assert torch.equal(tl[:k], torch.from_numpy(np.asarray(want["text_len"], np.int64).astype(np.int32)).cuda()), (key, i, "text_len")
            assert bool((tl[k:] == TSENT).all()), (key, i, "text_len behind the lines")

    def guards_intact(self, key=None):
        assert bool((self.d_dst[~self.may] == SENT).all()), (key, "bytes written outside the regions that may be written")
        assert bool((self.d_st[~self.tmay] == SSENT).all()), (key, "starts written outside the tables' regions")
        assert bool((self.d_tl[~self.tmay] == TSENT).all()), (key, "text lengths written outside the tables' regions")


def _single(p, c, d_img, nbytes, s, e, cap, lcap, count_only=False, max_line_len=lm.DEFAULT_MAX):
    """the single call with the same capacities -> (fields, d_dst, d_starts, d_text_len), guards checked"""
    d_dst = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    d_st = torch.full((lcap + 8,), SSENT, dtype=torch.int64, device="cuda")
    d_tl = torch.full((lcap + 8,), TSENT, dtype=torch.int32, device="cuda")
    if cap and (lcap or count_only):
        r = p.image_read_lines(d_img, s, e, d_dst[:cap], None if count_only else d_st[:lcap], None if count_only else d_tl[:lcap],
                               max_line_len=max_line_len, image_bytes=nbytes)
    else:                                                   # an empty slice of a tensor has no address: the C call, with capacity 0
        r = p.ImageLines()
        rc = p.lib().fourmc_gpu_image_read_lines(d_img.data_ptr(), nbytes, s, e, max_line_len, d_dst.data_ptr(), cap,
                                                 None if count_only else d_st.data_ptr(), None if count_only else d_tl.data_ptr(), lcap,
                                                 C.byref(r), None)
        assert rc == 0, (rc, p.lib().fourmc_gpu_last_error())
    torch.cuda.synchronize()
    assert bool((d_dst[cap:] == SENT).all()) and bool((d_st[lcap:] == SSENT).all()) and bool((d_tl[lcap:] == TSENT).all())
    return {f: int(getattr(r, f)) for f in FIELDS}, d_dst[:cap], d_st[:lcap], d_tl[:lcap]


def _equals_single(p, bt, i, c, d_img, nbytes, key, max_line_len=lm.DEFAULT_MAX):
    """item i of the batch against the single call on the same image with the same capacities: the fields, the content up to
    data_bytes, the tables' whole regions; a region the single call leaves untouched is untouched"""
    s, e, off, cap, toff, lcap = bt.items[i]
    res, dst, st, tl = _single(p, c, d_img, nbytes, s, e, cap, lcap, bt.count_only, max_line_len)
    got = bt.out[i]
    assert {f: got[f] for f in FIELDS} == res, (key, i, got, res)
    nb = res["data_bytes"] if res["result"] >= 0 or res["reserved"] else 0
    assert torch.equal(bt.region(i)[:nb], dst[:nb]), (key, i, "content")
    if bool((dst == SENT).all()):
        assert bool((bt.region(i) == SENT).all()), (key, i, "the single call leaves the region untouched")
    if not bt.count_only:
        bst, btl = bt.tables(i)
        assert torch.equal(bst, st) and torch.equal(btl, tl), (key, i, "tables")
    return res


def _rows_of(c, splits, exact=False, **kw):
    rows, wants = [], []
    for i, (s, e) in enumerate(splits):
        w = _want(c, s, e, **kw)
        rows.append((s, e, w["need"] + (0 if exact else (i * 7) % 23), max(w["result"], 0) + 1 + (0 if exact else i % 3)))
        wants.append(w)
    return rows, wants


def _family_call(p, c, splits, key, single=True, **kw):
    """all `splits` of one case in ONE call, each item against the model (and the single call)"""
    mx = kw.get("max_line_len", lm.DEFAULT_MAX)
    rows, wants = _rows_of(c, splits, exact=kw.pop("exact", False), max_line_len=mx)
    bt = Batch(p, c.d_img, c.size, rows, **kw)
    for i, w in enumerate(wants):
        bt.check(i, w, c.d_data[w["base"]:], key)
        if single:
            _equals_single(p, bt, i, c, c.d_img, c.size, key, mx)
    bt.guards_intact(key)
    return bt


# ---- 1, 2: every family, every split, one call ------------------------------------------------------------------------------
def test_every_split_of_every_family_in_one_call_equals_the_model_and_the_single_call(p, cases):
    rng = np.random.default_rng(11)
    n, residues, table_residues = 0, set(), set()
    for (name, tag), c in cases.items():
        splits = c.splits(rng)
        bt = _family_call(p, c, splits, (name, tag), phase=n)
        n += len(splits)
        residues |= {it[2] % 16 for it in bt.items if it[3]}
        table_residues |= {it[4] % 4 for it in bt.items}
    assert n > 200 and residues == set(range(16)) and table_residues == set(range(4))


def test_abutting_regions_of_exactly_the_needed_size(p, cases):
    """no guard between the regions and dst_cap == need: the end of one region and the start of the next share a 16-byte chunk"""
    rng = np.random.default_rng(11)
    shared = 0
    for (name, tag), c in cases.items():
        bt = _family_call(p, c, c.splits(rng), (name, tag), single=False, guards=False, exact=True)
        offs = [it[2] for it in bt.items if it[3]]
        shared += sum(1 for o in offs[1:] if o % 16)
        assert all(a[2] + a[3] == b[2] and a[4] + a[5] == b[4] for a, b in zip(bt.items, bt.items[1:]))
    assert shared > 100


# ---- 3: group cuts ----------------------------------------------------------------------------------------------------------
class _Env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("FOURMC_SPLIT_GROUP")
        if self.value is None:
            os.environ.pop("FOURMC_SPLIT_GROUP", None)
        else:
            os.environ["FOURMC_SPLIT_GROUP"] = str(self.value)

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("FOURMC_SPLIT_GROUP", None)
        else:
            os.environ["FOURMC_SPLIT_GROUP"] = self.old
        return False


GROUP_FAMILIES = ("three_blocks", "tail_only_cr_last", "tail_only_cr_last_lf", "cr_at_block_end", "mixed")


@pytest.mark.parametrize("group", [1, 2, 3])
def test_group_cuts_change_nothing_but_the_statistics(p, cases, group):
    for at, name in enumerate(GROUP_FAMILIES):
        for tag in (("4mc", "4mz")[at % 2],):               # both formats over the five families
            c = cases[(name, tag)]
            splits = c.splits(np.random.default_rng(13))
            key = (name, tag, group)
            with _Env(None):
                g0, r0, d0 = p.image_lines_batch_stats()
                base = _family_call(p, c, splits, key, single=False)
                g1, r1, d1 = p.image_lines_batch_stats()
            assert g1 - g0 == 1 and d1 - d0 <= (r1 - r0) + 1, key
            with _Env(group):
                cut = _family_call(p, c, splits, key, single=False)
                g2, r2, d2 = p.image_lines_batch_stats()
            assert g2 - g1 == -(-len(splits) // group), key
            assert d2 - d1 <= (r2 - r1) + (g2 - g1), key
            assert cut.out == base.out, key
            assert torch.equal(cut.d_st, base.d_st) and torch.equal(cut.d_tl, base.d_tl), key
            for i, w in enumerate(base.out):
                assert torch.equal(cut.region(i)[:w["data_bytes"]], base.region(i)[:w["data_bytes"]]), (key, i)


# ---- 4: tail rounds ---------------------------------------------------------------------------------------------------------
def test_tail_rounds_are_the_most_any_split_needs(p, cases):
    for tag in ("4mc", "4mz"):
        c = cases[("three_blocks", tag)]
        o = c.offsets
        assert len(o) == 4
        # the block-0 split stages block 1 (no line end) and block 2; the others one block or none
        g0, r0, d0 = p.image_lines_batch_stats()
        _family_call(p, c, [(0, o[1]), (o[2], o[3]), (o[3], c.size)], ("three_blocks", tag))
        g1, r1, d1 = p.image_lines_batch_stats()
        assert (g1 - g0, r1 - r0) == (1, 2) and d1 - d0 == 3, (tag, r1 - r0, d1 - d0)
        # alone, the split of block 2 needs one round
        _family_call(p, c, [(o[2], o[3]), (o[1], o[3])], ("three_blocks", tag))
        g2, r2, d2 = p.image_lines_batch_stats()
        assert (g2 - g1, r2 - r1, d2 - d1) == (1, 1, 2), tag
        # every split_end at or past the end mark: no round, one decode
        _family_call(p, c, [(0, c.size), (o[1], c.size), (o[3], c.size + 1000), (o[2], c.model.end_mark)], ("three_blocks", tag))
        g3, r3, d3 = p.image_lines_batch_stats()
        assert (g3 - g2, r3 - r2, d3 - d2) == (1, 0, 1), tag
        # the pending CR: block 1 is staged, ends with the CR, and block 2's first byte decides
        for name in ("tail_only_cr_last", "tail_only_cr_last_lf"):
            c = cases[(name, tag)]
            o = c.offsets
            _family_call(p, c, [(0, o[1])], (name, tag))
            g4, r4, d4 = p.image_lines_batch_stats()
            assert (g4 - g3, r4 - r3) == (1, 2), (name, tag)
            _family_call(p, c, [(o[1], o[2]), (0, o[1]), (o[2], c.size)], (name, tag))
            g5, r5, d5 = p.image_lines_batch_stats()
            assert (g5 - g4, r5 - r4) == (1, 2), (name, tag)
            g3, r3, d3 = g5, r5, d5


def test_three_blocks_first_split_stages_through_blocks_one_and_two(cases):
    c = cases[("three_blocks", "4mc")]
    w = _want(c, 0, c.offsets[1])
    assert w["data_bytes"] == 2 * B + B // 2 + 2            # hi lies in block 2: blocks 1 and 2 are staged, two rounds


# ---- 5: mixed verdicts in one call --------------------------------------------------------------------------------------------
def test_mixed_verdicts_in_one_call_equal_the_single_calls(p, cases):
    for tag in ("4mc", "4mz"):
        c = cases[("crlf_text", tag)]
        o = c.offsets
        body = bytearray(c.img); body[o[1] + 12 + 777] ^= 0x10          # block 1
        tail = bytearray(c.img); tail[o[2] + 12 + 5] ^= 0x10            # block 2
        s, e = o[1], o[2]                                               # block 1 is its body, block 2 its tail
        w = _want(c, s, e)
        nb, k = w["data_bytes"], w["result"]
        first = _want(c, 0, o[1])
        last = _want(c, o[2], c.size)
        inside = o[1] + 12 + 100
        for which, img in (("body", bytes(body)), ("tail", bytes(tail))):
            d_img = one._dev(img)
            rows = [(0, o[1], first["need"] + 5, first["result"] + 2),                  # reads block 0, stages block 1: clean unless that is damaged
                    (inside, c.size, 1000, 10),                                        # -3
                    (s, e, nb - 1, k + 1),                                             # dst_cap one short
                    (s, e, 0, k + 1),                                                  # the size query
                    (s, e, nb, k),                                                     # lines_cap one short
                    (s, e, nb + 3, k + 1),                                             # the damaged block itself
                    (o[2], c.size, last["need"], last["result"] + 1),                  # clean unless block 2 is damaged
                    (0, 5, 100, 3)]                                                    # -3
            bt = Batch(p, d_img, len(img), rows)
            key = (tag, which)
            res = [_equals_single(p, bt, i, c, d_img, len(img), key) for i in range(len(rows))]
            codes = [r["result"] for r in res]
            if which == "body":
                # block 1 is the tail block of block 0's split: the tail's -4, nothing written.  For block 1's own split the short
                # dst_cap wins over the body's -4, the body's -4 over the short tables; the split of block 2 is the clean one
                assert codes == [-4, -3, -5, -5, -4, -4, last["result"], -3], (key, codes)
                assert res[2]["data_bytes"] == res[3]["data_bytes"] == nb and res[4]["reserved"] == 0
                bt.check(6, last, c.d_data[last["base"]:], key)
                touched = (4, 5, 6)
            else:
                # the tail's -4 wins over everything behind it; block 0's split stages block 1 and is clean
                assert codes == [first["result"], -3, -4, -4, -4, -4, -4, -3], (key, codes)
                bt.check(0, first, c.d_data[first["base"]:], key)
                touched = (0, 6)
            for i in range(len(rows)):
                st, tl = bt.tables(i)
                if i not in touched:
                    assert bool((bt.region(i) == SENT).all()), (key, i)
                else:
                    bt.may[bt.items[i][2]:bt.items[i][2] + bt.items[i][3]] = True
                if codes[i] < 0:
                    assert bool((st == SSENT).all()) and bool((tl == TSENT).all()), (key, i)
            bt.guards_intact(key)
        # the clean image: both -5s as the model has them
        rows = [(s, e, nb - 1, k + 1), (s, e, 0, 0), (s, e, nb, k), (s, e, nb, k + 1)]
        bt = Batch(p, c.d_img, c.size, rows)
        wants = [_want(c, s, e, dst_cap=nb - 1), _want(c, s, e, dst_cap=0), _want(c, s, e, lines_cap=k), w]
        assert [x["result"] for x in wants] == [-5, -5, -5, k] and wants[2]["reserved"] == k and wants[1]["data_bytes"] == nb
        for i, x in enumerate(wants):
            bt.check(i, x, c.d_data[x["base"]:], tag)
            _equals_single(p, bt, i, c, c.d_img, c.size, tag)
        assert bool((bt.region(0) == SENT).all()) and bool((bt.tables(2)[0] == SSENT).all()) and bool((bt.tables(2)[1] == TSENT).all())
        bt.guards_intact(tag)


# ---- 6, 7 -------------------------------------------------------------------------------------------------------------------
def test_count_only_agrees_with_the_full_mode(p, cases):
    rng = np.random.default_rng(12)
    for (name, tag), c in cases.items():
        splits = c.splits(rng)[:4]
        full = _family_call(p, c, splits, (name, tag), single=False)
        count = _family_call(p, c, splits, (name, tag, "count"), single=False, count_only=True)
        assert count.out == full.out
        assert bool((count.d_st == SSENT).all()) and bool((count.d_tl == TSENT).all())
        for i, w in enumerate(full.out):
            assert torch.equal(count.region(i)[:w["data_bytes"]], full.region(i)[:w["data_bytes"]]), (name, tag, i)


def test_the_same_split_twice_gives_two_identical_results(p, cases):
    for key in (("mixed", "4mc"), ("cr_at_block_end", "4mz")):
        c = cases[key]
        s, e = c.offsets[1], c.offsets[2]
        bt = _family_call(p, c, [(s, e), (0, c.offsets[1]), (s, e)], key)
        assert bt.out[0] == bt.out[2] and bt.out[0]["result"] > 0
        nb = bt.out[0]["data_bytes"]
        assert torch.equal(bt.region(0)[:nb], bt.region(2)[:nb])
        k = bt.out[0]["result"]
        assert torch.equal(bt.tables(0)[0][:k + 1], bt.tables(2)[0][:k + 1]) and torch.equal(bt.tables(0)[1][:k], bt.tables(2)[1][:k])


# ---- 8: index codes -----------------------------------------------------------------------------------------------------------
def test_images_that_cannot_be_indexed_give_every_item_the_index_code(p, cases):
    for tag in ("4mc", "4mz"):
        c = cases[("crlf_text", tag)]
        small = cases[("one_block", tag)]
        foot = bytearray(c.img); foot[-1] ^= 1
        for img in (bytes(foot), c.img[:11], small.img + c.img):
            d_img = one._dev(img)
            info, _ = p.image_index(d_img, image_bytes=len(img))
            code = info["nblocks"] if info["nblocks"] < 0 else info["framing"]
            assert code < 0
            rows = [(0, len(img), 1000, 10), (c.offsets[1], c.offsets[2], 0, 0), (5, 7, 64, 1)]
            for count_only in (False, True):
                bt = Batch(p, d_img, len(img), rows, count_only=count_only)
                assert bt.out == [dict(UNTOUCHED, result=code)] * 3, (tag, len(img), bt.out)
                bt.guards_intact((tag, len(img)))
                assert _equals_single(p, bt, 0, c, d_img, len(img), tag)["result"] == code
        z = cases[("zero_blocks", tag)]
        rows = [(0, z.size, 16, 2), (0, 5, 0, 1), (12, z.size, 8, 1), (0, z.size + 9, 0, 0)]
        bt = Batch(p, z.d_img, z.size, rows)
        for i in range(len(rows)):
            _equals_single(p, bt, i, z, z.d_img, z.size, ("zero_blocks", tag))
        bt.tmay[:] = True                                   # the tables equal the single call's, entry for entry
        bt.guards_intact(("zero_blocks", tag))


# ---- 9: decode settings -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["seg", "tile", "zsingle"])
def test_decode_settings_give_the_same_lines(p, cases, setting):
    L = p.lib()
    path, split = L.fourmc_gpu_get_lz4_decode_path(), L.fourmc_gpu_get_zstd_decode_split()
    rng = np.random.default_rng(11)
    try:
        if setting == "zsingle":
            L.fourmc_gpu_set_zstd_decode_split(0)
        else:
            L.fourmc_gpu_set_lz4_decode_path({"seg": 11, "tile": 13}[setting])
        n = 0
        for name in ("crlf_text", "cr_at_block_end", "stored_block", "one_block"):
            for tag in ("4mc", "4mz"):
                splits = cases[(name, tag)].splits(rng)
                _family_call(p, cases[(name, tag)], splits, (name, tag, setting), single=False)
                n += len(splits)
        assert n > 30
    finally:
        L.fourmc_gpu_set_lz4_decode_path(path)
        L.fourmc_gpu_set_zstd_decode_split(split)


# ---- 10: the seams of the scan ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["cr_lf", "lone_cr", "cr_cr", "lf_cr"])
def test_a_terminator_across_every_seam_for_every_alignment_of_two_spans(p, variant):
    """As the single call's seam test, with two spans in one call: span 0 has 13 tiles, so its last tile and the first three of
    span 1 are the waves of one workgroup, and span 1 carries the seams at every shift of its region."""
    n = 3 * one.GROUP + 777
    rng = np.random.default_rng(5)
    pair = {"cr_lf": (CR, LF), "lone_cr": (CR, 98), "cr_cr": (CR, CR), "lf_cr": (LF, CR)}[variant]
    for shift in range(16):
        data = np.full(n, 97, np.uint8)
        data[rng.integers(0, n, 150)] = LF
        for q in one.SEAMS:
            at = q - 1 - shift
            data[at - 3:at + 5] = 97
            data[at], data[at + 1] = pair
        d_img = torch.empty(p.image_bound(n), dtype=torch.uint8, device="cuda")
        k = p.compress_image(torch.from_numpy(data).cuda(), d_img, p.MAGIC_4MC, 1)
        m = lm.Model(data, [12], [n], k - 12 - 20 - 4)
        want = m.lines(0, k)
        lines = want["result"]
        # two spans of the same split: the first at offset 0, the second behind it at residue `shift`
        lead = n + (16 - n % 16) % 16 + shift                # span 1's region starts at residue `shift`
        d_dst = torch.full((lead + n + 64,), SENT, dtype=torch.uint8, device="cuda")
        assert d_dst.data_ptr() % 16 == 0
        d_st = torch.full((2 * (lines + 1) + 4,), SSENT, dtype=torch.int64, device="cuda")
        d_tl = torch.full((2 * (lines + 1) + 4,), TSENT, dtype=torch.int32, device="cuda")
        items = [(0, k, 0, n, 0, lines + 1), (0, k, lead, n, lines + 1, lines + 1)]
        out = p.image_read_lines_batch(d_img, items, d_dst, d_st, d_tl, image_bytes=k)
        torch.cuda.synchronize()
        key = (variant, shift)
        dst, st, tl = d_dst.cpu().numpy(), d_st.cpu().numpy(), d_tl.cpu().numpy()
        for i, (_, _, off, _, toff, _) in enumerate(items):
            assert out[i] == {"result": lines, "base": 0, "data_off": 0, "data_bytes": n, "reserved": 0}, (key, i, out[i])
            assert np.array_equal(dst[off:off + n], data), (key, i)
            assert np.array_equal(st[toff:toff + lines + 1], want["starts"]), (key, i)
            assert np.array_equal(tl[toff:toff + lines], want["text_len"]) and tl[toff + lines] == TSENT, (key, i)
        assert (dst[n:lead] == SENT).all() and (dst[lead + n:] == SENT).all() and (st[2 * (lines + 1):] == SSENT).all(), key
        count = p.image_read_lines_batch(d_img, items, d_dst, image_bytes=k)
        assert [c["result"] for c in count] == [lines, lines], key


def test_a_tile_seam_of_one_span_and_the_first_tile_of_the_next_share_a_workgroup(p):
    """span 0 of a tile and a half: its tiles 0, 1 and span 1's tiles 0, 1 are the four waves of workgroup 0; a CR LF across
    span 0's tile seam and a CR in span 1's last byte of tile 0, LF behind it"""
    T = one.TILE
    n = T + T // 2
    a = np.full(n, 97, np.uint8)
    a[T - 1], a[T] = CR, LF
    a[100], a[n - 1] = LF, CR
    b = np.full(2 * T + 5, 98, np.uint8)
    b[T - 1], b[T] = CR, LF
    b[0], b[2 * T + 4] = LF, 99
    for data in (a, b):
        d_img = torch.empty(p.image_bound(len(data)), dtype=torch.uint8, device="cuda")
        k = p.compress_image(torch.from_numpy(data).cuda(), d_img, p.MAGIC_4MC, 1)
        want = lm.Model(data, [12], [len(data)], k - 12 - 20 - 4).lines(0, k)
        lines, nb = want["result"], len(data)
        d_dst = torch.full((3 * nb + 64,), SENT, dtype=torch.uint8, device="cuda")
        d_st = torch.full((3 * (lines + 1),), SSENT, dtype=torch.int64, device="cuda")
        d_tl = torch.full((3 * (lines + 1),), TSENT, dtype=torch.int32, device="cuda")
        items = [(0, k, i * nb, nb, i * (lines + 1), lines + 1) for i in range(3)]          # abutting
        out = p.image_read_lines_batch(d_img, items, d_dst, d_st, d_tl, image_bytes=k)
        torch.cuda.synchronize()
        st, tl = d_st.cpu().numpy(), d_tl.cpu().numpy()
        for i in range(3):
            assert out[i]["result"] == lines and out[i]["data_bytes"] == nb
            assert np.array_equal(st[i * (lines + 1):(i + 1) * (lines + 1)], want["starts"]), i
            assert np.array_equal(tl[i * (lines + 1):i * (lines + 1) + lines], want["text_len"]), i


# ---- 11: a side stream, and the workspaces given back ---------------------------------------------------------------------------
def test_a_side_stream_then_released_workspaces_then_a_second_call(p, cases):
    c = cases[("mixed", "4mc")]
    splits = [(c.offsets[1], c.size), (0, c.offsets[1]), (c.offsets[1], c.offsets[2])]
    side = torch.cuda.Stream()
    first = _family_call(p, c, splits, "side", single=False, stream=side)
    p.release_workspaces()
    second = _family_call(p, c, splits, "after release")
    assert first.out == second.out
    if hasattr(torch, "uint32"):
        _family_call(p, c, splits, "uint32", single=False, tdtype=torch.uint32)


# ---- 12: the partition property -------------------------------------------------------------------------------------------------
def test_aligned_partitions_read_every_line_once_in_one_call(p, cases):
    rng = np.random.default_rng(14)
    for key in (("cr_at_block_end", "4mz"), ("three_blocks", "4mc"), ("mixed", "4mc"), ("alternating_lfcr", "4mz"), ("tail_only_cr_last", "4mc")):
        c = cases[key]
        for _ in range(2):
            cuts = sorted(set(int(v) for v in rng.integers(1, c.size, 4)))
            edges = [0] + cuts + [c.size]
            kept = [(sl["split_start"], sl["split_end"]) for sl in p.image_align_slices(c.d_img, list(zip(edges, edges[1:])), image_bytes=c.size)
                    if sl["result"]]
            bt = _family_call(p, c, kept, key, single=False)
            got = []
            for i, r in enumerate(bt.out):
                got.extend((r["base"] + bt.tables(i)[0][:r["result"]].cpu().numpy()).tolist())
            assert got == c.model.file_lines()[:-1].tolist(), key
