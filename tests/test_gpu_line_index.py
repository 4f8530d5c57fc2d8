"""Lines by number on the device (fourmc_gpu_image_line_index / _image_read_lines_at) against the model of
tests/line_index_model.py, on .4mc and .4mz images compress_image made from the input families of lines_model.families, on one
hand-framed image whose blocks are no multiple of anything, and - the one rule - against fourmc_gpu_image_read_lines on the device."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
import line_index_model as lim
import lines_model as lm

pytestmark = pytest.mark.gpu

B = helpers.B
PAD = 4096
SENT = 0x5A
TSENT = 0x5A5A5A5B
KINDS = [("4mc", False), ("4mz", True)]
LF, CR = 10, 13
EINVAL = -3
ROW_BYTES = (1, 16, 100, 4096)
MAXES = (0, 7, lm.DEFAULT_MAX)
NAMES = ["crlf_text", "cr_only", "lf_only", "mixed", "all_cr", "all_lf", "alternating_crlf", "alternating_lfcr", "no_terminator",
         "zero_blocks", "one_block", "stored_block", "cr_at_block_end", "ends_with_crlf", "ends_with_cr", "tail_only_cr_last",
         "tail_only_cr_last_lf", "three_blocks"]


def _dev(b, pad=PAD):
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    t = torch.zeros(len(a) + pad, dtype=torch.uint8, device="cuda")
    if len(a):
        t[:len(a)] = torch.from_numpy(a.copy()).cuda()
    return t


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


def _families():
    rng = np.random.default_rng(2028)
    logs = helpers.corpus(4 * B, logs=True)
    assert not (logs == CR).any()
    at = [0]

    def text(n):
        a = np.roll(logs, -at[0])[:n].copy()
        at[0] += 1234567
        return a

    def noise(n):
        return rng.integers(0, 256, n, dtype=np.uint8)
    return lm.families(B, text, noise)


class Case:
    """one image, its model (computed once, shared by the tests) and its device index (built once, on first use)"""

    def __init__(self, p, name, z, data=None, img=None, usizes=None):
        self.p, self.name, self.z, self.data = p, name, z, data
        if img is None:
            n = len(data)
            d_src = torch.from_numpy(data.copy()).cuda() if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
            d_img = torch.empty(p.image_bound(n), dtype=torch.uint8, device="cuda")
            k = p.compress_image(d_src, d_img, p.MAGIC_4MZ if z else p.MAGIC_4MC, 1)
            img = d_img[:k].cpu().numpy().tobytes()
        self.img, self.size = img, len(img)
        blocks, _ = p.split_container(self.img, p.MAGIC_4MZ if z else p.MAGIC_4MC)
        self.offsets = [int(o) - 12 for o in blocks["src_off"]]
        self.usizes = [int(u) for u in blocks["dst_cap"]]
        assert usizes is None or self.usizes == list(usizes)
        self.doff = np.concatenate([[0], np.cumsum(self.usizes)]).astype(np.int64)
        self.P = lm.line_ends(data)
        self.want_index, self.lines = lim.index(data, self.usizes)
        self.d_img = _dev(self.img)
        self._index = None

    def index(self):
        if self._index is None:
            self._index, info = self.p.image_line_index(self.d_img, image_bytes=self.size)
            assert info["result"] == 0, (self.name, info)
        return self._index

    def starts(self):
        """the starts of all lines and T behind them"""
        s = np.concatenate([[0], self.P + 1]) if len(self.data) else np.zeros(1, np.int64)
        return s if s[-1] == len(self.data) else np.append(s, len(self.data))

    def requests(self, rng):
        """every line of a small content; of a large one the first and last 64, every line that starts or ends within 2 bytes of a
        block seam, 2048 random ones with duplicates - shuffled - and two numbers past the last line"""
        n = self.lines
        if n <= 4096:
            ks = np.arange(n, dtype=np.int64)
        else:
            s = self.starts()
            near = []
            for z in self.doff[1:-1]:
                lo, hi = np.searchsorted(s, z - 2), np.searchsorted(s, z + 2, side="right")
                near.extend(range(max(int(lo) - 1, 0), min(int(hi) + 1, n)))     # lines that start there, and those that end there
            ks = np.concatenate([np.arange(64), np.arange(n - 64, n), np.asarray(near, dtype=np.int64), rng.integers(0, n, 2048)]).astype(np.int64)
        ks = np.concatenate([ks, [n, n + 5]]).astype(np.int64)
        rng.shuffle(ks)
        return ks


@pytest.fixture(scope="module")
def cases(p):
    out = {}
    for name, data in _families().items():
        for tag, z in KINDS:
            out[(name, tag)] = Case(p, name, z, data)
    assert sorted(n for n, _ in out) == sorted(NAMES * 2)
    yield out
    out.clear()                                             # hand the images, the engine's workspaces and torch's cache back
    p.release_workspaces()
    torch.cuda.empty_cache()


def _entries(index):
    return index.cpu().numpy().view(np.uint8).reshape(-1).view(lim.ENTRY)


def _index_raw(p, c, d_index, cap, d_img=None, size=None):
    info = p.ImageLineInfo()
    rc = p.lib().fourmc_gpu_image_line_index((c.d_img if d_img is None else d_img).data_ptr(), c.size if size is None else size,
                                             d_index.data_ptr() if d_index is not None else None, cap, C.byref(info),
                                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0, p.lib().fourmc_gpu_last_error()
    return {f: int(getattr(info, f)) for f, _ in p.ImageLineInfo._fields_}


def _check_read(c, got, ks, row_bytes, mx, pad, key):
    rows, tl, st = lim.lines_at(c.data, ks, row_bytes, mx, pad, P=c.P)
    g_st, g_tl, g_rows = got["status"].cpu().numpy(), got["text_len"].cpu().numpy(), got["rows"].cpu().numpy()
    assert np.array_equal(g_st, st), (key, np.flatnonzero(g_st != st)[:5], ks[np.flatnonzero(g_st != st)[:5]])
    assert np.array_equal(g_tl, tl), (key, ks[np.flatnonzero(g_tl != tl)[:5]])
    bad = np.flatnonzero((g_rows != rows).any(axis=1))
    assert not len(bad), (key, ks[bad[:5]], g_rows[bad[0]][:32], rows[bad[0]][:32])
    assert got["out"]["result"] == got["out"]["served"] == int((st == 1).sum()), (key, got["out"])


# ---- the index ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_index_equals_the_model(p, cases, name):
    for tag, _ in KINDS:
        c = cases[(name, tag)]
        index, info = p.image_line_index(c.d_img, image_bytes=c.size)
        torch.cuda.synchronize()
        nb = len(c.usizes)
        assert info == {"result": 0, "lines": c.lines, "ends": len(c.P), "total_bytes": len(c.data), "nblocks": nb}, (name, tag, info)
        got = _entries(index)
        assert len(got) == nb + 1 and np.array_equal(got, c.want_index), (name, tag, got, c.want_index)
        assert tuple(got[nb]) == (len(c.P), 0, 0)


def test_the_seam_cases_are_what_they_claim_to_be(cases):
    f = lambda name: [int(x) & 3 for x in cases[(name, "4mc")].want_index["flags"]]  # noqa: E731
    assert f("cr_at_block_end") == [1, 2, 0, 0]             # CR | LF, CR | x, CR at the end of the content
    assert f("tail_only_cr_last_lf")[1:3] == [1, 2] and f("tail_only_cr_last")[1:3] == [0, 0]
    assert f("alternating_lfcr")[:2] == [1, 3] and set(f("alternating_crlf")) == {0}        # B is even: only LF CR puts a pair on a seam
    assert set(f("all_cr")) == {0} and cases[("all_cr", "4mz")].lines == B + 500
    assert cases[("zero_blocks", "4mc")].usizes == [] and cases[("zero_blocks", "4mc")].lines == 0


def test_index_count_only_and_the_capacity_code(p, cases):
    for key in (("mixed", "4mc"), ("cr_at_block_end", "4mz"), ("zero_blocks", "4mc")):
        c = cases[key]
        nb = len(c.usizes)
        want = {"result": 0, "lines": c.lines, "ends": len(c.P), "total_bytes": len(c.data), "nblocks": nb, "pad": 0}
        assert _index_raw(p, c, None, 0) == want, key
        assert _index_raw(p, c, None, 1 << 40) == want, key
        d_index = torch.full((2 * (nb + 4),), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
        short = _index_raw(p, c, d_index, nb)               # one entry short: -5 with the counts, nothing written
        assert short == dict(want, result=-5), (key, short)
        assert bool((d_index == -0x5A5A5A5A5A5A5A5B).all()), key
        assert _index_raw(p, c, d_index, nb + 1) == want
        flat = d_index.cpu().numpy()
        assert np.array_equal(flat[:2 * (nb + 1)].view(np.uint8).view(lim.ENTRY), c.want_index), key
        assert (flat[2 * (nb + 1):] == -0x5A5A5A5A5A5A5A5B).all(), key


def test_index_of_damaged_images(p, cases):
    for tag in ("4mc", "4mz"):
        c = cases[("crlf_text", tag)]
        nb = len(c.usizes)
        body = bytearray(c.img); body[c.offsets[1] + 12 + 777] ^= 0x10
        d_index = torch.full((2 * (nb + 1),), 7, dtype=torch.int64, device="cuda")
        info = _index_raw(p, c, d_index, nb + 1, d_img=_dev(bytes(body)))
        assert info["result"] == -4 and bool((d_index == 7).all()), (tag, info)
        assert _index_raw(p, c, d_index, 1, d_img=_dev(bytes(body)))["result"] == -4          # before the -5 of index_cap
        foot = bytearray(c.img); foot[-1] ^= 1
        info = _index_raw(p, c, d_index, nb + 1, d_img=_dev(bytes(foot)))
        assert info["result"] == -2 and bool((d_index == 7).all()), (tag, info)
        assert _index_raw(p, c, None, 0, d_img=_dev(c.img[:11]), size=11)["result"] == -1
        index, info = p.image_line_index(_dev(bytes(foot)), image_bytes=c.size)
        assert index is None and info["result"] == -2


@pytest.mark.parametrize("group", ["1", "2"])
def test_the_group_knob_changes_no_index(p, cases, monkeypatch, group):
    monkeypatch.setenv("FOURMC_LINES_AT_GROUP", group)
    for key in (("cr_at_block_end", "4mc"), ("tail_only_cr_last_lf", "4mz"), ("alternating_crlf", "4mc"), ("three_blocks", "4mz")):
        c = cases[key]
        index, info = p.image_line_index(c.d_img, image_bytes=c.size)
        assert info["result"] == 0 and info["lines"] == c.lines and np.array_equal(_entries(index), c.want_index), (key, group)


# ---- the reads ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_reads_equal_the_model(p, cases, name):
    rng = np.random.default_rng(NAMES.index(name))
    ks = cases[(name, "4mc")].requests(rng)
    d_ks = torch.from_numpy(ks).cuda()
    for row_bytes in ROW_BYTES:
        for mx in MAXES:
            pad = (row_bytes + mx) & 0xFF
            for tag, _ in KINDS:
                c = cases[(name, tag)]
                got = p.image_read_lines_at(c.d_img, c.index(), d_ks, row_bytes, max_line_len=mx, pad=pad, image_bytes=c.size)
                torch.cuda.synchronize()
                _check_read(c, got, ks, row_bytes, mx, pad, (name, tag, row_bytes, mx))


@pytest.mark.parametrize("key", [("mixed", "4mc"), ("cr_at_block_end", "4mz")])
def test_the_one_rule_against_image_read_lines_on_the_device(p, cases, key):
    c = cases[key]
    n, T = c.lines, len(c.data)
    d_dst = torch.empty(T + 64, dtype=torch.uint8, device="cuda")
    d_st = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    for mx, row_bytes in ((lm.DEFAULT_MAX, 100), (7, 16)):
        d_tl = torch.empty(n, dtype=torch.int32, device="cuda")
        r = p.image_read_lines(c.d_img, 0, c.size, d_dst[:T], d_st, d_tl, max_line_len=mx, image_bytes=c.size)
        assert r.result == n
        ks = torch.arange(n, dtype=torch.int64, device="cuda")
        got = p.image_read_lines_at(c.d_img, c.index(), ks, row_bytes, max_line_len=mx, pad=0xEE, image_bytes=c.size)
        assert got["out"]["result"] == n and bool((got["status"] == 1).all())
        assert torch.equal(got["text_len"], d_tl)
        cut = torch.minimum(d_tl, torch.tensor(row_bytes, device="cuda", dtype=torch.int32)).to(torch.int64)
        col = torch.arange(row_bytes, device="cuda")[None, :]
        at = torch.clamp(d_st[:n, None] + col, max=T - 1)
        want = torch.where(col < cut[:, None], d_dst[at], torch.tensor(0xEE, dtype=torch.uint8, device="cuda"))
        assert torch.equal(got["rows"], want), (key, mx, row_bytes)


def _long_line(c):
    k = int(np.searchsorted(c.P, B // 2))
    assert c.P[k] >= 2 * B and c.P[k - 1] < B               # it starts in block 0 and ends in block 2
    return k


@pytest.mark.parametrize("group", [None, "1"])
def test_a_line_over_three_blocks(p, cases, monkeypatch, group):
    if group:
        monkeypatch.setenv("FOURMC_LINES_AT_GROUP", group)  # the line's start, middle and end in three rounds
    for tag, _ in KINDS:
        c = cases[("three_blocks", tag)]
        k = _long_line(c)
        ks = np.array([k, k - 1, k + 1, k], dtype=np.int64)
        d_ks = torch.from_numpy(ks).cuda()
        s0 = p.image_lines_at_stats()
        got = p.image_read_lines_at(c.d_img, c.index(), d_ks[:1], 64, image_bytes=c.size)
        _check_read(c, got, ks[:1], 64, lm.DEFAULT_MAX, 0, (tag, 64))
        assert got["out"]["blocks_staged"] == 2 == len(lim.needed_blocks(c.data, c.usizes, ks[:1], 64)), got["out"]      # not the middle block
        assert got["out"]["rounds"] == (2 if group else 1)
        s1 = p.image_lines_at_stats()
        assert tuple(b - a for a, b in zip(s0, s1)) == ((2, 2, 2) if group else (1, 1, 2))
        for row_bytes in (B + 100, 3 * B):                  # a seam inside the copy; the whole line
            got = p.image_read_lines_at(c.d_img, c.index(), d_ks, row_bytes, pad=1, image_bytes=c.size)
            _check_read(c, got, ks, row_bytes, lm.DEFAULT_MAX, 1, (tag, row_bytes))
            assert got["out"]["blocks_staged"] == 3 and got["out"]["rounds"] == (3 if group else 1)
        got = p.image_read_lines_at(c.d_img, c.index(), d_ks, 3 * B, max_line_len=9, image_bytes=c.size)
        _check_read(c, got, ks, 3 * B, 9, 0, (tag, "max 9"))
        assert got["out"]["blocks_staged"] == 2


def test_requests_inside_one_block_stage_one_block(p, cases):
    c = cases[("cr_at_block_end", "4mc")]
    assert len(c.usizes) == 3
    inside = np.flatnonzero((c.starts()[:-1] > B + 10) & (c.starts()[1:] < 2 * B - 10))
    ks = inside[np.random.default_rng(3).integers(0, len(inside), 500)].astype(np.int64)
    got = p.image_read_lines_at(c.d_img, c.index(), torch.from_numpy(ks).cuda(), 100, image_bytes=c.size)
    _check_read(c, got, ks, 100, lm.DEFAULT_MAX, 0, "one block")
    assert got["out"]["blocks_staged"] == 1 and got["out"]["rounds"] == 1


def test_lines_past_the_last_and_the_last_line_itself(p, cases):
    for name in ("no_terminator", "ends_with_cr", "ends_with_crlf", "all_lf", "one_block"):
        for tag, _ in KINDS:
            c = cases[(name, tag)]
            n = c.lines
            ks = np.array([n - 1, n, n + 1, 1 << 62, n - 1, (1 << 64) - 1], dtype=np.uint64).view(np.int64)
            got = p.image_read_lines_at(c.d_img, c.index(), torch.from_numpy(ks).cuda(), 100, pad=0x20, image_bytes=c.size)
            _check_read(c, got, ks.view(np.uint64), 100, lm.DEFAULT_MAX, 0x20, (name, tag))
            assert got["status"].tolist() == [1, -3, -3, -3, 1, -3]
            assert bool((got["rows"][1] == 0x20).all()) and got["text_len"].tolist()[1:4] == [0, 0, 0]
    assert cases[("no_terminator", "4mc")].lines == 1 and len(cases[("no_terminator", "4mc")].P) == 0


def test_an_image_without_blocks_refuses_every_request(p, cases):
    for tag, _ in KINDS:
        c = cases[("zero_blocks", tag)]
        assert c.index().shape == (1, 2)
        ks = np.array([0, 1, 5], dtype=np.int64)
        got = p.image_read_lines_at(c.d_img, c.index(), torch.from_numpy(ks).cuda(), 16, pad=9, image_bytes=c.size)
        assert got["status"].tolist() == [-3, -3, -3] and bool((got["rows"] == 9).all()) and got["text_len"].tolist() == [0, 0, 0]
        assert got["out"] == {"result": 0, "served": 0, "blocks_staged": 0, "rounds": 0}


def test_a_damaged_block_fails_only_the_requests_that_need_it(p, cases):
    for tag, _ in KINDS:
        c = cases[("crlf_text", tag)]
        body = bytearray(c.img); body[c.offsets[1] + 12 + 777] ^= 0x10          # block 1
        d_bad = _dev(bytes(body))
        s = c.starts()
        first_b = np.searchsorted(c.doff, s[:-1], side="right") - 1             # the block of each line's first byte ...
        last_b = np.searchsorted(c.doff, np.maximum(s[1:] - 1, 0), side="right") - 1     # ... and of its last, terminator included
        bp = np.searchsorted(c.doff, np.maximum(s[:-1] - 1, 0), side="right") - 1        # the block holding the end before it
        rng = np.random.default_rng(8)
        over = np.searchsorted(s, c.doff[1:-1], side="right") - 1                # the lines that lie over the seams, and their neighbours
        ks = np.concatenate([rng.integers(0, c.lines, 3000), over - 1, over, over + 1]).astype(np.int64)
        needs = (bp[ks] <= 1) & (last_b[ks] >= 1)
        assert needs.any() and (~needs).any() and (first_b[ks][needs] != last_b[ks][needs]).any()
        got = p.image_read_lines_at(d_bad, c.index(), torch.from_numpy(ks).cuda(), 100, pad=3, image_bytes=c.size)
        rows, tl, st = lim.lines_at(c.data, ks, 100, lm.DEFAULT_MAX, 3, P=c.P)
        g_st, g_tl, g_rows = got["status"].cpu().numpy(), got["text_len"].cpu().numpy(), got["rows"].cpu().numpy()
        assert np.array_equal(g_st, np.where(needs, -4, 1)), tag
        assert (g_tl[needs] == 0).all() and np.array_equal(g_tl[~needs], tl[~needs]) and np.array_equal(g_rows[~needs], rows[~needs]), tag
        assert got["out"]["result"] == int((~needs).sum())
        foot = bytearray(c.img); foot[-1] ^= 1
        got = p.image_read_lines_at(_dev(bytes(foot)), c.index(), torch.from_numpy(ks).cuda(), 100, image_bytes=c.size)
        assert got["out"]["result"] == -2 and bool((got["status"] == -2).all()) and bool((got["text_len"] == 0).all())


def _raw(p, c, index, entries, d_ks, n, rows, row_bytes, tl, st, mx=lm.DEFAULT_MAX, pad=0):
    out = p.ImageLinesAt()
    rc = p.lib().fourmc_gpu_image_read_lines_at(c.d_img.data_ptr(), c.size, index.data_ptr(), entries, d_ks.data_ptr(), n, mx, rows.data_ptr(),
                                                row_bytes, pad, tl.data_ptr(), st.data_ptr(), C.byref(out), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out


def test_guard_bytes_odd_addresses_and_odd_row_sizes(p, cases):
    c = cases[("mixed", "4mz")]
    rng = np.random.default_rng(21)
    for row_bytes, shift, n in ((37, 1, 300), (16, 7, 64), (4099, 3, 40), (1, 5, 1000)):
        ks = np.concatenate([rng.integers(0, c.lines, n - 2), [c.lines, 0]]).astype(np.int64)
        d_ks = torch.from_numpy(ks).cuda()
        rows = torch.full((shift + n * row_bytes + 64,), SENT, dtype=torch.uint8, device="cuda")
        tl = torch.full((n + 8,), TSENT, dtype=torch.int32, device="cuda")
        st = torch.full((n + 8,), TSENT, dtype=torch.int32, device="cuda")
        rc, out = _raw(p, c, c.index(), len(c.usizes) + 1, d_ks, n, rows[shift:], row_bytes, tl, st, pad=0xA5)
        assert rc == 0 and out.result == n - 1
        want_rows, want_tl, want_st = lim.lines_at(c.data, ks, row_bytes, lm.DEFAULT_MAX, 0xA5, P=c.P)
        flat = rows.cpu().numpy()
        assert (flat[:shift] == SENT).all() and (flat[shift + n * row_bytes:] == SENT).all(), (row_bytes, shift)
        assert np.array_equal(flat[shift:shift + n * row_bytes].reshape(n, row_bytes), want_rows), (row_bytes, shift)
        assert np.array_equal(tl.cpu().numpy()[:n], want_tl) and bool((tl[n:] == TSENT).all())
        assert np.array_equal(st.cpu().numpy()[:n], want_st) and bool((st[n:] == TSENT).all())


def test_an_index_of_the_wrong_length_is_refused(p, cases):
    c = cases[("mixed", "4mc")]
    d_ks = torch.zeros(4, dtype=torch.int64, device="cuda")
    rows = torch.full((64,), SENT, dtype=torch.uint8, device="cuda")
    tl = torch.full((4,), TSENT, dtype=torch.int32, device="cuda")
    st = torch.full((4,), TSENT, dtype=torch.int32, device="cuda")
    for entries in (len(c.usizes), len(c.usizes) + 2, 0):
        rc, out = _raw(p, c, c.index(), entries, d_ks, 4, rows, 16, tl, st)
        assert rc == EINVAL and b"image_read_lines_at" in p.lib().fourmc_gpu_last_error()
        assert bool((rows == SENT).all()) and bool((tl == TSENT).all()) and bool((st == TSENT).all())
    with pytest.raises(p.EngineError, match=r"failed \(-3\)"):
        p.image_read_lines_at(c.d_img, c.index()[:-1].contiguous(), d_ks, 16, image_bytes=c.size)


def test_an_index_of_another_image_stays_inside_the_calls_regions(p, cases):
    """wrong rows are allowed, a write outside the rows, or a fault, is not"""
    c = cases[("mixed", "4mc")]
    donor = cases[("crlf_text", "4mc")]
    assert len(donor.usizes) == len(c.usizes)
    n, row_bytes = 500, 100
    ks = np.random.default_rng(4).integers(0, 3 * c.lines, n).astype(np.int64)
    rows = torch.full((n * row_bytes + 64,), SENT, dtype=torch.uint8, device="cuda")
    tl = torch.full((n + 8,), TSENT, dtype=torch.int32, device="cuda")
    st = torch.full((n + 8,), TSENT, dtype=torch.int32, device="cuda")
    garbage = torch.from_numpy(np.random.default_rng(5).integers(-(1 << 62), 1 << 62, donor.index().numel())).cuda().view(-1, 2)
    for index in (donor.index(), garbage):
        rc, out = _raw(p, c, index, len(c.usizes) + 1, torch.from_numpy(ks).cuda(), n, rows, row_bytes, tl, st)
        assert rc == 0
        assert bool((rows[n * row_bytes:] == SENT).all()) and bool((tl[n:] == TSENT).all()) and bool((st[n:] == TSENT).all())


def test_a_hand_framed_image_whose_blocks_align_with_nothing(p):
    """stored blocks of 1, 15, 16385, B - 1 and 17 bytes (tiles and chunks never line up with the blocks), a CR or an LF on every seam"""
    usizes = [1, 15, 16385, B - 1, 17]
    T = sum(usizes)
    rng = np.random.default_rng(77)
    data = rng.choice(np.frombuffer(b"abcdefgh \n", np.uint8), T).copy()
    doff = np.concatenate([[0], np.cumsum(usizes)])
    data[0] = CR; data[1] = LF                               # block 0 is a CR whose LF opens block 1
    data[doff[2] - 1] = CR; data[doff[2]] = 120              # a lone CR in block 1's last byte
    data[doff[3] - 3:doff[3] + 1] = np.frombuffer(b"\r\n\r\n", np.uint8)   # CR LF, CR | LF over the seam of blocks 2 and 3
    data[doff[4] - 1] = LF; data[doff[4]] = LF               # an empty line opens block 4
    data[-1] = 122                                           # and the content ends unterminated
    L = p.lib()
    sums = [L.fourmc_XXH32(data[a:z].ctypes.data, int(z - a), 0) for a, z in zip(doff, doff[1:])]
    img = p.assemble_container(p.MAGIC_4MC, usizes, usizes, sums, [data[a:z].tobytes() for a, z in zip(doff, doff[1:])])
    c = Case(p, "hand_framed", False, data, img=img, usizes=usizes)
    assert [int(f) & 3 for f in c.want_index["flags"][:5]] == [1, 2, 1, 2, 0]
    index, info = p.image_line_index(c.d_img, image_bytes=c.size)
    assert info == {"result": 0, "lines": c.lines, "ends": len(c.P), "total_bytes": T, "nblocks": 5}
    assert np.array_equal(_entries(index), c.want_index), (_entries(index), c.want_index)
    ks = c.requests(np.random.default_rng(6))
    assert c.lines > 4096
    for row_bytes, mx in ((1, lm.DEFAULT_MAX), (16, 7), (100, lm.DEFAULT_MAX), (4096, 0)):
        got = p.image_read_lines_at(c.d_img, index, torch.from_numpy(ks).cuda(), row_bytes, max_line_len=mx, pad=0x7E, image_bytes=c.size)
        _check_read(c, got, ks, row_bytes, mx, 0x7E, ("hand_framed", row_bytes, mx))
    first = np.arange(8, dtype=np.int64)                    # the lines of the first three blocks
    got = p.image_read_lines_at(c.d_img, index, torch.from_numpy(first).cuda(), 64, image_bytes=c.size)
    _check_read(c, got, first, 64, lm.DEFAULT_MAX, 0, "hand_framed first")
