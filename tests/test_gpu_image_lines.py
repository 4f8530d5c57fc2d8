"""The lines of a split by Hadoop's default rule on the device (fourmc_gpu_image_read_lines) against the model of
tests/lines_model.py, on .4mc and .4mz images compress_image made from the input families the CPU model test covers."""
import numpy as np
import pytest
import torch

import helpers
import lines_model as lm

pytestmark = pytest.mark.gpu

B = helpers.B
PAD = 4096
SENT = 0x5A
SSENT = -0x5A5A5A5A5A5A5A5B
TSENT = 0x5A5A5A5B
KINDS = [("4mc", False), ("4mz", True)]
FIELDS = ("result", "base", "data_off", "data_bytes", "reserved")
LF, CR = 10, 13


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
    rng = np.random.default_rng(2027)
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
    def __init__(self, p, name, z, data):
        self.name, self.z, self.data = name, z, data
        n = len(data)
        d_src = torch.from_numpy(data.copy()).cuda() if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
        d_img = torch.empty(p.image_bound(n), dtype=torch.uint8, device="cuda")
        k = p.compress_image(d_src, d_img, p.MAGIC_4MZ if z else p.MAGIC_4MC, 1)
        self.img = d_img[:k].cpu().numpy().tobytes()
        self.size = k
        blocks, _ = p.split_container(self.img, p.MAGIC_4MZ if z else p.MAGIC_4MC)
        self.offsets = [int(o) - 12 for o in blocks["src_off"]]
        self.usizes = [int(u) for u in blocks["dst_cap"]]
        self.csizes = [int(c) for c in blocks["src_len"]]
        end_mark = self.offsets[-1] + 12 + self.csizes[-1] if self.offsets else 12
        self.model = lm.Model(data, self.offsets, self.usizes, end_mark)
        self.d_img = _dev(self.img)

    def splits(self, rng):
        """each block alone, everything, and random contiguous partitions of the blocks"""
        heads = self.offsets + [self.size]
        out = {(0, self.size)}
        n = len(self.offsets)
        for i in range(n):
            out.add((heads[i] if i else 0, heads[i + 1]))
            out.add((heads[i], heads[i + 1]))                # block 0 from its header: not the start of the file
        for _ in range(3):
            cuts = sorted(set(int(c) for c in rng.integers(0, n + 1, 3))) if n else []
            edges = [0] + [heads[c] for c in cuts] + [self.size]
            out.update((a, z) for a, z in zip(edges, edges[1:]) if a < self.size)
        return sorted(out)


@pytest.fixture(scope="module")
def cases(p):
    out = {}
    for name, data in _families().items():
        for tag, z in KINDS:
            out[(name, tag)] = Case(p, name, z, data)
    yield out
    out.clear()                                             # hand the images, the engine's workspaces and torch's cache back
    p.release_workspaces()
    torch.cuda.empty_cache()


def _want(c, s, e, max_line_len, **kw):
    c.model.max_line_len = max_line_len
    return c.model.lines(s, e, **kw)


def _read(p, c, s, e, dst_cap=None, lines_cap=None, count_only=False, image=None, stream=None, max_line_len=lm.DEFAULT_MAX,
          tdtype=torch.int32):
    """-> (the struct as a dict, d_dst's bytes, d_starts' words, d_text_len's words), each table lines_cap long; the guards behind
    all three buffers are checked here, in every case"""
    want = _want(c, s, e, max_line_len)
    if dst_cap is None:
        dst_cap = want["need"] + 100
    if lines_cap is None:
        lines_cap = max(want["result"], 0) + 3
    d_dst = torch.full((dst_cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    d_st = None if count_only else torch.full((lines_cap + 8,), SSENT, dtype=torch.int64, device="cuda")
    d_tl = None if count_only else torch.full((lines_cap + 8,), TSENT, dtype=torch.int32, device="cuda").view(tdtype)
    d_img = c.d_img if image is None else _dev(image)
    nbytes = c.size if image is None else len(image)
    r = p.image_read_lines(d_img, s, e, d_dst[:dst_cap], None if count_only else d_st[:lines_cap], None if count_only else d_tl[:lines_cap],
                           max_line_len=max_line_len, image_bytes=nbytes, stream=stream)
    torch.cuda.synchronize()
    res = {f: int(getattr(r, f)) for f, _ in p.ImageLines._fields_}
    dst = d_dst.cpu().numpy()
    assert (dst[dst_cap:] == SENT).all(), "bytes written behind dst_cap"
    if count_only:
        return res, dst[:dst_cap], None, None
    st, tl = d_st.cpu().numpy(), d_tl.view(torch.int32).cpu().numpy()
    assert (st[lines_cap:] == SSENT).all(), "starts written behind lines_cap"
    assert (tl[lines_cap:] == TSENT).all(), "text lengths written behind lines_cap"
    return res, dst[:dst_cap], st[:lines_cap], tl[:lines_cap]


def _compare(p, c, s, e, max_line_len=lm.DEFAULT_MAX, **kw):
    want = _want(c, s, e, max_line_len)
    res, dst, st, tl = _read(p, c, s, e, max_line_len=max_line_len, **kw)
    key = (c.name, c.z, s, e, max_line_len)
    for f in FIELDS:
        assert res[f] == want[f], (key, f, res, {k: v for k, v in want.items() if k not in ("starts", "text_len")})
    nb = want["data_bytes"]
    assert np.array_equal(dst[:nb], c.data[want["base"]:want["base"] + nb]), key
    k = want["result"]
    assert np.array_equal(st[:k + 1], want["starts"]), key
    assert (st[k + 1:] == SSENT).all(), key
    assert np.array_equal(tl[:k], want["text_len"]), key
    assert (tl[k:] == TSENT).all(), key
    return res


def _all_splits(p, cases, names=None, **kw):
    rng = np.random.default_rng(11)
    n = 0
    for (name, tag), c in cases.items():
        if names is not None and name not in names:
            continue
        for s, e in c.splits(rng):
            _compare(p, c, s, e, **kw)
            n += 1
    return n


def test_every_split_of_every_family_equals_the_model(p, cases):
    assert _all_splits(p, cases) > 200
    stored = cases[("stored_block", "4mc")]
    assert any(u == cs for u, cs in zip(stored.usizes, stored.csizes)), "no stored block in the stored-block family"
    assert cases[("zero_blocks", "4mz")].offsets == [] and len(cases[("one_block", "4mc")].offsets) == 1
    # the block-end CR cases are what they claim to be: CR + LF, CR + another byte, CR + nothing, each at a block boundary
    c = cases[("cr_at_block_end", "4mc")]
    assert c.usizes == [B, B, B] and c.data[B - 1] == CR and c.data[B] == LF and c.data[2 * B - 1] == CR and c.data[2 * B] != LF
    assert c.data[-1] == CR and len(c.data) == 3 * B
    ends = c.model.P
    assert B - 1 not in ends and B in ends and 2 * B - 1 in ends and 3 * B - 1 in ends
    # ... and the split that ends behind block 0 stops behind the LF in block 1, the one that ends behind block 1 owns the line that starts block 2
    assert _want(c, 0, c.offsets[1], lm.DEFAULT_MAX)["data_bytes"] == B + 1
    assert _want(c, 0, c.offsets[2], lm.DEFAULT_MAX)["data_bytes"] > 2 * B      # the line that starts at de is this split's
    assert _want(c, c.offsets[2], c.size, lm.DEFAULT_MAX)["data_off"] > 0
    for name, nb in (("tail_only_cr_last", 2 * B), ("tail_only_cr_last_lf", 2 * B + 1)):
        c = cases[(name, "4mz")]
        assert not ((c.model.P >= B) & (c.model.P < 2 * B - 1)).any()
        assert _want(c, 0, c.offsets[1], lm.DEFAULT_MAX)["data_bytes"] == nb
    c = cases[("three_blocks", "4mc")]
    assert _want(c, 0, c.offsets[1], lm.DEFAULT_MAX)["data_bytes"] == 2 * B + B // 2 + 2


@pytest.mark.parametrize("setting", ["seg", "tile", "zsingle"])
def test_decode_settings_give_the_same_lines(p, cases, setting):
    L = p.lib()
    path, split = L.fourmc_gpu_get_lz4_decode_path(), L.fourmc_gpu_get_zstd_decode_split()
    try:
        if setting == "zsingle":
            L.fourmc_gpu_set_zstd_decode_split(0)
        else:
            L.fourmc_gpu_set_lz4_decode_path({"seg": 11, "tile": 13}[setting])
        assert _all_splits(p, cases, names=("crlf_text", "cr_at_block_end", "stored_block", "one_block")) > 30
    finally:
        L.fourmc_gpu_set_lz4_decode_path(path)
        L.fourmc_gpu_set_zstd_decode_split(split)


def test_count_only_agrees_with_the_full_mode(p, cases):
    rng = np.random.default_rng(12)
    for (name, tag), c in cases.items():
        for s, e in c.splits(rng)[:4]:
            want = _want(c, s, e, lm.DEFAULT_MAX)
            res, dst, _, _ = _read(p, c, s, e, count_only=True)
            assert {f: res[f] for f in FIELDS} == {f: want[f] for f in FIELDS}, (name, tag, s, e)
            assert np.array_equal(dst[:want["data_bytes"]], c.data[want["base"]:want["base"] + want["data_bytes"]])


# ---- the seams of the scan --------------------------------------------------------------------------------------------------
CHUNK, STEP, TILE, GROUP = 16, 1024, 16 * 1024, 64 * 1024
SEAMS = [3 * CHUNK, 40 * CHUNK, STEP, 5 * STEP, TILE - STEP, TILE, 2 * TILE, 3 * TILE, GROUP, GROUP + TILE, 2 * GROUP, 2 * GROUP + STEP,
         3 * GROUP - CHUNK]


@pytest.mark.parametrize("variant", ["cr_lf", "lone_cr", "cr_cr", "lf_cr"])
def test_a_terminator_across_every_seam_for_every_alignment_of_the_destination(p, variant):
    """The scan addresses d_dst in 16-byte chunks from d_dst rounded DOWN to 16, so byte q of the chunk walk is d_dst[q - shift]:
    for each shift of the destination the two bytes are placed with the first in the last byte of a chunk, of a 1 KiB wave
    step, of a 16 KiB tile and of a four-tile workgroup."""
    n = 3 * GROUP + 777
    rng = np.random.default_rng(5)
    pair = {"cr_lf": (CR, LF), "lone_cr": (CR, 98), "cr_cr": (CR, CR), "lf_cr": (LF, CR)}[variant]
    for shift in range(16):
        data = np.full(n, 97, np.uint8)
        data[rng.integers(0, n, 150)] = LF
        for q in SEAMS:
            at = q - 1 - shift
            data[at - 3:at + 5] = 97
            data[at], data[at + 1] = pair
        d_img = torch.empty(p.image_bound(n), dtype=torch.uint8, device="cuda")
        k = p.compress_image(torch.from_numpy(data).cuda(), d_img, p.MAGIC_4MC, 1)
        m = lm.Model(data, [12], [n], k - 12 - 20 - 4)
        want = m.lines(0, k)
        lines = want["result"]
        if variant == "cr_lf":
            assert all(q - 1 - shift not in m.P and q - shift in m.P for q in SEAMS)
        else:
            assert all(q - 1 - shift in m.P for q in SEAMS)
        d_dst = torch.full((n + 64,), SENT, dtype=torch.uint8, device="cuda")
        assert d_dst.data_ptr() % 16 == 0
        d_st = torch.full((lines + 1 + 4,), SSENT, dtype=torch.int64, device="cuda")
        d_tl = torch.full((lines + 4,), TSENT, dtype=torch.int32, device="cuda")
        r = p.image_read_lines(d_img, 0, k, d_dst[shift:shift + n], d_st[:lines + 1], d_tl[:lines], image_bytes=k)
        torch.cuda.synchronize()
        out, st, tl = d_dst.cpu().numpy(), d_st.cpu().numpy(), d_tl.cpu().numpy()
        key = (variant, shift)
        assert (r.result, r.base, r.data_off, r.data_bytes, r.reserved) == (lines, 0, 0, n, 0), key
        assert (out[:shift] == SENT).all() and (out[shift + n:] == SENT).all(), key
        assert np.array_equal(out[shift:shift + n], data), key
        assert np.array_equal(st[:lines + 1], want["starts"]) and (st[lines + 1:] == SSENT).all(), key
        assert np.array_equal(tl[:lines], want["text_len"]) and (tl[lines:] == TSENT).all(), key
        # count only sees the same seams
        assert p.image_read_lines(d_img, 0, k, d_dst[shift:shift + n], image_bytes=k).result == lines, key


def test_an_unaligned_destination_a_side_stream_and_uint32_lengths(p, cases):
    c = cases[("mixed", "4mc")]
    s, e = c.offsets[1], c.size
    want = _want(c, s, e, lm.DEFAULT_MAX)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert _compare(p, c, s, e, stream=side)["result"] == want["result"]
    p.release_workspaces()
    _compare(p, c, s, e)
    if hasattr(torch, "uint32"):
        _compare(p, c, s, e, tdtype=torch.uint32)


# ---- the one-byte call --------------------------------------------------------------------------------------------------------
def test_lf_only_text_agrees_with_image_read_records(p, cases):
    rng = np.random.default_rng(15)
    for tag in ("4mc", "4mz"):
        c = cases[("lf_only", tag)]
        assert not (c.data == CR).any()
        for s, e in c.splits(rng):
            res, dst, st, tl = _read(p, c, s, e)
            cap = len(st)
            d_dst = torch.full((len(dst),), SENT, dtype=torch.uint8, device="cuda")
            d_st = torch.full((cap,), SSENT, dtype=torch.int64, device="cuda")
            r = p.image_read_records(c.d_img, s, e, d_dst, d_st, delim=10, image_bytes=c.size)
            torch.cuda.synchronize()
            assert {f: int(getattr(r, f)) for f in FIELDS} == res, (tag, s, e)
            k = res["result"]
            one = d_st.cpu().numpy()
            assert np.array_equal(one[:k + 1], st[:k + 1]), (tag, s, e)
            if k:
                ends_open = c.data[res["base"] + res["data_bytes"] - 1] != LF           # an unterminated last line
                length = st[1:k + 1] - st[:k] - 1
                if ends_open:
                    length[-1] += 1
                assert np.array_equal(tl[:k], length), (tag, s, e)


# ---- max_line_len -------------------------------------------------------------------------------------------------------------
def test_truncation_changes_the_lengths_and_nothing_else(p, cases):
    rng = np.random.default_rng(16)
    for tag in ("4mc", "4mz"):
        c = cases[("mixed", tag)]
        for s, e in c.splits(rng)[:5]:
            full = _read(p, c, s, e)
            assert (full[3][:full[0]["result"]] > 5).any()
            for mx in (0, 1, 5, 0x7FFFFFFF):
                res = _compare(p, c, s, e, max_line_len=mx)
                got = _read(p, c, s, e, max_line_len=mx)
                assert got[0] == full[0] == res and np.array_equal(got[2], full[2]), (tag, s, e, mx)
                k = res["result"]
                assert np.array_equal(got[3][:k], np.minimum(full[3][:k], mx)), (tag, s, e, mx)


# ---- capacity and failure -----------------------------------------------------------------------------------------------------
def test_capacity_codes(p, cases):
    for key in (("crlf_text", "4mc"), ("stored_block", "4mz"), ("cr_at_block_end", "4mc"), ("three_blocks", "4mz"), ("ends_with_cr", "4mz")):
        c = cases[key]
        # three_blocks: the split of block 0 alone reaches through blocks 1 and 2 for the end of its last line
        for s, e in ((0, c.size), (0, c.offsets[1])) + (() if key[0] == "three_blocks" else ((c.offsets[1], c.offsets[2]),)):
            want = _want(c, s, e, lm.DEFAULT_MAX)
            nb, k = want["data_bytes"], want["result"]
            assert nb > 0 and k > 0
            # dst_cap one byte short: -5, the size that works, and not a byte of d_dst or of the tables touched
            short = c.model.lines(s, e, dst_cap=nb - 1)
            res, dst, st, tl = _read(p, c, s, e, dst_cap=nb - 1)
            assert short["result"] == -5 and res == {f: short[f] for f in FIELDS}, (key, s, e, res)
            assert (dst == SENT).all() and (st == SSENT).all() and (tl == TSENT).all()
            # exactly enough of everything
            res, dst, st, tl = _read(p, c, s, e, dst_cap=nb, lines_cap=k + 1)
            assert res["result"] == k and np.array_equal(st, want["starts"]) and np.array_equal(dst, c.data[want["base"]:want["base"] + nb])
            assert np.array_equal(tl[:k], want["text_len"]) and tl[k] == TSENT
            # lines_cap one short: -5 with the count, neither table written
            few = c.model.lines(s, e, lines_cap=k)
            res, dst, st, tl = _read(p, c, s, e, lines_cap=k)
            assert few["result"] == -5 and res == {f: few[f] for f in FIELDS}, (key, s, e, res)
            assert res["reserved"] == k and (st == SSENT).all() and (tl == TSENT).all()
    # a text_len table of one entry per line serves a starts table of one more
    c = cases[("crlf_text", "4mc")]
    want = _want(c, 0, c.size, lm.DEFAULT_MAX)
    k = want["result"]
    d_dst = torch.empty(want["data_bytes"], dtype=torch.uint8, device="cuda")
    d_st = torch.full((k + 1,), SSENT, dtype=torch.int64, device="cuda")
    d_tl = torch.full((k + 8,), TSENT, dtype=torch.int32, device="cuda")
    assert p.image_read_lines(c.d_img, 0, c.size, d_dst, d_st, d_tl[:k], image_bytes=c.size).result == k
    assert np.array_equal(d_tl.cpu().numpy()[:k], want["text_len"]) and bool((d_tl[k:] == TSENT).all())
    assert p.image_read_lines(c.d_img, 0, c.size, d_dst, d_st, d_tl[:k - 1], image_bytes=c.size).result == -5


def test_bad_split_offsets(p, cases):
    c = cases[("crlf_text", "4mc")]
    inside = c.offsets[1] + 12 + 100                          # inside block 1's payload
    for s, e in ((inside, c.size), (0, inside), (c.offsets[1] + 1, c.size), (c.offsets[2], c.offsets[1]), (5, c.size), (0, 5)):
        assert c.model.lines(s, e)["result"] == -3
        res, dst, st, tl = _read(p, c, s, e, dst_cap=1000, lines_cap=10)
        assert res == {"result": -3, "base": 0, "data_off": 0, "data_bytes": 0, "reserved": 0}, (s, e, res)
        assert (dst == SENT).all() and (st == SSENT).all() and (tl == TSENT).all()
    end_mark = c.offsets[-1] + 12 + c.csizes[-1]
    for e in (end_mark, end_mark + 1, c.size + 1000):
        assert _read(p, c, c.offsets[1], e)[0] == _read(p, c, c.offsets[1], c.size)[0]


def test_damaged_blocks_footers_and_multi_stream_images(p, cases):
    for tag in ("4mc", "4mz"):
        c = cases[("crlf_text", tag)]
        body = bytearray(c.img); body[c.offsets[1] + 12 + 777] ^= 0x10          # block 1
        tail = bytearray(c.img); tail[c.offsets[2] + 12 + 5] ^= 0x10            # block 2
        # a split of block 1 alone reads block 1 as its body and block 2 as its tail
        s, e = c.offsets[1], c.offsets[2]
        nb = _want(c, s, e, lm.DEFAULT_MAX)["data_bytes"]
        for img in (body, tail):
            res, dst, st, tl = _read(p, c, s, e, image=bytes(img))
            assert res["result"] == -4 and (st == SSENT).all() and (tl == TSENT).all(), tag
        # precedence: the tail's -4 comes before the -5 of dst_cap (hi is unknown), the -5 of dst_cap before the body's -4
        assert _read(p, c, s, e, image=bytes(tail), dst_cap=nb - 1)[0]["result"] == -4
        res, dst, st, tl = _read(p, c, s, e, image=bytes(body), dst_cap=nb - 1)
        assert (res["result"], res["data_bytes"]) == (-5, nb) and (dst == SENT).all()
        # ... and the body's -4 before the -5 of the tables
        assert _read(p, c, s, e, image=bytes(body), lines_cap=1)[0]["result"] == -4
        # splits that touch neither damaged block still read
        for img, (s2, e2) in ((body, (c.offsets[2], c.size)), (tail, (0, c.offsets[1]))):
            want = _want(c, s2, e2, lm.DEFAULT_MAX)
            res, dst, st, tl = _read(p, c, s2, e2, image=bytes(img))
            assert res["result"] == want["result"] and np.array_equal(st[:want["result"] + 1], want["starts"]), (tag, s2, e2)
            assert np.array_equal(tl[:want["result"]], want["text_len"])
        foot = bytearray(c.img); foot[-1] ^= 1
        res, dst, st, tl = _read(p, c, 0, c.size, image=bytes(foot))
        assert res["result"] == -2 and (dst == SENT).all() and (st == SSENT).all() and (tl == TSENT).all()
        assert _read(p, c, 0, 11, image=c.img[:11])[0]["result"] == -1
        # two streams back to back: the last stream's footer does not index the bytes before it, and the call gives the index
        # code, the one image_index and image_read_records give
        small = cases[("one_block", tag)]
        twice = small.img + c.img
        d_two = _dev(twice)
        info, _ = p.image_index(d_two, image_bytes=len(twice))
        code = info["nblocks"] if info["nblocks"] < 0 else info["framing"]
        assert code < 0
        d_dst = torch.full((1 << 20,), SENT, dtype=torch.uint8, device="cuda")
        one = p.image_read_records(d_two, 0, len(twice), d_dst, image_bytes=len(twice))
        res, dst, st, tl = _read(p, small, 0, len(twice), image=twice, dst_cap=1 << 20, lines_cap=10)
        assert res == {"result": code, "base": 0, "data_off": 0, "data_bytes": 0, "reserved": 0} and one.result == code
        assert (dst == SENT).all() and (st == SSENT).all() and (tl == TSENT).all()
    # the block behind a block-ending CR is a tail block too: staged to look at its first byte, -4 when it is damaged
    c = cases[("tail_only_cr_last", "4mc")]
    behind = bytearray(c.img); behind[c.offsets[2] + 12 + 5] ^= 0x10
    assert _read(p, c, 0, c.offsets[1], image=bytes(behind))[0]["result"] == -4


def test_aligned_partitions_read_every_line_once(p, cases):
    rng = np.random.default_rng(14)
    for key in (("cr_at_block_end", "4mz"), ("three_blocks", "4mc"), ("mixed", "4mc"), ("alternating_lfcr", "4mz"), ("tail_only_cr_last", "4mc")):
        c = cases[key]
        for _ in range(2):
            cuts = sorted(set(int(v) for v in rng.integers(1, c.size, 4)))
            edges = [0] + cuts + [c.size]
            got = []
            for sl in p.image_align_slices(c.d_img, list(zip(edges, edges[1:])), image_bytes=c.size):
                if sl["result"]:
                    res, dst, st, tl = _read(p, c, sl["split_start"], sl["split_end"])
                    got.extend((res["base"] + st[:res["result"]]).tolist())
            assert got == c.model.file_lines()[:-1].tolist(), key
