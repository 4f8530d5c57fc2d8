"""The line records of a split on the device (fourmc_gpu_image_align_slices / fourmc_gpu_image_read_records) against the model
of tests/records_model.py, on .4mc and .4mz images compress_image made from the input families the CPU model test covers."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers
import records_model as rm

pytestmark = pytest.mark.gpu

B = helpers.B
PAD = 4096
SENT = 0x5A
SSENT = -0x5A5A5A5A5A5A5A5B
KINDS = [("4mc", False), ("4mz", True)]


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
    rng = np.random.default_rng(2026)
    logs = helpers.corpus(4 * B, logs=True)
    at = [0]

    def text(n):
        a = np.roll(logs, -at[0])[:n].copy()
        at[0] += 1234567
        return a

    def noise(n):
        return rng.integers(0, 256, n, dtype=np.uint8)
    return rm.families(B, text, noise)


class Case:
    def __init__(self, p, name, z, data, delim):
        self.name, self.z, self.data, self.delim = name, z, data, delim
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
        self.model = rm.Model(data, self.offsets, self.usizes, end_mark, delim)
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
    for name, (data, delim) in _families().items():
        for tag, z in KINDS:
            out[(name, tag)] = Case(p, name, z, data, delim)
    return out


def _read(p, c, s, e, dst_cap=None, starts_cap=None, count_only=False, image=None, stream=None):
    """-> (the struct as a dict, d_dst's bytes with their guard, d_starts' words with their guard)"""
    want = c.model.records(s, e)
    if dst_cap is None:
        dst_cap = want["need"] + 100
    if starts_cap is None:
        starts_cap = max(want["result"], 0) + 3
    d_dst = torch.full((dst_cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    d_st = None if count_only else torch.full((starts_cap + 8,), SSENT, dtype=torch.int64, device="cuda")
    d_img = c.d_img if image is None else _dev(image)
    nbytes = c.size if image is None else len(image)
    r = p.image_read_records(d_img, s, e, d_dst[:dst_cap], None if count_only else d_st[:starts_cap], delim=c.delim,
                             image_bytes=nbytes, stream=stream)
    torch.cuda.synchronize()
    res = {f: int(getattr(r, f)) for f, _ in p.ImageRecords._fields_}
    dst = d_dst.cpu().numpy()
    st = None if count_only else d_st.cpu().numpy()
    assert (dst[dst_cap:] == SENT).all(), "bytes written behind dst_cap"
    assert st is None or (st[starts_cap:] == SSENT).all(), "starts written behind starts_cap"
    return res, dst[:dst_cap], None if st is None else st[:starts_cap]


def _compare(p, c, s, e, **kw):
    want = c.model.records(s, e)
    res, dst, st = _read(p, c, s, e, **kw)
    key = (c.name, c.z, s, e)
    for f in ("result", "base", "data_off", "data_bytes", "reserved"):
        assert res[f] == want[f], (key, f, res, {k: v for k, v in want.items() if k != "starts"})
    nb = want["data_bytes"]
    assert np.array_equal(dst[:nb], c.data[want["base"]:want["base"] + nb]), key
    k = want["result"] + 1
    assert np.array_equal(st[:k], want["starts"]), key
    assert (st[k:] == SSENT).all(), key
    return res


def _all_splits(p, cases, names=None):
    rng = np.random.default_rng(11)
    n = 0
    for (name, tag), c in cases.items():
        if names is not None and name not in names:
            continue
        for s, e in c.splits(rng):
            _compare(p, c, s, e)
            n += 1
    return n


def test_every_split_of_every_family_equals_the_model(p, cases):
    assert _all_splits(p, cases) > 100
    stored = cases[("stored_block", "4mc")]
    assert any(u == cs for u, cs in zip(stored.usizes, stored.csizes)), "no stored block in the stored-block family"
    assert cases[("zero_blocks", "4mz")].offsets == [] and len(cases[("one_block", "4mc")].offsets) == 1


@pytest.mark.parametrize("setting", ["seg", "tile", "zsingle"])
def test_decode_settings_give_the_same_records(p, cases, setting):
    L = p.lib()
    path, split = L.fourmc_gpu_get_lz4_decode_path(), L.fourmc_gpu_get_zstd_decode_split()
    try:
        if setting == "zsingle":
            L.fourmc_gpu_set_zstd_decode_split(0)
        else:
            L.fourmc_gpu_set_lz4_decode_path({"seg": 11, "tile": 13}[setting])
        assert _all_splits(p, cases, names=("block_edges", "three_blocks", "stored_block", "empty_records", "one_block")) > 40
    finally:
        L.fourmc_gpu_set_lz4_decode_path(path)
        L.fourmc_gpu_set_zstd_decode_split(split)


def test_count_only_agrees_with_the_full_mode(p, cases):
    rng = np.random.default_rng(12)
    for (name, tag), c in cases.items():
        for s, e in c.splits(rng)[:4]:
            want = c.model.records(s, e)
            res, dst, _ = _read(p, c, s, e, count_only=True)
            assert {f: res[f] for f in ("result", "base", "data_off", "data_bytes")} == {f: want[f] for f in ("result", "base", "data_off", "data_bytes")}, (name, tag, s, e)
            assert np.array_equal(dst[:want["data_bytes"]], c.data[want["base"]:want["base"] + want["data_bytes"]])


def test_an_unaligned_destination_and_a_side_stream(p, cases):
    c = cases[("empty_records", "4mc")]
    s, e = c.offsets[1], c.size
    want = c.model.records(s, e)
    for shift in (1, 7, 15):
        cap = want["data_bytes"]
        d_dst = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
        d_st = torch.full((want["result"] + 1,), SSENT, dtype=torch.int64, device="cuda")
        r = p.image_read_records(c.d_img, s, e, d_dst[shift:shift + cap], d_st, delim=c.delim, image_bytes=c.size)
        torch.cuda.synchronize()
        out = d_dst.cpu().numpy()
        assert r.result == want["result"] and r.data_bytes == cap
        assert (out[:shift] == SENT).all() and (out[shift + cap:] == SENT).all()
        assert np.array_equal(out[shift:shift + cap], c.data[want["base"]:want["base"] + cap])
        assert np.array_equal(d_st.cpu().numpy(), want["starts"])
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    res = _compare(p, c, s, e, stream=side)
    assert res["result"] == want["result"]
    p.release_workspaces()
    _compare(p, c, s, e)


def test_capacity_codes(p, cases):
    for key in (("block_edges", "4mc"), ("stored_block", "4mz"), ("no_trailing_delimiter", "4mc"), ("three_blocks", "4mz")):
        c = cases[key]
        # three_blocks: the split of block 0 alone reaches through blocks 1 and 2 for the end of its last record
        for s, e in ((0, c.size), (0, c.offsets[1])) + (() if key[0] == "three_blocks" else ((c.offsets[1], c.offsets[2]),)):
            want = c.model.records(s, e)
            nb, k = want["data_bytes"], want["result"]
            assert nb > 0 and k > 0
            # dst_cap one byte short: -5, the size that works, and not a byte of d_dst touched
            short = c.model.records(s, e, dst_cap=nb - 1)
            res, dst, st = _read(p, c, s, e, dst_cap=nb - 1)
            assert short["result"] == -5 and {f: res[f] for f in res} == {f: short[f] for f in res}, (key, s, e, res)
            assert (dst == SENT).all() and (st == SSENT).all()
            # exactly enough of both
            res, dst, st = _read(p, c, s, e, dst_cap=nb, starts_cap=k + 1)
            assert res["result"] == k and np.array_equal(st, want["starts"]) and np.array_equal(dst, c.data[want["base"]:want["base"] + nb])
            # starts_cap one short: -5 with the count, no start written
            few = c.model.records(s, e, starts_cap=k)
            res, dst, st = _read(p, c, s, e, starts_cap=k)
            assert few["result"] == -5 and {f: res[f] for f in res} == {f: few[f] for f in res}, (key, s, e, res)
            assert res["reserved"] == k and (st == SSENT).all()


def test_bad_split_offsets(p, cases):
    c = cases[("block_edges", "4mc")]
    inside = c.offsets[1] + 12 + 100                          # inside block 1's payload
    for s, e in ((inside, c.size), (0, inside), (c.offsets[1] + 1, c.size), (c.offsets[2], c.offsets[1]), (5, c.size), (0, 5)):
        assert c.model.records(s, e)["result"] == -3
        res, dst, st = _read(p, c, s, e, dst_cap=1000, starts_cap=10)
        assert res == {"result": -3, "base": 0, "data_off": 0, "data_bytes": 0, "reserved": 0}, (s, e, res)
        assert (dst == SENT).all() and (st == SSENT).all()
    # at or past the end mark is the end of the content, whatever the value
    end_mark = c.offsets[-1] + 12 + c.csizes[-1]
    for e in (end_mark, end_mark + 1, c.size + 1000):
        assert _read(p, c, c.offsets[1], e)[0] == _read(p, c, c.offsets[1], c.size)[0]


def test_damaged_blocks_and_footers(p, cases):
    for tag in ("4mc", "4mz"):
        c = cases[("block_edges", tag)]
        body = bytearray(c.img); body[c.offsets[1] + 12 + 777] ^= 0x10          # block 1
        tail = bytearray(c.img); tail[c.offsets[2] + 12 + 5] ^= 0x10            # block 2
        # a split of block 1 alone reads block 1 as its body and block 2 as its tail
        s, e = c.offsets[1], c.offsets[2]
        assert _read(p, c, s, e, image=bytes(body))[0]["result"] == -4
        assert _read(p, c, s, e, image=bytes(tail))[0]["result"] == -4
        # splits that touch neither damaged block still read
        for img, (s2, e2) in ((body, (c.offsets[2], c.size)), (tail, (0, c.offsets[1]))):
            want = c.model.records(s2, e2)
            res, dst, st = _read(p, c, s2, e2, image=bytes(img))
            assert res["result"] == want["result"] and np.array_equal(st[:want["result"] + 1], want["starts"]), (tag, s2, e2)
        foot = bytearray(c.img); foot[-1] ^= 1
        res, dst, st = _read(p, c, 0, c.size, image=bytes(foot))
        assert res["result"] == -2 and (dst == SENT).all() and (st == SSENT).all()
        res = p.image_align_slices(_dev(bytes(foot)), [(0, 100), (100, c.size)], image_bytes=c.size)
        assert [r["result"] for r in res] == [-2, -2]
        assert _read(p, c, 0, 11, image=c.img[:11])[0]["result"] == -1


def test_align_slices_equals_the_model_and_the_host_functions(p, cases):
    L = p.lib()
    rng = np.random.default_rng(13)
    for key in (("block_edges", "4mc"), ("stored_block", "4mz"), ("one_block", "4mc"), ("zero_blocks", "4mc")):
        c = cases[key]
        off = c.offsets
        raw = [(0, c.size), (0, 5), (0, 12), (0, 13), (5, 8), (c.size - 3, c.size), (c.size, c.size)]
        for o in off:
            raw += [(o, o + 1), (o + 1, o + 2), (o - 1, o), (o + 1, c.size), (1, o)]
        for _ in range(200):
            a, z = sorted(int(v) for v in rng.integers(0, c.size + 1, 2))
            raw.append((a, z))
        got = p.image_align_slices(c.d_img, raw, image_bytes=c.size)
        a64 = np.asarray(off, dtype=np.uint64)
        dropped = 0
        for (a, z), g in zip(raw, got):
            assert g == rm.align_slice(off, a, z, c.size), (key, a, z, g)
            if off:
                assert g["split_start"] == L.fourmc_index_align_start(a64.ctypes.data, len(off), a, z)
                assert g["split_end"] == L.fourmc_index_align_end(a64.ctypes.data, len(off), z, c.size)
            dropped += g["result"] == 0
        assert dropped > 0 or not off
        if off:
            small = got[raw.index((0, 5))]
            assert (small["split_start"], small["split_end"], small["block_count"], small["result"]) == (0, 12, 0, 1)
        assert p.image_align_slices(c.d_img, [], image_bytes=c.size) == []


def test_aligned_partitions_read_every_record_once(p, cases):
    rng = np.random.default_rng(14)
    for key in (("block_edges", "4mz"), ("three_blocks", "4mc"), ("empty_records", "4mc"), ("delimiter_0", "4mz")):
        c = cases[key]
        for _ in range(2):
            cuts = sorted(set(int(v) for v in rng.integers(1, c.size, 4)))
            edges = [0] + cuts + [c.size]
            got = []
            for sl in p.image_align_slices(c.d_img, list(zip(edges, edges[1:])), image_bytes=c.size):
                if sl["result"]:
                    res, dst, st = _read(p, c, sl["split_start"], sl["split_end"])
                    got.extend((res["base"] + st[:res["result"]]).tolist())
            assert got == c.model.file_records()[:-1].tolist(), key


def test_64_blocks_of_log_text_as_one_split(p):
    nb = 64
    data = helpers.corpus(nb * B + 54321, logs=True)
    d_src = torch.from_numpy(data).cuda()
    d_img = torch.empty(p.image_bound(len(data)) + PAD, dtype=torch.uint8, device="cuda")
    k = p.compress_image(d_src, d_img, p.MAGIC_4MC, 1)
    want = np.flatnonzero(data == 10) + 1
    open_end = data[-1] != 10
    records = len(want) + int(open_end)
    d_dst = torch.full((len(data) + 64,), SENT, dtype=torch.uint8, device="cuda")
    d_st = torch.full((records + 1 + 8,), SSENT, dtype=torch.int64, device="cuda")
    r = p.image_read_records(d_img, 0, k, d_dst[:len(data)], d_st[:records + 1], image_bytes=k)
    torch.cuda.synchronize()
    assert (r.result, r.base, r.data_off, r.data_bytes) == (records, 0, 0, len(data))
    assert torch.equal(d_dst[:len(data)], d_src) and bool((d_dst[len(data):] == SENT).all())
    st = d_st.cpu().numpy()
    full = np.concatenate([[0], want, [len(data)] if open_end else []]).astype(np.int64)
    assert np.array_equal(st[:records + 1], full) and (st[records + 1:] == SSENT).all()
    # the second half as a split of its own: the starts are the same records, from the first one that starts behind its first block's start
    info, ent = p.image_index(d_img, image_bytes=k)
    s = int(ent["image_off"][32])
    ds = 32 * B
    mine = full[full > ds]
    d_st.fill_(SSENT)
    r = p.image_read_records(d_img, s, k, d_dst[:len(data) - ds], d_st[:len(mine)], image_bytes=k)
    torch.cuda.synchronize()
    assert (r.result, r.base, r.data_off, r.data_bytes) == (len(mine) - 1, ds, int(mine[0]) - ds, len(data) - ds)
    assert np.array_equal(d_st.cpu().numpy()[:len(mine)], mine - ds)
