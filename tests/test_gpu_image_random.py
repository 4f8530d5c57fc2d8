"""Random access into single-stream .4mc / .4mz images in device memory (fourmc_gpu_image_index / _decode_blocks / _read).
The oracle is the file API's own random access (fourmc_file_block_count / fourmc_file_decode_blocks) on the same bytes written to a
file, and the input the images were made from."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

B = helpers.B
PAD = 4096                                       # device images keep slack behind them, as the block decode's callers do
SENT = 0x5A
SIZES = [0, 1000, 2 * B, 12 * B + 12345]
KINDS = [("4mc-1", False, 1), ("4mc-3", False, 3), ("4mz-1", True, 1)]


def _dev(b, pad=PAD):
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    t = torch.zeros(len(a) + pad, dtype=torch.uint8, device="cuda")
    if len(a):
        t[:len(a)] = torch.from_numpy(a.copy()).cuda()
    return t


def _be(v):
    return int(v).to_bytes(4, "big")


def _refoot(img):
    """recompute the footer checksum of a single-stream image after an edit of its footer"""
    b = bytearray(img)
    fsz = int.from_bytes(b[-12:-8], "big")
    f0 = len(b) - fsz
    b[-4:] = _be(helpers.orc_xxh32(np.frombuffer(bytes(b[f0:-4]), np.uint8)))
    return bytes(b)


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


@pytest.fixture(scope="module")
def data():
    return helpers.corpus(12 * B + 12345, first_block=1)


@pytest.fixture(scope="module")
def images(p, data):
    out = {}
    for tag, z, level in KINDS:
        for n in SIZES:
            src = data[:n]
            d_src = torch.from_numpy(src.copy()).cuda() if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
            d_img = torch.empty(p.image_bound(n), dtype=torch.uint8, device="cuda")
            k = p.compress_image(d_src, d_img, p.MAGIC_4MZ if z else p.MAGIC_4MC, level)
            out[(tag, n)] = d_img[:k].cpu().numpy().tobytes()
    return out


class FileOracle:
    def __init__(self, p, tmp_path):
        self.L, self.dir, self.k = p.lib(), tmp_path, 0

    def _file(self, img):
        self.k += 1
        f = self.dir / f"img{self.k}.4mc"
        f.write_bytes(bytes(img))
        return str(f).encode()

    def count(self, img):
        z = C.c_int(-7)
        n = self.L.fourmc_file_block_count(self._file(img), C.byref(z))
        return n, z.value

    def decode(self, img, first, count, cap):
        buf = np.full(cap + 64, SENT, np.uint8)
        r = self.L.fourmc_file_decode_blocks(self._file(img), first, count, buf.ctypes.data, cap)
        return r, buf[:max(r, 0)].tobytes()


def dev_decode(p, img, first, count, cap, stream=None):
    d_img = _dev(img)
    d_dst = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    r = p.image_decode_blocks(d_img, first, count, d_dst[:cap], image_bytes=len(img), stream=stream)
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    assert (out[cap:] == SENT).all()                         # nothing beyond the capacity
    return r, out[:max(r, 0)].tobytes()


def host_index(p, img, z):
    blocks, _ = p.split_container(img, p.MAGIC_4MZ if z else p.MAGIC_4MC)
    return blocks


# ---- the index ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,z,level", KINDS)
def test_index_equals_the_host_walk_and_the_file_count(p, images, data, tmp_path, tag, z, level):
    orc = FileOracle(p, tmp_path)
    for n in SIZES:
        img = images[(tag, n)]
        info, ent = p.image_index(_dev(img), image_bytes=len(img))
        blocks = host_index(p, img, z)
        fn, fz = orc.count(img)
        assert info["nblocks"] == fn == len(blocks) and info["is_zstd"] == fz == int(z), (tag, n, info, fn, fz)
        assert info["framing"] == 0 and info["total_bytes"] == n, (tag, n, info)
        assert np.array_equal(ent["image_off"], blocks["src_off"] - 12)
        assert np.array_equal(ent["data_off"], blocks["dst_off"])
        assert np.array_equal(ent["usize"], blocks["dst_cap"]) and np.array_equal(ent["csize"], blocks["src_len"])
        assert np.array_equal(ent["xxh32"], blocks["xxh32"]) and not ent["pad"].any()


def _stored_image(p, nblocks, seed):
    """a single stream of `nblocks` stored blocks of 1..64 bytes (variable block sizes are legal: Hadoop's writer flushes)"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 65, nblocks)
    raw = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8)
    L = p.lib()
    pays, sums, at = [], [], 0
    for s in sizes.tolist():
        pay = raw[at:at + s]
        at += s
        pays.append(pay.tobytes())
        sums.append(L.fourmc_XXH32(pay.ctypes.data, s, 0))
    return raw, p.assemble_container(p.MAGIC_4MC, sizes, sizes, sums, pays)


def test_index_and_reads_at_16384_blocks(p, tmp_path):
    raw, img = _stored_image(p, 16384, 3)
    d_img = _dev(img)
    info, ent = p.image_index(d_img, image_bytes=len(img))
    blocks = host_index(p, img, False)
    assert info == {"nblocks": 16384, "framing": 0, "total_bytes": len(raw), "is_zstd": 0}
    assert np.array_equal(ent["image_off"], blocks["src_off"] - 12) and np.array_equal(ent["data_off"], blocks["dst_off"])
    # entries_cap below n: only the first entries are written
    L = p.lib()
    d_ent = torch.full((1000 * 32 + 64,), SENT, dtype=torch.uint8, device="cuda")
    ii = p.ImageIndexInfo()
    assert L.fourmc_gpu_image_index(d_img.data_ptr(), len(img), d_ent.data_ptr(), 1000, C.byref(ii), 0) == 0
    torch.cuda.synchronize()
    got = d_ent.cpu().numpy()
    assert ii.nblocks == 16384 and (got[1000 * 32:] == SENT).all()
    assert np.array_equal(got[:1000 * 32].view(p.IMAGE_ENTRY_DTYPE), ent[:1000])
    orc = FileOracle(p, tmp_path)
    for first, count in ((0, 16384), (16383, 1), (5000, 7000), (100, 1)):
        want = orc.decode(img, first, count, 64 * count)
        assert dev_decode(p, img, first, count, 64 * count) == want, (first, count)
    rng = np.random.default_rng(9)
    off = rng.integers(0, len(raw) - 2000, 512)
    ln = rng.integers(1, 2000, 512)
    dst = np.concatenate([[0], np.cumsum(ln[:-1] + 3)])
    d_dst = torch.full((int(dst[-1] + ln[-1]) + 64,), SENT, dtype=torch.uint8, device="cuda")
    res = p.image_read(d_img, np.stack([off, ln, dst], 1), d_dst, image_bytes=len(img))
    out = d_dst.cpu().numpy()
    assert np.array_equal(res, ln)
    for o, n_, d in zip(off, ln, dst):
        assert np.array_equal(out[d:d + n_], raw[o:o + n_])


# ---- the block-range twin -------------------------------------------------------------------------------------------
def _grid(n):
    g = [(0, 0), (0, n), (n, 1), (0, n + 1), (n + 3, 0)]
    if n:
        g += [(n - 1, 1), (max(n - 3, 0), 3), (n - 1, 2)]
    if n > 4:
        g += [(1, 1), (2, 5), (5, n - 5), (3, 0)]
    return g


@pytest.mark.parametrize("tag,z,level", KINDS)
def test_block_ranges_equal_the_file_api(p, images, tmp_path, tag, z, level):
    orc = FileOracle(p, tmp_path)
    for n_bytes in SIZES:
        img = images[(tag, n_bytes)]
        n = orc.count(img)[0]
        for first, count in _grid(n):
            cap = count * B
            want = orc.decode(img, first, count, cap)
            got = dev_decode(p, img, first, count, cap)
            assert got[0] == want[0] and got[1] == want[1], (tag, n_bytes, first, count, got[0], want[0])
            if want[0] > 0:                                      # one byte short: -5
                short = orc.decode(img, first, count, want[0] - 1)
                assert short[0] == -5 and dev_decode(p, img, first, count, want[0] - 1)[0] == -5
        if n:
            assert dev_decode(p, img, 0, n, n_bytes)[0] == n_bytes


def _crafted(p, images):
    base = images[("4mc-1", 12 * B + 12345)]
    n = len(base)
    fsz = int.from_bytes(base[-12:-8], "big")
    f0 = n - fsz
    ioff = [12]
    for _ in range(12):
        ioff.append(ioff[-1] + 12 + int.from_bytes(base[ioff[-1] + 4:ioff[-1] + 8], "big"))
    c = {}
    m = bytearray(base); m[1] ^= 0x40; c["bad_magic"] = bytes(m)
    m = bytearray(base); m[7] = 2; c["bad_version"] = bytes(m)
    m = bytearray(base); m[11] ^= 1; c["bad_header_checksum"] = bytes(m)
    m = bytearray(base); m[-1] ^= 1; c["bad_footer_checksum"] = bytes(m)
    m = bytearray(base); m[f0 + 7] = 2; c["bad_footer_version"] = _refoot(bytes(m))
    m = bytearray(base); m[-12:-8] = _be(fsz + 4); c["bad_tail_size"] = bytes(m)
    m = bytearray(base); m[-12:-8] = _be(fsz - 4); c["small_tail_size"] = bytes(m)
    m = bytearray(base); m[f0:f0 + 4] = _be(fsz - 4); c["bad_footer_size"] = _refoot(bytes(m))
    m = bytearray(base); m[-8:-4] = _be(p.MAGIC_4MZ); c["footer_magic"] = _refoot(bytes(m))
    for blk, d in ((3, 1), (3, -1), (0, 4), (11, 100), (12, -12)):
        m = bytearray(base)
        at = f0 + 8 + 4 * blk
        m[at:at + 4] = _be(int.from_bytes(m[at:at + 4], "big") + d)
        c[f"delta_{blk}_{d}"] = _refoot(bytes(m))
    m = bytearray(base); h = ioff[2]; m[h + 4:h + 8] = _be(B + 1); c["csize_beyond"] = bytes(m)
    m = bytearray(base); h = ioff[4]; m[h:h + 4] = _be(B + 1); c["usize_beyond"] = bytes(m)
    m = bytearray(base); m[ioff[5] + 12 + 777] ^= 0x10; c["flipped_payload"] = bytes(m)
    m = bytearray(base); m[ioff[12] + 2] ^= 1; c["tail_usize_changed"] = bytes(m)           # decodes to another size: -4
    m = bytearray(base); m[f0 - 5] = 1; c["end_mark_damaged"] = bytes(m)                   # never read by the file API
    for k in (1, 12, 30):
        c[f"trunc_{k}"] = base[:n - k]
    c["trunc_short"] = base[:11]
    c["trunc_header"] = base[:12]
    c["empty"] = b""
    c["trailing_3"] = base + b"xyz"
    c["trailing_44"] = base + bytes(range(44))
    c["concat"] = base + base
    c["concat_small"] = base + images[("4mc-1", 1000)]
    c["concat_4mz"] = images[("4mz-1", 1000)] + images[("4mz-1", 2 * B)]
    return c


def test_crafted_images_end_as_the_file_api_ends(p, images, tmp_path):
    orc = FileOracle(p, tmp_path)
    seen = set()
    for name, img in _crafted(p, images).items():
        n, _ = orc.count(img)
        info, _ = p.image_index(_dev(img), image_bytes=len(img))
        assert info["nblocks"] == n, (name, info, n)
        grid = [(0, 0), (0, 1), (0, 12), (11, 1), (1, 1), (2, 3), (3, 2), (4, 8), (0, 13), (5, 1), (12, 1)]
        for first, count in grid:
            cap = count * B + 64
            want, _ = orc.decode(img, first, count, cap)
            got, _ = dev_decode(p, img, first, count, cap)
            assert got == want, (name, first, count, got, want)
            seen.add(want)
        # the index's verdict is decode_blocks(0, n) with unlimited capacity - but for the payloads, which it does not decode
        want = orc.decode(img, 0, n, max(n, 0) * B + 64)[0] if n >= 0 else n
        payload_only = name in ("flipped_payload", "tail_usize_changed")
        assert info["framing"] == (0 if want >= 0 or payload_only else want), (name, info, want)
    assert {-1, -2, -3, -4}.issubset(seen), seen


# ---- byte ranges ----------------------------------------------------------------------------------------------------
def _read(p, img, triples, cap=None, stream=None):
    d_img = _dev(img)
    t = np.asarray(triples, dtype=np.uint64).reshape(-1, 3)
    if cap is None:
        cap = int((t[:, 1] + t[:, 2]).max()) if len(t) else 0
    d_dst = torch.full((cap + 64,), SENT, dtype=torch.uint8, device="cuda")
    res = p.image_read(d_img, t, d_dst[:cap], image_bytes=len(img), stream=stream)
    torch.cuda.synchronize()
    return res, d_dst.cpu().numpy()


def _check(res, out, triples, data, want=None):
    """results, bytes in every exact range, the sentinel everywhere else"""
    mask = np.zeros(len(out), bool)
    for i, (o, ln, d) in enumerate(triples):
        w = ln if want is None else want[i]
        assert res[i] == w, (i, o, ln, d, res[i], w)
        if w > 0:
            assert np.array_equal(out[d:d + ln], data[o:o + ln]), (i, o, ln, d)
        if w > 0 or w == -4:
            mask[d:d + ln] = True
    assert (out[~mask] == SENT).all()


def _layout(pairs, start=3, gap=5):
    out, d = [], start
    for o, ln in pairs:
        out.append((o, ln, d))
        d += ln + gap
    return out


@pytest.mark.parametrize("tag,z,level", KINDS)
def test_byte_ranges_equal_the_input(p, images, data, tag, z, level):
    n = 12 * B + 12345
    img = images[(tag, n)]
    pairs = [(100, 1000), (B, B), (B - 500, 1000), (B - 500, B + 1000), (0, n), (n - 1, 1), (5, 0), (100, 5000), (200, 5000),
             (3 * B + 10, 100), (3 * B + 1000, 100), (3 * B + 5000, 100), (12 * B, 12345), (12 * B - 1, 2), (7 * B, 2 * B)]
    t = _layout(pairs)
    res, out = _read(p, img, t)
    _check(res, out, t, data)
    # 4096 seeded random ranges in one call, unaligned destinations
    rng = np.random.default_rng(17)
    ln = np.where(rng.random(4096) < 0.02, rng.integers(1, 2 * B, 4096), rng.integers(1, 40000, 4096))
    off = (rng.random(4096) * (n - ln)).astype(np.int64)
    t = _layout(zip(off.tolist(), ln.tolist()), start=7, gap=3)
    res, out = _read(p, img, t)
    _check(res, out, t, data)
    # small images
    for m in (1000, 2 * B):
        t = _layout([(0, m), (m - 1, 1), (m // 2, m // 3), (0, 0)])
        res, out = _read(p, images[(tag, m)], t)
        _check(res, out, t, data)


def test_flipped_payload_fails_only_the_ranges_that_touch_it(p, images, data):
    n = 12 * B + 12345
    base = bytearray(images[("4mc-1", n)])
    ioff = [12]
    for _ in range(6):
        ioff.append(ioff[-1] + 12 + int.from_bytes(base[ioff[-1] + 4:ioff[-1] + 8], "big"))
    base[ioff[5] + 12 + 999] ^= 0x10                       # block 5
    pairs = [(5 * B + 10, 100), (5 * B - 10, 20), (4 * B, B), (6 * B, B), (0, n), (6 * B - 1, 1), (6 * B, 1), (5 * B, B),
             (4 * B + 7, 3 * B), (100, 100)]
    want = [-4, -4, B, B, -4, -4, 1, -4, -4, 100]
    t = _layout(pairs)
    res, out = _read(p, bytes(base), t)
    _check(res, out, t, data, want)


def test_out_of_range_capacity_and_unindexable_images(p, images, data):
    n = 12 * B + 12345
    img = images[("4mc-1", n)]
    t = [(n - 10, 11, 0), (0, 10, 296), (n, 1, 200), (5, 20, 400), (n, 0, 400)]
    res, out = _read(p, img, t, cap=305)
    assert res.tolist() == [-3, -5, -3, -5, 0]
    assert (out == SENT).all()
    t = [(0, 10, 0), (3, 5, 20), (B + 1, 40, 30)]
    res, out = _read(p, img, t, cap=300)
    _check(res, out, t, data)
    # an image the file API cannot index: every range gets its code
    crafted = _crafted(p, images)
    for name, code in (("bad_footer_checksum", -2), ("trunc_short", -1), ("delta_3_1", -2), ("csize_beyond", -4), ("empty", -1)):
        t = [(0, 10, 0), (5, 0, 20), (1, 1, 30)]
        res, out = _read(p, crafted[name], t)
        assert res.tolist() == [code] * 3, (name, res)
        assert (out == SENT).all()
    # an empty image indexes to nothing: every non-empty range is out of range
    res, out = _read(p, images[("4mc-1", 0)], [(0, 1, 0), (0, 0, 1)])
    assert res.tolist() == [-3, 0]


# ---- streams and workspaces -----------------------------------------------------------------------------------------
def test_a_side_stream_gives_the_same_results(p, images, data, tmp_path):
    n = 12 * B + 12345
    img = images[("4mz-1", n)]
    t = _layout([(B - 3, 10), (2 * B, 3 * B), (n - 5000, 5000)])
    want, want_out = _read(p, img, t)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    got, got_out = _read(p, img, t, stream=s)
    assert np.array_equal(got, want) and np.array_equal(got_out, want_out)
    _check(got, got_out, t, data)
    assert dev_decode(p, img, 2, 4, 4 * B, stream=s) == dev_decode(p, img, 2, 4, 4 * B)
    with torch.cuda.stream(s):
        info, ent = p.image_index(_dev(img), image_bytes=len(img), stream=s)
    assert info["nblocks"] == 13 and info["framing"] == 0


def test_reads_after_releasing_the_workspaces(p, images, data):
    n = 12 * B + 12345
    img = images[("4mc-1", n)]
    t = _layout([(B - 3, 10), (2 * B, 3 * B)])
    res, out = _read(p, img, t)
    _check(res, out, t, data)
    p.release_workspaces()
    res, out = _read(p, img, t)
    _check(res, out, t, data)
    p.release_workspaces()
    assert dev_decode(p, img, 0, 13, n)[0] == n
