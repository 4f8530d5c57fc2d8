"""Hadoop block streams in device memory (fourmc_gpu_bstream_* / compress_bstream, decompress_bstream, decompress_bstreams).

The oracle is tests/bstream_model.py: BlockCompressorStream over Lz4Compressor's buffer logic restated in Python, with the oracle's
block compressors, and the reader rule of include/fourmc_gpu.h with the oracle's decoders.  No file written by a JVM is available
(Hadoop's classes are not in the reference tree and there is no JVM), so tests/golden holds nothing for this format.
The streams the clean and the many-streams cases decode are built once on the CPU and shared; the big shapes (M + 1, 2M, 2M + 5)
use compressible corpus bytes and the fast codecs, the slow levels (HC 8, zstd 12) see a few KiB in groups of 1000 bytes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bstream_model as bm
import helpers

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CANARY = 0xC3
SLACK = 4096                             # behind an image: the decoders may read 64 bytes past a payload
PAIRS = [(".lz4_fast", 0, 0), (".lz4_mc", 1, 0), (".lz4_hc", 2, 4), (".lz4_uc", 2, 8),
         (".zstd_fast", 3, 1), (".zstd_mc", 3, 3), (".zstd_hc", 3, 6), (".zstd_uc", 3, 12)]
FIELDS = ("decoded_bytes", "total_bytes", "fail_offset", "groups", "chunks", "reason")
_MEMO = {}


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


def text():
    if "text" not in _MEMO:
        _MEMO["text"] = helpers.corpus(2 * bm.max_input(True) + 4096).tobytes()
    return _MEMO["text"]


def block(zstd, raw):
    """one chunk's payload by the oracle (LZ4 fast / zstd 1), memoized: the same M-byte pieces serve several shapes"""
    key = ("blk", zstd, raw)
    if key not in _MEMO:
        _MEMO[key] = bm.oracle_compressor(3 if zstd else 0, 1)(raw)
    return _MEMO[key]


def written(zstd, pattern):
    """(stream, its content) of the model writer after write() calls of these sizes over the corpus"""
    key = ("w", zstd, tuple(pattern))
    if key not in _MEMO:
        src = text()[:sum(pattern)]
        _MEMO[key] = (bm.write_stream(src, list(pattern), lambda b: block(zstd, b), zstd), src)
    return _MEMO[key]


def group(zstd, raw):
    """BE32(rawlen) BE32(clen) payload: a one-chunk group made by hand (the damage cases need three small groups, which no writer
    with a 4 MiB buffer produces: the reader rule is about the format, not about who wrote it)"""
    c = block(zstd, bytes(raw))
    return bm.be32(len(raw)) + bm.be32(len(c)) + c


def up(data, slack=SLACK):
    buf = np.zeros(len(data) + slack, np.uint8)
    buf[:len(data)] = np.frombuffer(bytes(data), np.uint8)
    return torch.from_numpy(buf).cuda()


def codec_of(zstd):
    return 3 if zstd else 0


def want_of(img, zstd, cap):
    key = ("r", zstd, img, cap)
    if key not in _MEMO:
        _MEMO[key] = bm.read_stream(img, zstd, cap)
    return _MEMO[key]


def check_single(p, img, zstd, cap=None, codec=None):
    """decompress_bstream on `img` against the model reader: the status field for field, the bytes, the guards around the
    destination; cap None: total_bytes + 9.  Returns the status."""
    d_img = up(img)
    q = p.decompress_bstream(d_img, None, codec_of(zstd), image_bytes=len(img))
    wq, _ = want_of(img, zstd, "query")
    assert {k: q[k] for k in FIELDS} == wq, (q, wq)
    cap = wq["total_bytes"] + 9 if cap is None else cap          # (a capacity of 0 is passed as 1: an empty tensor has no address)
    want, wbytes = want_of(img, zstd, cap)
    d_dst = torch.full((64 + cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
    st = p.decompress_bstream(d_img, d_dst[64:64 + max(cap, 1)], codec_of(zstd) if codec is None else codec, image_bytes=len(img))
    assert {k: st[k] for k in FIELDS} == want, (st, want)
    assert st["name"] == p.BSTREAM_REASONS[st["reason"]] and (st["message"] == "") == (st["reason"] == 0)
    out = d_dst.cpu().numpy()
    n = st["decoded_bytes"]
    assert out[64:64 + n].tobytes() == wbytes, "decoded bytes differ from the model's"
    wrote = 0 if st["reason"] == bm.DST_SMALL else min(st["total_bytes"], cap)
    assert (out[:64] == CANARY).all() and (out[64 + wrote:] == CANARY).all(), "bytes written outside [d_dst, d_dst + total_bytes)"
    return st


# ---- encode -------------------------------------------------------------------------------------------------------------------
def encode(p, src, codec, level, G, extra=0):
    """(stream bytes, bound): compress_bstream into a buffer of exactly the bound (+ extra) with guard bytes behind it"""
    bound = p.bstream_bound(len(src), codec, G)
    d_src = up(src, 64) if len(src) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    d_img = torch.full((bound + extra + 256,), CANARY, dtype=torch.uint8, device="cuda")
    n = p.compress_bstream(d_src[:len(src)], d_img[:bound + extra], codec, level, G)
    out = d_img.cpu().numpy()
    assert n <= bound
    assert (out[n:] == CANARY).all(), "bytes written behind the stream"
    return out[:n].tobytes(), bound


@pytest.mark.parametrize("ext,codec,level", PAIRS, ids=[e for e, _, _ in PAIRS])
def test_encode_small(p, ext, codec, level):
    assert p.bstream_codec(ext) == (codec, level)
    cb = bm.oracle_compressor(codec, level)
    for n in (2500, 0, 3000):
        src = text()[777:777 + n]
        want = bm.write_groups(src, 1000, cb, codec == 3)         # the model writer fed the same pieces, the oracle as block compressor
        got, bound = encode(p, src, codec, level, 1000)
        assert got == want, (ext, n)
        assert len(got) == len(want) <= bound
        st, back = bm.read_stream(got, codec == 3)
        assert st["reason"] == bm.OK and back == src and st["groups"] == -(-n // 1000)
        if n == 0:
            assert got == b"\0\0\0\0"


@pytest.mark.parametrize("ext,codec,level", [PAIRS[0], PAIRS[4]], ids=["lz4_fast", "zstd_fast"])
def test_encode_a_source_of_m_plus_1(p, ext, codec, level):
    zstd = codec == 3
    M = p.bstream_max_input(codec)
    want, src = written(zstd, (M, 1))            # each write() longer than M / 2: one group per write
    got, bound = encode(p, src, codec, level, 0)
    assert len(got) == len(want) <= bound == 8 + bm.block_bound(M, zstd) + 8 + bm.block_bound(1, zstd)
    assert got == want


def test_encode_matches_the_stream_of_small_writes(p):
    """writes of w bytes each: the stream's groups hold floor(M / w) * w bytes"""
    M = p.bstream_max_input(0)
    w = 1 << 20
    want, src = written(False, (w,) * 5)
    got, _ = encode(p, src, 0, 0, (M // w) * w)
    assert got == want


def test_encode_more_groups_than_one_staging_piece(p):
    """650 groups are staged as 512 + 138: the scan's 64-bit carry and the descriptors' source offsets go on into the second piece"""
    for codec, level in ((0, 0), (3, 1)):
        src = text()[9000:9000 + 1299]
        got, _ = encode(p, src, codec, level, 2)
        assert got == bm.write_groups(src, 2, bm.oracle_compressor(codec, level), codec == 3), codec


def test_encode_under_the_parallel_lz4_encoder(p):
    L = p.lib()
    src = text()[:300000]
    exact, _ = encode(p, src, 0, 0, 100000)
    L.fourmc_gpu_set_lz4_encode_mode(1)
    try:
        got, bound = encode(p, src, 0, 0, 100000)
    finally:
        L.fourmc_gpu_set_lz4_encode_mode(0)
    st, back = bm.read_stream(got, False)
    assert st["reason"] == bm.OK and st["groups"] == 3 and back == src and len(got) <= bound
    assert bm.read_stream(exact, False)[1] == src


def test_encode_argument_errors_on_the_device(p):
    d_src = up(text()[:5000], 0)
    d_img = torch.full((8192,), CANARY, dtype=torch.uint8, device="cuda")
    M = p.bstream_max_input(0)
    for kw in (dict(codec=7), dict(group_bytes=M + 1), dict(codec=3, level=13)):
        with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstream_compress failed \(-[35]\)"):
            p.compress_bstream(d_src, d_img, **kw)
    with pytest.raises(p.EngineError, match=r"failed \(-3\)"):
        p.compress_bstream(d_src, d_img[:p.bstream_bound(5000, 0, 1000) - 1], group_bytes=1000)
    torch.cuda.synchronize()
    assert bool((d_img == CANARY).all())


# ---- decode, clean ------------------------------------------------------------------------------------------------------------
def clean_streams(zstd):
    """[(name, stream)]: every shape the reader rule names"""
    M = bm.max_input(zstd)
    one = written(zstd, (5000,))[0]
    two = written(zstd, (M + 1,))[0]
    assert two.endswith(b"\0\0\0\0")
    out = [("one chunk", one), ("two chunks, M + 1, trailing zero", two), ("exactly 2M", written(zstd, (2 * M,))[0]),
           ("three chunks after a small group", written(zstd, (100, 2 * M + 5))[0]),
           ("two groups of accumulated writes", written(zstd, (1 << 20,) * 5)[0]),
           ("1 trailing byte", one + b"\x01"), ("2 trailing bytes", one + b"\x01\x02"), ("3 trailing bytes", one + b"\x01\x02\x03"),
           ("bytes after a zero rawlen", two + bytes(range(1, 41))), ("the empty stream", written(zstd, ())[0]), ("no bytes", b"")]
    assert out[-2][1] == b"\0\0\0\0"
    return out


def run_clean(p, zstd):
    M = bm.max_input(zstd)
    chunks = {"one chunk": 1, "two chunks, M + 1, trailing zero": 2, "exactly 2M": 2, "three chunks after a small group": 4,
              "two groups of accumulated writes": 2}
    for name, img in clean_streams(zstd):
        st = check_single(p, img, zstd)
        assert st["reason"] == 0 and st["decoded_bytes"] == st["total_bytes"] and st["fail_offset"] == len(img), (name, st)
        if name in chunks:
            assert st["chunks"] == chunks[name], (name, st)
        if name == "exactly 2M":
            assert st["total_bytes"] == 2 * M


@pytest.mark.parametrize("path", [13, 11, 2], ids=["tile", "seg", "exact"])
def test_decode_clean_lz4(p, path):
    """the walk is new, the decoders are not: it must hand every FOURMC_DECODE path correct descriptors"""
    L = p.lib()
    L.fourmc_gpu_set_lz4_decode_path(path)
    try:
        run_clean(p, False)
    finally:
        L.fourmc_gpu_set_lz4_decode_path(6)


@pytest.mark.parametrize("split", [1, 0], ids=["split", "single"])
def test_decode_clean_zstd(p, split):
    L = p.lib()
    L.fourmc_gpu_set_zstd_decode_split(split)
    try:
        run_clean(p, True)
    finally:
        L.fourmc_gpu_set_zstd_decode_split(1)


@pytest.mark.parametrize("zstd", [False, True], ids=["lz4", "zstd"])
def test_dst_small_and_the_family_selectors(p, zstd):
    M = bm.max_input(zstd)
    img, src = written(zstd, (100, 2 * M + 5))
    n = len(src)
    st = check_single(p, img, zstd, cap=n - 1)
    assert st["reason"] == bm.DST_SMALL and st["decoded_bytes"] == 0 and st["total_bytes"] == n
    assert check_single(p, img, zstd, cap=n)["reason"] == 0                      # exactly enough
    small = written(zstd, (5000,))[0]
    assert check_single(p, small, zstd, cap=0)["reason"] == bm.DST_SMALL
    assert check_single(p, b"\0\0\0\0", zstd, cap=0)["reason"] == 0              # nothing needs no room
    if not zstd:
        for codec in (1, 2):                                                     # any LZ4 selector means LZ4
            assert check_single(p, small, False, codec=codec)["reason"] == 0
    d = up(small)
    for bad in (4, -1):
        with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstream_decompress failed \(-3\)"):
            p.decompress_bstream(d, None, bad, image_bytes=len(small))


# ---- decode, damaged ----------------------------------------------------------------------------------------------------------
def three_groups(zstd):
    t = text()
    raws = [t[1000:4000], t[50000:52000], t[90000:91500]]
    return raws, [group(zstd, r) for r in raws]


def failing_flip(zstd, g, raw):
    """the group with one payload byte changed so that the codec fails (not every flip does: the oracle says which)"""
    dec = helpers.orc_zstd_decompress if zstd else helpers.orc_decompress
    for at in list(range(8, 16)) + list(range(len(g) - 1, len(g) - 9, -1)):
        for x in (0xFF, 0x80, 0x01):
            m = bytearray(g)
            m[at] ^= x
            if dec(np.frombuffer(bytes(m[8:]), np.uint8), len(raw))[0] < 0:
                return bytes(m)
    raise AssertionError("no flip makes the codec fail")


def damage(zstd, k):
    """{name: stream}: each damage class in group k of a three-group stream"""
    raws, gs = three_groups(zstd)
    key = ("dmg", zstd, k)
    if key in _MEMO:
        return _MEMO[key]
    head, g, tail = b"".join(gs[:k]), gs[k], b"".join(gs[k + 1:])
    raw = raws[k]
    out = {"rawlen top bit": head + bytes([g[0] | 0x80]) + g[1:] + tail}
    for cut in range(4):
        out["cut %d bytes into the clen" % cut] = head + g[:4 + cut]
    out["clen 0"] = head + g[:4] + bm.be32(0) + g[8:] + tail
    out["clen 4 MiB + 1"] = head + g[:4] + bm.be32((4 << 20) + 1) + g[8:] + tail
    out["clen beyond the bytes left"] = head + g[:4] + bm.be32(len(g) - 8 + len(tail) + 1) + g[8:] + tail
    out["flipped payload byte"] = head + failing_flip(zstd, g, raw) + tail
    fewer, more = block(zstd, raw[:-1]), block(zstd, raw + b"!")
    out["a chunk that decodes to fewer bytes"] = head + g[:4] + bm.be32(len(fewer)) + fewer + tail
    out["a chunk that decodes to more bytes"] = head + g[:4] + bm.be32(len(more)) + more + tail
    _MEMO[key] = out
    return out


WANT_REASON = {"rawlen top bit": bm.BAD_RAWLEN, "clen 0": bm.BAD_CLEN, "clen 4 MiB + 1": bm.BAD_CLEN,
               "clen beyond the bytes left": bm.DATA_UNREADABLE, "flipped payload byte": bm.CORRUPT,
               "a chunk that decodes to fewer bytes": bm.SHAPE, "a chunk that decodes to more bytes": bm.CORRUPT}


@pytest.mark.parametrize("k", [0, 1, 2], ids=["first", "middle", "last"])
@pytest.mark.parametrize("zstd", [False, True], ids=["lz4", "zstd"])
def test_decode_damaged(p, zstd, k):
    raws, gs = three_groups(zstd)
    before = sum(len(r) for r in raws[:k])
    at = sum(len(g) for g in gs[:k])
    for name, img in damage(zstd, k).items():
        st = check_single(p, img, zstd)                          # every field and the bytes before the failure: the model's
        want = WANT_REASON.get(name, bm.CLEN_UNREADABLE)
        assert st["reason"] == want, (name, st)                  # and the damage is what it is meant to be
        assert st["decoded_bytes"] == before and st["groups"] == k == st["chunks"], (name, st)
        assert st["fail_offset"] == (at if want == bm.BAD_RAWLEN else at + 4), (name, st)
    # the first failing chunk wins over a framing error behind it, and a framing error over a failing chunk behind it
    d0, d2 = damage(zstd, 0), damage(zstd, 2)
    if k == 0:
        both = d0["flipped payload byte"][:len(gs[0])] + gs[1] + d2["clen 0"][len(gs[0]) + len(gs[1]):]
        assert check_single(p, both, zstd)["reason"] == bm.CORRUPT
        both = d0["clen 0"][:len(gs[0])] + gs[1] + d2["flipped payload byte"][len(gs[0]) + len(gs[1]):]
        st = check_single(p, both, zstd)
        assert st["reason"] == bm.BAD_CLEN and st["decoded_bytes"] == 0 and st["total_bytes"] == 0
        # DST_SMALL wins over both
        assert check_single(p, d2["flipped payload byte"], zstd, cap=100)["reason"] == bm.DST_SMALL


# ---- many streams -------------------------------------------------------------------------------------------------------------
def many_streams(zstd):
    """12 streams: clean ones small and multi-chunk, each damage class once, the empty stream, one stream twice, one of 70 groups"""
    M = bm.max_input(zstd)
    t = text()
    d1, d2 = damage(zstd, 1), damage(zstd, 2)
    one = written(zstd, (5000,))[0]
    seventy = b"".join(group(zstd, t[3000 * j:3000 * j + 40 + j]) for j in range(70))
    return [one, written(zstd, (M + 1,))[0], d1["rawlen top bit"], d1["cut 2 bytes into the clen"], b"\0\0\0\0", d2["clen 0"],
            one, d1["clen beyond the bytes left"], seventy, d1["flipped payload byte"], d2["a chunk that decodes to fewer bytes"],
            written(zstd, (100, 2 * M + 5))[0]]


def check_many(p, zstd, small=(11,)):
    """one decompress_bstreams over the 12 streams against the single call on each; the item numbers in `small` get a region one
    byte short (FOURMC_BS_DST_SMALL).  The output regions abut: item i + 1 starts where item i's capacity ends."""
    images = many_streams(zstd)
    offs, pos = [], 3
    for i, img in enumerate(images):
        offs.append(pos)
        pos += len(img) + (i * 37) % 71                          # uneven gaps: the decoders' over-read lands in them
    buf = np.full(pos + SLACK, 0x5A, np.uint8)
    for img, o in zip(images, offs):
        buf[o:o + len(img)] = np.frombuffer(img, np.uint8)
    d_buf = torch.from_numpy(buf).cuda()
    singles, caps = [], []
    for i, img in enumerate(images):
        total = want_of(img, zstd, "query")[0]["total_bytes"]
        cap = total - 1 if i in small else total
        key = ("single", zstd, img, cap)
        if key not in _MEMO:
            view = d_buf[offs[i]:offs[i] + len(img)]
            d_one = torch.full((cap + 64,), CANARY, dtype=torch.uint8, device="cuda")
            if cap:
                st = p.decompress_bstream(view, d_one[:cap], codec_of(zstd), image_bytes=len(img))
            else:                                                # an empty tensor would be the size query: ask the model
                st = dict(want_of(img, zstd, 0)[0])
            _MEMO[key] = ({k: st[k] for k in FIELDS}, d_one[:st["decoded_bytes"]].cpu().numpy().tobytes())
            assert _MEMO[key][0] == want_of(img, zstd, cap)[0], (i, _MEMO[key][0])
        singles.append(_MEMO[key])
        caps.append(cap)
    dsts, at = [], 64
    for cap in caps:
        dsts.append(at)
        at += cap
    d_dst = torch.full((at + 64,), CANARY, dtype=torch.uint8, device="cuda")
    items = [(offs[i], len(images[i]), dsts[i], caps[i]) for i in range(len(images))]
    q = p.decompress_bstreams(d_buf, items, None, codec_of(zstd), images_bytes=pos)
    got = p.decompress_bstreams(d_buf, items, d_dst, codec_of(zstd), images_bytes=pos)
    out = d_dst.cpu().numpy()
    covered = np.zeros(len(out), bool)
    for i, (st, (wst, wbytes)) in enumerate(zip(got, singles)):
        assert {k: st[k] for k in FIELDS} == wst, (i, st, wst)
        assert {k: q[i][k] for k in FIELDS} == want_of(images[i], zstd, "query")[0], (i, q[i])
        n = st["decoded_bytes"]
        assert out[dsts[i]:dsts[i] + n].tobytes() == wbytes, (i, "decoded bytes differ from the single call's")
        if st["reason"] != bm.DST_SMALL:
            covered[dsts[i]:dsts[i] + n] = True                  # bytes in [decoded_bytes, total_bytes) are unspecified ...
            covered[dsts[i] + n:dsts[i] + min(st["total_bytes"], caps[i])] = True
    assert (out[~covered] == CANARY).all(), "bytes written outside [dst_off, dst_off + total_bytes) of the items"
    return got


@pytest.mark.parametrize("zstd", [False, True], ids=["lz4", "zstd"])
def test_many_streams(p, zstd):
    got = check_many(p, zstd)
    reasons = [st["reason"] for st in got]
    assert reasons == [0, 0, bm.BAD_RAWLEN, bm.CLEN_UNREADABLE, 0, bm.BAD_CLEN, 0, bm.DATA_UNREADABLE, 0, bm.CORRUPT, bm.SHAPE,
                       bm.DST_SMALL], reasons
    assert got[0] == got[6] and got[8]["chunks"] == 70 and got[1]["chunks"] == 2 and got[4]["total_bytes"] == 0
    # neighbours of damage are whole: check_many compared their bytes with the single call's; the single call's with the source
    src = written(zstd, (bm.max_input(zstd) + 1,))[1]
    assert _MEMO[("single", zstd, many_streams(zstd)[1], len(src))][1] == src
    # every item fits now; n == 0 is fine
    assert check_many(p, zstd, small=())[11]["reason"] == 0
    d = up(b"\0\0\0\0")
    assert p.decompress_bstreams(d, [], d) == [] and p.decompress_bstreams(d, [], None, codec_of(zstd)) == []
    with pytest.raises(p.EngineError, match=r"fourmc_gpu_bstreams_decompress failed \(-3\)"):
        p.decompress_bstreams(d, [(0, 4, 0, 3), (0, 4, 2, 2)], d, codec_of(zstd))


def child_main():
    """the limits are read once per process: this one has them low"""
    p = helpers.pkg()
    p.gpu_init(0)
    got = check_many(p, False)
    torch.cuda.synchronize()
    print("RESULT " + json.dumps({"chunks": sum(st["chunks"] for st in got), "reasons": [st["reason"] for st in got]}))


def test_many_streams_with_the_decode_cut_into_several_launches(p):
    """FOURMC_BATCH_BLOCKS is the file API's and the sharded writer's batch; the launches of a device-resident LZ4 decode are cut by
    FOURMC_TILE_BATCH / FOURMC_SEG_BATCH, whose pieces are never smaller than 64 blocks.  The child has all three low; the 12
    streams list 85 chunks, 9 of them in front of the 70-group stream, so the decode takes two launches with the cut inside it."""
    env = dict(os.environ, FOURMC_BATCH_BLOCKS="4", FOURMC_TILE_BATCH="64", FOURMC_SEG_BATCH="64")
    r = subprocess.run([sys.executable, "-c", "import test_gpu_bstream as T; T.child_main()"], cwd=HERE, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, r.stdout[-2000:]
    res = json.loads(line[-1][7:])
    assert res["reasons"] == [0, 0, 1, 2, 0, 3, 0, 4, 0, 5, 6, 7] and res["chunks"] == 1 + 2 + 1 + 1 + 0 + 2 + 1 + 1 + 70 + 1 + 2 + 0


# ---- the Python API -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [e for e, _, _ in PAIRS])
def test_round_trip_by_extension(p, ext):
    codec, level = p.bstream_codec("part-00000" + ext)
    src = text()[4321:4321 + 10240]
    d_src = up(src, 64)[:len(src)]
    d_img = torch.empty(p.bstream_bound(len(src), codec, 1000) + SLACK, dtype=torch.uint8, device="cuda")
    n = p.compress_bstream(d_src, d_img, codec, level, group_bytes=1000)
    assert p.decompress_bstream(d_img, None, codec, image_bytes=n)["total_bytes"] == len(src)
    d_dst = torch.full((len(src) + 64,), CANARY, dtype=torch.uint8, device="cuda")
    st = p.decompress_bstream(d_img, d_dst[:len(src)], codec, image_bytes=n)
    assert st["reason"] == 0 and st["name"] == "OK" and st["decoded_bytes"] == len(src) and st["groups"] == 11 == st["chunks"]
    assert st["fail_offset"] == n
    out = d_dst.cpu().numpy()
    assert out[:len(src)].tobytes() == src and (out[len(src):] == CANARY).all()
