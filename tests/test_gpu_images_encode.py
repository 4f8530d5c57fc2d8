"""Many sources of one device buffer encoded into many .4mc / .4mz images of one device buffer with one call
(fourmc_gpu_images_compress / compress_images).

The oracle is compress_image on the same slice: for every item the batch's length and bytes equal the single call's, and every byte
of the image buffer outside the images keeps the canary it was filled with.  A single call's answer is computed once per (source
bytes, format, level, encoder mode) and shared by the cases that need it."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = helpers.ROOT
B = helpers.B
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "corpus_manifest.json")))
CANARY = 0xC3
SLACK = 4096                             # behind the last image, for the decoders of the round trip
SIZES = [0, 1, B - 1, B, B + 1, 2 * B + 5]
LEVEL_SIZES = [0, 1, 4097, 65546, 65547, 70001]          # 65546 | 65547: the LZ4 encoders' switch between their two table layouts
HC_WS = (4 << 15) + 2 * (0x1FFFF + 1)                    # lz4hc_encode.hip: fourmc_lz4hc_work_bytes per block
_ZSTD_STORE = 3 * (32768 + 64) * 4 + 3 * (32768 + 64) + 64 + 128 * 1024 + 256 + 4736 + 512 + 192
ZSTD1_WS = _ZSTD_STORE + (4 << 15)                       # zstd_encode.hip: fourmc_zstd_enc_work_bytes(1, level 1)

_MEMO = {}


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


def golden():
    if "golden" not in _MEMO:
        c = MANIFEST["corpus"]
        _MEMO["golden"] = helpers.corpus(c["bytes"], first_block=c["first_block"], seed=c["seed"])
    return _MEMO["golden"]


def _magic(p, z):
    return p.MAGIC_4MZ if z else p.MAGIC_4MC


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def single(p, src, d_src, so, sb, z, level, mode=0, fresh=False):
    """compress_image of d_src[so, so + sb) where it lies; the image as bytes.  src: the host copy of d_src (numpy), for the key"""
    what = src[so:so + sb] if sb <= 4 * B else np.concatenate([src[so:so + 4096], src[so + sb - 4096:so + sb]])     # large: named by its ends
    key = ("img", hashlib.sha1(what.tobytes()).digest(), so, sb, z, level, mode)
    if key not in _MEMO or fresh:
        d_img = torch.full((p.image_bound(sb) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
        view = d_src[so:so + sb] if sb else torch.zeros(0, dtype=torch.uint8, device="cuda")
        k = p.compress_image(view, d_img[:p.image_bound(sb)], _magic(p, z), level)
        assert k <= p.image_bound(sb) and bool((d_img[p.image_bound(sb):] == 0x5A).all())
        _MEMO[key] = d_img[:k].cpu().numpy().tobytes()
    return _MEMO[key]


def pack_sources(chunks):
    """the sources back to back at uneven (odd and even) offsets; returns (host buffer, [(src_off, src_bytes)])"""
    offs, pos = [], 3
    for i, c in enumerate(chunks):
        offs.append(pos)
        pos += len(c) + (i * 5 + 1) % 23
    buf = np.full(pos + 64, 0x11, np.uint8)
    for c, o in zip(chunks, offs):
        buf[o:o + len(c)] = c
    return buf, [(o, len(c)) for o, c in zip(offs, chunks)]


def regions(p, spans, gap=lambda i: 1 + (i * i * 7) % 97, start=5):
    """image regions of exactly image_bound bytes each, in order, `gap(i)` canary bytes in front of region i"""
    rows, pos = [], start
    for i, (so, sb) in enumerate(spans):
        pos += gap(i)
        rows.append((so, sb, pos, p.image_bound(sb)))
        pos += p.image_bound(sb)
    return rows, pos + 64 + SLACK


def check_batch(p, src, rows, total, z, level, mode=0, stream=None, fresh=False, d_src=None):
    """1 prefill d_images with a canary, 2 run the batch over `rows` (src_off, src_bytes, image_off, image_cap), 3 compare every
    image and length with compress_image of the same slice, 4 check every byte outside the images.  Returns (lengths, d_images)."""
    if d_src is None:
        d_src = torch.from_numpy(src).cuda()
    d_images = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    lens = p.compress_images(d_src, rows, d_images, _magic(p, z), level, stream=stream)
    if stream is not None:
        stream.synchronize()
    assert len(lens) == len(rows)
    outside = torch.ones(total, dtype=torch.bool, device="cuda")
    for i, ((so, sb, io, ic), k) in enumerate(zip(rows, lens)):
        want = single(p, src, d_src, so, sb, z, level, mode, fresh)
        assert k == len(want), (i, (so, sb, io, ic), k, len(want))
        assert k <= ic
        got = d_images[io:io + k].cpu().numpy().tobytes()
        assert got == want, (i, (so, sb, io, ic), "image differs from the single call's",
                             next(j for j in range(k) if got[j] != want[j]))
        outside[io:io + k] = False
    assert not bool(((d_images != CANARY) & outside).any()), "bytes written outside the images"
    return lens, d_images


# ---- 1: sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", [False, True], ids=["4mc", "4mz"])
def test_sizes(p, z):
    data = golden()
    src, spans = pack_sources([data[:n] for n in SIZES])
    rows, total = regions(p, spans)
    lens, d_images = check_batch(p, src, rows, total, z, 1)
    assert lens[0] == 44
    for n, (_, _, io, _), k in zip(SIZES, rows, lens):
        img = d_images[io:io + k].cpu().numpy().tobytes()
        assert int.from_bytes(img[-12:-8], "big") == 20 + 4 * ((n + B - 1) // B)          # the footer: one delta per block
        if n:
            assert int.from_bytes(img[k - (20 + 4 * ((n + B - 1) // B)) + 8:][:4], "big") == 12      # the first one: the in-image 12
        want = MANIFEST["levels"]["4mz-1" if z else "4mc-1"]
        if n == MANIFEST["corpus"]["bytes"]:              # a golden file of that prefix
            assert k == want["file_bytes"] and _sha(img) == want["sha256"]


# ---- 2: levels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 2, 3, 4])
@pytest.mark.parametrize("z", [False, True], ids=["4mc", "4mz"])
def test_levels(p, z, level):
    data = golden()
    src, spans = pack_sources([data[7 * i:7 * i + n] for i, n in enumerate(LEVEL_SIZES)])
    rows, total = regions(p, spans)
    check_batch(p, src, rows, total, z, level)


# ---- 3: seams, many images ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [65, 130, 257])
def test_seams_many_images(p, count):
    """65 and 130 items cross 64-lane seams, 257 the 256 of a workgroup, whatever the engine scans images with; 23 distinct
    sources of 0 - 3000 bytes (empty ones among them) keep the single calls few"""
    data = golden()
    sizes = [0, 1, 3000, 2999, 17, 0, 1500, 255, 256, 257, 4, 12, 13, 1000, 2047, 2048, 0, 5, 64, 63, 65, 777, 2500]
    src, spans = pack_sources([data[3001 * j:3001 * j + n] for j, n in enumerate(sizes)])
    rows, total = regions(p, [spans[i % len(spans)] for i in range(count)])
    lens, _ = check_batch(p, src, rows, total, False, 1)
    assert [k for k, (_, sb, _, _) in zip(lens, rows) if sb == 0] == [44] * sum(sb == 0 for _, sb, _, _ in rows)


# ---- 4: seams, many blocks ----------------------------------------------------------------------------------------------------
def test_seams_many_blocks(p):
    """one image of 65 blocks and one of 130 cross the 64-block seams of the per-image scan and of the descriptor loop, with
    descriptor, staging and image bases that are not zero: one-block images lie before, between and behind them.  Compressible
    bytes (a period of 251 that drifts every 64 KiB), made on the device; the 65 blocks are the first half of the 130."""
    idx = torch.arange(B, dtype=torch.int64, device="cuda")
    one = ((idx % 251) ^ (idx >> 16)).to(torch.uint8)                     # block j: this pattern xor j
    d_src = torch.cat([(one[None, :] ^ torch.arange(130, dtype=torch.uint8, device="cuda")[:, None]).reshape(-1), one[:3]])
    del idx, one
    src = d_src.cpu().numpy()
    spans = [(1, 5000), (3, 65 * B - 7), (B + 2, 70001), (0, 130 * B), (2 * B + 5, 4097)]
    assert [(sb + B - 1) // B for _, sb in spans] == [1, 65, 1, 130, 1]
    rows, total = regions(p, spans)
    lens, _ = check_batch(p, src, rows, total, False, 1, d_src=d_src)
    assert max(lens) < 40 * B


# ---- 5: layout ----------------------------------------------------------------------------------------------------------------
def _small_sources():
    data = golden()
    return [data[:5000], data[100:100], data[B:B + 70001], data[9:10], data[2 * B:2 * B + 12345], data[77:77 + 300000]]


def test_layout_regions_in_reverse_order_with_gaps(p):
    """item 0's region lies last in the buffer and the last item's first, with gaps and 3 spare bytes of capacity each"""
    src, spans = pack_sources(_small_sources())
    pos, rows = 9, []
    for so, sb in spans[::-1]:
        pos += 50 + sb % 41
        rows.append((so, sb, pos, p.image_bound(sb) + 3))
        pos += p.image_bound(sb) + 3
    rows = rows[::-1]
    assert [r[2] for r in rows] == sorted((r[2] for r in rows), reverse=True)
    check_batch(p, src, rows, pos + 64 + SLACK, False, 1)


def test_layout_every_residue_mod_16(p):
    data = golden()
    chunks = [data[1000 * r:1000 * r + 3000 + 17 * r] for r in range(16)]
    buf = np.full(16 * 4096 + 64, 0x11, np.uint8)
    rows, pos = [], 0
    for r, c in enumerate(chunks):
        so = 4096 * r + r                                 # src_off = r mod 16
        buf[so:so + len(c)] = c
        io = pos + 64
        io += ((r * 7 + 3) % 16 - io) % 16                # image_off = (7 r + 3) mod 16: every residue once
        rows.append((so, len(c), io, p.image_bound(len(c))))
        pos = io + p.image_bound(len(c))
    assert sorted(r[0] % 16 for r in rows) == list(range(16)) == sorted(r[2] % 16 for r in rows)
    for z in (False, True):
        check_batch(p, buf, rows, pos + 64 + SLACK, z, 1)


def test_layout_the_same_source_twice_and_overlapping_sources(p):
    data = golden()
    src = np.concatenate([data[:200000], np.zeros(64, np.uint8)])
    spans = [(0, 70001), (0, 70001), (30000, 100000), (65000, 70001), (0, 200000), (199999, 1)]
    rows, total = regions(p, spans)
    lens, d_images = check_batch(p, src, rows, total, False, 1)
    assert lens[0] == lens[1]
    assert torch.equal(d_images[rows[0][2]:rows[0][2] + lens[0]], d_images[rows[1][2]:rows[1][2] + lens[1]])
    check_batch(p, src, rows, total, True, 1)


def test_layout_regions_that_touch_exactly_at_the_bound(p):
    src, spans = pack_sources(_small_sources())
    rows, total = regions(p, spans, gap=lambda i: 0, start=0)
    assert rows[0][2] == 0 and all(a[2] + a[3] == b[2] for a, b in zip(rows, rows[1:]))
    assert all(ic == p.image_bound(sb) for _, sb, _, ic in rows)
    check_batch(p, src, rows, total, False, 1)


# ---- 6: round trip ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z", [False, True], ids=["4mc", "4mz"])
def test_round_trip_through_decompress_images(p, z):
    data = golden()
    chunks = _small_sources() + [data[:B + 1]]
    src, spans = pack_sources(chunks)
    rows, total = regions(p, spans)
    lens, d_images = check_batch(p, src, rows, total, z, 1)
    items, at = [], 0
    for (_, sb, io, _), k in zip(rows, lens):
        items.append((io, k, at, sb))
        at += sb + 64
    d_dst = torch.full((at + 64,), CANARY, dtype=torch.uint8, device="cuda")
    st = p.decompress_images(d_images, items, d_dst, _magic(p, z))
    out = d_dst.cpu().numpy()
    for s, c, (_, _, do, _) in zip(st, chunks, items):
        assert s["reason"] == 0 and s["exit_code"] == 0 and s["decoded_bytes"] == len(c) == s["total_bytes"], s
        assert s["blocks"] == (len(c) + B - 1) // B and s["streams"] == 1
        assert out[do:do + len(c)].tobytes() == c.tobytes()


# ---- 7: the encode in pieces --------------------------------------------------------------------------------------------------
PIECES_LIMIT = 3 * HC_WS                 # LZ4 HC: 4 blocks -> pieces of 2; zstd level 1: 2 * ZSTD1_WS is above it -> pieces of 1


def _pieces_job(p):
    """4 blocks: 0 | 1 2 | 3.  Pieces of 2 cut between the two blocks of the second image, pieces of 1 everywhere"""
    data = golden()
    src, spans = pack_sources([data[:70001], data[B - 50:2 * B + 50], data[5:5005]])
    assert [(sb + B - 1) // B for _, sb in spans] == [1, 2, 1]
    rows, total = regions(p, spans)
    d_src = torch.from_numpy(src).cuda()
    out = {}
    for name, z, level in (("4mz-1", True, 1), ("4mc-3", False, 3)):
        d_images = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
        lens = p.compress_images(d_src, rows, d_images, _magic(p, z), level)
        out[name] = [_sha(d_images[io:io + k].cpu().numpy().tobytes()) for (_, _, io, _), k in zip(rows, lens)]
    return out


def child_main():
    """FOURMC_WS_FAIL_ABOVE is read once per process: this one has it"""
    p = helpers.pkg()
    p.gpu_init(0)
    out = _pieces_job(p)
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(out))


def test_encode_in_pieces(p):
    assert HC_WS * 2 <= PIECES_LIMIT < HC_WS * 4 and ZSTD1_WS <= PIECES_LIMIT < 2 * ZSTD1_WS
    env = dict(os.environ, FOURMC_WS_FAIL_ABOVE=str(PIECES_LIMIT))
    r = subprocess.run([sys.executable, "-c", "import test_gpu_images_encode as T; T.child_main()"], cwd=HERE, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, r.stdout[-2000:]
    assert json.loads(line[-1][7:]) == _pieces_job(p)


# ---- 8: modes and plumbing ------------------------------------------------------------------------------------------------------
def test_parallel_lz4_encode_mode(p):
    """under fourmc_gpu_set_lz4_encode_mode(1) the batch gives the bytes the single call gives in that mode"""
    L = p.lib()
    src, spans = pack_sources(_small_sources())
    rows, total = regions(p, spans)
    old = L.fourmc_gpu_get_lz4_encode_mode()
    L.fourmc_gpu_set_lz4_encode_mode(1)
    try:
        par, _ = check_batch(p, src, rows, total, False, 1, mode=1)
    finally:
        L.fourmc_gpu_set_lz4_encode_mode(old)
    assert L.fourmc_gpu_get_lz4_encode_mode() == old
    exact, _ = check_batch(p, src, rows, total, False, 1)
    assert par[1] == exact[1] == 44 and len(par) == len(exact)


def test_a_batch_on_another_stream(p):
    s = torch.cuda.Stream()
    src, spans = pack_sources(_small_sources())
    rows, total = regions(p, spans)
    check_batch(p, src, rows, total, False, 1, stream=s)
    check_batch(p, src, rows, total, True, 1, stream=s)


def test_release_workspaces_between_batches(p):
    data = golden()
    src, spans = pack_sources(_small_sources())
    rows, total = regions(p, spans)
    a, _ = check_batch(p, src, rows, total, False, 1)
    p.release_workspaces()
    src2, spans2 = pack_sources(_small_sources() + [data[:B + 1]])        # a larger batch: the workspace grows
    rows2, total2 = regions(p, spans2)
    b, _ = check_batch(p, src2, rows2, total2, False, 1, fresh=True)
    p.release_workspaces()
    c, _ = check_batch(p, src, rows, total, False, 1, fresh=True)
    assert a == c == b[:len(a)]


def test_a_single_call_after_a_batch(p):
    """the two share the image workspace of the stream: a compress_image after a batch still gives its bytes, and so does a batch after it"""
    data = golden()
    src, spans = pack_sources(_small_sources())
    rows, total = regions(p, spans)
    check_batch(p, src, rows, total, False, 1)
    d_src = torch.from_numpy(np.ascontiguousarray(data[:B + 1])).cuda()
    d_img = torch.empty(p.image_bound(B + 1), dtype=torch.uint8, device="cuda")
    k = p.compress_image(d_src, d_img, p.MAGIC_4MC, 1)
    assert d_img[:k].cpu().numpy().tobytes() == helpers.orc_container(data[:B + 1]).tobytes()
    check_batch(p, src, rows, total, False, 1, fresh=True)


# ---- 9: errors on the device ----------------------------------------------------------------------------------------------------
def test_argument_errors_on_the_device(p):
    src, spans = pack_sources(_small_sources())
    rows, total = regions(p, spans)
    d_src = torch.from_numpy(src).cuda()
    d_images = torch.full((total,), CANARY, dtype=torch.uint8, device="cuda")
    (s0, b0, i0, c0), (s1, b1, i1, c1) = rows[0], rows[2]
    bad = {"overlap": [(s0, b0, i0, c0), (s1, b1, i0 + c0 - 1, c1)],
           "overlap, listed the other way round": [(s1, b1, i0 + c0 - 1, c1), (s0, b0, i0, c0)],
           "short image_cap": [(s0, b0, i0, c0), (s1, b1, i1, c1 - 1)],
           "source beyond the buffer": [(s0, b0, i0, c0), (len(src) - 10, 11, i1, c1)],
           "region beyond the images": [(s0, b0, i0, c0), (s1, b1, total - c1 + 1, c1)]}
    for name, items in bad.items():
        arr = (p.ImageEncItem * len(items))()
        for j, (so, sb, io, ic) in enumerate(items):
            arr[j].src_off, arr[j].src_bytes, arr[j].image_off, arr[j].image_cap, arr[j].image_bytes = so, sb, io, ic, 9900 + j
        rc = p.lib().fourmc_gpu_images_compress(int(d_src.data_ptr()), len(src), int(d_images.data_ptr()), total, p.MAGIC_4MC, 1,
                                                C.cast(arr, C.c_void_p), len(items), int(torch.cuda.current_stream().cuda_stream))
        assert rc == -3, (name, rc)
        assert [(a.src_off, a.src_bytes, a.image_off, a.image_cap, a.image_bytes) for a in arr] == \
            [it + (9900 + j,) for j, it in enumerate(items)], name
        with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_compress failed \(-3\)"):
            p.compress_images(d_src, items, d_images)
        torch.cuda.synchronize()
        assert bool((d_images == CANARY).all()), name
    with pytest.raises(p.EngineError, match=r"failed \(-3\)"):
        p.compress_images(d_src, rows, d_images, magic=0x11223344)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_images(d_src.cpu(), rows, d_images)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.compress_images(d_src, rows, d_images.cpu())
    with pytest.raises(p.EngineError, match="beyond the tensor"):
        p.compress_images(d_src, rows, d_images, images_bytes=total + 1)
    assert p.compress_images(d_src, [], d_images) == []
    assert bool((d_images == CANARY).all())
    # and the same items, made right, encode
    lens = p.compress_images(d_src, [rows[0], rows[2]], d_images)
    assert lens == [len(single(p, src, d_src, s0, b0, False, 1)), len(single(p, src, d_src, s1, b1, False, 1))]


# ---- 10: the staging the batch relies on --------------------------------------------------------------------------------------
STAGE_LENS = [1, 255, 256, 257, 4097, 65546, 65547, 70001, 12288, 100000, 33, 300001, 512, 5]
STAGE_CODECS = {"lz4 fast": (0, 0, 0), "lz4 parallel": (0, 0, 1), "lz4 mc": (1, 0, 0), "lz4 hc 4": (2, 4, 0), "lz4 hc 9": (2, 9, 0),
                "lz4 hc 12": (2, 12, 0), "zstd 1": (3, 1, 0), "zstd 12": (3, 12, 0)}


def _stage_run(p, d_src, soffs, lens, doffs, size, codec, level):
    d_dst = torch.full((size,), CANARY, dtype=torch.uint8, device="cuda")
    batch = p.DeviceBatch(p.make_blocks(soffs, doffs, lens, lens))
    p.encode_blocks(d_src, d_dst, batch, codec, level)
    torch.cuda.synchronize()
    return batch.download(), d_dst.cpu().numpy()


@pytest.mark.parametrize("name", list(STAGE_CODECS))
def test_encoders_stay_inside_abutting_slots(p, name):
    """What the batch's staging formula assumes, through the public container encode: block i's slot is [dst_off, dst_off + src_len)
    with dst_cap = src_len, the slots start 256-byte aligned and abut (the next starts at the next multiple of 256), and no encoder
    writes a byte past dst_off + dst_cap - neither into the canary bytes up to the next slot nor into the next slot's payload.
    The payloads are those of the same blocks in slots a page apart.  Compressible text and stored (random) blocks, odd lengths,
    lengths that are multiples of 256 (no canary between those slots: only the neighbour's payload shows a trespass)."""
    codec, level, mode = STAGE_CODECS[name]
    data = golden()
    rng = np.random.default_rng(77)
    chunks = [data[11 * i:11 * i + n] if i % 3 != 2 else rng.integers(0, 256, n, dtype=np.uint8) for i, n in enumerate(STAGE_LENS)]
    src, spans = pack_sources(chunks)
    d_src = torch.from_numpy(src).cuda()
    soffs, lens = [s[0] for s in spans], [s[1] for s in spans]
    tight, roomy, a, b = [], [], 0, 0
    for n in lens:
        tight.append(a); roomy.append(b)
        a += (n + 255) & ~255
        b += ((n + 255) & ~255) + 4096
    L = p.lib()
    old = L.fourmc_gpu_get_lz4_encode_mode()
    L.fourmc_gpu_set_lz4_encode_mode(mode)
    try:
        rb, rbuf = _stage_run(p, d_src, soffs, lens, roomy, b + 4096, codec, level)
        tb, tbuf = _stage_run(p, d_src, soffs, lens, tight, a + 4096, codec, level)
    finally:
        L.fourmc_gpu_set_lz4_encode_mode(old)
    trespass = []
    for i, n in enumerate(lens):
        r = int(tb["result"][i])
        assert 1 <= r <= n and r == int(rb["result"][i]) and tb["xxh32"][i] == rb["xxh32"][i], (name, i, n, r, int(rb["result"][i]))
        if i % 3 == 2:
            assert r == n                                  # stored
        end = tight[i + 1] if i + 1 < len(lens) else a + 4096
        if (tbuf[tight[i] + n:end] != CANARY).any():
            trespass.append((i, n, int(np.flatnonzero(tbuf[tight[i] + n:end] != CANARY)[-1]) + 1))
        if (rbuf[roomy[i] + n:roomy[i] + n + 4096] != CANARY).any():
            trespass.append((i, n, "roomy", int(np.flatnonzero(rbuf[roomy[i] + n:roomy[i] + n + 4096] != CANARY)[-1]) + 1))
    assert not trespass, (name, "bytes written past dst_off + dst_cap: (block, src_len, bytes past)", trespass)
    for i, n in enumerate(lens):
        r = int(tb["result"][i])
        assert tbuf[tight[i]:tight[i] + r].tobytes() == rbuf[roomy[i]:roomy[i] + r].tobytes(), (name, i, "payload differs")
        assert helpers.orc_xxh32(tbuf[tight[i]:tight[i] + r]) == int(tb["xxh32"][i]), (name, i)
