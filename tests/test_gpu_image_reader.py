"""The streaming image reader (fourmc_gpu_image_reader_*, ImageReader): for every way an image is cut into appends, the status and
the decoded bytes are the ones decompress_image gives for the concatenation - and so the CLI's verdict - with bounded staging,
stream-order safety, other engine calls and other readers in between, and the Python lifecycle."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

ROOT = helpers.ROOT
B = helpers.B
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "corpus_manifest.json")))
EINVAL = -3
GUARD = 4096
CONFIGS = [(False, lv) for lv in (1, 2, 3, 4)] + [(True, lv) for lv in (1, 2, 3)]


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _magic(p, z):
    return p.MAGIC_4MZ if z else p.MAGIC_4MC


def _cuda(b):
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    return torch.from_numpy(a.copy()).cuda() if len(a) else torch.zeros(0, dtype=torch.uint8, device="cuda")


def _be(v):
    return int(v).to_bytes(4, "big")


def compress(p, data, z, level):
    d_src = _cuda(np.ascontiguousarray(data).tobytes())
    d_img = torch.empty(p.image_bound(len(data)), dtype=torch.uint8, device="cuda")
    n = p.compress_image(d_src, d_img, _magic(p, z), level)
    return d_img[:n].cpu().numpy().tobytes()


def _cap(p, image, z):
    return p.decompress_image(_cuda(image) if len(image) else torch.zeros(64, dtype=torch.uint8, device="cuda"), None,
                              _magic(p, z), image_bytes=len(image))["total_bytes"]


def oracle(p, image, z, cap):
    """decompress_image of the whole image into a destination of cap bytes: (status, bytes up to decoded_bytes)"""
    d_img = torch.zeros(len(image) + 4096, dtype=torch.uint8, device="cuda")
    if len(image):
        d_img[:len(image)] = _cuda(image)
    d_dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    st = p.decompress_image(d_img, d_dst[:cap], _magic(p, z), image_bytes=len(image))
    return st, d_dst[:st["decoded_bytes"]].cpu().numpy().tobytes()


def pieces(n, cuts):
    """[(a, b)] of the image [0, n) cut into the sizes `cuts` (None: the rest; zeros are empty appends)"""
    out, at = [], 0
    for c in cuts:
        c = n - at if c is None else c
        out.append((at, at + c))
        at += c
    assert at == n, (at, n)
    return out


def read(p, image, z, cuts, cap, batch_blocks=4, own=True):
    """ImageReader over `image` appended in the pieces `cuts`.  own: every chunk is its own tensor of exactly its size, else a
    view of one device copy.  Checks the guard bytes behind cap.  Returns (status, bytes up to decoded_bytes)."""
    d_dst = torch.full((cap + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    whole = None if own else _cuda(image)
    with p.ImageReader(d_dst[:cap], _magic(p, z), batch_blocks) as r:
        for a, b in pieces(len(image), cuts):
            r.append(_cuda(image[a:b]) if own else whole[a:b])
        st = r.finish()
    assert bool((d_dst[cap:] == 0x5A).all()), "bytes behind dst_cap were written"
    return st, d_dst[:st["decoded_bytes"]].cpu().numpy().tobytes()


def check(p, image, z, cuts, cap=None, batch_blocks=4, want=None, own=True, tag=""):
    cap = max(_cap(p, image, z) if cap is None else cap, 1)          # a destination of 0 bytes would be a NULL pointer
    want = oracle(p, image, z, cap) if want is None else want
    got = read(p, image, z, cuts, cap, batch_blocks, own)
    assert got[0] == want[0], (tag, cuts if len(cuts) < 8 else len(cuts), got[0], want[0])
    assert got[1] == want[1], (tag, len(got[1]), len(want[1]))
    return got


def random_cuts(n, seed, hi=3 * B // 2, empties=True):
    rng = np.random.default_rng(seed)
    cuts, at = [], 0
    while at < n:
        if empties and rng.integers(0, 4) == 0:
            cuts.append(0)
        c = int(min(rng.integers(1, hi), n - at))
        cuts.append(c)
        at += c
    return cuts + ([0] if empties else [])


def framing_offsets(image):
    """every byte offset of every framing field of a single-stream image: the file header, each block header, the end mark and the
    footer (its size field and its body)"""
    offs = list(range(0, 13))
    p = 12
    while True:
        u, c, s = (int.from_bytes(image[p + k:p + k + 4], "big") for k in (0, 4, 8))
        offs += range(p + 1, p + 13)
        if u == c == s == 0:
            break
        p += 12 + c
    offs += range(p + 12, len(image) + 1)
    return sorted(set(offs))


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


@pytest.fixture(scope="module")
def golden():
    c = MANIFEST["corpus"]
    data = helpers.corpus(c["bytes"], first_block=c["first_block"], seed=c["seed"])
    assert _sha(data) == c["sha256"]
    return data


def _inputs(golden):
    return {"0": golden[:0], "1": golden[:1], "4M-1": golden[:B - 1], "4M": golden[:B], "4M+1": golden[:B + 1],
            "3B+tail": golden[:3 * B + 54321]}


# ---- cuts ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z,level", CONFIGS)
def test_every_cut_gives_the_whole_image_status(p, golden, z, level):
    for name, data in _inputs(golden).items():
        image = compress(p, data, z, level)
        cap = max(len(data), 1)
        want = oracle(p, image, z, cap)
        assert want[0]["reason"] == 0 and want[1] == data.tobytes(), name
        n = len(image)
        check(p, image, z, [None], cap, want=want, tag=name)
        check(p, image, z, [None], cap, batch_blocks=0, want=want, tag=name)
        for q in framing_offsets(image):
            check(p, image, z, [q, None], cap, want=want, own=False, tag=(name, q))
        for seed in range(3):
            check(p, image, z, random_cuts(n, seed, hi=max(2, n // 5)), cap, want=want, tag=(name, seed))
        if name == "3B+tail":
            check(p, image, z, [None], cap, batch_blocks=1, want=want, tag="batch 1")
            check(p, image, z, [B + 17, None], cap, batch_blocks=2, want=want, tag="batch 2")


@pytest.mark.parametrize("z", [False, True])
def test_one_byte_appends(p, golden, z):
    data = golden[:60000] if not z else golden[:70000]
    image = compress(p, data, z, 1)
    assert len(image) < 64000, len(image)
    st, out = check(p, image, z, [1] * len(image), len(data), own=False)
    assert st["reason"] == 0 and out == data.tobytes()


# ---- damage ----------------------------------------------------------------------------------------------------------------
def _refoot(img):
    b = bytearray(img)
    fsz = int.from_bytes(b[-12:-8], "big")
    f0 = len(b) - fsz
    b[-4:] = _be(helpers.orc_xxh32(np.frombuffer(bytes(b[f0:-4]), np.uint8)))
    return bytes(b)


def _damage_cases(p, golden):
    # three blocks: compressed, stored (random bytes do not shrink), a compressed tail
    data = np.concatenate([golden[:B], np.random.default_rng(5).integers(0, 256, B, dtype=np.uint8), golden[2 * B:2 * B + 40000]])
    base = compress(p, data, False, 1)
    n = len(base)
    c0 = int.from_bytes(base[16:20], "big")
    h1 = 24 + c0
    c1 = int.from_bytes(base[h1 + 4:h1 + 8], "big")
    assert c1 == B == int.from_bytes(base[h1:h1 + 4], "big")
    h2 = h1 + 12 + c1
    c2 = int.from_bytes(base[h2 + 4:h2 + 8], "big")
    eos = h2 + 12 + c2
    foot = eos + 12
    assert base[eos:eos + 12] == b"\0" * 12 and foot + 20 + 12 == n
    cases = {"empty": b"", "trunc_2": base[:2], "trunc_8": base[:8], "trunc_12": base[:12], "trunc_hdr1": base[:18],
             "trunc_after_hdr": base[:24], "trunc_payload": base[:24 + c0 // 2], "trunc_block_boundary": base[:h1],
             "trunc_block1_hdr": base[:h1 + 7], "trunc_before_eos": base[:eos], "trunc_in_eos": base[:eos + 5],
             "trunc_after_eos": base[:foot], "trunc_footer_2": base[:foot + 2], "trunc_footer_size": base[:foot + 4],
             "trunc_footer_last": base[:n - 1]}
    m = bytearray(base); m[1] ^= 0x40; cases["bad_magic"] = bytes(m)
    m = bytearray(base); m[7] = 2; cases["bad_version"] = bytes(m)
    m = bytearray(base); m[11] ^= 1; cases["bad_header_checksum"] = bytes(m)
    m = bytearray(base); m[h1 + 4:h1 + 8] = _be(B + 1); cases["csize_beyond"] = bytes(m)
    m = bytearray(base); m[12:16] = _be(B + 1); cases["usize_beyond_sum_ok"] = bytes(m)
    m = bytearray(base); m[12:16] = _be(B + 1); m[30] ^= 1; cases["usize_beyond_sum_bad"] = bytes(m)
    m = bytearray(base); m[24 + c0 // 3] ^= 0x10; cases["flipped_payload"] = bytes(m)
    m = bytearray(base); m[h2 + 12:h2 + 12 + c2] = b"\xff" * c2
    m[h2 + 8:h2 + 12] = _be(helpers.orc_xxh32(np.frombuffer(bytes(m[h2 + 12:h2 + 12 + c2]), np.uint8))); cases["corrupt_payload_sum_ok"] = bytes(m)
    cases["missing_eos"] = base[:eos] + base[foot:]
    m = bytearray(base); m[-1] ^= 1; cases["bad_footer_checksum"] = bytes(m)
    m = bytearray(base); m[foot + 7] = 2; cases["bad_footer_version"] = _refoot(bytes(m))
    m = bytearray(base); m[foot:foot + 4] = _be(5); cases["footer_size_below_8"] = bytes(m)
    cases["trailing_3"] = base + b"xyz"
    cases["trailing_16"] = base + bytes(range(16))
    second = bytearray(base); second[24 + 100] ^= 1
    cases["second_stream_flip"] = base + bytes(second)
    cases["second_stream_trunc"] = base + base[:h1 + 3]
    return cases


def cli_decode(exe, tmp_path, image, z, tag):
    src = tmp_path / f"dmg_{tag}"
    out = tmp_path / f"dec_{tag}"
    src.write_bytes(bytes(image))
    r = subprocess.run([exe, "-d"] + (["-z"] if z else []) + ["-f", str(src), str(out)], capture_output=True, timeout=300)
    return r.returncode, r.stderr.decode(errors="replace"), out.read_bytes() if out.exists() else b""


def _schedules(n):
    return {"whole": [None], "random": random_cuts(n, 11, hi=B // 3), "65537": [65537] * (n // 65537) + [None]}


def test_damaged_images_end_as_the_whole_image_decode_and_the_cli(p, golden, tmp_path):
    seen = set()
    for name, img in _damage_cases(p, golden).items():
        cap = _cap(p, img, False)
        want = oracle(p, img, False, cap)
        for sname, cuts in _schedules(len(img)).items():
            check(p, img, False, cuts, cap, want=want, own=sname != "65537", tag=(name, sname))
        code, err, out = cli_decode(p.cli_path(), tmp_path, img, False, name)
        assert want[0]["exit_code"] == code, (name, want[0], err)
        if code:
            assert want[0]["message"] and want[0]["message"] in err, (name, want[0]["message"], err)
        assert want[1] == out, name
        seen.add(want[0]["reason"])
    assert seen == set(range(16)), sorted(seen)


def test_damaged_4mz(p, golden):
    base = compress(p, golden[:B + 3000], True, 1)
    c0 = int.from_bytes(base[16:20], "big")
    m = bytearray(base); m[24 + c0 - 1] ^= 0x55
    m[20:24] = _be(helpers.orc_xxh32(np.frombuffer(bytes(m[24:24 + c0]), np.uint8)))
    cases = {"z_flip": base[:24] + bytes([base[24] ^ 1]) + base[25:], "z_corrupt": bytes(m), "z_trunc": base[:-3],
             "z_cat_second": base + base[:30], "z_usize_beyond": base[:12] + _be(B + 9) + base[16:]}
    for name, img in cases.items():
        cap = _cap(p, img, True)
        want = oracle(p, img, True, cap)
        for sname, cuts in _schedules(len(img)).items():
            check(p, img, True, cuts, cap, want=want, tag=(name, sname))


def test_footers_that_claim_a_large_size(p, golden):
    base = compress(p, golden[:B // 2], False, 1)
    fsz = int.from_bytes(base[-12:-8], "big")
    f0 = len(base) - fsz
    # a size field claiming 64 MiB, followed by 6 MiB of bytes in several appends: the footer is short
    img = base[:f0] + _be(64 << 20) + base[f0 + 4:] + bytes(np.random.default_rng(3).integers(0, 256, 6 << 20, dtype=np.uint8))
    cap = B // 2
    st, _ = check(p, img, False, [f0 + 2, 3, 1 << 20, 0, 999999, None], cap)
    assert st["reason"] == 13 and st["fail_offset"] == f0
    # a well-formed 5 MiB footer whose checksum spans many appends: the stream ends cleanly
    big = 5 * (1 << 20) + 8
    foot = bytearray(_be(big) + _be(1) + bytes(np.random.default_rng(4).integers(0, 256, big - 12, dtype=np.uint8)))
    foot += _be(helpers.orc_xxh32(np.frombuffer(bytes(foot), np.uint8)))
    img = base[:f0] + bytes(foot)
    st, out = check(p, img, False, random_cuts(len(img), 5, hi=1 << 20), cap)
    assert st["reason"] == 0 and st["fail_offset"] == len(img) and out == golden[:B // 2].tobytes()
    bad = bytearray(img); bad[f0 + 100] ^= 1
    st, _ = check(p, bytes(bad), False, [f0 + 7, 12345, 1, None], cap)
    assert st["reason"] == 14


def test_bytes_after_an_empty_stream_and_a_second_stream_cut_in_its_header(p, golden):
    empty = compress(p, golden[:0], False, 1)
    base = compress(p, golden[:B + 99], False, 2)
    img = empty + base                               # the empty stream ends the file: nothing after it is read
    for q in list(range(len(empty) + 16)) + [len(img) // 2, len(img)]:
        st, out = check(p, img, False, [q, None], B + 99, own=False)
    assert st["reason"] == 0 and st["decoded_bytes"] == 0 and st["fail_offset"] == len(img) and st["streams"] == 1
    for tail in (b"x", bytes(5), bytes(100)):
        st, _ = check(p, empty + tail, False, [3, None], 64)
        assert st["reason"] == 0
    img = base + base[:7]
    cap = B + 99
    for q in list(range(len(base) - 40, len(img) + 1)):
        st, out = check(p, img, False, [q, None], cap, own=False)
    assert st["reason"] == 3 and st["fail_offset"] == len(base) and out == golden[:B + 99].tobytes()


# ---- destination -----------------------------------------------------------------------------------------------------------
def test_a_destination_one_byte_short(p, golden):
    data = golden[:3 * B + 777]
    for z in (False, True):
        image = compress(p, data, z, 1)
        for cuts in ([None], random_cuts(len(image), 21, hi=B), [1 << 20] * (len(image) >> 20) + [None]):
            st, _ = check(p, image, z, cuts, len(data) - 1, batch_blocks=2)
            assert st["reason"] == 16 and st["exit_code"] == 1
        # an earlier block that fails its checksum: DST_SMALL still wins, as in the whole-image decode
        bad = bytearray(image); bad[30] ^= 1
        st, _ = check(p, bytes(bad), z, [None], len(data) - 1, batch_blocks=2)
        assert st["reason"] == 16
        st, _ = check(p, bytes(bad), z, [B // 3, None], len(data), batch_blocks=2)
        assert st["reason"] == 10 and st["fail_offset"] == 12


# ---- scale -----------------------------------------------------------------------------------------------------------------
def test_512_blocks_in_random_chunks_at_batch_64(p, golden):
    unit = torch.from_numpy(np.ascontiguousarray(golden[:4 * B])).cuda()
    d_src = unit.repeat(128)
    d_src[-1] ^= 1
    n = d_src.numel()
    assert n == 512 * B
    d_img = torch.empty(p.image_bound(n), dtype=torch.uint8, device="cuda")
    m = p.compress_image(d_src, d_img, p.MAGIC_4MC, 1)
    d_want = torch.empty(n, dtype=torch.uint8, device="cuda")
    want = p.decompress_image(d_img, d_want, p.MAGIC_4MC, image_bytes=m)
    assert want["reason"] == 0 and want["blocks"] == 512
    del d_want
    d_dst = torch.full((n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(512)
    with p.ImageReader(d_dst[:n], p.MAGIC_4MC, 64) as r:
        at = 0
        while at < m:
            c = int(min(rng.integers(1, 48 * B), m - at))
            r.append(d_img[at:at + c])
            at += c
        st = r.finish()
    assert st == want
    assert torch.equal(d_dst[:n], d_src)
    assert bool((d_dst[n:] == 0x5A).all())


@pytest.mark.parametrize("name", ["4mc-1", "4mc-2", "4mc-3", "4mc-4", "4mz-1", "4mz-2", "4mz-3", "4mz-4"])
def test_golden_corpus_images(p, golden, name):
    z, level = name.startswith("4mz"), int(name[-1])
    image = compress(p, golden, z, level)
    assert _sha(image) == MANIFEST["levels"][name]["sha256"]
    cap = len(golden)
    st, out = read(p, image, z, random_cuts(len(image), level, hi=3 * B), cap, batch_blocks=5, own=False)
    assert st["reason"] == 0 and st["blocks"] == 13 and st["decoded_bytes"] == cap
    assert _sha(out) == MANIFEST["corpus"]["sha256"]


# ---- round trip ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("z,level", [(False, 1), (False, 3), (True, 1)])
def test_writer_to_reader_round_trip(p, golden, z, level):
    data = golden[:5 * B + 4321]
    d_src = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    d_img = torch.empty(p.image_bound(len(data)), dtype=torch.uint8, device="cuda")
    with p.ImageWriter(d_img, _magic(p, z), level, 2) as w:
        for a, b in pieces(len(data), random_cuts(len(data), 7, empties=False)):
            w.append(d_src[a:b])
        m = w.finish()
    d_dst = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    with p.ImageReader(d_dst, _magic(p, z), 3) as r:
        for a, b in pieces(m, random_cuts(m, 8, hi=B)):
            r.append(d_img[a:b])
        st = r.finish()
    assert st["reason"] == 0 and st["decoded_bytes"] == len(data)
    assert torch.equal(d_dst, d_src)


# ---- lifetime and independence ---------------------------------------------------------------------------------------------
def test_chunks_overwritten_after_their_append(p, golden):
    data = golden[:3 * B + 5]
    image = compress(p, data, False, 1)
    d_dst = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    with p.ImageReader(d_dst, p.MAGIC_4MC, 2) as r:
        for a, b in pieces(len(image), random_cuts(len(image), 9, hi=B)):
            c = _cuda(image[a:b])
            r.append(c)
            c.fill_(0xEE)                            # on the stream, behind the append's work
        st = r.finish()
    assert st["reason"] == 0 and d_dst.cpu().numpy().tobytes() == data.tobytes()


def test_other_engine_calls_between_appends(p, golden):
    data = golden[:2 * B + 999]
    image = compress(p, data, True, 1)
    other = golden[B:B + 300000]
    d_other = torch.from_numpy(np.ascontiguousarray(other)).cuda()
    d_dst = torch.zeros(len(data), dtype=torch.uint8, device="cuda")
    with p.ImageReader(d_dst, p.MAGIC_4MZ, 1) as r:
        for i, (a, b) in enumerate(pieces(len(image), random_cuts(len(image), 13, hi=B // 2))):
            r.append(_cuda(image[a:b]))
            d_img = torch.empty(p.image_bound(len(other)), dtype=torch.uint8, device="cuda")
            k = p.compress_image(d_other, d_img, p.MAGIC_4MC if i % 2 else p.MAGIC_4MZ, 1 + i % 3)
            d_back = torch.zeros(len(other), dtype=torch.uint8, device="cuda")
            assert p.decompress_image(d_img, d_back, p.MAGIC_4MC if i % 2 else p.MAGIC_4MZ, image_bytes=k)["reason"] == 0
            assert torch.equal(d_back, d_other)
            if i % 3 == 2:
                p.release_workspaces()
        st = r.finish()
    assert st["reason"] == 0 and d_dst.cpu().numpy().tobytes() == data.tobytes()


@pytest.mark.parametrize("two_streams", [False, True])
def test_two_readers_at_once(p, golden, two_streams):
    da, db = golden[:2 * B + 1], golden[B:3 * B + 777]
    ia, ib = compress(p, da, False, 2), compress(p, db, True, 2)
    sa = torch.cuda.Stream() if two_streams else torch.cuda.current_stream()
    sb = torch.cuda.Stream() if two_streams else sa
    oa = torch.zeros(len(da), dtype=torch.uint8, device="cuda")
    ob = torch.zeros(len(db), dtype=torch.uint8, device="cuda")
    ca, cb = pieces(len(ia), random_cuts(len(ia), 1, hi=B)), pieces(len(ib), random_cuts(len(ib), 2, hi=B))
    with p.ImageReader(oa, p.MAGIC_4MC, 2, stream=sa) as ra, p.ImageReader(ob, p.MAGIC_4MZ, 3, stream=sb) as rb:
        for k in range(max(len(ca), len(cb))):
            if k < len(ca):
                with torch.cuda.stream(sa):
                    ra.append(_cuda(ia[ca[k][0]:ca[k][1]]))
            if k < len(cb):
                with torch.cuda.stream(sb):
                    rb.append(_cuda(ib[cb[k][0]:cb[k][1]]))
        sta, stb = ra.finish(), rb.finish()
    torch.cuda.synchronize()
    assert sta["reason"] == 0 and stb["reason"] == 0
    assert oa.cpu().numpy().tobytes() == da.tobytes() and ob.cpu().numpy().tobytes() == db.tobytes()


def test_python_lifecycle_and_poisoning(p, golden):
    image = compress(p, golden[:1000], False, 1)
    d_dst = torch.zeros(1000, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="boom"):
        with p.ImageReader(d_dst) as r:
            r.append(_cuda(image[:10]))
            raise RuntimeError("boom")
    assert r.closed
    with pytest.raises(p.EngineError, match="finished or aborted"):
        r.append(_cuda(image[10:]))
    r = p.ImageReader(d_dst)
    r.append(_cuda(image))
    assert r.finish()["reason"] == 0
    with pytest.raises(p.EngineError, match="finished or aborted"):
        r.finish()
    with pytest.raises(p.EngineError, match="finished or aborted"):
        r.append(_cuda(image))
    with p.ImageReader(d_dst) as r:                  # leaving without finish aborts
        r.append(_cuda(image[:100]))
    assert r.closed
    L = p.lib()
    L.fourmc_gpu_image_reader_abort(None)
    # argument checks leave the reader usable
    h = C.c_void_p(0)
    s = int(torch.cuda.current_stream().cuda_stream)
    assert L.fourmc_gpu_image_reader_begin(C.byref(h), int(d_dst.data_ptr()), 1000, p.MAGIC_4MC, 1, s) == 0 and h.value
    assert L.fourmc_gpu_image_reader_append(h, None, 5) == EINVAL
    c = _cuda(image)
    assert L.fourmc_gpu_image_reader_append(h, int(c.data_ptr()), len(image)) == 0
    st = p.ImageStatus()
    assert L.fourmc_gpu_image_reader_finish(h, C.byref(st)) == 0 and st.reason == 0 and st.decoded_bytes == 1000


POISON = r"""
import ctypes as C, sys
import numpy as np, torch
sys.path[:0] = [sys.argv[2], sys.argv[2] + "/tests"]
import helpers
p = helpers.pkg()
p.gpu_init(0)
img = torch.from_numpy(np.fromfile(sys.argv[1], np.uint8)).cuda()
d = torch.zeros(helpers.B + 5, dtype=torch.uint8, device="cuda")
L, h, s = p.lib(), C.c_void_p(0), int(torch.cuda.current_stream().cuda_stream)
st = p.ImageStatus()
print(L.fourmc_gpu_image_reader_begin(C.byref(h), int(d.data_ptr()), d.numel(), p.MAGIC_4MZ, 1, s),
      L.fourmc_gpu_image_reader_append(h, int(img.data_ptr()), img.numel()),
      L.fourmc_gpu_image_reader_append(h, int(img.data_ptr()), 10),
      L.fourmc_gpu_image_reader_finish(h, C.byref(st)))
"""


def test_a_failure_poisons_the_reader(p, golden, tmp_path):
    """A decode workspace the engine cannot have (FOURMC_WS_FAIL_ABOVE, in a process of its own) fails the append that fills the
    first batch; the next append and finish return the same error."""
    path = tmp_path / "img.4mz"
    path.write_bytes(compress(p, golden[:B + 5], True, 1))
    env = dict(os.environ, FOURMC_WS_FAIL_ABOVE="1")
    r = subprocess.run([os.sys.executable, "-c", POISON, str(path), ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["0", "-4", "-4", "-4"], r.stdout
