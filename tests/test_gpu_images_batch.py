"""Many .4mc / .4mz images of one device buffer decoded with one call (fourmc_gpu_images_decompress / decompress_images).

The oracle is decompress_image on the same bytes: for every item the batch's status equals the single call's field for field, the
decoded bytes are the same, and nothing is written outside [dst_off, dst_off + total_bytes) of any item.  The images are packed
with uneven gaps between them and 4096 bytes of slack behind the last; the outputs lie between gaps filled with a canary byte.
A single call's answer is computed once per (image, capacity, parser) and shared by the cases that need it."""
import ctypes as C
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
SLACK = 4096
CANARY = 0xC3
PLAN_THREADS = 256                       # image.hip: kPlanThreads, the chunk of images_plan_kernel's scan
DST_SMALL = 16
SIZES = [0, 1, B - 1, B, B + 1, 2 * B + 5]


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


def golden():
    if "golden" not in _MEMO:
        c = MANIFEST["corpus"]
        _MEMO["golden"] = helpers.corpus(c["bytes"], first_block=c["first_block"], seed=c["seed"])
    return _MEMO["golden"]


_MEMO = {}


def _magic(p, z):
    return p.MAGIC_4MZ if z else p.MAGIC_4MC


class _parser:
    """FOURMC_IMAGE_PARSE for the calls inside (the engine reads it at every call)"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.old = os.environ.pop("FOURMC_IMAGE_PARSE", None)
        if self.name:
            os.environ["FOURMC_IMAGE_PARSE"] = self.name

    def __exit__(self, *exc):
        os.environ.pop("FOURMC_IMAGE_PARSE", None)
        if self.old is not None:
            os.environ["FOURMC_IMAGE_PARSE"] = self.old


def compressed(p, n, z):
    """the image compress_image writes for the first n bytes of the golden corpus at level 1"""
    key = ("img", n, z)
    if key not in _MEMO:
        data = golden()[:n]
        d_src = torch.from_numpy(np.ascontiguousarray(data)).cuda() if n else torch.zeros(0, dtype=torch.uint8, device="cuda")
        d_img = torch.empty(p.image_bound(n), dtype=torch.uint8, device="cuda")
        k = p.compress_image(d_src, d_img, _magic(p, z), 1)
        _MEMO[key] = d_img[:k].cpu().numpy().tobytes()
    return _MEMO[key]


def crafted(p, z, blocks):
    """an image of the given blocks (uint8 arrays), each compressed by the oracle or stored when that does not shrink it;
    returns (image, [csize per block])"""
    us, cs, sums, pays = [], [], [], []
    for blk in blocks:
        blk = np.ascontiguousarray(blk, dtype=np.uint8)
        r, comp = (0, None)
        if len(blk) > 16:
            r, comp = helpers.orc_zstd_compress(blk, 1, len(blk) - 1) if z else helpers.orc_compress(blk, len(blk) - 1)
        pay = comp[:r].tobytes() if r > 0 else blk.tobytes()
        us.append(len(blk)); cs.append(len(pay)); sums.append(helpers.orc_xxh32(np.frombuffer(pay, np.uint8))); pays.append(pay)
    return p.assemble_container(_magic(p, z), us, cs, sums, pays), cs


def tiny(p, k, seed, z=False):
    """k stored blocks of 1 - 3 bytes (usize == csize)"""
    rng = np.random.default_rng(1000 + seed)
    return crafted(p, z, [rng.integers(0, 256, 1 + (seed + j) % 3, dtype=np.uint8) for j in range(k)])[0]


def _status_of(p, st):
    res = {name: int(getattr(st, name)) for name, _ in p.ImageStatus._fields_}
    res["message"] = p.lib().fourmc_gpu_image_reason_text(st.reason).decode()
    return res


def single(p, d_view, n, z, cap, query, scratch):
    """the single call on the image's bytes where they lie in the packed buffer; (status, decoded bytes)"""
    if query:
        return p.decompress_image(d_view, None, _magic(p, z), image_bytes=n), b""
    scratch[:cap + 64].fill_(CANARY)
    if cap:
        st = p.decompress_image(d_view, scratch[:cap], _magic(p, z), image_bytes=n)
    else:
        # a capacity of 0 with a destination: decompress_image would pass the empty tensor as NULL, which is the size query
        raw = p.ImageStatus()
        rc = p.lib().fourmc_gpu_image_decompress(int(d_view.data_ptr()), n, int(scratch.data_ptr()), 0, _magic(p, z), C.byref(raw),
                                                 int(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, p.lib().fourmc_gpu_last_error()
        st = _status_of(p, raw)
    return st, scratch[:st["decoded_bytes"]].cpu().numpy().tobytes()


def check_batch(p, images, z, parser=None, refs=None, caps=None, query=False, stream=None, fresh=False):
    """Packs `images`, runs one batch over the items `refs` (indices into images; default: each once) and checks every item
    against the single call.  caps: {item: dst_cap} overrides (default: total_bytes plus 0, 7 or 130 bytes).  Returns the statuses."""
    refs = list(range(len(images))) if refs is None else refs
    caps = caps or {}
    offs, pos = [], 5
    for i, img in enumerate(images):
        offs.append(pos)
        pos += len(img) + (i * i * 7 + 3) % 97                       # uneven gaps; the decoders' 64 bytes of over-read land in them
    buf = np.full(pos + SLACK, 0x5A, np.uint8)
    for img, o in zip(images, offs):
        buf[o:o + len(img)] = np.frombuffer(img, np.uint8)
    d_buf = torch.from_numpy(buf).cuda()
    with _parser(parser):
        # the single calls: the sizes, then the decode at the item's capacity
        totals, want = [], []
        views = [d_buf[offs[r]:offs[r] + len(images[r])] if len(images[r]) else d_buf[offs[r]:offs[r] + 1] for r in refs]
        for k, r in enumerate(refs):
            key = ("q", images[r], z, parser)
            if key not in _MEMO or fresh:
                _MEMO[key] = single(p, views[k], len(images[r]), z, 0, True, None)[0]
            totals.append(_MEMO[key]["total_bytes"])
        cap_of = [caps.get(k, totals[k] + (0, 7, 130)[k % 3]) for k in range(len(refs))]
        scratch = torch.empty(max(cap_of, default=0) + 64, dtype=torch.uint8, device="cuda")
        for k, r in enumerate(refs):
            if query:
                want.append((_MEMO[("q", images[r], z, parser)], b""))
                continue
            key = ("d", images[r], z, parser, cap_of[k])
            if key not in _MEMO or fresh:
                _MEMO[key] = single(p, views[k], len(images[r]), z, cap_of[k], False, scratch)
            want.append(_MEMO[key])
        # the outputs between canary gaps
        dsts, dpos = [], 64 + 3
        for k in range(len(refs)):
            dsts.append(dpos)
            dpos += cap_of[k] + 32 + (k * 13) % 61
        d_dst = torch.full((dpos + 64,), CANARY, dtype=torch.uint8, device="cuda")
        items = [(offs[r], len(images[r]), dsts[k], cap_of[k]) for k, r in enumerate(refs)]
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        got = p.decompress_images(d_buf, items, None if query else d_dst, _magic(p, z), images_bytes=pos, stream=stream)
        if stream is not None:
            stream.synchronize()
    out = d_dst.cpu().numpy()
    assert len(got) == len(refs)
    covered = np.zeros(len(out), bool)
    for k, (st, (wst, wbytes)) in enumerate(zip(got, want)):
        assert st == wst, (k, refs[k], st, wst)
        d, cap, n = dsts[k], cap_of[k], st["decoded_bytes"]
        assert n <= cap
        if query or st["reason"] == DST_SMALL:
            assert n == 0
        else:
            assert out[d:d + n].tobytes() == wbytes, (k, "decoded bytes differ from the single call's")
            covered[d:d + min(st["total_bytes"], cap)] = True      # bytes in [decoded_bytes, total_bytes) are unspecified
    assert (out[~covered] == CANARY).all(), "bytes written outside [dst_off, dst_off + total_bytes) of the items"
    return got


# ---- 1: sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parser", ["auto", "walk"])
@pytest.mark.parametrize("z", [False, True], ids=["4mc", "4mz"])
def test_sizes(p, z, parser):
    images = [compressed(p, n, z) for n in SIZES]
    got = check_batch(p, images, z, parser)
    data = golden()
    for n, st in zip(SIZES, got):
        assert st["reason"] == 0 and st["exit_code"] == 0 and st["decoded_bytes"] == n == st["total_bytes"], (n, st)
        assert st["blocks"] == (n + B - 1) // B and st["streams"] == 1
    # the single call is the oracle; that it decodes to the input is test_gpu_image.py's, checked once more for the largest
    assert _MEMO[("d", images[-1], z, parser, SIZES[-1] + (0, 7, 130)[5 % 3])][1] == data[:SIZES[-1]].tobytes()


# ---- 2: wave seams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("parser", ["auto", "walk"])
@pytest.mark.parametrize("count", [65, 130, PLAN_THREADS + 1])
def test_wave_seams(p, count, parser):
    """65 and 130 images cross the 64-lane seams of the scan over images; one image of 65 blocks and one of 130, behind the
    others, cross the seam of the per-image descriptor loop with descriptor, source and destination bases that are not zero;
    kPlanThreads + 1 images take the plan's carry into a second chunk."""
    images = [tiny(p, i % 4, i) for i in range(count)]
    if count <= 130:
        images += [tiny(p, 65, 7000), tiny(p, 130, 7001)]
    got = check_batch(p, images, False, parser)
    for i in range(count):
        assert got[i]["reason"] == 0 and got[i]["blocks"] == i % 4, (i, got[i])
    if count <= 130:
        assert [g["blocks"] for g in got[count:]] == [65, 130] and all(g["reason"] == 0 for g in got[count:])


# ---- 3: damage in company -----------------------------------------------------------------------------------------------------
def _be(v):
    return int(v).to_bytes(4, "big")


def _refoot(img):
    b = bytearray(img)
    fsz = int.from_bytes(b[-12:-8], "big")
    b[-4:] = _be(helpers.orc_xxh32(np.frombuffer(bytes(b[len(b) - fsz:-4]), np.uint8)))
    return bytes(b)


def damaged_and_clean(p, z):
    """[(name, image)]: clean images interleaved with one damaged image per rule, from a three-block base (compressed, stored,
    compressed)"""
    key = ("damage", z)
    if key in _MEMO:
        return _MEMO[key]
    text = golden()
    noise = np.random.default_rng(5).integers(0, 256, 5000, dtype=np.uint8)
    base, (c0, c1, c2) = crafted(p, z, [text[:70000], noise, text[B:B + 30000]])
    assert c0 < 70000 and c1 == 5000 and c2 < 30000
    n = len(base)
    h1 = 24 + c0
    h2 = h1 + 12 + c1
    eos = h2 + 12 + c2
    foot = eos + 12
    assert base[eos:eos + 12] == b"\0" * 12 and foot + 20 + 12 == n
    other = crafted(p, z, [text[2 * B:2 * B + 40000], text[5:9]])[0]
    empty = crafted(p, z, [])[0]
    assert len(empty) == 44
    cases = {}
    m = bytearray(base); m[24 + c0 // 3] ^= 0x10; cases["flipped_payload"] = bytes(m)
    m = bytearray(base); m[h2 + 12:h2 + 12 + c2] = b"\xff" * c2
    m[h2 + 8:h2 + 12] = _be(helpers.orc_xxh32(np.frombuffer(bytes(m[h2 + 12:h2 + 12 + c2]), np.uint8))); cases["corrupt_behind_good_sum"] = bytes(m)
    cases.update({"trunc_file_header": base[:8], "trunc_block_header": base[:h1 + 7], "trunc_payload": base[:24 + c0 // 2],
                  "trunc_end_mark": base[:eos + 5], "trunc_footer_size": base[:foot + 2], "trunc_footer_body": base[:n - 1]})
    m = bytearray(base); m[1] ^= 0x40; cases["wrong_magic"] = bytes(m)
    m = bytearray(base); m[11] ^= 1; cases["wrong_header_checksum"] = bytes(m)
    m = bytearray(base); m[-1] ^= 1; cases["wrong_footer_checksum"] = bytes(m)
    m = bytearray(base); m[foot + 7] = 2; cases["wrong_footer_version"] = _refoot(bytes(m))
    m = bytearray(base); m[h1 + 4:h1 + 8] = _be(B + 1); cases["csize_beyond"] = bytes(m)
    m = bytearray(base); m[12:16] = _be(B + 1); cases["usize_beyond_good_hash"] = bytes(m)
    m = bytearray(base); m[12:16] = _be(B + 1); m[30] ^= 1; cases["usize_beyond_bad_hash"] = bytes(m)
    cases["two_streams"] = base + other
    cases["trailing_bytes"] = base + b"xyz"
    cases["empty_stream_then_garbage"] = empty + bytes(range(40))
    cases["no_bytes"] = b""
    second = bytearray(other); second[30] ^= 1
    cases["second_stream_flipped"] = base + bytes(second)
    clean = [base, other, crafted(p, z, [text[B + 7:B + 7 + 100000]])[0], empty]
    out = []
    for i, (name, img) in enumerate(cases.items()):
        out.append(("clean%d" % (i % len(clean)), clean[i % len(clean)]))
        out.append((name, img))
    out.append(("clean_last", base))
    _MEMO[key] = out
    return out


@pytest.mark.parametrize("parser", ["auto", "walk"])
@pytest.mark.parametrize("z", [False, True], ids=["4mc", "4mz"])
def test_damage_in_company(p, z, parser):
    named = damaged_and_clean(p, z)
    got = check_batch(p, [img for _, img in named], z, parser)
    reasons = {}
    for (name, _), st in zip(named, got):
        if name.startswith("clean"):
            assert st["reason"] == 0 and st["decoded_bytes"] == st["total_bytes"], (name, st)     # bytes: check_batch
        else:
            reasons[name] = st["reason"]
    # the damage is what it is meant to be: every verdict but "wrong version" (4) is among the statuses compared
    assert set(reasons.values()) == set(range(16)) - {4}, reasons
    assert reasons["two_streams"] == 0 and reasons["empty_stream_then_garbage"] == 0
    assert reasons["flipped_payload"] == 10 and reasons["corrupt_behind_good_sum"] == 11
    two = got[[n for n, _ in named].index("two_streams")]
    assert two["streams"] == 2 and two["blocks"] == 5


# ---- 4 .. 7 -------------------------------------------------------------------------------------------------------------------
def small_batch(p, z):
    text = golden()
    return [crafted(p, z, [text[:50000], text[B:B + 20]])[0], crafted(p, z, [])[0], crafted(p, z, [text[77:30077]])[0],
            tiny(p, 3, 1, z), crafted(p, z, [text[3 * B:3 * B + 200000], text[:1], text[9:5009]])[0]]


@pytest.mark.parametrize("z", [False, True], ids=["4mc", "4mz"])
def test_dst_small(p, z):
    images = small_batch(p, z)
    total = [50020, 0, 30000, None, 205001]
    for short in (0, 2, 4):
        got = check_batch(p, images, z, caps={short: total[short] - 1, 1: 0})          # the empty image: a capacity of 0 is enough
        for k, st in enumerate(got):
            if k == short:
                assert st["reason"] == DST_SMALL and st["exit_code"] == 1 and st["decoded_bytes"] == 0 and st["blocks"] == 0, st
                assert st["total_bytes"] == total[short]
            else:
                assert st["reason"] == 0 and st["decoded_bytes"] == st["total_bytes"], (k, st)
    got = check_batch(p, images, z, caps={k: 0 for k in range(5)})                     # every item short but the empty one
    assert [st["reason"] for st in got] == [DST_SMALL, 0, DST_SMALL, DST_SMALL, DST_SMALL]


@pytest.mark.parametrize("parser", ["auto", "walk"])
def test_size_query(p, parser):
    for z in (False, True):
        named = damaged_and_clean(p, z)
        got = check_batch(p, [img for _, img in named] + small_batch(p, z), z, parser, query=True)
        assert all(st["decoded_bytes"] == 0 for st in got)
        assert {st["reason"] for st in got} >= {0, 1, 2, 3, 5, 6, 7, 8, 9, 12, 13, 14, 15}


def test_the_same_image_twice(p):
    images = small_batch(p, False)
    got = check_batch(p, images, False, refs=[0, 4, 0, 2, 4, 4])
    assert got[0] == got[2] and got[1] == got[4] == got[5] and got[0]["reason"] == 0


def test_argument_errors_on_the_device(p):
    images = small_batch(p, False)
    buf = b"".join(images)
    d_buf = torch.from_numpy(np.frombuffer(buf + b"\0" * SLACK, np.uint8).copy()).cuda()
    d_dst = torch.full((1 << 20,), CANARY, dtype=torch.uint8, device="cuda")
    n0, n1 = len(images[0]), len(images[1])
    bad = {"overlap": [(0, n0, 0, 60000), (n0, n1, 59999, 10)],
           "overlap, listed the other way round": [(n0, n1, 59999, 10), (0, n0, 0, 60000)],
           "image beyond the buffer": [(0, n0, 0, 60000), (len(buf) - 10, 11, 70000, 10)],
           "region beyond the destination": [(0, n0, 0, 60000), (n0, n1, (1 << 20) - 9, 10)]}
    for name, items in bad.items():
        with pytest.raises(p.EngineError, match=r"fourmc_gpu_images_decompress failed \(-3\)"):
            p.decompress_images(d_buf, items, d_dst, images_bytes=len(buf))
        torch.cuda.synchronize()
        assert bool((d_dst == CANARY).all()), name
    with pytest.raises(p.EngineError, match=r"failed \(-3\)"):
        p.decompress_images(d_buf, [(0, n0, 0, 60000)], d_dst, magic=0x11223344, images_bytes=len(buf))
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.decompress_images(d_buf.cpu(), [(0, n0, 0, 60000)], d_dst)
    with pytest.raises(p.EngineError, match="CUDA tensor"):
        p.decompress_images(d_buf, [(0, n0, 0, 60000)], d_dst.cpu())
    assert bool((d_dst == CANARY).all())
    assert p.decompress_images(d_buf, [], d_dst) == []
    # and the same items, made right, decode
    st = p.decompress_images(d_buf, [(0, n0, 0, 60000), (n0, n1, 60000, 10)], d_dst, images_bytes=len(buf))
    assert [s["reason"] for s in st] == [0, 0] and st[0]["decoded_bytes"] == 50020


# ---- 8: the block decode in several launches ------------------------------------------------------------------------------------
def child_main():
    """FOURMC_TILE_BATCH / FOURMC_SEG_BATCH are read once per process: this one has them at 64 blocks.  The images of the sizes
    case hold 8 blocks, and the LZ4 decode has no pieces below 64: a 60-block image in front of them and a 130-block image
    behind make 198 blocks, cut after 64, 128 and 192 - the first cut inside the images of the sizes case."""
    p = helpers.pkg()
    p.gpu_init(0)
    images = [tiny(p, 60, 1)] + [compressed(p, n, False) for n in SIZES] + [tiny(p, 130, 2)]
    got = check_batch(p, images, False)
    assert all(st["reason"] == 0 for st in got), got
    data = golden()
    for k, n in enumerate(SIZES):
        assert _MEMO[("d", images[1 + k], False, None, n + (0, 7, 130)[(1 + k) % 3])][1] == data[:n].tobytes(), n
    torch.cuda.synchronize()
    print("RESULT " + json.dumps({"blocks": sum(st["blocks"] for st in got)}))


def test_block_decode_in_pieces(p):
    env = dict(os.environ, FOURMC_TILE_BATCH="64", FOURMC_SEG_BATCH="64")
    env.pop("FOURMC_IMAGE_PARSE", None)
    r = subprocess.run([sys.executable, "-c", "import test_gpu_images_batch as T; T.child_main()"], cwd=HERE, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line and json.loads(line[-1][7:]) == {"blocks": 60 + 8 + 130}, r.stdout[-2000:]


# ---- 9: plumbing ----------------------------------------------------------------------------------------------------------------
def test_a_batch_on_another_stream(p):
    s = torch.cuda.Stream()
    named = damaged_and_clean(p, False)
    check_batch(p, [img for _, img in named][:12] + small_batch(p, False), False, stream=s)


@pytest.mark.parametrize("parser", ["auto", "walk"])
def test_parse_stats_count_each_image_once(p, parser):
    named = damaged_and_clean(p, False)
    images = [img for _, img in named]
    f0, w0 = p.image_parse_stats()
    d_buf = torch.from_numpy(np.frombuffer(b"".join(images) + b"\0" * SLACK, np.uint8).copy()).cuda()
    d_dst = torch.empty(len(images) * 160000, dtype=torch.uint8, device="cuda")
    items, at = [], 0
    for k, img in enumerate(images):
        items.append((at, len(img), k * 160000, 160000))
        at += len(img)
    with _parser(parser):
        p.decompress_images(d_buf, items, d_dst, images_bytes=at)
        f1, w1 = p.image_parse_stats()
        p.decompress_images(d_buf, items, None, images_bytes=at)
        f2, w2 = p.image_parse_stats()
        for (o, n, _, _) in items:
            p.decompress_image(d_buf[o:o + max(n, 1)], None, image_bytes=n)
        f3, w3 = p.image_parse_stats()
    assert (f1 - f0) + (w1 - w0) == len(images)
    assert (f1 - f0, w1 - w0) == (f2 - f1, w2 - w1) == (f3 - f2, w3 - w2)
    if parser == "walk":
        assert f1 == f0
    else:                                   # the fast path: every clean image, and damage that leaves the framing whole
        assert f1 - f0 >= sum(name.startswith("clean") for name, _ in named) and w1 - w0 >= 15


def test_release_workspaces_between_batches(p):
    images = small_batch(p, False)
    a = check_batch(p, images, False)
    p.release_workspaces()
    b = check_batch(p, images + [tiny(p, 130, 9)], False, fresh=True)       # the descriptor table grows after the first read-back
    p.release_workspaces()
    c = check_batch(p, images, False, fresh=True)
    assert a == c == b[:len(images)]
