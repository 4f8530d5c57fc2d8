"""Launches cut into pieces by the workspace the device can give, against the oracle.

When a codec cannot have its per-block workspace for a whole launch, the engine cuts the launch into pieces that run with
`d_blocks + b0` and a smaller workspace (engine.hip: in_pieces for the encoders and the zstd decode, lease_lz4_decode +
fourmc_lz4_decode_plan for the LZ4 decode); without any workspace an automatic LZ4 decode ends at the exact walker, an explicit
tile / seg choice fails with FOURMC_ENOMEM.  FOURMC_WS_FAIL_ABOVE=N makes every codec workspace lease above N bytes fail as an
out-of-memory would, so the piece sizes are chosen here: N = bytes(k), with bytes() a codec's per-block workspace formula copied
from its source below (the product library does not export them).  Each copy is pinned: one byte below one block's worth (64
blocks' for the LZ4 decoders) the call fails with FOURMC_ENOMEM, at exactly that much it succeeds.

The engine reads its FOURMC_* settings once per process, so every configuration runs in a child process of its own, one after
another.  The children report result codes, digests of the bytes they wrote and whether the guard bytes around every destination
slot survived; the parent compares those with the oracle (helpers.orc_*).  Launches are 37 blocks for the encoders and the zstd
decode (pieces of 1, 2 and 3, the last one short) and 200 for the LZ4 decode (pieces of 64 / 128), with empty, tiny,
incompressible, full 4 MiB and damaged blocks first and last in the pieces."""
import functools
import hashlib
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers
from helpers import B

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ENOMEM = -4                     # FOURMC_ENOMEM (include/fourmc_gpu.h)
BADSUM, CORRUPT = -1000000001, -1000000002
GUARD, G = 0xA5, 64             # guard byte, guard bytes on each side of a destination slot
PATHS = {"exact": 2, "auto": 6, "seg": 11, "tile": 13}
N_ENC = N_ZSTD = 37
CODEC = {"fast": 0, "par": 0, "mc": 1, "hc": 2, "zstd": 3}


# ---- per-block workspace bytes, copied from the sources ------------------------------------------------------------------
def lz4_fast_ws(m):
    """lz4_encode.hip:640-641 fourmc_lz4_fast_work_bytes: record counts (lz4emit.h:22) + an area of FOURMC_BLOCKSIZE / 4 +
    2 * kRecSlack (lz4emit.h:19, lz4_encode.hip:632-636) 16-byte records (lz4emit.h:23) per block"""
    return ((m * 4 + 255) & ~255) + m * (B // 4 + 2 * 128) * 16


def lz4_par_ws(m):
    """lz4_par_encode.hip:410-411 fourmc_lz4_par_work_bytes: kMetaBytes = kSegs * 8 + kSegs * kSegStride (:42-47) per block"""
    return m * (64 * 8 + 64 * 66048) + 256


def lz4hc_ws(m):
    """lz4hc_encode.hip:609 fourmc_lz4hc_work_bytes: kWorkBytes = (4 << kHashLog) + 2 * (kChainMask + 1) (:33-42); MC too"""
    return m * ((4 << 15) + 2 * (0x1FFFF + 1))


def lz4hc_opt_ws(m):
    """lz4hc_opt_encode.hip:304 fourmc_lz4hc_opt_work_bytes: kHeadBytes + kOptBytes (:33-36), HO_OPT_RECS = 4096 + 3 + 5
    records of 16 bytes rounded to 256 (lz4hc_opt_core.h:22-32)"""
    return m * ((4 << 15) + (((4096 + 3 + 5) * 16 + 255) & ~255))


_ZSTD_STORE = 3 * (32768 + 64) * 4 + 3 * (32768 + 64) + 64 + 128 * 1024 + 256 + 4736 + 512 + 192      # zstd_encode.hip:41-52
_ZSTD_HMAX = (15, 16, 17, 18, 19, 19, 20, 20, 21, 22, 22, 23)
_ZSTD_CMAX = (14, 15, 16, 18, 18, 18, 19, 19, 20, 21, 21, 22)


def zstd_enc_ws(m, level):
    """zstd_encode.hip:3247 fourmc_zstd_enc_work_bytes: kStoreBytes + table_bytes(level) (:78-85) per block"""
    special = {12: (4 << 23) + (2 << 23), 6: (4 << 19) + (2 << 19), 3: (4 << 17) + (4 << 16), 1: 4 << 15}
    t = special.get(level) or (6 << max(_ZSTD_HMAX[level - 1], 17)) + (8 << _ZSTD_CMAX[level - 1]) + (1 << 20)
    return m * (_ZSTD_STORE + t)


def zstd_scratch(m):
    """zstd_decode.hip:1345 fourmc_zstd_scratch_bytes: kV2Bytes = kMaxInner * kV2State + kV2Lit + kSeqArea * 8 + kBlockMax + 64
    (:753-758; kV2State: sizeof(ZState) = 20480 rounded to 256)"""
    return m * (64 * 20480 + (4 << 20) + 64 * 64 + 256 + (1 << 20) * 8 + (128 << 10) + 64)


_SRC_MAX = 4210768 + 32                                          # lz4par.h:25 kSrcMax
TILE_BLOCK = 4 * ((48 + (_SRC_MAX + 31) // 32 + 512 + 32 + 3) & ~3)                 # lz4tile.h:36-44 kWsWords, lz4_tile.hip:807
SEG_BLOCK = 4 * ((320 + 2 * (64 * (128 + 8) + _SRC_MAX // 3 + 512) + 3) & ~3)       # lz4seg.h:22-39 kWsWords, lz4_seg.hip:655


# ---- encoder families: one workspace formula each ---------------------------------------------------------------------------
FAMILIES = {"fast": lz4_fast_ws, "par": lz4_par_ws, "hc": lz4hc_ws, "hcopt": lz4hc_opt_ws}
FAMILIES.update({f"z{lv}": functools.partial(zstd_enc_ws, level=lv) for lv in range(1, 13)})
PINNED = ("fast", "par", "hc", "hcopt", "z3", "z12")
_HALVES = (37, 19, 10, 5, 3, 2, 1)          # in_pieces' piece sizes for 37 blocks: halved, rounded up (engine.hip: in_pieces)


def piece_of(fam, limit):
    """the piece size in_pieces settles on under FOURMC_WS_FAIL_ABOVE=limit (0: not even one block fits)"""
    return next((m for m in _HALVES if FAMILIES[fam](m) <= limit), 0)


def _limits():
    """Few limits (a greedy cover) under which every family runs in pieces of 1, 2 and 3 blocks, and bytes(1) - 1 and bytes(1) of
    the pinned families.  Returns the sorted limits and, per (family, k), the first limit that gives it."""
    want = {(f, k) for f in FAMILIES for k in (1, 2, 3)} | {(f, d) for f in PINNED for d in (-1, 0)}
    cands = {FAMILIES[f](k) for f in FAMILIES for k in (1, 2, 3)} | {FAMILIES[f](1) - 1 for f in PINNED}

    def covers(lim):
        s = {(f, piece_of(f, lim)) for f in FAMILIES if piece_of(f, lim) in (1, 2, 3)}
        return s | {(f, lim - FAMILIES[f](1)) for f in PINNED if lim - FAMILIES[f](1) in (-1, 0)}
    out = []
    while want:
        lim = max(sorted(cands), key=lambda x: len(covers(x) & want))
        out.append(lim)
        want -= covers(lim)
    out.sort()
    first = {}
    for lim in out:
        for f in FAMILIES:
            first.setdefault((f, piece_of(f, lim)), lim)
    return out, first


LIMITS, FIRST = _limits()


def _runs(fam, k):
    """(codec, level) launches of a family at pieces of k; the levels that share a formula take turns"""
    if fam == "hc":
        return [("hc", lv) for lv in range(k, 9, 3)] + [("mc", 0)]
    if fam == "hcopt":
        return {1: [("hc", 9), ("hc", 12)], 2: [("hc", 10), ("hc", 0)], 3: [("hc", 11), ("hc", 13)]}[k]      # 0 / 13: lz4hc.c:840
    if fam.startswith("z"):
        return [("zstd", int(fam[1:]))]
    return [(fam, 0)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def heavy(codec, level):
    """HC 10..12 and zstd 7..12 spend long on a 4 MiB block, and pieces of one block run them one after another"""
    return (codec == "hc" and (level >= 10 or level < 1)) or (codec == "zstd" and level >= 7)


@functools.lru_cache(None)
def enc_blocks(light=False):
    """37 blocks: i % 3 == 1 ordinary text, the others the unusual ones (first and last in every piece of 1, 2 or 3): empty,
    1 / 12 / 13 / 64 / 4095 / 65536 / 65547 / 300 000 bytes of text and of noise, and full 4 MiB blocks of noise (first) and
    text (last); `light`: those two cut to 200 000 bytes"""
    text = helpers.corpus(2 * B, first_block=5)
    rng = np.random.default_rng(0x9ECE)
    noise = rng.integers(0, 256, B, dtype=np.uint8)
    odd = [noise]
    for i, n in enumerate((0, 1, 12, 13, 64, 4095, 65536, 65547, 300000)):
        odd += [text[B + 1000 * i:B + 1000 * i + n], noise[7 * i:7 * i + n]]
    odd += [text[B:B + 200000], np.zeros(0, np.uint8), noise[:13], text[:65547], noise[:300000], text[:B]]
    blocks, it = [], iter(odd)
    for i in range(N_ENC):
        if i % 3 == 1:
            o = (i * 7919) % B
            blocks.append(text[o:o + 5000 + (i * 3001) % 60000])
        else:
            blocks.append(next(it))
    assert next(it, None) is None and len(blocks[0]) == B and len(blocks[-1]) == B
    return [np.ascontiguousarray(b[:200000] if light else b) for b in blocks]


def raw_caps(codec, blocks):
    """the compress bound, n - 1 (the container's), n / 2 and 0 in turn"""
    bound = helpers.zstd_bound if codec == "zstd" else helpers.oracle().orc_lz4_compress_bound
    return [(bound(len(s)), max(len(s) - 1, 0), len(s) // 2, 0)[i % 4] for i, s in enumerate(blocks)]


def _damage(rng, c, kind):
    """the mutations of test_gpu_parity.py::test_lz4_decode_corrupt_streams_match_oracle_codes"""
    m = np.array(c, dtype=np.uint8, copy=True)
    if len(m) == 0:
        return np.frombuffer(b"\x00", np.uint8).copy()
    if kind == 0:
        m[rng.integers(0, len(m))] ^= np.uint8(1 << int(rng.integers(0, 8)))
    elif kind == 1:
        m = m[: rng.integers(1, len(m)) if len(m) > 1 else 1]
    elif kind == 2:
        i = int(rng.integers(0, len(m))); m[i:i + 4] = rng.integers(0, 256, len(m[i:i + 4]), dtype=np.uint8)
    else:
        m = np.concatenate([m, rng.integers(0, 256, int(rng.integers(1, 20)), dtype=np.uint8)])
    return m


N_DEC = 200


def _at_boundary(i):
    return i % 64 in (0, 63) or i == N_DEC - 1          # first / last of the pieces of 64 and 128


@functools.lru_cache(None)
def lz4_dec_set():
    """(streams, caps, usizes): 200 raw LZ4 streams of the encoder mix, damaged copies among them (some at piece boundaries),
    capacities of the decoded size, above it, one below it, half of it and below kMinCap (lz4tile.h / lz4seg.h: the exact walker's)"""
    text = helpers.corpus(2 * B, first_block=9)
    rng = np.random.default_rng(0xDEC4)
    noise = rng.integers(0, 256, B, dtype=np.uint8)
    sizes = (0, 1, 12, 13, 64, 255, 256, 4095, 65536, 65547, 300000)
    comps, caps, usz = [], [], []
    for i in range(N_DEC):
        if i in (0, 127, N_DEC - 1):
            src = noise if i != 127 else text[:B]
        elif _at_boundary(i) or i % 7 == 0:
            n = sizes[i % len(sizes)]
            src = noise[i:i + n] if i % 2 else text[3 * i:3 * i + n]
        else:
            src = text[(i * 10007) % B:][: 2000 + (i * 4099) % 90000]
        c = helpers.orc_compress(src)[1]
        damaged = (_at_boundary(i) and i % 3 != 0) or i % 11 == 5
        if damaged:
            c = _damage(rng, c, i % 4)
        cap = (len(src), len(src) + 77, len(src) - 1, len(src) // 2, len(src))[i % 5] if len(src) else (0, 5)[i % 2]
        if i % 13 == 6:
            cap = min(cap, 200)
        comps.append(c); caps.append(max(cap, 0)); usz.append(len(src))
    return comps, caps, usz


@functools.lru_cache(None)
def container_set():
    """(payloads, usizes, sums): 4mc blocks - LZ4 payloads, stored blocks, damaged payloads and wrong checksums"""
    comps, caps, usz = lz4_dec_set()
    rng = np.random.default_rng(0x4C0)
    text = helpers.corpus(2 * B, first_block=11)
    noise = rng.integers(0, 256, B, dtype=np.uint8)
    pays, us, sums = [], [], []
    for i in range(N_DEC):
        u = usz[i]
        src = noise[:u] if i == 0 else text[(i * 131) % 1000:][:u]
        r, pay = helpers.orc_compress(src, max(u - 1, 0))
        if r <= 0 or i % 17 == 3:
            pay = src.copy()                                    # stored (src_len == dst_cap)
        else:
            pay = pay[:r]
        if (_at_boundary(i) and i % 2) or i % 19 == 4:
            pay = _damage(rng, pay, i % 4)
            s = helpers.orc_xxh32(pay)                          # the checksum fits the damaged payload: the decoder must reject it
        else:
            s = helpers.orc_xxh32(pay) ^ (1 if i % 23 == 8 else 0)
        pays.append(pay); us.append(u); sums.append(s)
    return pays, us, sums


@functools.lru_cache(None)
def zstd_dec_set():
    """37 zstd frames of levels 1, 3, 6 and 12, damaged ones at piece boundaries"""
    text = helpers.corpus(B, first_block=13)
    rng = np.random.default_rng(0x2D)
    noise = rng.integers(0, 256, 300000, dtype=np.uint8)
    frames, caps = [], []
    for i in range(N_ZSTD):
        n = (0, 1, 13, 4095, 65547, 131073, 300000, B)[i % 8]
        src = noise[:n] if i % 5 == 2 else text[:n]
        f = helpers.orc_zstd_compress(src, (1, 3, 6, 12)[i % 4])[1]
        if i % 3 != 1 and i % 2:
            f = _damage(rng, f, i % 4)
        frames.append(f); caps.append(max(n + (0, 77, -1)[i % 3], 0))
    return frames, caps


@functools.lru_cache(None)
def zstd_container_set():
    """(payloads, usizes, sums): .4mz blocks - the frames above with their checksums, stored blocks, a few wrong checksums"""
    frames, caps = zstd_dec_set()
    text = helpers.corpus(B, first_block=13)
    pays, us, sums = [], [], []
    for i, f in enumerate(frames):
        u = (0, 1, 13, 4095, 65547, 131073, 300000, B)[i % 8]
        pay = text[:u].copy() if i % 9 == 4 else f                # stored (src_len == dst_cap)
        pays.append(pay); us.append(u); sums.append(helpers.orc_xxh32(pay) ^ (1 if i % 7 == 3 else 0))
    return pays, us, sums


def _dig(a):
    return hashlib.sha1(np.ascontiguousarray(a, dtype=np.uint8).tobytes()).hexdigest()[:20]


# ---- what the oracle answers ----------------------------------------------------------------------------------------------
def _orc_encode(codec, level, s, cap):
    if codec == "fast":
        return helpers.orc_compress(s, cap)
    if codec == "mc":
        return helpers.orc_compress_mc(s, cap)
    if codec == "hc" and 1 <= level <= 8:
        return helpers.orc_compress_hc(s, level, cap)
    if codec == "hc":                                           # levels 9..12 (and their aliases): the reference's own build
        ref = helpers.ref()
        assert ref is not None, "oracle/_ref/libref4mc.so is missing (__graft_entry__.build() makes it)"
        d = np.zeros(max(cap, 1) + 64, np.uint8)
        r = ref.LZ4_compress_HC(s.ctypes.data, d.ctypes.data, len(s), cap, level)
        return r, d[:max(r, 0)]
    r, out = helpers.orc_zstd_compress(s, level, cap)
    return int(r), out


@functools.lru_cache(None)
def want_encode(codec, level, mode):
    """per block [result, digest (, xxh32)] of the oracle; container mode: capacity n - 1, stored when that gives <= 0
    (native/4mc.c:301-329)"""
    blocks = enc_blocks(heavy(codec, level))
    caps = raw_caps(codec, blocks) if mode == "raw" else [max(len(s) - 1, 0) for s in blocks]

    def one(i):
        r, out = _orc_encode(codec, level, blocks[i], caps[i])
        if mode == "raw":
            return [int(r), _dig(out[:max(r, 0)])]
        if r <= 0:
            r, out = len(blocks[i]), blocks[i]
        return [int(r), _dig(out[:r]), int(helpers.orc_xxh32(out[:r]))]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:      # the oracle's calls let go of the GIL
        return list(ex.map(one, range(len(blocks))))


@functools.lru_cache(None)
def want_zstd_container_decode():
    pays, us, sums = zstd_container_set()
    out = []
    for p, u, s in zip(pays, us, sums):
        if helpers.orc_xxh32(p) != s:
            out.append([BADSUM, _dig(p[:0])])
        elif len(p) == u:
            out.append([u, _dig(p)])
        else:
            r, o = helpers.orc_zstd_decompress(p, u)
            out.append([r if r >= 0 else CORRUPT, _dig(o)])
    return out


@functools.lru_cache(None)
def want_lz4_decode():
    comps, caps, _ = lz4_dec_set()
    return [[r, _dig(o)] for r, o in (helpers.orc_decompress(c, cap) for c, cap in zip(comps, caps))]


@functools.lru_cache(None)
def want_container_decode():
    pays, us, sums = container_set()
    out = []
    for p, u, s in zip(pays, us, sums):
        if helpers.orc_xxh32(p) != s:
            out.append([BADSUM, _dig(p[:0])])
        elif len(p) == u:
            out.append([u, _dig(p)])
        else:
            r, o = helpers.orc_decompress(p, u)
            out.append([r if r >= 0 else CORRUPT, _dig(o)])
    return out


@functools.lru_cache(None)
def want_zstd_decode():
    frames, caps = zstd_dec_set()
    return [[r, _dig(o)] for r, o in (helpers.orc_zstd_decompress(f, c) for f, c in zip(frames, caps))]


# ---- the children ----------------------------------------------------------------------------------------------------------
def _child(env, job, timeout=400):
    e = dict(os.environ, **env)
    r = subprocess.run([sys.executable, "-c", "import sys, test_gpu_pieces as T; T.child_main(sys.argv[1])", json.dumps(job)],
                       cwd=HERE, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (env, job, r.stdout[-2000:] + r.stderr[-4000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads(line[-1][7:])


class _Dev:
    """packs blocks into device buffers: sources back to back (odd offsets), each destination slot between GUARD bytes"""

    def __init__(self, p, srcs, caps, usz=None, sums=None):
        import torch
        self.torch, self.p = torch, p
        offs, pos = [], 3
        for s in srcs:
            offs.append(pos); pos += len(s)
        buf = np.zeros(pos + 64, np.uint8)
        for s, o in zip(srcs, offs):
            buf[o:o + len(s)] = s
        self.dsts, dpos = [], G + 5
        for c in caps:
            self.dsts.append(dpos); dpos += c + 2 * G
        self.caps = caps
        blocks = p.make_blocks(offs, self.dsts, [len(s) for s in srcs], caps, sums)
        self.batch = p.DeviceBatch(blocks)
        self.d_src = torch.from_numpy(buf).cuda()
        self.d_dst = torch.full((dpos + G,), GUARD, dtype=torch.uint8, device="cuda")
        self.args = (int(self.d_src.data_ptr()), int(self.d_dst.data_ptr()), self.batch.ptr, self.batch.n)
        self.stream = int(torch.cuda.current_stream().cuda_stream)

    def report(self, rc, container=False):
        """the call's return code; unless it failed, per block [result, digest of the bytes it accounts for (, xxh32)], and the
        blocks whose guard bytes changed; after a failure: the message and whether the destination is untouched"""
        self.torch.cuda.synchronize()
        out = self.d_dst.cpu().numpy()
        if rc:
            return {"rc": rc, "err": self.p.lib().fourmc_gpu_last_error().decode(), "untouched": bool((out == GUARD).all())}
        got = self.batch.download()
        res = [int(r) for r in got["result"]]
        blocks = []
        for i, (d, c, r) in enumerate(zip(self.dsts, self.caps, res)):
            row = [r, _dig(out[d:d + max(0, min(r, c))])]
            if container:
                row.append(int(got["xxh32"][i]))
            blocks.append(row)
        bad = [i for i, (d, c) in enumerate(zip(self.dsts, self.caps))
               if not ((out[d - G:d] == GUARD).all() and (out[d + c:d + c + G] == GUARD).all())]
        return {"rc": 0, "blocks": blocks, "guard_broken": bad}


def _encode(p, codec, level, mode):
    L = p.lib()
    blocks = enc_blocks(heavy(codec, level))
    caps = raw_caps(codec, blocks) if mode == "raw" else [len(s) for s in blocks]
    d = _Dev(p, blocks, caps)
    L.fourmc_gpu_set_lz4_encode_mode(1 if codec == "par" else 0)
    if mode == "container":
        rc = L.fourmc_gpu_4mc_encode_blocks(*d.args, CODEC[codec], level, d.stream)
    elif codec in ("fast", "par"):
        rc = L.fourmc_gpu_lz4_compress_fast(*d.args, d.stream)
    elif codec == "mc":
        rc = L.fourmc_gpu_lz4_compress_mc(*d.args, d.stream)
    elif codec == "hc":
        rc = L.fourmc_gpu_lz4_compress_hc(*d.args, level, d.stream)
    else:
        rc = L.fourmc_gpu_zstd_compress(*d.args, level, d.stream)
    rep = d.report(rc, mode == "container")
    L.fourmc_gpu_set_lz4_encode_mode(0)
    return rep


def _lz4_decode(p, path, container):
    L = p.lib()
    L.fourmc_gpu_set_lz4_decode_path(PATHS[path])
    if container:
        pays, us, sums = container_set()
        d = _Dev(p, pays, us, sums=sums)
        rc = L.fourmc_gpu_4mc_decode_blocks(*d.args, 0, d.stream)
    else:
        comps, caps, _ = lz4_dec_set()
        d = _Dev(p, comps, caps)
        rc = L.fourmc_gpu_lz4_decompress(*d.args, d.stream)
    return d.report(rc)


def _zstd_decode(p, split, container):
    L = p.lib()
    L.fourmc_gpu_set_zstd_decode_split(split)
    if container:
        pays, us, sums = zstd_container_set()
        d = _Dev(p, pays, us, sums=sums)
        return d.report(L.fourmc_gpu_4mc_decode_blocks(*d.args, CODEC["zstd"], d.stream))
    frames, caps = zstd_dec_set()
    d = _Dev(p, frames, caps)
    return d.report(L.fourmc_gpu_zstd_decompress(*d.args, d.stream))


def _image_calls(p, img, usize):
    """what the image calls answer for one .4mc image: decompress_image, image_decode_blocks, image_read, ImageReader"""
    import torch
    d_img = torch.from_numpy(img).cuda()
    out = {}
    d_dst = torch.full((usize + 4096,), GUARD, dtype=torch.uint8, device="cuda")
    st = p.decompress_image(d_img, d_dst)
    torch.cuda.synchronize()
    out["decompress_image"] = [st, _dig(d_dst[:usize].cpu().numpy()), bool((d_dst[usize:] == GUARD).all())]
    d_dst.fill_(GUARD)
    r = p.image_decode_blocks(d_img, 1, 3, d_dst)
    out["image_decode_blocks"] = [r, _dig(d_dst[:max(r, 0)].cpu().numpy())]
    d_dst.fill_(GUARD)
    rr = p.image_read(d_img, [(B - 100, 300, 0), (12345, 2 * B, 1000), (usize - 10, 50, 3 * B)], d_dst)
    out["image_read"] = [rr.tolist(), _dig(d_dst.cpu().numpy())]
    d_dst.fill_(GUARD)
    with p.ImageReader(d_dst) as rd:
        for o in range(0, len(img), 3 * B // 2):
            rd.append(d_img[o:o + 3 * B // 2])
        st = rd.finish()
    torch.cuda.synchronize()
    out["ImageReader"] = [st, _dig(d_dst[:usize].cpu().numpy())]
    return out


@functools.lru_cache(None)
def image_case():
    """a .4mc image of four blocks (the oracle's) and a copy with one payload byte changed (checksum failure in block 2)"""
    data = helpers.corpus(3 * B + 12345, first_block=17)
    img = helpers.orc_container(data)
    bad = img.copy()
    bad[len(img) // 2] ^= 1                                  # a payload byte of the second or third block
    return data, img, bad


def child_main(job_json):
    import torch
    job = json.loads(job_json)
    p = helpers.pkg()
    p.gpu_init(0)
    L = p.lib()
    out = {}
    for step in job["steps"]:
        kind = step[0]
        if kind == "encode":
            out["/".join(map(str, step[1:]))] = _encode(p, *step[1:])
        elif kind == "lz4":
            _, path, container = step
            out[f"{path}/{container}"] = _lz4_decode(p, path, container)
        elif kind == "zstd":
            out[f"zstd/{step[1]}/{step[2]}"] = _zstd_decode(p, step[1], step[2])
        elif kind == "images":
            data, img, bad = image_case()
            out["good"] = _image_calls(p, img, len(data))
            out["bad"] = _image_calls(p, bad, len(data))
        torch.cuda.synchronize()
    L.fourmc_gpu_set_lz4_decode_path(PATHS["auto"])
    print("RESULT " + json.dumps(out))


# ---- checks --------------------------------------------------------------------------------------------------------------
def _same_blocks(got, want, what):
    assert got["rc"] == 0, (what, got)
    assert got["guard_broken"] == [], (what, "bytes written outside the destination", got["guard_broken"])
    for i, (g, w) in enumerate(zip(got["blocks"], want)):
        assert g[0] == w[0], (what, i, "result", g[0], w[0])
        if w[0] > 0:
            assert g[1:] == w[1:], (what, i, "bytes / checksum differ")
    assert len(got["blocks"]) == len(want)


@pytest.mark.parametrize("limit", LIMITS)
def test_encoders_in_pieces(gpu, limit):
    """Every encoder family under one FOURMC_WS_FAIL_ABOVE, raw and container mode: in pieces of 1, 2 or 3 blocks the result codes,
    bytes and XXH32 are the oracle's (the ratio-tolerance encoder's: those of its own unsplit launch); a family that cannot have one
    block's workspace fails with FOURMC_ENOMEM and writes nothing - at bytes(1) - 1 of a pinned formula it must."""
    steps, expect = [], {}
    for fam in FAMILIES:
        k = piece_of(fam, limit)
        if k == 0:
            runs, modes = _runs(fam, 1)[:1], ("raw",)
        elif k in (1, 2, 3) and FIRST[(fam, k)] == limit:
            runs, modes = _runs(fam, k), ("raw", "container")
        else:
            continue
        for codec, level in runs:
            for mode in modes:
                steps.append(["encode", codec, level, mode])
                expect[f"{codec}/{level}/{mode}"] = k
    for fam in PINNED:
        assert limit != FAMILIES[fam](1) - 1 or piece_of(fam, limit) == 0
        assert limit != FAMILIES[fam](1) or piece_of(fam, limit) == 1
    if not steps:
        return
    got = _child({"FOURMC_WS_FAIL_ABOVE": str(limit)}, {"steps": steps})
    for key, k in expect.items():
        codec, level, mode = key.split("/")
        if k == 0:
            assert got[key]["rc"] == ENOMEM and got[key]["untouched"] and got[key]["err"], (key, got[key])
        elif codec == "par":
            _same_blocks(got[key], _par_unsplit(gpu)[mode], (key, f"pieces of {k}"))
        else:
            _same_blocks(got[key], want_encode(codec, int(level), mode), (key, f"pieces of {k}"))


def test_limits_cover_every_family():
    """every family runs in pieces of 1, 2 and 3 under LIMITS, and bytes(1) - 1 / bytes(1) of every pinned formula are among them"""
    for fam in FAMILIES:
        assert {piece_of(fam, lim) for lim in LIMITS} >= {1, 2, 3}, fam
    for fam in PINNED:
        assert FAMILIES[fam](1) - 1 in LIMITS and FAMILIES[fam](1) in LIMITS, fam


_PAR = {}


def _par_unsplit(gpu):
    """the ratio-tolerance encoder in one launch of this process (its bytes are not the reference's): raw and container rows,
    after checking that every raw payload decodes back to its block"""
    if not _PAR:
        blocks = enc_blocks()
        for mode in ("raw", "container"):
            _PAR[mode] = _encode(gpu, "par", 0, mode)
            assert _PAR[mode]["rc"] == 0 and _PAR[mode]["guard_broken"] == [], _PAR[mode]
        L = gpu.lib()
        caps = raw_caps("par", blocks)
        d = _Dev(gpu, blocks, caps)
        L.fourmc_gpu_set_lz4_encode_mode(1)
        try:
            assert L.fourmc_gpu_lz4_compress_fast(*d.args, d.stream) == 0
            d.torch.cuda.synchronize()
        finally:
            L.fourmc_gpu_set_lz4_encode_mode(0)
        res = [int(r) for r in d.batch.download()["result"]]
        out = d.d_dst.cpu().numpy()
        for i, (s, r, dd, c) in enumerate(zip(blocks, res, d.dsts, caps)):
            if r > 0:
                n, back = helpers.orc_decompress(out[dd:dd + r], len(s))
                assert n == len(s) and np.array_equal(back, s), i
            else:
                assert r == 0 and c < helpers.oracle().orc_lz4_compress_bound(len(s)), (i, r, c)
        _PAR["raw"] = _PAR["raw"]["blocks"]
        _PAR["container"] = _PAR["container"]["blocks"]
    return _PAR


_DEC_CONFIGS = [
    ("batch 64", {"FOURMC_TILE_BATCH": "64", "FOURMC_SEG_BATCH": "64"}, {"tile": 1, "seg": 1, "exact": 1, "auto": 1}),
    ("tile 64", {"FOURMC_WS_FAIL_ABOVE": str(64 * TILE_BLOCK)}, {"tile": 1, "auto": 1, "seg": 0}),
    ("tile 64 - 1", {"FOURMC_WS_FAIL_ABOVE": str(64 * TILE_BLOCK - 1)}, {"tile": 0, "auto": 1}),     # auto: the exact walker
    ("tile 128", {"FOURMC_WS_FAIL_ABOVE": str(128 * TILE_BLOCK)}, {"tile": 1, "auto": 1}),
    ("seg 64", {"FOURMC_WS_FAIL_ABOVE": str(64 * SEG_BLOCK)}, {"seg": 1}),
    ("seg 64 - 1", {"FOURMC_WS_FAIL_ABOVE": str(64 * SEG_BLOCK - 1)}, {"seg": 0}),
    ("seg 128", {"FOURMC_WS_FAIL_ABOVE": str(128 * SEG_BLOCK)}, {"seg": 1}),
]


@pytest.mark.parametrize("name,env,paths", _DEC_CONFIGS, ids=[c[0] for c in _DEC_CONFIGS])
def test_lz4_decode_in_pieces(gpu, name, env, paths):
    """200 raw streams and 200 container blocks per path, cut into pieces of 64 or 128 blocks by FOURMC_TILE_BATCH /
    FOURMC_SEG_BATCH or by the workspace limit: result codes and accepted bytes are the oracle's.  A path that cannot have 64
    blocks' workspace fails with FOURMC_ENOMEM when chosen explicitly (nothing written), auto ends at the exact walker."""
    steps = [["lz4", path, c] for path in paths for c in (0, 1)]
    got = _child(env, {"steps": steps})
    for path, ok in paths.items():
        for c in (0, 1):
            g = got[f"{path}/{c}"]
            if not ok:
                assert g["rc"] == ENOMEM and g["untouched"] and g["err"], (name, path, c, g)
                continue
            _same_blocks(g, want_container_decode() if c else want_lz4_decode(), (name, path, c))


def test_no_workspace_at_all(gpu, tmp_path):
    """FOURMC_WS_FAIL_ABOVE=1: an automatic LZ4 decode ends at the exact walker (include/fourmc_gpu.h) - raw, container,
    the image calls and the streaming reader answer as without the limit and as the oracle; an explicit tile / seg decode fails with
    FOURMC_ENOMEM and a message, writes nothing, and the engine serves the next call."""
    steps = [["lz4", "auto", 0], ["lz4", "auto", 1], ["images"], ["lz4", "tile", 0], ["lz4", "seg", 1], ["lz4", "exact", 0],
             ["lz4", "tile", 1], ["lz4", "exact", 1]]
    got = _child({"FOURMC_WS_FAIL_ABOVE": "1"}, {"steps": steps})
    free = _child({}, {"steps": [["lz4", "auto", 0], ["lz4", "auto", 1], ["images"]]})
    _same_blocks(got["auto/0"], want_lz4_decode(), "auto raw")
    _same_blocks(got["auto/1"], want_container_decode(), "auto container")
    assert got["auto/0"] == free["auto/0"] and got["auto/1"] == free["auto/1"]
    for key in ("tile/0", "seg/1", "tile/1"):
        g = got[key]
        assert g["rc"] == ENOMEM and g["untouched"] and g["err"], (key, g)
    _same_blocks(got["exact/0"], want_lz4_decode(), "exact after ENOMEM")
    _same_blocks(got["exact/1"], want_container_decode(), "exact after ENOMEM")
    # the image calls: the same answers as without the limit, and the oracle's bytes
    data, img, bad = image_case()
    assert got["good"] == free["good"] and got["bad"] == free["bad"]
    n, want, _ = helpers.orc_container_decode(img, len(data))
    assert n == len(data) and np.array_equal(want, data)
    st, dig, clean = got["good"]["decompress_image"]
    assert st["reason"] == 0 and dig == _dig(data) and clean, st
    assert got["good"]["ImageReader"][1] == _dig(data)
    assert got["good"]["image_decode_blocks"] == [len(data) - B, _dig(data[B:])]
    assert got["bad"]["decompress_image"][0]["reason"] != 0
    assert helpers.orc_container_decode(bad, len(data))[0] < 0
    # the CLI
    src = tmp_path / "in.4mc"; src.write_bytes(img.tobytes())
    back = tmp_path / "back"
    r = subprocess.run([gpu.cli_path(), "-d", "-f", str(src), str(back)], capture_output=True, timeout=300,
                       env=dict(os.environ, FOURMC_WS_FAIL_ABOVE="1"))
    assert r.returncode == 0, r.stderr
    assert back.read_bytes() == data.tobytes()


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_zstd_decode_in_pieces(gpu, k):
    """37 frames of levels 1 / 3 / 6 / 12 with damaged ones at piece boundaries, in pieces of k blocks through the split and the
    single-kernel decode, raw (fourmc_gpu_zstd_decompress) and as .4mz blocks (fourmc_gpu_4mc_decode_blocks, with stored blocks
    and wrong checksums).  Raw: a rejected frame is any negative result - the API promises the reference's verdict, not its
    ZSTD error code (include/fourmc_gpu.h:112-113) - and an accepted one has the oracle's size and bytes.  Container: the codes
    (FOURMC_BLK_BADSUM / _CORRUPT), sizes and bytes are the oracle's.  k = 0: one block's scratch minus one byte, FOURMC_ENOMEM."""
    limit = zstd_scratch(k) if k else zstd_scratch(1) - 1
    steps = [["zstd", split, c] for split in (1, 0) for c in (0, 1)]
    got = _child({"FOURMC_WS_FAIL_ABOVE": str(limit)}, {"steps": steps})
    want = want_zstd_decode()
    for split in (1, 0):
        for c in (0, 1):
            g = got[f"zstd/{split}/{c}"]
            if not k:
                assert g["rc"] == ENOMEM and g["untouched"] and g["err"], g
                continue
            if c:
                _same_blocks(g, want_zstd_container_decode(), ("4mz", split))
                continue
            assert g["rc"] == 0 and g["guard_broken"] == [], (split, g)
            for i, (gg, w) in enumerate(zip(g["blocks"], want)):
                assert (gg[0] < 0) == (w[0] < 0), (split, i, gg[0], w[0])
                if w[0] >= 0:
                    assert gg == w, (split, i)


_EMPTY = [("fast", 0), ("par", 0), ("mc", 0)] + [("hc", lv) for lv in range(14)] + [("zstd", lv) for lv in range(1, 13)]


@pytest.mark.parametrize("codec,level", _EMPTY, ids=[f"{c}{lv}" for c, lv in _EMPTY])
def test_empty_block_in_container_mode(gpu, codec, level):
    """An empty block between two others in a container encode, every encoder and level: the codec's capacity is n - 1
    (native/4mc.c:301), which for n = 0 must be 0, not -1 (HC 1..8 took -1 as no limit and MC as LZ4_compressMC: one token byte
    written into a slot of 0 bytes).  The block is stored: result 0, XXH32 of nothing, every slot's guard bytes untouched."""
    text = helpers.corpus(70000, first_block=3)
    blocks = [text[:30000], np.zeros(0, np.uint8), text[30000:]]
    d = _Dev(gpu, blocks, [len(s) for s in blocks])
    gpu.lib().fourmc_gpu_set_lz4_encode_mode(1 if codec == "par" else 0)
    try:
        rc = gpu.lib().fourmc_gpu_4mc_encode_blocks(*d.args, CODEC[codec], level, d.stream)
        rep = d.report(rc, container=True)
    finally:
        gpu.lib().fourmc_gpu_set_lz4_encode_mode(0)
    assert rep["rc"] == 0 and rep["guard_broken"] == [], rep
    assert rep["blocks"][1] == [0, _dig(np.zeros(0, np.uint8)), helpers.orc_xxh32(np.zeros(0, np.uint8))], rep["blocks"][1]
