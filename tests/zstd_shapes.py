"""zstd frames of every shape the reference can write, for the decoder tests (plain module, like hc_opt_inputs.py).

  frames()        (name, frame bytes, expected output) triples written by the reference through helpers.ref(): ZSTD_compress at
                  the levels outside 1..12, ZSTD_compress2 with single parameters, ZSTD_compressStream2 cut by flushes,
                  ZSTD_compressSequences with chosen sequences, chosen inputs for the rare entropy shapes, and header surgery
                  (pure byte edits of valid frames).  Needs oracle/_ref.
  inspect()       a header-level parser (no entropy decoding): ledger keys, mutation sites and what the split path's decline
                  rules (zstd_decode.hip, zstd_decode_frame_v2 steps 0 and 1a) see.
  REQUIRED        the ledger keys the frame set must reach.  A missing key is a test failure.
  damaged()       structure-aware damage at the inspector's offsets.
  fixture_*()     tests/golden/zstd_shapes.json: one small frame per REQUIRED key, so that the core runs without oracle/_ref.

Limits of the split path (read from zstd_decode.hip):
  kMaxInner   64 and 65 inner blocks: streamed frames of 64 / 65 chunks, one flush each.
  kSeqArea    1024 * 1024 sequences of one payload: more than that fit 4 MiB only with 3-byte matches and no literals
              (4 MiB / 3 = 1398101), so the pair comes from ZSTD_compressSequences with minMatch 3.
  kV2Lit      NOT reachable by a valid frame of at most 4 MiB of output.  The rule declines when the sum over inner blocks of
              (regenerated literals of a Huffman-coded section, rounded up to 64) exceeds kV2Lit - 256 = 4 MiB + kMaxInner * 64.
              Literals are part of the output, so their sum is at most 4 MiB = 4194304; at most kMaxInner = 64 blocks reach the
              rule and each rounds up by at most 63, so the sum is at most 4194304 + 64 * 63 = 4198336 < 4198400 = kV2Lit - 256.
              Only a damaged literals header (a size the block does not have) gets there; damaged() produces such headers.
Content-size widths: the 2-byte field stores size - 256 and the 1-byte field sizes below 256, so no body takes both; the widths
are 1/4/8 on a 200-byte body and 2/4/8 on a 30000-byte body."""
import collections
import ctypes as C
import functools
import hashlib
import json
import os
import re
import struct

import numpy as np

import helpers
from helpers import B

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "zstd_shapes.json")
MAGIC = 0xFD2FB528


@functools.lru_cache(None)
def limits():
    """kMaxInner, kSeqArea and the literal limit kV2Lit - 256 as zstd_decode.hip states them."""
    txt = open(os.path.join(helpers.ROOT, "4mc_amd", "csrc", "zstd_decode.hip")).read()
    inner = int(re.search(r"kMaxInner\s*=\s*(\d+);", txt).group(1))
    m = re.search(r"kSeqArea\s*=\s*(\d+)\s*\*\s*(\d+);", txt)
    seq = int(m.group(1)) * int(m.group(2))
    assert re.search(r"kV2Lit\s*=\s*\(size_t\(4\) << 20\) \+ kMaxInner \* 64 \+ 256;", txt)
    return {"inner": inner, "seq": seq, "lit": (4 << 20) + inner * 64}


# ---------------------------------------------------------------------------------------------- inspector
LIT_TYPES = ("raw", "rle", "huf", "treeless")
MODES = ("predef", "rle", "fse", "repeat")
NEAR = 65536                     # "just under / over" a limit: within this many of it


def inspect(payload):
    """-> (ledger Counter, sites [(kind, offset, nbytes)], frames [dict]) of a VALID payload (frames and skippable frames)."""
    p = bytes(payload)
    led, sites, frames = collections.Counter(), [], []
    pos, n = 0, len(p)
    while n - pos >= 5:
        magic = struct.unpack_from("<I", p, pos)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            led["skippable"] += 1
            sites.append(("skip_size", pos + 4, 4))
            pos += 8 + struct.unpack_from("<I", p, pos + 4)[0]
            sites.append(("trunc", pos, 0))
            continue
        assert magic == MAGIC, hex(magic)
        fhd = p[pos + 4]
        fcs_id, single, has_sum, did = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
        did_sz, fcs_sz = (0, 1, 2, 4)[did], (single if fcs_id == 0 else 1 << fcs_id)
        led[f"hdr:single:{single}"] += 1; led[f"hdr:fcs:{fcs_id}"] += 1; led[f"hdr:did:{did_sz}"] += 1
        if has_sum: led["hdr:checksum"] += 1
        sites.append(("fhd", pos + 4, 1))
        hp = pos + 5
        if not single:
            led["hdr:window"] += 1; sites.append(("window", hp, 1)); hp += 1
        dict_id = int.from_bytes(p[hp:hp + did_sz], "little"); hp += did_sz
        if fcs_sz: sites.append(("fcs", hp, fcs_sz))
        hp += fcs_sz
        fr = {"start": pos, "nblk": 0, "nseq": 0, "lit_need": 0, "checksum": has_sum, "did": did, "dict_id": dict_id,
              "odd_block": False}
        pos = hp
        sites.append(("trunc", pos, 0))
        while True:
            bh = p[pos] | p[pos + 1] << 8 | p[pos + 2] << 16
            last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
            sites.append(("bh", pos, 3))
            pos += 3
            fr["nblk"] += 1
            led["block:" + ("raw", "rle", "compressed")[btype]] += 1
            if bsize == 0: led["block:zero_size"] += 1
            if btype == 2:
                if bsize < 2 or bsize >= (128 << 10): fr["odd_block"] = True
                _inspect_block(p, pos, bsize, led, sites, fr)
            pos += 1 if btype == 1 else bsize
            sites.append(("trunc", pos, 0))
            if last: break
        if has_sum: pos += 4
        frames.append(fr)
    if len(frames) > 1: led["multiframe"] += 1
    L = limits()
    for fr in frames:
        if fr["nblk"] > 32: led["inner>32"] += 1
        if fr["nblk"] > 64: led["inner>64"] += 1
    if len(frames) == 1 and not led["skippable"]:
        fr = frames[0]
        if fr["nblk"] == L["inner"]: led["limit:inner=max"] += 1
        if fr["nblk"] == L["inner"] + 1: led["limit:inner=max+1"] += 1
        if fr["nblk"] <= L["inner"]:
            if L["seq"] - NEAR < fr["nseq"] <= L["seq"]: led["limit:seq<=area"] += 1
            if L["seq"] < fr["nseq"] <= L["seq"] + NEAR: led["limit:seq>area"] += 1
    return led, sites, frames


def _inspect_block(p, pos, bsize, led, sites, fr):
    """One compressed block: literals section header, Huffman weight header, sequence count, symbol modes."""
    b0 = p[pos]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    if lt < 2:
        lh = (1, 2, 1, 3)[sf]
        lsize = (b0 >> 3) if lh == 1 else (b0 >> 4) + (p[pos + 1] << 4) + ((p[pos + 2] << 12) if lh == 3 else 0)
        lcsize = 1 if lt == 1 else lsize
        led[f"lit:{LIT_TYPES[lt]}:sz{lh}"] += 1
    else:
        lh = (3, 3, 4, 5)[sf]
        v = int.from_bytes(p[pos:pos + lh], "little") >> 4
        bits = (10, 10, 14, 18)[sf]
        lsize, lcsize = v & ((1 << bits) - 1), v >> bits
        led[f"lit:{LIT_TYPES[lt]}:sf{sf}"] += 1
        fr["lit_need"] += (lsize + 63) & ~63
        s = pos + lh
        if lt == 2:
            wh = p[s]
            led["weights:direct" if wh >= 128 else "weights:fse"] += 1
            sites.append(("whdr", s, 1))
            s += 1 + (wh if wh < 128 else (wh - 127 + 1) // 2)
        end = pos + lh + lcsize
        if sf:                                  # four streams behind a jump table of three sizes
            sites.append(("jump", s, 6))
            sz = struct.unpack_from("<HHH", p, s)
            s += 6
            for k in range(4):
                e = s + sz[k] if k < 3 else end
                if s < e <= end: sites.append(("stream_first", s, 1)); sites.append(("stream_last", e - 1, 1))
                s = e
        elif s < end:
            sites.append(("stream_first", s, 1)); sites.append(("stream_last", end - 1, 1))
    sites.append(("lithdr", pos, lh))
    s = pos + lh + lcsize
    sites.append(("trunc", s, 0))
    c0 = p[s]
    if c0 == 0: nseq, w = 0, 1
    elif c0 < 128: nseq, w = c0, 1
    elif c0 < 255: nseq, w = ((c0 - 128) << 8) + p[s + 1], 2
    else: nseq, w = p[s + 1] + (p[s + 2] << 8) + 0x7F00, 3
    led["nseq:0" if nseq == 0 else f"nseq:{w}B"] += 1
    sites.append(("nseq", s, w))
    fr["nseq"] += nseq
    if nseq:
        m = p[s + w]
        sites.append(("modes", s + w, 1))
        for name, sh in (("ll", 6), ("of", 4), ("ml", 2)):
            led[f"{name}:{MODES[(m >> sh) & 3]}"] += 1
        sites.append(("stream_first", s + w + 1, 1))          # a table description, an RLE symbol or the bitstream itself
        sites.append(("stream_last", pos + bsize - 1, 1))     # the sequence bitstream's end mark


REQUIRED = (["block:raw", "block:rle", "block:compressed", "block:zero_size"]
            + [f"lit:{t}:sz{w}" for t in ("raw", "rle") for w in (1, 2, 3)]
            + [f"lit:{t}:sf{f}" for t in ("huf", "treeless") for f in (0, 1, 2, 3)]
            + ["weights:direct", "weights:fse"]
            + [f"{s}:{m}" for s in ("ll", "of", "ml") for m in MODES]
            + ["nseq:0", "nseq:1B", "nseq:2B", "nseq:3B"]
            + ["hdr:single:0", "hdr:single:1", "hdr:window"] + [f"hdr:fcs:{i}" for i in range(4)]
            + [f"hdr:did:{w}" for w in (0, 1, 2, 4)] + ["hdr:checksum"]
            + ["skippable", "multiframe", "inner>32", "inner>64"]
            + ["limit:inner=max", "limit:inner=max+1", "limit:seq<=area", "limit:seq>area"])


def declines(payload, cap):
    """What zstd_decode_frame_v2 steps 0 and 1a do with a VALID payload: True when a decline rule names it (the serial one-wave
    path decodes it), False when the entropy stage and the execute kernel must complete it."""
    L = limits()
    if len(payload) < 9 or struct.unpack_from("<I", payload, 0)[0] != MAGIC: return True
    led, _, frames = inspect(payload)
    fr = frames[0]
    return bool(len(frames) > 1 or led["skippable"] or fr["checksum"] or fr["did"] or fr["nblk"] > L["inner"] or fr["odd_block"]
                or fr["nseq"] > L["seq"] or fr["lit_need"] > L["lit"] or cap > (4 << 20))


def rejected_by_design(payload):
    """The two documented deviations: a frame with a content checksum or a non-zero dictionary ID is
    rejected by the oracle and the device, whatever the reference makes of it."""
    _, _, frames = inspect(payload)
    return any(fr["checksum"] or fr["dict_id"] for fr in frames)


# ---------------------------------------------------------------------------------------------- reference drivers
P_LEVEL, P_WLOG, P_MINMATCH, P_STRATEGY, P_LDM, P_CSIZE, P_CHECKSUM = 100, 101, 105, 107, 160, 200, 201
P_LITMODE, P_TARGETCBLOCK, P_DELIMS, P_VALIDATE = 1002, 1003, 1008, 1009       # ZSTD_c_experimentalParam5/6/11/12
PS_ENABLE, PS_DISABLE = 1, 2


class _Cctx:
    def __init__(self, params):
        self.L = helpers.ref()
        self.c = self.L.ZSTD_createCCtx()
        for k, v in params.items():
            r = self.L.ZSTD_CCtx_setParameter(self.c, k, v)
            assert not self.L.ZSTD_isError(r), (k, v)

    def __enter__(self): return self

    def __exit__(self, *a): self.L.ZSTD_freeCCtx(self.c)


def _u8(x):
    return np.ascontiguousarray(np.frombuffer(bytes(x), np.uint8) if not isinstance(x, np.ndarray) else x, dtype=np.uint8)


def compress(src, level):
    src = _u8(src); L = helpers.ref()
    out = np.zeros(helpers.zstd_bound(len(src)) + 64, np.uint8)
    r = L.ZSTD_compress(out.ctypes.data, len(out), src.ctypes.data, len(src), level)
    assert not L.ZSTD_isError(r)
    return out[:r].tobytes()


def compress2(src, params):
    src = _u8(src)
    out = np.zeros(2 * len(src) + 4096, np.uint8)             # tiny target block sizes cost a header per block
    with _Cctx(params) as cx:
        r = cx.L.ZSTD_compress2(cx.c, out.ctypes.data, len(out), src.ctypes.data, len(src))
        assert not cx.L.ZSTD_isError(r)
    return out[:r].tobytes()


def stream(src, cuts, params, flush_before_end=False):
    """ZSTD_compressStream2: ZSTD_e_flush at every offset of `cuts` (a repeated offset flushes twice), then ZSTD_e_end."""
    src = _u8(src)
    out = np.zeros(2 * len(src) + 16 * len(cuts) + 4096, np.uint8)
    ob = helpers.ZstdOutBuffer(out.ctypes.data, len(out), 0)
    with _Cctx(params) as cx:
        def step(upto, directive):
            ib = helpers.ZstdInBuffer(src.ctypes.data, upto, step.pos)
            for _ in range(1 << 16):
                r = cx.L.ZSTD_compressStream2(cx.c, C.byref(ob), C.byref(ib), directive)
                assert not cx.L.ZSTD_isError(r)
                if r == 0 and ib.pos == upto: break
            else: raise AssertionError("stream did not drain")
            step.pos = upto
        step.pos = 0
        for c in cuts: step(c, 1)
        if flush_before_end: step(len(src), 1)
        step(len(src), 2)
    return out[:ob.pos].tobytes()


class SeqProg:
    """Builds an input and its explicit sequences together: lit() queues literal bytes, match() closes a sequence, block() a block."""
    def __init__(self):
        self.out, self.seqs, self.pend = bytearray(), [], 0

    def lit(self, data):
        self.out += bytes(data); self.pend += len(bytes(data)); return self

    def match(self, off, ml):
        assert 0 < off <= len(self.out) and ml >= 3
        self.seqs.append((off, self.pend, ml)); self.pend = 0
        while ml > 0:
            k = min(ml, off); self.out += self.out[len(self.out) - off: len(self.out) - off + k]; ml -= k
        return self

    def block(self):
        self.seqs.append((0, self.pend, 0)); self.pend = 0; return self


def _block_sums(seqs):
    ll = ml = 0
    for o, l, m in seqs:
        ll += l; ml += m
        if o == 0 and m == 0: yield 0, ll, ml; ll = ml = 0


def sequences(src, seqs, params=None):
    """ZSTD_compressSequences with explicit block delimiters and validation; seqs = (offset, litLength, matchLength) rows."""
    src = _u8(src)
    a = np.zeros((len(seqs), 4), np.uint32)                   # ZSTD_Sequence {offset, litLength, matchLength, rep}
    a[:, :3] = np.asarray(seqs, np.uint32).reshape(-1, 3)
    out = np.zeros(helpers.zstd_bound(len(src)) + 4096, np.uint8)
    with _Cctx({P_DELIMS: 1, P_VALIDATE: 1, P_MINMATCH: 3, **(params or {})}) as cx:
        r = cx.L.ZSTD_compressSequences(cx.c, out.ctypes.data, len(out), a.ctypes.data, len(a), src.ctypes.data, len(src))
        assert not cx.L.ZSTD_isError(r), -(r - (1 << 64))
    return out[:r].tobytes()


# ---------------------------------------------------------------------------------------------- header surgery
def split_header(frame):
    """-> (size of the frame header, content size or None) of a frame that starts with the zstd magic."""
    fhd = frame[4]
    fcs_id, single, did = fhd >> 6, (fhd >> 5) & 1, fhd & 3
    fcs_sz = single if fcs_id == 0 else 1 << fcs_id
    h = 5 + (0 if single else 1) + (0, 1, 2, 4)[did]
    fcs = int.from_bytes(frame[h:h + fcs_sz], "little") + (256 if fcs_id == 1 else 0) if fcs_sz else None
    return h + fcs_sz, fcs


def header(size, fcs_id, single, did_width=0, dict_id=0, checksum=0, window=None):
    """A frame header from its fields.  window: the descriptor byte (needed when single == 0)."""
    did = {0: 0, 1: 1, 2: 2, 4: 3}[did_width]
    h = struct.pack("<IB", MAGIC, fcs_id << 6 | single << 5 | checksum << 2 | did)
    if not single: h += bytes([window])
    h += dict_id.to_bytes(did_width, "little")
    if fcs_id == 0: h += bytes([size]) if single else b""
    else: h += (size - 256 if fcs_id == 1 else size).to_bytes(1 << fcs_id, "little")
    return h


def raw_literals_to_rle(frame):
    """Rewrites the first compressed block whose raw literals (1-byte header) are all one byte value into RLE literals."""
    f = bytearray(frame)
    pos = split_header(f)[0]
    while True:
        bh = f[pos] | f[pos + 1] << 8 | f[pos + 2] << 16
        btype, bsize = (bh >> 1) & 3, bh >> 3
        if btype == 2 and f[pos + 3] & 7 == 0:
            n = f[pos + 3] >> 3
            lits = f[pos + 4: pos + 4 + n]
            if n > 1 and len(set(lits)) == 1:
                f[pos:pos + 3] = ((bh & 7) | (bsize - (n - 1)) << 3).to_bytes(3, "little")
                f[pos + 3: pos + 4 + n] = bytes([n << 3 | 1, lits[0]])
                return bytes(f)
        assert not bh & 1, "no such block"
        pos += 3 + (1 if btype == 1 else bsize)


def skippable(nibble, payload):
    return struct.pack("<II", 0x184D2A50 + nibble, len(payload)) + bytes(payload)


def _window_byte(size):
    """The smallest window descriptor that covers `size` bytes."""
    for wb in range(256):
        wl = (wb >> 3) + 10
        if (1 << wl) + ((1 << wl) >> 3) * (wb & 7) >= size: return wb
    raise ValueError(size)


# ---------------------------------------------------------------------------------------------- the frame set
def _entropy_inputs():
    rng = np.random.default_rng(0x5A)
    return {"sym16_20k_x2": rng.integers(0, 16, 40000, dtype=np.uint8),     # no matches to speak of, Huffman-friendly literals
            "sym16_5k_x2": rng.integers(0, 16, 10000, dtype=np.uint8),
            "sym16_600_x2": rng.integers(0, 16, 1200, dtype=np.uint8),
            "sym16_200_x2": rng.integers(0, 16, 400, dtype=np.uint8)}


def _seq_frames():
    """ZSTD_compressSequences frames aimed at the executor's special cases (names say which)."""
    rng = np.random.default_rng(0x5E9)
    R = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    out = []

    def add(name, prog, params=None):
        if prog.pend or not prog.seqs or prog.seqs[-1][2]: prog.block()
        assert max(ll + ml for _, ll, ml in _block_sums(prog.seqs)) <= (128 << 10), name
        out.append((name, sequences(prog.out, prog.seqs, params), bytes(prog.out)))

    # repeat codes 1/2/3 with ll > 0 and ll == 0 ("rep 3 with ll = 0 is rep1 - 1"); the history is set by three real offsets first
    p = SeqProg().lit(R(400))
    p.match(100, 8); p.lit(R(3)).match(57, 9); p.lit(R(2)).match(211, 7)            # rep = 211, 57, 100
    p.lit(R(1)).match(211, 5)          # ll > 0, rep1
    p.lit(R(1)).match(57, 6)           # ll > 0, rep2 -> 57, 211, 100
    p.lit(R(1)).match(100, 6)          # ll > 0, rep3 -> 100, 57, 211
    p.match(57, 5)                     # ll = 0, code 1 = rep2 -> 57, 100, 211
    p.match(211, 5)                    # ll = 0, code 2 = rep3 -> 211, 57, 100
    p.match(210, 5)                    # ll = 0, code 3 = rep1 - 1 -> 210, 211, 57
    p.match(210, 4)                    # ll = 0 and rep1 again: a real offset, not a repeat code
    p.lit(R(2)).match(57, 4).match(209, 6).lit(R(5))
    add("seq_repcodes", p)
    # the same rules across a block boundary and after a raw block: the history lives per frame, not per block
    p = SeqProg().lit(R(300)).match(37, 6).lit(R(1)).match(91, 5).lit(R(2)).match(143, 5).block()
    p.lit(R(70)).block()
    p.match(142, 5).match(91, 4).lit(R(1)).match(142, 9).match(37, 3).lit(R(9))
    add("seq_repcodes_across_blocks", p)
    # offsets 1..8 with long matches (overlapping copies), one per offset, 2 KiB to 70 KiB
    p = SeqProg().lit(R(64))
    for off in range(1, 9): p.lit(R(off)).match(off, 2000 + off * 1500)
    p.block()
    for off in (8, 3, 1, 5): p.lit(R(off + 1)).match(off, 9000 + off)
    p.block().lit(R(7)).match(7, 100000).block().match(1, 131071)
    add("seq_offsets_1_to_8_long", p)
    # an offset equal to all the bytes produced so far, at the start of the frame, after a block, and at the window's far end
    p = SeqProg().lit(R(5)).match(5, 5).match(10, 30).lit(R(1)).match(41, 41).block()
    p.match(82, 82).lit(R(3)).match(167, 100)
    add("seq_offset_is_everything", p)
    p = SeqProg().lit(R(100000)).block().lit(R(100000)).block().lit(R(62144)).block().match(262144, 70000).match(332144, 3)
    add("seq_offset_is_everything_256k", p)
    # match lengths and literal lengths in the top codes (16 extra bits): ml >= 65539, ll >= 65536
    # (a block holds at most 128 KiB, so the two top codes cannot share one)
    p = SeqProg().lit(R(60000)).match(60000, 65539 + 5000).block().lit(R(65536 + 100)).match(3, 60000).block()
    p.lit(R(131071)).block().lit(R(1)).match(131072, 131071).block().lit(R(60000)).match(70000, 65539)
    add("seq_top_length_codes", p)
    # every sequence of a block has the same LL, OF and ML code: the RLE table mode for all three (and each alone)
    p = SeqProg().lit(R(4000))
    for _ in range(40): p.lit(R(4)).match(300, 7)
    p.block()
    for k in range(40): p.lit(R(4)).match(300 + 17 * k, 4 + k % 5)               # LL alone
    p.block()
    for k in range(40): p.lit(R(k % 6)).match(2100 + k, 5 + k % 9)               # OF alone (one code: 2048..4095)
    p.block()
    for k in range(40): p.lit(R(k % 7)).match(40 + 90 * k, 11)                   # ML alone
    add("seq_rle_modes", p)
    # literals that are one byte value: RLE literals with 1-, 2- and 3-byte headers, next to matches into random history
    p = SeqProg().lit(R(9000)).block()
    p.lit(b"a" * 20).match(400, 50).lit(b"a" * 5).match(33, 12).block()
    p.lit(b"\x00" * 2000).match(2500, 80).lit(b"\x00" * 1000).match(5000, 400).block()
    p.lit(b"z" * 3000).match(9000, 3000).lit(b"z" * 3000).match(2, 500)
    add("seq_rle_literals", p)
    # literals over very few low symbols: directly coded Huffman weights; a block with no sequence at all
    few = lambda n: rng.choice(np.array([0, 1, 2], np.uint8), n, p=[0.7, 0.2, 0.1]).tobytes()
    p = SeqProg().lit(few(300)).block().lit(few(900)).match(700, 40).lit(few(500)).block().lit(few(6000))
    add("seq_direct_weights", p, {P_LITMODE: PS_ENABLE})
    return out


def _seq_area_frame(total):
    """`total` sequences in at most 64 inner blocks: "ab" then 3-byte matches at offset 2 with no literals (minMatch 3)."""
    per = 40000
    nb = -(-total // per)
    counts = [per] * (total // per) + ([total % per] if total % per else [])
    assert len(counts) == nb <= limits()["inner"]
    seqs = np.zeros((total + nb, 3), np.uint32)
    at, first = 0, True
    for c in counts:
        seqs[at:at + c] = (2, 0, 3)
        if first: seqs[at, 1] = 2; first = False
        at += c + 1                                            # the delimiter row stays (0, 0, 0): no last literals
    src = np.tile(np.frombuffer(b"ab", np.uint8), (2 + 3 * total + 1) // 2)[: 2 + 3 * total]
    assert len(src) <= B
    return sequences(src, seqs), src.tobytes()


@functools.lru_cache(None)
def frames():
    """The whole set: [(name, frame bytes, expected bytes)].  Needs helpers.ref()."""
    assert helpers.ref() is not None
    L = limits()
    smix, logs = helpers.corpus(B), helpers.corpus(B, logs=True)
    ed = helpers.edge_inputs()
    rng = np.random.default_rng(0x2E5D)
    out = []
    add = lambda name, f, exp: out.append((name, bytes(f), bytes(_u8(exp).tobytes())))
    # 1. ZSTD_compress outside levels 1..12: one 4 MiB block per strategy (13 btlazy2, 16 btopt, 18 btultra, 19 btultra2: the
    #    block splitter cuts these), the rest at 600 KB, 40 KB and under 16 KiB
    for lvl, src in ((13, smix), (16, logs), (18, smix), (19, logs), (0, smix), (-1, logs), (-5, smix), (-50, logs)):
        add(f"L{lvl}_4m", compress(src, lvl), src)
    for lvl in (22, 19, 16, 13, 0, -1, -5, -50):
        add(f"L{lvl}_600k", compress(logs[:600000], lvl), logs[:600000])
        add(f"L{lvl}_40k", compress(smix[7000:47000], lvl), smix[7000:47000])
    for lvl in (22, 17, 14, 0, -3):
        add(f"L{lvl}_9k", compress(ed["text_60k"][:9000], lvl), ed["text_60k"][:9000])
    for name in ("empty", "one", "thirteen", "zeros_64k", "zeros_1m", "period3", "period37", "lit_then_run", "two_symbols", "far_repeat", "random_small"):
        add(f"L19_{name}", compress(ed[name], 19), ed[name]); add(f"L-5_{name}", compress(ed[name], -5), ed[name])
    # 2. ZSTD_compress2, one parameter each
    mid = logs[:600000]
    add("tcb_300_4m", compress2(smix[:2000000], {P_LEVEL: 3, P_TARGETCBLOCK: 1340}), smix[:2000000])
    add("tcb_2k_600k", compress2(mid, {P_LEVEL: 3, P_TARGETCBLOCK: 2000}), mid)
    add("nocsize_600k", compress2(mid, {P_LEVEL: 3, P_CSIZE: 0}), mid)
    add("nocsize_9k", compress2(mid[:9000], {P_LEVEL: 3, P_CSIZE: 0}), mid[:9000])
    add("wlog10_600k", compress2(mid, {P_LEVEL: 3, P_WLOG: 10}), mid)
    add("wlog10_L19_300k", compress2(smix[:300000], {P_LEVEL: 19, P_WLOG: 10}), smix[:300000])
    add("wlog27_4m", compress2(smix, {P_LEVEL: 3, P_WLOG: 27}), smix)
    add("ldm_4m", compress2(np.concatenate([smix[:1500000], logs[:1194304], smix[:1500000]]), {P_LEVEL: 3, P_LDM: 1}),
        np.concatenate([smix[:1500000], logs[:1194304], smix[:1500000]]))
    add("minmatch3_600k", compress2(mid, {P_LEVEL: 6, P_MINMATCH: 3}), mid)
    add("minmatch3_L19_40k", compress2(smix[:40000], {P_LEVEL: 19, P_MINMATCH: 3}), smix[:40000])
    add("lit_on_L-5_600k", compress2(mid, {P_LEVEL: -5, P_LITMODE: PS_ENABLE}), mid)
    add("lit_off_L6_600k", compress2(mid, {P_LEVEL: 6, P_LITMODE: PS_DISABLE}), mid)
    add("lit_on_random_small", compress2(ed["random_small"], {P_LEVEL: 3, P_LITMODE: PS_ENABLE}), ed["random_small"])
    add("checksum_40k", compress2(smix[:40000], {P_LEVEL: 3, P_CHECKSUM: 1}), smix[:40000])
    # 3. ZSTD_compressStream2 cut by flushes
    cuts = sorted(int(c) for c in rng.integers(1, 2000000, 90))
    add("stream_random_cuts_2m", stream(smix[:2000000], cuts, {P_LEVEL: 3}), smix[:2000000])
    add("stream_same_offset_600k", stream(mid, [1000, 1000, 1000, 250000, 250000, 599999], {P_LEVEL: 5}), mid)
    add("stream_flush_before_end_40k", stream(smix[:40000], [10000, 10000], {P_LEVEL: 1}, True), smix[:40000])
    add("stream_flush_before_end_L19_600k", stream(mid, [300000], {P_LEVEL: 19}, True), mid)
    t40 = ed["text_60k"][:40000]                               # small blocks that repeat their neighbour's FSE tables
    for lvl in (6, 19): add(f"stream_text_40k_16_cuts_L{lvl}", stream(t40, list(range(2500, 40000, 2500)), {P_LEVEL: lvl}), t40)
    for n in (L["inner"], L["inner"] + 1):                     # exactly kMaxInner and kMaxInner + 1 inner blocks
        src = ed["text_60k"][: 60 * n]
        add(f"stream_{n}_blocks", stream(src, [60 * k for k in range(1, n)], {P_LEVEL: 3}), src)
    src = smix[: 30000 * L["inner"]]
    add(f"stream_{L['inner']}_blocks_1m9", stream(src, [30000 * k for k in range(1, L["inner"])], {P_LEVEL: 3}), src)
    # treeless literals in every size format: two flushed halves with the same statistics, literal compression forced on
    for name, src in _entropy_inputs().items():
        add(f"stream_{name}", stream(src, [len(src) // 2], {P_LEVEL: 1, P_LITMODE: PS_ENABLE}), src)
    # 4. explicit sequences, and the sequence-area pair
    for name, f, exp in _seq_frames(): add(name, f, exp)
    for total in (L["seq"], L["seq"] + 1):
        f, exp = _seq_area_frame(total)
        add(f"seq_area_{total}", f, exp)
    # 5. header surgery on valid frames (pure byte edits)
    by = {n: (f, e) for n, f, e in out}
    small_src = ed["text_60k"][:200]; small = compress(small_src, 3)
    f30_src = ed["text_60k"][:30000]; f30 = compress(f30_src, 3)
    assert small[4] == 0x20 and f30[4] == 0x60
    sbody, fbody = small[split_header(small)[0]:], f30[split_header(f30)[0]:]
    for fid in (0, 2, 3): add(f"hdr_fcs{fid}_200", header(200, fid, 1) + sbody, small_src)
    for fid in (1, 2, 3): add(f"hdr_fcs{fid}_30k", header(30000, fid, 1) + fbody, f30_src)
    for fid in (0, 1, 3): add(f"hdr_window_fcs{fid}_30k", header(30000, fid, 0, window=_window_byte(30000)) + fbody, f30_src)
    add("hdr_window_max_30k", header(30000, 2, 0, window=(31 - 10) << 3 | 7) + fbody, f30_src)
    for w in (1, 2, 4):
        add(f"hdr_dictid0_w{w}_30k", header(30000, 1, 1, did_width=w) + fbody, f30_src)
        add(f"hdr_dictid0_w{w}_window_200", header(200, 0, 0, did_width=w, window=0) + sbody, small_src)
    add("hdr_dictid5_w1_30k", header(30000, 1, 1, did_width=1, dict_id=5) + fbody, f30_src)
    # RLE literals with the 1-byte header: the reference's encoder stores up to 63 literals raw unless a dictionary gave it a
    # Huffman table (zstd_compress_literals.c:123-125), so it never writes one.  The format allows it: a block whose raw literals
    # are 25 times one byte gets the RLE form by hand (two header bytes change and 24 literal bytes leave; nothing is re-coded)
    p = SeqProg().lit(rng.integers(0, 256, 300, dtype=np.uint8).tobytes()).block().lit(b"a" * 20).match(200, 50).lit(b"a" * 5).match(33, 12).block()
    add("hdr_rle_literals_1byte", raw_literals_to_rle(sequences(p.out, p.seqs)), p.out)
    sk = lambda k, n: skippable(k, rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    l19 = by["L19_40k"]; lm5 = by["L-5_40k"]; rep = by["seq_repcodes"]
    add("skip_before", sk(0, 77) + f30, f30_src)
    add("skip_after", f30 + sk(15, 0), f30_src)
    add("skip_between", small + sk(7, 1000) + f30, bytes(small_src) + bytes(f30_src))
    add("skip_everywhere", sk(1, 3) + l19[0] + sk(2, 0) + sk(3, 300) + rep[0] + sk(4, 9), l19[1] + rep[1])
    add("skip_only", sk(5, 40), b"")
    add("two_frames", l19[0] + lm5[0], l19[1] + lm5[1])
    add("three_frames", small + by["stream_flush_before_end_40k"][0] + rep[0], bytes(small_src) + by["stream_flush_before_end_40k"][1] + rep[1])
    add("two_frames_empty_first", by["L19_empty"][0] + f30, f30_src)
    return out


def ledger(triples):
    led = collections.Counter()
    for _, f, _ in triples: led.update(inspect(f)[0])
    return led


# ---------------------------------------------------------------------------------------------- structure-aware damage
KINDS = ("fhd", "window", "fcs", "bh", "lithdr", "jump", "whdr", "nseq", "modes", "stream_first", "stream_last", "trunc", "skip_size")


def damaged(name, frame, count, seed=0xDA):
    """`count` damaged copies of a valid frame: [(label, bytes)].  Walks the kinds of site the frame has round-robin; the site of a
    kind and the edit are drawn from a generator seeded by the frame's name."""
    rng = np.random.default_rng([seed, int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")])
    _, sites, _ = inspect(frame)
    by = collections.defaultdict(list)
    for k, o, n in sites:
        if k != "trunc" or 0 < o < len(frame): by[k].append((o, n))
    kinds = [k for k in KINDS if by[k]]
    out = []
    for t in range(count):
        k = kinds[t % len(kinds)]
        o, n = by[k][int(rng.integers(0, len(by[k])))]
        m = bytearray(frame)
        if k == "trunc":
            m = m[:o]; what = "cut"
        elif k == "bh":
            bh = m[o] | m[o + 1] << 8 | m[o + 2] << 16
            e = int(rng.integers(0, 6))
            if e < 3: bh = (bh & ~6) | ((((bh >> 1) & 3) + 1 + e) & 3) << 1; what = f"type+{1 + e}"
            elif e == 3: bh ^= 1; what = "last"
            else: bh = (bh + (8 if e == 4 else -8)) & 0xFFFFFF; what = "size" + "+-"[e - 4]
            m[o:o + 3] = bh.to_bytes(3, "little")
        else:
            j = o + int(rng.integers(0, n))
            if rng.integers(0, 2): m[j] ^= 1 << int(rng.integers(0, 8)); what = "bit"
            else: m[j] = int(rng.integers(0, 256)); what = "byte"
        if bytes(m) != bytes(frame): out.append((f"{name}/{k}@{o}/{what}", bytes(m)))
    return out


def damage_count(expected_len):
    """Damaged copies per frame class: 26 (two rounds of the 13 kinds of site) up to 600 KB of output, 8 above."""
    return 26 if expected_len <= 600000 else 8


def ref_decode(frame, cap):
    """ZSTD_decompress of the reference -> (result or -1, bytes)."""
    L = helpers.ref()
    src = np.frombuffer(bytes(frame), np.uint8); dst = np.zeros(cap + 64, np.uint8)
    r = L.ZSTD_decompress(dst.ctypes.data, cap, src.ctypes.data if len(src) else None, len(src))
    return (-1, b"") if L.ZSTD_isError(r) else (int(r), dst[:r].tobytes())


@functools.lru_cache(None)
def damaged_set():
    """The damaged copies of every frame class: [(label, bytes, capacity)].  The two classes that are rejected by design (content
    checksum, non-zero dictionary ID) are pinned as they are and give no copies."""
    out = []
    for name, f, e in frames():
        if rejected_by_design(f): continue
        out += [(label, m, len(e)) for label, m in damaged(name, f, damage_count(len(e)))]
    return out


# ---------------------------------------------------------------------------------------------- fixture
FIXTURE_FRAME_MAX = 40000        # bytes of one committed frame


def fixture_select(triples):
    """One small frame per REQUIRED key: for every key the smallest frame that has it (many keys share a frame)."""
    info = [(n, f, e, inspect(f)[0]) for n, f, e in triples if len(f) <= FIXTURE_FRAME_MAX]
    chosen = {}
    for key in REQUIRED:
        have = [t for t in info if t[3][key]]
        assert have, f"no frame of at most {FIXTURE_FRAME_MAX} bytes reaches {key}"
        n, f, e, _ = min(have, key=lambda t: (len(t[1]) + len(t[2]) // 64, t[0]))
        chosen[n] = (f, e)
    return {n: {"frame": f.hex(), "output_bytes": len(e), "output_sha256": hashlib.sha256(e).hexdigest()} for n, (f, e) in sorted(chosen.items())}


def fixture_frames():
    """[(name, frame bytes, output length, output sha256)] of the committed fixture."""
    z = json.load(open(FIXTURE))
    return [(n, bytes.fromhex(e["frame"]), e["output_bytes"], e["output_sha256"]) for n, e in z.items()]
