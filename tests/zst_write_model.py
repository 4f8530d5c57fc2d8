""".zst files written on the device (fourmc_gpu_zsts_compress): the geometry of the reference's streaming compressor, the inputs of
the tests, and the committed fixture of what the reference writes for them.

  modes(n, level)   per 128 KiB block: is the reference in external-dictionary mode (ZSTD_matchState_dictMode) when it parses it
  inputs()          name -> (source, level): geometry (G), planted copies in random bytes (P), degenerate sources (Z)
  reached(name, image)  the property the input is there for, read from the reference's image alone
  chunked(src, level, pieces)  the reference fed in pieces (zst_model.zstcodec feeds the whole source at once)
  fixture() / fixture_build()  tests/golden/zst_write.json: SHA-256 and length of every reference image, whole images up to 4 KiB

Geometry (compress/clevels.h, row 0 of a level - the row for an unknown source size - and zstd_compress.c:1591-1594): the input ring
holds windowSize + blockSize bytes; blockSize is 128 KiB.
"""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np

import helpers
import zst_model as zm
import zstd_shapes as zs

B = 131072
WINDOW = {1: 1 << 19, 2: 1 << 20, 3: 1 << 21, 4: 1 << 21}       # clevels.h row 0: windowLog 19, 20, 21, 21 (fast, fast, dfast, dfast)
K = 16384                                                        # a planted copy
FIXTURE = os.path.join(zs.HERE, "golden", "zst_write.json")


def ring(level):
    return WINDOW[level] + B


def modes(n, level):
    """Per block of a source of n bytes: True when window.lowLimit < window.dictLimit as the block is parsed.  A direct restatement
    of the reference's bookkeeping, addresses and all: the ring is [0, R); ZSTD_window_update (zstd_compress_internal.h:1177-1212)
    with its overlap rule, ZSTD_window_enforceMaxDist (:1086-1122) at the block's start (zstd_compress.c:4015), and the ring's
    advance (zstd_compress.c:5517-5519)."""
    W, R = WINDOW[level], ring(level)
    far = -(1 << 60)
    base = dict_base = far
    low = dct = 2
    next_src = base + 2
    at, pos, out = 0, 0, []
    while pos < n:
        ln = min(B, n - pos)
        ip = at
        if ip != next_src:                                       # not contiguous: the prefix becomes the external dictionary
            dist = next_src - base
            low, dct, dict_base, base = dct, dist, base, ip - dist
            if dct - low < 8: low = dct
        next_src = ip + ln
        if ip + ln > dict_base + low and ip < dict_base + dct:   # the input overwrites the dictionary's low end
            high = ip + ln - dict_base
            low = dct if high > dct else high
        idx = ip - base
        if idx > W:
            low = max(low, idx - W)
            dct = max(dct, low)
        out.append(low < dct)
        at = ip + ln
        if at + B > R: at = 0
        pos += ln
    return out


def _random(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _copy(buf, dst, src, n):
    buf[dst:dst + n] = buf[src:src + n].copy()


def _differ(buf, a, b):
    """make buf[a] != buf[b] (the byte that ends a planted match)"""
    if buf[a] == buf[b]: buf[a] ^= 0x55


def _planted(level):
    """name -> (source, block that holds the plant's destination).  Sources and destinations start where the parsers still
    examine every position (a block's first bytes, or right behind a match), or the copy is long enough for their growing step."""
    W, R = WINDOW[level], ring(level)
    m = R // B
    n = 2 * R + 2 * B
    out = {}
    seed = 0x5A00 + level

    def fresh(k, length=n):
        return _random(length, seed * 64 + k)
    # (a) destination at the first byte after the wrap, source wholly in front of it
    s = fresh(0); _copy(s, R, 3 * B, K); _differ(s, R + K, 3 * B + K)
    out["a"] = (s, m)
    # (b) source begins 100 bytes in front of the wrap point and runs across it.  A helper copy fills block m - 1 up to that byte,
    # so that the search behind it examines - and enters into the table - every position from R - 100 on
    s = fresh(1); _copy(s, R - B, B, B - 100); _differ(s, R - 100, 2 * B - 100)
    _copy(s, R + B, R - 100, K); _differ(s, R + B + K, R - 100 + K)
    out["b"] = (s, m + 1)
    # (c) destination across the boundary of two ext-dict blocks
    s = fresh(2); _copy(s, R + 2 * B - K // 2, W + 16, K)
    out["c"] = (s, m + 2)
    # (d) the source starts W - 1, W, W + 1 bytes in front of the END of the destination's block: the reference's lowest valid
    # index is blockEndIdx - maxDistance (ZSTD_getLowestMatchIndex with the block's end)
    for name, d in (("d:W-1", W - 1), ("d:W", W), ("d:W+1", W + 1)):
        s = fresh(3); end = R + 3 * B
        _copy(s, end - B, end - d, K)
        out[name] = (s, m + 2)
    # (e) one copy with five other bytes in its middle: the second half is found with the repeat offset, in the external part
    s = fresh(4); _copy(s, R + B, 3 * B + 64, K)
    for i in range(5): s[R + B + K // 2 + i] ^= 0xA5
    out["e"] = (s, m + 1)
    # (f) a copy deep in its block with 64 more equal bytes in front (and 16 in front of those): the match is found inside and
    # caught up backwards; f:low: the source's start is the first valid byte of the external part, where the catch-up must stop
    for name, src in (("f", R + 2 * B - W + B), ("f:low", R + 2 * B - W)):
        s = fresh(5); dst = R + B + 8192
        _copy(s, dst - 80, src - 16, K + 80)
        if name == "f": _differ(s, dst - 81, src - 17)
        out[name] = (s, m + 1)
    # (g) a copy in the last, short block behind the second wrap
    s = fresh(6, 2 * R + B + 40000); _copy(s, 2 * R + B, 2 * R - B, K)
    out["g"] = (s, 2 * m + 1)
    # (h) a repeat offset between window - block and window, carried into the last block before the wrap: the reference keeps it
    # (ZSTD_getLowestPrefixIndex measures from window.dictLimit).  A helper copy fills block m - 2 up to p; the copy at p, from
    # byte 48, is that block's last sequence and leaves the offset d = p - 48; block m - 1 starts with a copy at the same distance,
    # whose source lies below the block's prefix start: only the repeat offset finds it
    s = fresh(7); p = W - K - 16; d = p - 48
    _copy(s, W - B, B, p - (W - B)); _differ(s, p, B + p - (W - B))
    _copy(s, p, 48, K); _differ(s, p + K, 48 + K)
    _copy(s, W, W - d, K)
    out["h"] = (s, m - 1)
    return out


G1 = (0, 1, B - 1, B, B + 1, 2 * B)
# name -> ext-dict blocks by modes(): level 1 has 5 blocks in its ring, level 2 9, levels 3 and 4 17
EXT_BLOCKS = {**{f"G:l1:{n}": 0 for n in G1}, "G:l1:R-1": 0, "G:l1:R": 0, "G:l1:R+1": 1, "G:l1:R+B": 1, "G:l1:2R+1": 5,
              "G:l3:R": 0, "G:l3:R+1": 1, "G:l3:2R+B+5": 18, "G:l2:R+B+1": 2, "G:l4:R+B+1": 2}
P_CASES = ("a", "b", "c", "d:W-1", "d:W", "d:W+1", "e", "f", "f:low", "g", "h")
REQUIRED = tuple(EXT_BLOCKS) + tuple(f"P:l{lv}:{c}" for lv in (1, 3) for c in P_CASES) + ("Z:rle", "Z:rle:l3", "Z:runs:l3", "Z:rawmid")


@functools.lru_cache(None)
def _everything():
    out, block_of = {}, {}
    r1, r3 = ring(1), ring(3)
    logs = helpers.corpus(2 * r3 + B + 5, logs=True)
    for n in G1: out[f"G:l1:{n}"] = (logs[:n], 1)
    for name, n in (("R-1", r1 - 1), ("R", r1), ("R+1", r1 + 1), ("R+B", r1 + B), ("2R+1", 2 * r1 + 1)): out[f"G:l1:{name}"] = (logs[:n], 1)
    for name, n in (("R", r3), ("R+1", r3 + 1), ("2R+B+5", 2 * r3 + B + 5)): out[f"G:l3:{name}"] = (logs[:n], 3)
    out["G:l2:R+B+1"] = (logs[:ring(2) + B + 1], 2)
    out["G:l4:R+B+1"] = (logs[:ring(4) + B + 1], 4)
    for lv in (1, 3):
        for c, (src, blk) in _planted(lv).items():
            out[f"P:l{lv}:{c}"] = (src, lv); block_of[f"P:l{lv}:{c}"] = blk
    out["Z:rle"] = (np.full(3000000, 0x5A, np.uint8), 1)
    out["Z:rle:l3"] = (np.full(2 * r3 + 70000, 0x5A, np.uint8), 3)
    runs = _random(2 * r3 + 70000, 0x5AFD)                           # runs of 300 equal bytes with 20 random ones between: long matches at offset 1, both hashes of neighbours equal
    for at in range(0, len(runs), 320): runs[at:at + 300] = runs[at]
    out["Z:runs:l3"] = (runs, 3)
    out["Z:rawmid"] = (np.concatenate([helpers.corpus(1 << 20, logs=True), _random(1 << 20, 0x5AFF)]), 1)
    return out, block_of


def inputs():
    """name -> (source as a uint8 array, level)"""
    return _everything()[0]


def background():
    """P's background alone: 2 B of random bytes (every block raw)"""
    return _random(2 * B, 0x5AFE)


def reached(name, image):
    """Does the reference's image show what the input is there for?  G: the blocks are cut as the geometry says and modes() counts
    the listed number of ext-dict blocks.  P: the block that holds the plant's destination is a compressed block.  (d:W+1 is no raw
    block, as one might expect of a source that starts below the window; the reference compresses it: only the copy's first byte lies below the lowest valid
    index, the match is found one byte later and covers the rest.)  Z: an RLE block beyond the wrap; raw blocks in mid-stream."""
    src, level = inputs()[name]
    tab = zm.block_table(image)
    n = len(src)
    data = tab[:-1] if n % B == 0 else tab                           # ZSTD_endStream's empty block
    if len(data) != -(-n // B) or not tab[-1]["type"] in (0, 1, 2): return False
    if n % B == 0 and (tab[-1]["type"], tab[-1]["size"]) != (0, 0): return False
    if name.startswith("G:"):
        return sum(modes(n, level)) == EXT_BLOCKS[name] and len(modes(n, level)) == len(data)
    if name.startswith("P:"):
        blk = _everything()[1][name]
        others_raw = sum(1 for e in data if e["type"] == 2) <= 2     # the background never compresses
        if name.endswith(":h"): return not modes(n, level)[blk] and data[blk]["type"] == 2 and data[blk - 1]["type"] == 2
        if name.endswith(":d:W+1"):                                  # the match starts one byte later than d:W's: one literal more
            if len(image) != len(reference()[name[:-2]]) + 1: return False
        if name.endswith(":d:W-1") and len(image) != len(reference()[name[:-2]]): return False
        return modes(n, level)[blk] and data[blk]["type"] == 2 and others_raw
    if name == "Z:runs:l3":
        return any(modes(n, level)) and all(e["type"] == 2 for e in data)
    if name.startswith("Z:rle"):
        return all(e["type"] == 1 for e in data[1:]) and any(modes(n, level))
    m = ring(level) // B
    return any(e["type"] == 0 for e in data[m:-1]) and any(e["type"] == 2 for e in data[:m])


def chunked(src, level, pieces):
    """ZSTD_initCStream(level); ZSTD_compressStream per piece (sizes cycle through `pieces`), draining the output; ZSTD_endStream."""
    src = zs._u8(src)
    out = np.zeros(2 * len(src) + 4096, np.uint8)
    ob = helpers.ZstdOutBuffer(out.ctypes.data, len(out), 0)
    with zs._Cctx({zs.P_LEVEL: level}) as cx:
        at, k = 0, 0
        while at < len(src):
            ln = min(pieces[k % len(pieces)], len(src) - at); k += 1
            ib = helpers.ZstdInBuffer(src.ctypes.data + at, ln, 0)
            while ib.pos < ln:
                r = cx.L.ZSTD_compressStream2(cx.c, C.byref(ob), C.byref(ib), 0)
                assert not cx.L.ZSTD_isError(r)
            at += ln
        ib = helpers.ZstdInBuffer(None, 0, 0)
        for _ in range(1 << 16):
            r = cx.L.ZSTD_compressStream2(cx.c, C.byref(ob), C.byref(ib), 2)
            assert not cx.L.ZSTD_isError(r)
            if r == 0: break
        else: raise AssertionError("stream did not drain")
    return out[:ob.pos].tobytes()


@functools.lru_cache(None)
def reference():
    """name -> the reference's image (needs oracle/_ref)"""
    return {name: zm.zstcodec(src, level) for name, (src, level) in inputs().items()}


def fixture_build():
    out = {}
    for name, img in reference().items():
        e = {"sha256": hashlib.sha256(img).hexdigest(), "bytes": len(img)}
        if len(inputs()[name][0]) <= 4096: e["hex"] = img.hex()
        out[name] = e
    return out


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump(fixture_build(), f, indent=1, sort_keys=True)
        f.write("\n")
