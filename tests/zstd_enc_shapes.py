"""Inputs that walk the search, parse and entropy shapes of the zstd frame encoder at levels 1..12 (4mc_amd/csrc/zstd_encode.hip),
for the encoder tests (plain module, like hc_shapes.py; numpy + the oracle port's trace + zstd_shapes.inspect()).

  cases()         the deterministic input set: named inputs built for a purpose, each with the levels it runs at (None: all twelve).
  trace()         what the oracle port did on one input (oracle.h: orc_zstd_compress_ex), as numpy tables.
  ledger()        the keys a case set reaches.  Two sources only: that trace, and zstd_shapes.inspect() on the port's own frame.
  REQUIRED        the keys the set must reach.  A missing key is a test failure.  UNREACHED: keys the reference cannot reach
                  (DESIGN_NOTES.md has the argument); a test asserts that no case reaches them.
  caps()          the capacities one input runs at: bound, n - 1, r, r - 1, r - 7, n / 3 (r = the port's frame size at that level).
  expected()      every (input, capacity) pair of one level with the port's result and frame: what the GPU test launches.

A key is `L<level>:<family>:<value>` where the level decides, `<strategy>:...` or `<entropy group>:...` where it does not: the
entropy stage branches on the strategy at one point only (below lazy / lazy and above: compress_literals' preference for the
previous Huffman table and select_type's rule set), so format keys carry `lt-lazy` or `ge-lazy`.

Far matches need their source in the hash table when the probe arrives.  The tables of the fast levels are small (2^14 entries at
level 1 above 256 KiB), so the window inputs are zeros with a few random markers: a zero run is one match and enters two positions."""
import collections
import functools
import os
import re

import numpy as np

import helpers
import zstd_shapes

LEVELS = tuple(range(1, 13))
BLOCK = 128 << 10
STRATS = {1: "fast", 2: "dfast", 3: "greedy", 4: "lazy", 5: "lazy2", 6: "btlazy2", 7: "btopt"}
# clevels.h:25-130, levels 1..12: (windowLog, chainLog, hashLog, searchLog, minMatch, targetLength, strategy) for inputs > 256 KiB,
# <= 256 KiB, <= 128 KiB, <= 16 KiB - the numbers zstd_encode.hip:54 and the port's level_params() carry as well
ROWS = (
    ((19, 13, 14, 1, 7, 0, 1), (18, 13, 14, 1, 6, 0, 1), (17, 12, 13, 1, 6, 0, 1), (14, 14, 15, 1, 5, 0, 1)),
    ((20, 15, 16, 1, 6, 0, 1), (18, 14, 14, 1, 5, 0, 2), (17, 13, 15, 1, 5, 0, 1), (14, 14, 15, 1, 4, 0, 1)),
    ((21, 16, 17, 1, 5, 0, 2), (18, 16, 16, 1, 4, 0, 2), (17, 15, 16, 2, 5, 0, 2), (14, 14, 15, 2, 4, 0, 2)),
    ((21, 18, 18, 1, 5, 0, 2), (18, 16, 17, 3, 5, 2, 3), (17, 17, 17, 2, 4, 0, 2), (14, 14, 14, 4, 4, 2, 3)),
    ((21, 18, 19, 3, 5, 2, 3), (18, 17, 18, 5, 5, 2, 3), (17, 16, 17, 3, 4, 2, 3), (14, 14, 14, 3, 4, 4, 4)),
    ((21, 18, 19, 3, 5, 4, 4), (18, 18, 19, 3, 5, 4, 4), (17, 16, 17, 3, 4, 4, 4), (14, 14, 14, 4, 4, 8, 5)),
    ((21, 19, 20, 4, 5, 8, 4), (18, 18, 19, 4, 4, 4, 4), (17, 16, 17, 3, 4, 8, 5), (14, 14, 14, 6, 4, 8, 5)),
    ((21, 19, 20, 4, 5, 16, 5), (18, 18, 19, 4, 4, 8, 5), (17, 16, 17, 4, 4, 8, 5), (14, 14, 14, 8, 4, 8, 5)),
    ((22, 20, 21, 4, 5, 16, 5), (18, 18, 19, 5, 4, 8, 5), (17, 16, 17, 5, 4, 8, 5), (14, 15, 14, 5, 4, 8, 6)),
    ((22, 21, 22, 5, 5, 16, 5), (18, 18, 19, 6, 4, 8, 5), (17, 16, 17, 6, 4, 8, 5), (14, 15, 14, 9, 4, 8, 6)),
    ((22, 21, 22, 6, 5, 16, 5), (18, 18, 19, 5, 4, 12, 6), (17, 17, 17, 5, 4, 8, 6), (14, 15, 14, 3, 4, 12, 7)),
    ((22, 22, 23, 6, 5, 32, 5), (18, 19, 19, 7, 4, 12, 6), (17, 18, 17, 7, 4, 12, 6), (14, 15, 14, 4, 3, 24, 7)))
CLASSES = (">256K", "<=256K", "<=128K", "<=16K")
WINDOW_LEVELS = (1, 2, 3, 6)              # their windows (512 KiB, 1 MiB, 2 MiB, 2 MiB) are smaller than an input this catalogue can hold

Case = collections.namedtuple("Case", "name data levels marks")
Trace = collections.namedtuple("Trace", "result out search block arm emit")

# oracle.h
ZSEARCH = {0: "hc", 1: "row", 2: "bt", 3: "opt"}
END = {1: "attempts", 2: "low-limit", 3: "chain-end", 4: "input-end"}
ARM = {32: "row-cache-at-block", 1: "hit-ip0", 2: "hit-ip1", 3: "rep-ip2", 4: "d-rep-ip1", 5: "d-long", 6: "d-short", 7: "d-short-then-long", 8: "step-up", 9: "catchup",
       10: "rep2-after", 11: "rep-zeroed", 12: "rep-restored", 13: "start-near-rep", 14: "end-behind-ilimit", 15: "out-of-window",
       20: "rep-ip1", 21: "search-wins", 22: "d1-rep", 23: "d1-search", 24: "d2-rep", 25: "d2-search", 26: "catchup", 27: "rep-loop",
       28: "step-grown", 29: "ntu-limit", 30: "bt-batch-full", 31: "row-wraps",
       40: "predef-prices", 41: "block-stats", 42: "immediate", 43: "array-full", 44: "ll0-shift", 45: "not-greedy"}
LIT = {0: "raw", 1: "rle", 2: "huf", 3: "treeless"}
HUF_DROPPED = {0: "kept", 1: "too-small", 2: "no-gain", 3: "one-symbol"}
SEL = {1: "one-symbol", 2: "repeat-small", 3: "predef-few", 4: "fse-default", 5: "cost-predef", 6: "cost-repeat", 7: "cost-fse"}
OUTCOME = {0: "compressed", 1: "raw-not-smaller", 2: "raw-too-small", 3: "rle", 4: "raw-short", 5: "refused"}
B_NUMBER, B_START, B_LEN, B_STRAT, B_NSEQ, B_NLIT, B_LIT, B_STREAMS, B_DROPPED, B_LL, B_OUT, B_REP_IN, B_REP_OUT, B_PARAMS = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 19, 22


@functools.lru_cache(None)
def held():
    """kFwHeld as zstd_encode.hip states it: the bytes behind pos + 4 that a dense-window lane holds of itself and its candidate"""
    txt = open(os.path.join(helpers.ROOT, "4mc_amd", "csrc", "zstd_encode.hip")).read()
    m = re.search(r"constexpr uint32_t kFwHeld = (\d+);", txt)
    assert m, "zstd_encode.hip no longer states `constexpr uint32_t kFwHeld = N;`: the held-length inputs are built from it"
    return int(m.group(1))


def params(level, n):
    """the row of the level table ZSTD_compress(level) runs an n-byte input with, after ZSTD_adjustCParams_internal's clamps"""
    cls = (n <= 256 * 1024) + (n <= 128 * 1024) + (n <= 16 * 1024)
    wlog, clog, hlog, slog, mml, tlen, strat = ROWS[level - 1][cls]
    src_log = 6 if n < 64 else (n - 1).bit_length()
    wlog = min(wlog, src_log)
    hlog = min(hlog, wlog + 1)
    if clog - (strat >= 6) > wlog: clog = wlog + (strat >= 6)
    return {"class": CLASSES[cls], "wlog": max(wlog, 10), "clog": clog, "hlog": hlog, "slog": slog, "mml": mml, "tlen": tlen, "strat": strat}


def group(strat):
    return "lt-lazy" if strat < 4 else "ge-lazy"


def trace(data, level, cap=None):
    r, out, tabs = helpers.orc_zstd_compress_ex(data, level, cap)
    return Trace(r, out, *tabs)


def port(data, level, cap):
    return helpers.orc_zstd_compress(data, level, cap)


def caps(data, level):
    n = len(data)
    r = port(data, level, helpers.zstd_bound(n))[0]
    out = []
    for c in (helpers.zstd_bound(n), n - 1, r, r - 1, r - 7, n // 3):
        c = max(c, 0)
        if c not in out: out.append(c)
    return out


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(list(name.encode()))


def _arr(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def _text(name, n):
    rng = _rng("text" + name)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9))).astype(np.uint8)) for _ in range(300)]
    out = b" ".join(words[int(i)] for i in rng.integers(0, 300, n // 3 + 8))
    assert len(out) >= n
    return _arr(out[:n])


def _skew(name, n, symbols):
    """`symbols` different bytes with geometric frequencies: Huffman literals; few matches where symbols is large"""
    rng = _rng("skew" + name)
    w = 0.93 ** np.arange(symbols) if symbols > 24 else 0.7 ** np.arange(symbols)
    return rng.choice(np.arange(symbols, dtype=np.uint8) + 33, n, p=w / w.sum()).astype(np.uint8)


RESET = bytes(12)         # a zero run: a match, behind which every finder searches with its smallest step again


def _head(rng, size):
    """random bytes in 64-byte pieces behind zero runs: the fast finders scan it with step 2 and enter every position"""
    out = bytearray()
    while len(out) < size:
        out += RESET + rng.integers(1, 256, 64, dtype=np.uint8).tobytes()
    return out


def _seqs(name, specs, head=4096, levels=None, recent=None):
    """a head of random bytes, then per (literal length, match length, distance) that many fresh random bytes and a copy from the
    head (distance None) or from `distance` back.  The byte behind a copy differs from the one behind its source.  What the
    encoder makes of it at each level is read off the trace: no key is taken from the specs."""
    rng = _rng(name)
    out = _head(rng, head)
    stop = None
    for ll, ml, dist in specs:
        lit = bytearray(rng.integers(1, 256, ll, dtype=np.uint8).tobytes())
        if lit and stop is not None and lit[0] == out[stop]: lit[0] = lit[0] % 255 + 1
        out += lit
        if dist is None:
            if ml <= 64: src = 76 * int(rng.integers(0 if recent is None else (head - recent) // 76, head // 76)) + len(RESET) + int(rng.integers(0, 64 - ml + 1))     # inside one random piece
            else: src = int(rng.integers(0, head - ml - 1))
        else:
            src = len(out) - dist
        assert 0 <= src < len(out)
        for i in range(ml): out.append(out[src + i])
        stop = src + ml
    tail = bytearray(rng.integers(1, 256, 13, dtype=np.uint8).tobytes())
    if stop is not None and tail[0] == out[stop]: tail[0] = tail[0] % 255 + 1
    return Case(name, _arr(out + tail), levels, {})


LL_TOPS = (15, 16, 17, 18, 19, 21, 23, 27, 31, 39, 47, 63, 127, 255, 511, 1023, 2047, 4095, 8191, 16383, 32767, 65535)      # the last value of every literal-length code from 15 on
ML_TOPS = (34, 35, 36, 38, 40, 42, 46, 50, 58, 66, 82, 98, 130, 258, 514, 1026, 2050, 4098, 8194, 16386, 32770, 65538)      # ... and of every match-length code from 31 on


def _ml_for(ll):
    return max(12, ll // 16 + 12)          # long enough for a finder whose step has grown over `ll` literals to land in it


def _ll_small():
    return _seqs("ll_sweep", [(ll, 12, None) for ll in list(range(0, 132)) + [255, 256, 511, 512, 1023]] + [(ll, 13, None) for ll in range(131, -1, -1)], head=2048)


def _ll_big():
    """literal runs up to 65535 and one above 65535; each lies inside one 128 KiB inner block"""
    specs = [(65536 + 100, _ml_for(65636), None), (16383, _ml_for(16383), None), (2047, 140, None)]
    specs += [(BLOCK, 0, None)]                                      # (filled in below: the rest of block 0)
    specs += [(65535, _ml_for(65535), None), (32767, _ml_for(32767), None), (8191, _ml_for(8191), None), (4095, 268, None)] + [(ll, 76, None) for ll in LL_TOPS[:-6]]
    rng = _rng("ll_big")
    out = _head(rng, 8192)
    stop = None
    for ll, ml, _ in specs:
        if ml == 0:
            ll = BLOCK + 8 - len(out)                                 # the next run starts in block 1
            assert ll > 0
        lit = bytearray(rng.integers(1, 256, ll, dtype=np.uint8).tobytes())
        if stop is not None and lit[0] == out[stop]: lit[0] = lit[0] % 255 + 1
        out += lit
        if ml == 0: continue
        src = int(rng.integers(0, 8192 - ml - 1))
        out += out[src:src + ml]
        stop = src + ml
    out += rng.integers(1, 256, 13, dtype=np.uint8).tobytes()
    return Case("ll_big", _arr(out), None, {})


def _ml_codes():
    return _seqs("ml_sweep", [(3, ml, None) for ml in list(range(3, 60)) + [m + d for m in ML_TOPS[:14] for d in (0, 1)]], head=4096)


def _ml_big():
    """match lengths up to 65538 and one above; one of them runs over the end of inner block 0 and goes on as a repeat offset"""
    return _seqs("ml_big", [(5, ml, None) for ml in (65539 + 40, 32770, 16386, 8194, 4098, 2050, 1026, 514, 65538)], head=70000)


def _offsets(name, top):
    """distances 1, 2, 3 and every power of two up to 2^top, each from a marker the input holds once; zeros fill the long gaps, so
    that the small tables of the fast levels still hold the marker when the probe arrives"""
    rng = _rng(name)
    out = bytearray()
    marks = {}
    for d in (1, 2, 3, 4, 8, 16, 32):
        out += RESET + rng.integers(1, 256, 3, dtype=np.uint8).tobytes()
        unit = rng.integers(1, 256, d, dtype=np.uint8).tobytes()
        out += (unit * 40)[:d + 24]
    for k in range(6, 12):                                            # marker, filler and probe in a row
        out += RESET; at = len(out); out += rng.integers(1, 256, 32, dtype=np.uint8).tobytes()
        out += rng.integers(1, 256, (1 << k) - 32 - len(RESET) - 1, dtype=np.uint8).tobytes() + RESET + b"\xEE"
        assert len(out) == at + (1 << k)
        out += out[at:at + 32]
    for k in range(12, top + 1):
        out += RESET; marks[k] = len(out); out += rng.integers(1, 256, 32, dtype=np.uint8).tobytes()
    for k in range(12, top + 1):
        at = marks[k] + (1 << k)
        pad = at - len(out) - len(RESET) - 1
        assert pad >= 0, (k, pad)
        out += rng.integers(1, 256, 40, dtype=np.uint8).tobytes() + bytes(pad - 40) + RESET + b"\xEE"
        assert len(out) == at
        out += out[marks[k]:marks[k] + 32]
    out += rng.integers(1, 256, 13, dtype=np.uint8).tobytes()
    return Case(name, _arr(out), None, {})


def _window(level):
    """zeros of windowSize + 128 KiB with random markers (see the module's text): sources either side of the last inner block's
    window edge and of each probe's own reach, and a far match at the end of the block before the last, whose offset the last
    block puts aside"""
    wlog = ROWS[level - 1][0][0]
    w = 1 << wlog
    n = w + BLOCK
    rng = _rng(f"window{level}")
    d = np.zeros(n, np.uint8)
    marks = {"w": w}
    M = [rng.integers(1, 256, 48, dtype=np.uint8) for _ in range(8)]

    def put(at, m): d[at:at + len(m)] = m
    # the last block is [w, w + BLOCK): the fast finders' window starts at its end - w = BLOCK for all of it
    put(BLOCK - 300, M[0]); put(w + 1000, M[0]); marks["below-edge"] = (w + 1000, w + 1000 - (BLOCK - 300))
    put(BLOCK, M[1]); put(w + 2000, M[1]); marks["edge+0"] = (w + 2000, w + 2000 - BLOCK)
    d[w + 3000 - 1] = 0x77; put(w + 3000, M[1][1:]); marks["edge+1"] = (w + 3000, w + 3000 - (BLOCK + 1))
    put(BLOCK + 600, M[2]); put(w + 4000, M[2]); marks["inside"] = (w + 4000, w + 4000 - (BLOCK + 600))
    # the lazy finders' window follows the position: sources w - 1, w and w + 1 before their probes
    for k, dist in enumerate((w - 1, w, w + 1)):
        put(1000 * (k + 7), M[3 + k]); put(1000 * (k + 7) + dist, M[3 + k]); marks[f"w{dist - w:+d}"] = (1000 * (k + 7) + dist, dist)
    # a far match as the last sequence but one of the block before the last: the zeros behind it are a repeat-offset-2 match
    put(5000, M[6]); put(w - 5000, M[6]); marks["far-before-last-block"] = (w - 5000, w - 10000)
    return Case(f"window_L{level}", d, (level,), marks)


def _blocks32():
    """4 MiB: 32 inner blocks, text whose words repeat within and across blocks"""
    t = _text("blocks32", 1 << 20)
    return Case("blocks32", np.concatenate([t, t[::-1], t[3:], t[:3], t[::-1]])[:4 << 20].copy(), (1, 3), {})


def _tops(name, head, more_ll):
    """the literal-length and match-length class tops that fit, the lengths either side of what a dense-window lane holds, and the
    32-byte steps of the lazy finders' length count; `head` sets the size class"""
    fw = held() + 4
    specs = [(ll, 24, None) for ll in LL_TOPS[:14]] + [(4, ml, None) for ml in ML_TOPS[:14] + (fw - 1, fw, fw + 1, 31, 32, 33, 64, 65)]
    specs += [(ll, _ml_for(ll) + 500, None) for ll in more_ll]
    return _seqs(name, specs, head=head)


def _same_of_code():
    """fifteen matches at fifteen distances of one offset code (256 .. 511), no repeat offset among them"""
    rng = _rng("same_of_code")
    out = bytearray(rng.integers(1, 256, 600, dtype=np.uint8).tobytes())
    for i in range(15):
        out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes()
        src = len(out) - (400 + 7 * i)
        out += out[src:src + 16]
    out += rng.integers(1, 256, 13, dtype=np.uint8).tobytes()
    return Case("same_of_code", _arr(out), None, {})


def _mix(n):
    """low-entropy input for the parsers' arbitration: fragments of a short base, cut and joined at random, a few fresh bytes between"""
    rng = _rng(f"mix{n}")
    base = rng.integers(0, 256, 4000, dtype=np.uint8)
    parts, total = [], 0
    while total < n:
        a = int(rng.integers(0, len(base) - 130))
        parts.append(base[a:a + int(rng.integers(3, 120))]); total += len(parts[-1])
        if rng.integers(0, 3) == 0:
            parts.append(rng.integers(0, 256, int(rng.integers(1, 6)), dtype=np.uint8)); total += len(parts[-1])
    return np.concatenate(parts)[:n].copy()


def _lit_rle_zeros():
    """block 0: zeros with 120 random markers of 20 bytes, which every finder enters whole; block 1: the markers, one 0xEE between
    two, ending on a marker: its literals are 0xEE alone.  (lit_rle's random block 0 leaves the fast finders' tables nearly empty.)"""
    rng = _rng("lit_rle_zeros")
    d = np.zeros(BLOCK, np.uint8)
    M = rng.integers(1, 238, (120, 20), dtype=np.uint8)
    for i in range(120): d[1000 * i + 40:1000 * i + 60] = M[i]
    tail = b"".join(M[i].tobytes() + b"\xEE" for i in range(119)) + M[119].tobytes()
    return Case("lit_rle_zeros", np.concatenate([d, _arr(tail)]), None, {})


def _same_ll(ll, count):
    """`count` sequences of `ll` fresh bytes and a 20-byte copy out of the first `ll`: one literal-length code, one match length"""
    rng = _rng(f"same_ll{ll}")
    out = bytearray(rng.integers(1, 256, ll, dtype=np.uint8).tobytes())
    first = bytes(out)
    for i in range(count):
        if i: out += rng.integers(1, 256, ll, dtype=np.uint8).tobytes()
        a = int(rng.integers(1, ll - 21))
        while out[-1] == first[a - 1]: a += 1                        # no catch-up into the literals
        out += first[a:a + 20]
    out += rng.integers(1, 256, 9, dtype=np.uint8).tobytes()
    return Case(f"same_ll{ll}", _arr(out), None, {})


def _rep_chain(name="rep_chain", head=1520):
    """matches without literals that take two distances in turn: behind the first two every one is a repeat-offset-2 match, so the
    loop behind a match goes round several times"""
    rng = _rng(name)
    out = _head(rng, head)
    for turn in range(6):
        out += rng.integers(1, 256, 5, dtype=np.uint8).tobytes()
        for k in range(8):
            src = len(out) - (300 if k % 2 == 0 else 517)
            out += out[src:src + 9]
    out += rng.integers(1, 256, 13, dtype=np.uint8).tobytes()
    return Case(name, _arr(out), None, {})


def _near_slots():
    """a 12-byte word three times within 64 bytes, eight such groups: the second occurrence matches at what the first wrote into the
    hash table a few positions before, the third at what the second wrote (the dense window's 'second' and 'dirty' lanes)"""
    rng = _rng("near_slots")
    out = bytearray()
    for g in range(8):
        w = rng.integers(1, 256, 12, dtype=np.uint8).tobytes()
        out += RESET + rng.integers(1, 256, 3 + g, dtype=np.uint8).tobytes()
        out += w + rng.integers(1, 256, 7, dtype=np.uint8).tobytes() + w + rng.integers(1, 256, 5 + g % 3, dtype=np.uint8).tobytes() + w
        out += rng.integers(1, 256, 30, dtype=np.uint8).tobytes()
    return Case("near_slots", _arr(out), None, {})


def _nseq(count):
    """`count` sequences: three fresh bytes and an 8-byte copy out of the first 600 bytes, each from a place of its own"""
    rng = _rng(f"nseq{count}")
    out = bytearray(rng.integers(1, 256, 600, dtype=np.uint8).tobytes())
    for i in range(count):
        out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes() + out[4 * i + 1:4 * i + 9]
    out += rng.integers(1, 256, 9, dtype=np.uint8).tobytes()
    return Case(f"nseq{count}", _arr(out), None, {})


def _tlen_opt():
    """twelve groups: 26 bytes T whose first 14 stand at one earlier place and whose last 24 at another.  Level 11's optimal parser
    (targetLength 12) takes the 14-byte match at T's start at once; level 12's (targetLength 24) prices it against two literals
    and the 24-byte match"""
    rng = _rng("tlen_opt")
    out = bytearray(rng.integers(1, 256, 100, dtype=np.uint8).tobytes())
    T = [rng.integers(1, 256, 26, dtype=np.uint8).tobytes() for _ in range(12)]
    for t in T:
        out += t[:14] + bytes([t[14] ^ 0x55]) + rng.integers(1, 256, 9, dtype=np.uint8).tobytes() + bytes([t[1] ^ 0x55]) + t[2:] + rng.integers(1, 256, 7, dtype=np.uint8).tobytes()
    for t in T:
        out += rng.integers(1, 256, 6, dtype=np.uint8).tobytes() + t
    out += rng.integers(1, 256, 13, dtype=np.uint8).tobytes()
    return Case("tlen_opt", _arr(out), None, {})


def _bt_batch():
    """one word 530 times, three fresh bytes between two; all of it once more, which is one long match; then the word again: the
    tree finder takes the positions the match covered in unsorted, 530 of them with the probe's hash - more than level 10's 512"""
    rng = _rng("bt_batch")
    W = bytes([0x61, 0x17, 0xC3, 0x5E])
    reg = b"".join(W + rng.integers(1, 256, 3, dtype=np.uint8).tobytes() for _ in range(530))
    out = rng.integers(1, 256, 200, dtype=np.uint8).tobytes() + reg + b"\x01\x02\x03" + reg + b"\x09\x08" + W + rng.integers(1, 256, 13, dtype=np.uint8).tobytes()
    return Case("bt_batch", _arr(out), None, {})


def _records():
    """fixed-size records over two inner blocks: block 1's sequence statistics are block 0's, so its tables can repeat"""
    rng = _rng("records")
    rec = np.zeros((20000, 16), np.uint8)
    rec[:, :6] = np.frombuffer(b"key=00", np.uint8)
    rec[:, 6:10] = rng.integers(48, 58, (20000, 4))
    rec[:, 10:] = np.frombuffer(b";v=ab\n", np.uint8)
    rec[:, 13] = rng.integers(97, 101, 20000)
    return rec.reshape(-1)[:2 * BLOCK + 4000].copy()


def _lit_rle():
    """block 0 random (a raw block); block 1 copies 20-byte pieces of it, one 0xEE between two: its literals are 0xEE alone"""
    rng = _rng("lit_rle")
    out = bytearray(rng.integers(1, 238, BLOCK, dtype=np.uint8).tobytes())
    for i in range(120):
        out += out[1000 * i + 40:1000 * i + 60] + b"\xEE"
    return Case("lit_rle", _arr(out), None, {})


@functools.lru_cache(None)
def _colliders4(hlog, count):
    """`count` + 1 four-byte words of one hash of `hlog` bits (zhash, mls 4), no byte twice in a word"""
    v = np.arange(1 << (24 if count > 400 else 23), dtype=np.uint32) + np.uint32(0x61000000)
    b = np.sort(v.view(np.uint8).reshape(-1, 4), axis=1)
    v = v[(b[:, 1:] != b[:, :-1]).all(axis=1)]
    h = ((v.astype(np.uint64) * 2654435761) & 0xFFFFFFFF) >> (32 - hlog)
    vals, cnt = np.unique(h, return_counts=True)
    w = v[h == vals[np.argmax(cnt)]]
    assert len(w) > count, (hlog, len(w))
    return [int(x).to_bytes(4, "little") for x in w[:count + 1]]


def _behind(k):
    """hash-chain finder (window log 14 and below: 8 KiB < n <= 16 KiB, hash log 14, minMatch 4): the source W, k words of W's hash,
    then the probe W.  2^searchLog attempts reach the source iff 2^searchLog > k.  The match is W's four bytes and no more: a longer
    one would be found again by the search one position on, whose chain holds no colliding word, and the frame would not tell."""
    rng = _rng(f"behind{k}")
    words = _colliders4(14, k)
    tail = b""
    out = _head(rng, 9000)                                          # (zero runs all along: the parsers' step stays 1)
    out += words[0] + tail + b"\x01"
    for c in words[1:]:
        out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes() + c
    out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes() + RESET + b"\xEE"           # (a match: the parsers search every position behind it)
    source = 9044                                                   # (the head is whole pieces of 76 bytes)
    assert bytes(out[source:source + 4]) == words[0]
    probe = len(out)
    out += words[0] + tail + b"\x02" + rng.integers(1, 256, 13, dtype=np.uint8).tobytes()
    assert 8192 < len(out) <= 16384
    return Case(f"behind{k}", _arr(out), None, {"probe": probe, "k": k, "source": source})


@functools.lru_cache(None)
def _colliders_row():
    """66 four-byte words of one 21-bit hash (zhash, mls 4): one row and one tag for the row finder's tables of the rows for
    16 KiB < n <= 128 KiB at levels 5..10 (hashLog 17, 16 / 32 / 64 entries: 21, 20 and 19 bits, each the top of the one before)"""
    out = []
    for base in range(0x61000000, 0x61000000 + (1 << 29), 1 << 24):
        v = np.arange(base, base + (1 << 24), dtype=np.uint32)
        h = ((v.astype(np.uint64) * 2654435761) & 0xFFFFFFFF) >> 11
        for x in v[h == 0x12345].tolist():
            b = x.to_bytes(4, "little")
            if len(set(b)) == 4 and 0 not in b: out.append(b)
        if len(out) >= 66: return out[:66]
    raise AssertionError("too few colliding words")


def _row_behind(k):
    """as _behind, for the row finder: 16 KiB < n <= 128 KiB, the words share row and tag (here the hash has 20, 19 and 18 bits: the
    input's size clamps hashLog to 16).  A row holds its last 16 / 32 / 64 positions whatever their tags, so the first seed is taken
    at which no other position from the source on falls into the words' row."""
    words = _colliders_row()
    for seed in range(40):
        c = _row_behind_seeded(k, seed, words)
        d = c.data.astype(np.uint64)
        w = d[:-3] | d[1:-2] << 8 | d[2:-1] << 16 | d[3:] << 24
        row = ((w * 2654435761) & 0xFFFFFFFF) >> 22                  # the 10 bits all three row widths share
        at = np.flatnonzero(row[c.marks["source"]:c.marks["probe"] + 1] == 0x12345 >> 11) + c.marks["source"]
        if len(at) == k + 2: return c
    raise AssertionError("no clean seed")


def _row_behind_seeded(k, seed, words):
    rng = _rng(f"row_behind{k}_{seed}")
    out = _head(rng, 17024)
    source = len(out)
    out += words[0] + b"\x01"
    for c in words[1:k + 1]:
        out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes() + c
    out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes() + RESET + b"\xEE"
    probe = len(out)
    out += words[0] + b"\x02" + rng.integers(1, 256, 29, dtype=np.uint8).tobytes()
    return Case(f"row_behind{k}", _arr(out), None, {"probe": probe, "k": k, "source": source})


@functools.lru_cache(None)
def _colliders5():
    """66 five-byte words of one 22-bit hash (zhash, mls 5): one row and one tag for the row finder's rows above 128 KiB that
    these inputs serve (level 4 at 128 KiB < n <= 256 KiB: hashLog 17, 16 entries, 21 bits; levels 11 and 12 above 256 KiB with
    n < 512 KiB: hashLog 20, 64 entries, 22 bits)"""
    out = []
    for hi in range(0x6A71, 0x6A71 + 200):
        if hi & 0xFF in (0, hi >> 8): continue
        v = np.arange(1 << 24, dtype=np.uint64) + np.uint64(hi << 24)
        h = ((v << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(42)
        for x in v[h == 0x12345].tolist():
            b = x.to_bytes(5, "little")
            if len(set(b)) == 5 and 0 not in b: out.append(b)
        if len(out) >= 66: return out[:66]
    raise AssertionError("too few colliding words")


def _row5_behind(k, head, levels, rowbits):
    """as _row_behind, with five-byte words for the rows whose minMatch is 5; `head` sets the size class and `rowbits` is
    hashLog - rowLog of the rows that `levels` run it with"""
    words = _colliders5()
    for seed in range(40):
        rng = _rng(f"row5_behind{k}_{head}_{seed}")
        out = _head(rng, head)
        source = len(out)
        out += words[0] + b"\x01"
        for c in words[1:k + 1]:
            out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes() + c
        out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes() + RESET + b"\xEE"
        probe = len(out)
        out += words[0] + b"\x02" + rng.integers(1, 256, 29, dtype=np.uint8).tobytes()
        d = _arr(out)
        w = d[source:probe + 8].astype(np.uint64)
        v = w[:-4] | w[1:-3] << np.uint64(8) | w[2:-2] << np.uint64(16) | w[3:-1] << np.uint64(24) | w[4:] << np.uint64(32)
        row = ((v << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(64 - rowbits)
        if int((row[:probe - source + 1] == 0x12345 >> (22 - rowbits)).sum()) == k + 2:
            return Case(f"row5_behind{k}", d, levels, {"probe": probe, "k": k, "source": source, "wlen": 5})
    raise AssertionError("no clean seed")


def _bt_behind(k, hlog, head):
    """the binary trees of btlazy2: the source W, then k words of W's hash, each above W and above the word before it, then the
    probe W.  Every word stands behind a zero run and is searched itself, so it goes into the tree sorted: the newest is the
    root, the one before it the root of its smaller side, and so on down to W.  The probe's walk compares the k words and then
    the source, which 2^searchLog compares reach iff 2^searchLog > k."""
    rng = _rng(f"bt_behind{k}_{hlog}")
    words = sorted(_colliders4(hlog, k))
    out = _head(rng, head)
    source = len(out)
    out += words[0] + b"\x01"
    for c in words[1:k + 1]:
        out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes() + RESET + b"\xEE" + c
    out += rng.integers(1, 256, 3, dtype=np.uint8).tobytes() + RESET + b"\xEE"
    probe = len(out)
    out += words[0] + b"\x02" + rng.integers(1, 256, 13, dtype=np.uint8).tobytes()
    return Case(f"bt_behind{k}_h{hlog}", _arr(out), None, {"probe": probe, "k": k, "source": source})


def _nseq_words(count):
    """191 four-byte words with 191 first bytes: all of them once (the literals), then `count` words in an order in which no
    word follows the same word twice (0, s, 2s, ... mod 191 for s = 2, 3, ...).  A finder with minMatch 4 that searches at a
    word's start finds the word and not a byte more, so each is a sequence of its own with no literals: 0x7F00 and more in one
    128 KiB block, where the sequence count takes three bytes."""
    rng = _rng("nseq_words")
    A = 191
    W = rng.integers(1, 256, (A, 4), dtype=np.uint8)
    W[:, 0] = np.arange(1, A + 1)
    order = [(j * s) % A for s in range(2, A) for j in range(A)][:count]
    assert len(order) == count
    out = np.concatenate([W.reshape(-1), W[order].reshape(-1), rng.integers(1, 256, 24, dtype=np.uint8)])
    assert 16384 < len(out) <= BLOCK
    return Case(f"nseq_words{count}", out, None, {})


ROW_BEHIND = (7, 8, 15, 16, 31, 32, 63, 64)
BT_BEHIND = ((31, 14, 8300), (32, 14, 8300), (511, 14, 300), (512, 14, 300), (31, 16, 17024), (32, 16, 17024), (127, 16, 17024), (128, 16, 17024))     # (k, hashLog, head): levels 9 and 10 at 16 KiB and less, 11 and 12 above
ROW5_BEHIND = ((7, 131100, (4,), 13), (8, 131100, (4,), 13), (63, 262200, (11, 12), 14), (64, 262200, (11, 12), 14))
BEHIND = (1, 2, 7, 8, 15, 16, 63, 64, 255, 256)          # 2^searchLog - 1 and 2^searchLog of the hash-chain rows: searchLog 1, 3, 4, 6, 8 (levels 4..8)
SIZES = (0, 1, 2, 6, 7, 8, 9, 17, 18, 19, 63, 64, 65, 255, 256, 1024, 1025, 16384, 16385, 65791, 65792, 131072, 131073, 262144, 262145)


@functools.lru_cache(None)
def cases():
    out = []
    t = _text("sizes", 262145)
    for n in SIZES:
        out.append(Case(f"text{n}", t[:n].copy(), None, {}))
    rng = _rng("cases")
    r = rng.integers(0, 256, 6000, dtype=np.uint8)
    out += [Case("random2000", r[:2000].copy(), None, {}),                                          # a raw block
            Case("zeros1000", np.zeros(1000, np.uint8), None, {}),                                  # a first block of one byte: not an RLE block
            Case("zeros_2blocks", np.zeros(BLOCK + 5000, np.uint8), None, {}),                      # ... and the RLE block behind it
            Case("zeros_then_random", np.concatenate([np.zeros(BLOCK, np.uint8), r[:3000]]), None, {}),    # at capacity r the random block is raw because nothing else fits
            Case("zeros_then_text", np.concatenate([np.zeros(BLOCK, np.uint8), t[:3000]]), None, {}),
            Case("lits20", np.concatenate([r[:20], r[:20]]), None, {}),                             # raw literals, size formats 1, 2, 3
            Case("lits1000", np.concatenate([r[:1000], r[:1000]]), None, {}),
            Case("lits5000", np.concatenate([r[:5000], r[:5000]]), None, {}),
            _lit_rle()]
    for n, sym in ((150, 12), (600, 12), (5000, 12), (40000, 12), (200, 120), (3000, 120), (30000, 200)):
        out.append(Case(f"skew{sym}_{n}", _skew(f"{sym}_{n}", n, sym), None, {}))
    sk = _skew("2b", BLOCK + 30000, 200)
    out += [Case("skew_block_plus200", np.concatenate([sk[:BLOCK], sk[BLOCK + 1000:BLOCK + 1200]]), None, {}),     # few literals under block 0's table: one stream / four
            Case("skew_block_plus700", np.concatenate([sk[:BLOCK], sk[BLOCK + 1000:BLOCK + 1700]]), None, {}),
            Case("lowsym300", _skew("low", 300, 6) - 33, None, {}),                                  # byte values 0..5: the weights go out direct
            _seqs("same_ll_ml", [(1, 20, None)] * 60, head=1024),                                   # one literal-length code, one match-length code: rle tables
            _seqs("same_of", [(2 + i % 3, 16 + i % 5, 300 + i) for i in range(60)], head=1024),    # one offset code
            Case("records", _records(), None, {})]
    out.append(Case("skew_2blocks", _skew("2b", BLOCK + 30000, 200), None, {}))                    # block 1 under block 0's statistics: treeless, repeat tables
    out.append(Case("text_2blocks_small_tail", np.concatenate([t[:BLOCK], t[5000:5900]]), None, {}))
    out += [_ll_small(), _ll_big(), _ml_codes(), _ml_big(), _offsets("offsets", 17), _offsets("offsets_small", 12), _tops("tops_small", 2048, ()), _tops("tops_mid", 20000, (8191, 2047, 1023, 700, 900, 1500, 600, 1100)), _tops("tops_140k", 110000, (8191,)),
            _tops("tops_295k", 262200, (8191, 2047, 1023, 700, 900, 600)),
            _same_of_code(), _lit_rle_zeros(), _same_ll(100, 40), _rep_chain(), _rep_chain("rep_chain_mid", 20000), _near_slots(), _bt_batch(),
            Case("four_symbols14000", (_rng("four_symbols").integers(0, 4, 14000, dtype=np.uint8) + 97).astype(np.uint8), None, {}),      # matches everywhere, few beyond targetLength: the optimal parser's series run to the end of its price array
            _seqs("ll_sweep_150k", [(ll, 15 + p, None) for p in (0, 1, 2, 3) for ll in range(131, 40, -1)], head=100000, recent=6000), _tlen_opt(),
            _seqs("ll_sweep_small", [(ll, 12, None) for ll in range(0, 132)], head=1024),
            _seqs("ll_sweep_140k", [(ll, 12 + p, None) for p in (0, 1, 2) for ll in range(0, 132)], head=110000, recent=6000),       # (sources the small tables of level 2's dfast row still hold)
            _seqs("ll_sweep_mid2", [(ll, 14 + p, None) for p in (0, 1) for ll in range(131, -1, -1)], head=30000), _seqs("ll_long_mid", [(ll, 40, None) for ll in range(300, 2400, 37)], head=20000)]     # matches found with a grown step, 16 KiB < n <= 128 KiB
    out += [Case(f"mix{n}", _mix(n), None, {}) for n in (12000, 40000, 200000, 300000)]
    out += [_behind(k) for k in BEHIND]
    out += [_nseq(k) for k in range(124, 130)]
    out += [_row_behind(k) for k in ROW_BEHIND]
    out += [_row5_behind(*a) for a in ROW5_BEHIND] + [_bt_behind(*a) for a in BT_BEHIND]
    out += [_nseq_words(0x7EFF), _nseq_words(0x7F00), _nseq_words(0x7F00 + 40)]
    m3 = _rng("match3")
    w3 = [m3.integers(1, 256, 3, dtype=np.uint8).tobytes() for _ in range(8)]
    out.append(Case("match3", _arr(b"".join(w3[int(m3.integers(0, 8))] + m3.integers(1, 256, 5, dtype=np.uint8).tobytes() for _ in range(400))), None, {}))   # 3-byte repeats 8 .. 100 bytes back
    out += [_window(lv) for lv in WINDOW_LEVELS]
    out.append(_blocks32())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def runs_at(c, level):
    return c.levels is None or level in c.levels


# ---- ledger -----------------------------------------------------------------------------------------------------------------------
def _ll_code(v):
    return v if v < 16 else 16 + ((v - 16) >> 1) if v < 24 else (18 + (v >> 2) - 4) if v < 32 else 22 + ((v - 32) >> 3) if v < 48 else 24 if v < 64 else v.bit_length() + 18


def _ml_code(ml):
    v = ml - 3
    if v > 127: return v.bit_length() + 35
    if v < 32: return v
    if v < 40: return 32 + ((v - 32) >> 1)
    if v < 48: return 36 + ((v - 40) >> 2)
    if v < 64: return 38 + ((v - 48) >> 3)
    if v < 96: return 40 + ((v - 64) >> 4)
    return 42


def keys_of(c, level, t=None):
    """the keys one case reaches at one level"""
    t = t or trace(c.data, level)
    d, n = c.data, len(c.data)
    keys = set()
    if t.result < 0: return {f"L{level}:refused:{t.result}"}
    Bk, E, A, S = t.block, t.emit, t.arm, t.search
    strat = int(Bk[0, B_STRAT]) if len(Bk) else params(level, n)["strat"]
    sname, grp = STRATS[strat], group(strat)
    # -- the frame, header level
    led, _, frames = zstd_shapes.inspect(t.out)
    for k in led: keys.add(f"{grp}:fmt:{k}")
    nblk = frames[0]["nblk"]
    if nblk in (1, 2, 32): keys.add(f"L{level}:inner={nblk}")
    p = params(level, n)                                            # (ROWS is held to the row the port ran on every trace)
    if len(Bk): assert tuple(Bk[0, B_PARAMS:B_PARAMS + 6]) == (p["wlog"], p["clog"], p["hlog"], p["slog"], p["mml"], p["tlen"]) and strat == p["strat"], (level, n)
    if n in SIZES or n == 0:
        keys.add(f"L{level}:n={n}:{p['class']}:{STRATS[p['strat']]}")
    # -- blocks
    for row in Bk.tolist():
        b, start, ln = row[B_NUMBER], row[B_START], row[B_LEN]
        out = OUTCOME[row[B_OUT]]
        keys.add(f"{grp}:block:{out}")
        one_byte = ln > 0 and bool((d[start:start + ln] == d[start]).all())
        if out == "rle" and b > 0: keys.add(f"{grp}:block:rle-not-first")
        if one_byte and b == 0 and ln >= 7 and out == "compressed": keys.add(f"{grp}:block:first-of-one-byte-stays-compressed")
        if row[B_LIT] >= 0:
            keys.add(f"{grp}:lit:{LIT[row[B_LIT]]}:streams={row[B_STREAMS]}")
            if row[B_DROPPED]: keys.add(f"{grp}:lit:huffman-dropped:{HUF_DROPPED[row[B_DROPPED]]}")
        for nm, k in (("ll", B_LL), ("of", B_LL + 2), ("ml", B_LL + 4)):
            if row[k] >= 0: keys.add(f"{grp}:{nm}:{zstd_shapes.MODES[row[k]]}:{SEL[row[k + 1]]}")
        if row[B_NSEQ] in (0, 1, 127, 128, 0x7EFF, 0x7F00): keys.add(f"{grp}:nseq={row[B_NSEQ]}")
        if row[B_NSEQ] >= 0x7F00: keys.add(f"{grp}:nseq>=0x7F00")
    # -- sequences
    seq = E[E[:, 4] > 0]
    for at, ll, ofb, ml in seq[:, 1:].tolist():
        lc, mc = _ll_code(ll), _ml_code(ml)
        if lc >= 15: keys.add(f"{sname}:ll-code={lc}")
        if ll in LL_TOPS: keys.add(f"{sname}:ll={ll}")
        if ll >= 65536: keys.add(f"{sname}:ll>=65536")
        if mc >= 31: keys.add(f"{sname}:ml-code={mc}")
        if ml in ML_TOPS or ml == 3: keys.add(f"{sname}:ml={ml}")
        if ofb > 3:
            keys.add(f"{sname}:of-code={(ofb).bit_length() - 1}")
            if ofb - 3 in (1, 2, 3) or (ofb - 3) & (ofb - 4) == 0: keys.add(f"{sname}:dist={ofb - 3}")
        else:
            keys.add(f"{sname}:off_base={ofb}:{'ll0' if ll == 0 else 'll>0'}")
        if (at + ll + ml) % BLOCK == 0 and at + ll + ml < n: keys.add(f"{sname}:match-to-block-end")
    if strat <= 2:
        # matches at what the same 64 positions wrote: a distance below 64 found through the table, and two such in a row within 64 bytes
        near = [(at + ll, ofb - 3) for at, ll, ofb, ml in seq[:, 1:].tolist() if 3 < ofb < 64 + 3 and ofb - 3 >= 12]
        if near: keys.add(f"L{level}:{sname}:slot-written-in-window:second")
        if any(b[0] - a[0] < 64 and b[0] - a[0] == b[1] for a, b in zip(near, near[1:])): keys.add(f"L{level}:{sname}:slot-written-in-window:dirty")
    for b in np.unique(E[:, 0]):
        rows = E[(E[:, 0] == b) & (E[:, 4] > 0)]
        if b > 0 and len(rows) and rows[0, 3] <= 3:
            keys.add(f"{sname}:rep-carried-into-block")
            prev = E[(E[:, 0] == b - 1)]
            if len(prev) and prev[-1, 2] == 0: keys.add(f"{sname}:match-to-block-end-goes-on-as-rep")
    # -- arms
    for arm, ip, v in A.tolist():
        nm = ARM[arm]
        keys.add(f"L{level}:{sname}:arm:{nm}")
        if nm == "catchup": keys.add(f"L{level}:{sname}:catchup={min(v, 5)}{'+' if v >= 5 else ''}")
        if nm in ("rep2-after", "rep-loop"): keys.add(f"L{level}:{sname}:{nm}:{'once' if v == 1 else 'again'}")
        if nm == "row-cache-at-block": keys.add(f"L{level}:{sname}:row-cache:" + ("starts-in-previous-block" if v > 100000 else "starts-in-this-block"))
        if nm in ("rep-zeroed", "rep-restored"): keys.add(f"L{level}:{sname}:{nm}={v}")
        if nm == "step-up": keys.add(f"L{level}:{sname}:step-up")
        if nm in ("hit-ip0", "hit-ip1", "rep-ip2", "d-long", "d-short", "d-short-then-long", "d-rep-ip1") and v > 2: keys.add(f"L{level}:{sname}:{nm}:step>2")
    if strat <= 2:
        # where in its search a match was found: the hit position less the literals' start (ll + the catch-up)
        starts = {int(at + ll): int(ll) for at, ll in seq[:, 1:3].tolist()}
        cu = A[A[:, 0] == 9]
        for ip, v in cu[:, 1:].tolist():
            if ip in starts:
                off = starts[ip] + v
                keys.add(f"L{level}:{sname}:found-at-search-offset={off if off <= 124 else '>124'}")
                keys.add(f"L{level}:{sname}:found-at-{'even' if ip + v & 1 == 0 else 'odd'}-position")
        fw = held() + 4
        for ml in np.unique(seq[:, 4]):
            if int(ml) in (fw - 1, fw, fw + 1): keys.add(f"L{level}:{sname}:ml=held{int(ml) - fw:+d}")
        ends = seq[:, 1] + seq[:, 2] + seq[:, 4]
        for b, start, ln in Bk[:, :3].tolist():
            il = start + ln - 8
            e = ends[(seq[:, 0] == b)]
            if ((e <= il) & (e > il - 200)).any(): keys.add(f"L{level}:{sname}:match-ends-within-200-of-ilimit")
    # -- searches
    if strat >= 3 and len(S):
        for kind, ip, walked, why, win, ln in S.tolist():
            kn = ZSEARCH[kind]
            if kind == 3:
                keys.add(f"L{level}:opt:matches={min(walked, 3)}{'+' if walked >= 3 else ''}")
                if why: keys.add(f"L{level}:opt:sufficient")
                if win: keys.add(f"L{level}:opt:hash3-match")
                if ln >= 4096: keys.add(f"L{level}:opt:match>=4096")
                continue
            keys.add(f"L{level}:{kn}:end:{END[why]}")
            if win >= 0 and ln in (31, 32, 33, 64, 65): keys.add(f"L{level}:{kn}:len={ln}")
            if win >= 0 and ln > 1 and int(Bk[0, B_PARAMS + 5]) > 1: keys.add(f"L{level}:{sname}:target-length>1")
            if ip == c.marks.get("probe"):
                if win == c.marks["k"] and ln == c.marks.get("wlen", 4): keys.add(f"L{level}:{kn}:found:behind={win}")
                if (win < 0 or ln < 4) and why == 1 and c.marks["k"] >= walked: keys.add(f"L{level}:{kn}:missed:behind={walked}")
            if kind == 1: keys.add(f"L{level}:row:entries={1 << min(max(int(Bk[0, B_PARAMS + 3]), 4), 6)}")
        big = np.flatnonzero(seq[:, 4] >= 384 + 192)
        if len(big) and (S[:, 1] > seq[big[0], 1] + seq[big[0], 2] + seq[big[0], 4]).any(): keys.add(f"L{level}:{sname}:ml>=576-then-search")
    # -- the window's edges
    for nm, val in c.marks.items():
        if not isinstance(val, tuple): continue
        at, dist = val
        found = ((seq[:, 1] + seq[:, 2] >= at - 1) & (seq[:, 1] + seq[:, 2] < at + 40) & (seq[:, 3] == dist + 3)).any()
        refused = ((A[:, 0] == 15) & (A[:, 1] >= at - 1) & (A[:, 1] < at + 40) & (A[:, 2] == dist)).any()
        if found: keys.add(f"L{level}:window:{nm}:found")
        if refused: keys.add(f"L{level}:window:{nm}:refused")
    return keys


def cap_keys(c, level):
    """what the capacities of one case do: refusals and the raw-because-too-small rule"""
    keys = set()
    for cap in caps(c.data, level):
        t = trace(c.data, level, cap)
        strat = params(level, len(c.data))["strat"]
        if t.result == -70: keys.add(f"{group(strat)}:cap:refused")
        if len(t.block) and (t.block[:, B_OUT] == 2).any() and t.result > 0: keys.add(f"{group(strat)}:block:raw-too-small")
    return keys


def ledger(case_list, levels=LEVELS, capacities=True):
    """key -> names of the cases that reach it"""
    led = collections.defaultdict(list)
    for c in case_list:
        for lv in levels:
            if not runs_at(c, lv): continue
            keys = keys_of(c, lv)
            if capacities and (len(c.data) <= 20000 or c.name.startswith("zeros_then")): keys |= cap_keys(c, lv)      # (group-level keys: the small inputs and the two-block ones reach them)
            for k in keys: led[k].append(c.name)
    return dict(led)


@functools.lru_cache(None)
def expected(level):
    """[(label, data, cap, result, frame)] of one level"""
    out = []
    for c in cases():
        if not runs_at(c, level): continue
        for cap in caps(c.data, level):
            r, f = port(c.data, level, cap)
            out.append((f"{c.name}|cap={cap}", c.data, cap, int(r), f))
    return tuple(out)


# ---- what the set must reach --------------------------------------------------------------------------------------------------------
def strategies_of(level):
    return sorted({r[6] for r in ROWS[level - 1]})


def _required():
    req = set()
    for g in ("lt-lazy", "ge-lazy"):
        req |= {f"{g}:fmt:block:{b}" for b in ("raw", "rle", "compressed")} | {f"{g}:block:rle-not-first", f"{g}:block:first-of-one-byte-stays-compressed",
                f"{g}:block:raw-not-smaller", f"{g}:block:raw-short", f"{g}:block:raw-too-small", f"{g}:cap:refused"}
        req |= {f"{g}:fmt:lit:raw:sz{w}" for w in (1, 2, 3)} | {f"{g}:fmt:lit:huf:sf{f}" for f in (0, 1, 2, 3)} | {f"{g}:fmt:lit:treeless:sf{f}" for f in (0, 1, 2)}
        req |= {f"{g}:fmt:weights:direct", f"{g}:fmt:weights:fse", f"{g}:lit:huffman-dropped:too-small", f"{g}:lit:huffman-dropped:no-gain"}
        req |= {f"{g}:fmt:nseq:0", f"{g}:fmt:nseq:1B", f"{g}:fmt:nseq:2B", f"{g}:nseq=0", f"{g}:nseq=1"}
        req |= {f"{g}:fmt:{t}:{m}" for t in ("ll", "of", "ml") for m in ("predef", "fse")} | {f"{g}:fmt:of:rle", f"{g}:fmt:ml:rle"}
        req |= {f"{g}:fmt:hdr:fcs:{i}" for i in (0, 1, 2)} | {f"{g}:fmt:hdr:single:0", f"{g}:fmt:hdr:single:1", f"{g}:fmt:hdr:window"}
    req |= {f"{g}:fmt:lit:rle:sz2" for g in ("lt-lazy", "ge-lazy")} | {f"{g}:fmt:ll:rle" for g in ("lt-lazy", "ge-lazy")} | {f"{g}:nseq={k}" for g in ("lt-lazy", "ge-lazy") for k in (127, 128)}
    req |= {"lt-lazy:fmt:lit:treeless:sf3"} | {f"ge-lazy:fmt:{t}:repeat" for t in ("ll", "of", "ml")}
    req |= {f"lt-lazy:{t}:{m}" for t in ("ll", "of", "ml") for m in ("predef:one-symbol", "predef:predef-few", "fse:fse-default")}
    req |= {f"ge-lazy:{t}:{m}" for t in ("ll", "of", "ml") for m in ("predef:one-symbol", "predef:cost-predef", "fse:cost-fse", "repeat:cost-repeat")}
    for st in STRATS.values():
        small = st == "btopt"                                   # 16 KiB and less: no literal run, match or distance beyond that
        req |= {f"{st}:ll-code={c}" for c in range(15, 29 if small else 34)} | {f"{st}:ll={v}" for v in (LL_TOPS[:14] if small else LL_TOPS[:-2])}
        req |= {f"{st}:ml-code={c}" for c in range(31, 46 if small else 53) if not (st == "btlazy2" and c in (49, 50, 51))}
        req |= {f"{st}:ml={v}" for v in ML_TOPS[:14]}
        req |= {f"{st}:dist={d}" for d in (1, 2, 3)} | {f"{st}:dist={1 << k}" for k in range(2, 13 if small else 15)}
        req |= {f"{st}:off_base=1:ll0", f"{st}:off_base=1:ll>0"}
        if not small: req |= {f"{st}:ll-code=35", f"{st}:ll>=65536", f"{st}:match-to-block-end", f"{st}:dist=131072"}
        if st not in ("btopt", "btlazy2"): req |= {f"{st}:rep-carried-into-block", f"{st}:match-to-block-end-goes-on-as-rep"}
    req |= {f"btopt:off_base={b}:{l}" for b in (2, 3) for l in ("ll0", "ll>0")} | {"btopt:ml=3"}
    for lv in LEVELS:
        req |= {f"L{lv}:n={n}:{params(lv, n)['class']}:{STRATS[params(lv, n)['strat']]}" for n in SIZES}
        req |= {f"L{lv}:inner=1", f"L{lv}:inner=2"}
        for strat in strategies_of(lv):
            st = STRATS[strat]
            if strat <= 2:
                hits = ("hit-ip0", "hit-ip1", "rep-ip2") if strat == 1 else ("d-rep-ip1", "d-long", "d-short", "d-short-then-long")
                req |= {f"L{lv}:{st}:arm:{a}" for a in hits + ("catchup", "rep2-after", "step-up", "start-near-rep", "end-behind-ilimit")}
                req |= {f"L{lv}:{st}:{a}:step>2" for a in hits if a != "d-rep-ip1"}
                req |= {f"L{lv}:{st}:catchup={v}" for v in ("0", "1", "2", "3", "4", "5+")} | {f"L{lv}:{st}:rep2-after:once", f"L{lv}:{st}:rep2-after:again", f"L{lv}:{st}:match-ends-within-200-of-ilimit"}
                req |= {f"L{lv}:{st}:found-at-search-offset={o}" for o in list(range(125)) + [">124"]} | {f"L{lv}:{st}:found-at-even-position", f"L{lv}:{st}:found-at-odd-position"}
                req |= {f"L{lv}:{st}:slot-written-in-window:second", f"L{lv}:{st}:slot-written-in-window:dirty"}
                req |= {f"L{lv}:{st}:ml=held{d:+d}" for d in (-1, 0, 1)}
            elif strat <= 6:
                req |= {f"L{lv}:{st}:arm:{a}" for a in ("rep-ip1", "search-wins", "catchup", "rep-loop", "step-grown")}
                if strat >= 4: req |= {f"L{lv}:{st}:arm:{a}" for a in ("d1-rep", "d1-search")}
                if strat >= 5: req |= {f"L{lv}:{st}:arm:{a}" for a in ("d2-rep", "d2-search")}
                req |= {f"L{lv}:{st}:catchup={v}" for v in ("0", "1", "2", "5+")} | {f"L{lv}:{st}:rep-loop:once", f"L{lv}:{st}:rep-loop:again", f"L{lv}:{st}:ml>=576-then-search"}
                if strat == 6: req |= {f"L{lv}:bt:len={v}" for v in (31, 32, 33, 64, 65)}
                if strat == 6: req |= {f"L{lv}:bt:end:low-limit"} | {f"L{lv}:btlazy2:arm:bt-batch-full"}
            else:
                req |= {f"L{lv}:btopt:arm:{a}" for a in ("predef-prices", "block-stats", "immediate", "ll0-shift", "not-greedy", "array-full")}
                req |= {f"L{lv}:opt:{a}" for a in ("matches=0", "matches=1", "matches=2", "matches=3+", "sufficient", "match>=4096")}
        # the hash-chain finder of the 16 KiB rows: the source behind 2^searchLog - 1 words of its hash is found, behind 2^searchLog it is not
        p = params(lv, 10000)
        if 3 <= p["strat"] <= 5:
            req |= {f"L{lv}:hc:found:behind={(1 << p['slog']) - 1}", f"L{lv}:hc:missed:behind={1 << p['slog']}", f"L{lv}:hc:end:attempts", f"L{lv}:hc:end:low-limit"}
            req |= {f"L{lv}:hc:len={v}" for v in (31, 32, 33, 64, 65)}
        p = params(lv, 20000)
        if 3 <= p["strat"] <= 5 and p["mml"] == 4:          # the row finder of the rows for 16 KiB < n <= 128 KiB: min(2^searchLog, entries) attempts
            att = 1 << min(p["slog"], 6)
            req |= {f"L{lv}:row:found:behind={att - 1}", f"L{lv}:row:missed:behind={att}"}
        if any(3 <= r[6] <= 5 and r[0] > 14 for r in ROWS[lv - 1]):
            req |= {f"L{lv}:{STRATS[r[6]]}:row-cache:starts-in-previous-block" for r in ROWS[lv - 1][:2] if 3 <= r[6] <= 5}     # (inputs above 128 KiB: more than one block)
            req |= {f"L{lv}:row:len={v}" for v in (31, 32, 33, 64, 65)} | {f"L{lv}:{STRATS[r[6]]}:arm:row-wraps" for r in ROWS[lv - 1][:3] if 3 <= r[6] <= 5}
            req |= {f"L{lv}:row:end:{e}" for e in ("attempts", "chain-end")} | {f"L{lv}:row:entries={1 << min(max(r[3], 4), 6)}" for r in ROWS[lv - 1][:3] if 3 <= r[6] <= 5}
    req |= {"L1:inner=32", "L3:inner=32", "L12:opt:hash3-match"}
    # the sequence count in three bytes, and either side of it: one 128 KiB block of four-byte matches without literals
    req |= {f"{g}:{k}" for g in ("lt-lazy", "ge-lazy") for k in ("fmt:nseq:3B", "nseq=32511", "nseq=32512", "nseq>=0x7F00")}
    # the binary trees (levels 9 and 10 at 16 KiB and less, 11 and 12 above) and the row finder's rows with minMatch 5 (level 4 above 128 KiB, levels 11 and 12 above 256 KiB)
    for lv, slog in ((9, 5), (10, 9), (11, 5), (12, 7)): req |= {f"L{lv}:bt:found:behind={(1 << slog) - 1}", f"L{lv}:bt:missed:behind={1 << slog}"}
    for lv, att in ((4, 8), (11, 64), (12, 64)): req |= {f"L{lv}:row:found:behind={att - 1}", f"L{lv}:row:missed:behind={att}"}
    req |= {f"L{lv}:{STRATS[r[6]]}:target-length>1" for lv in LEVELS for r in ROWS[lv - 1] if 3 <= r[6] <= 6 and r[5] > 1}
    for lv in WINDOW_LEVELS:
        st = STRATS[ROWS[lv - 1][0][6]]
        req |= {f"L{lv}:window:far-before-last-block:found", f"L{lv}:window:w+1:refused", f"L{lv}:{st}:arm:rep-zeroed", f"L{lv}:{st}:arm:rep-restored", f"L{lv}:{st}:arm:out-of-window"}
        if lv < 6: req |= {f"L{lv}:window:below-edge:refused", f"L{lv}:window:edge+0:found", f"L{lv}:window:w-1:refused"}     # the fast finders' window ends with the block
        else: req |= {f"L{lv}:window:w-1:found", f"L{lv}:window:w+0:found", f"L{lv}:lazy:arm:ntu-limit"}
    return frozenset(req)


REQUIRED = _required()
# what the reference cannot reach (DESIGN_NOTES.md, "zstd encoder catalogue"), as patterns over ledger keys
UNREACHED = tuple(re.compile(p) for p in (
    r"lt-lazy:fmt:(ll|of|ml):repeat", r"lt-lazy:(ll|of|ml):repeat:.*",                 # a repeat table below lazy needs a table known valid: a dictionary's
    r"(fast|dfast|greedy|lazy|lazy2|btlazy2):off_base=[23]:.*",                        # only the optimal parser tries the second and third repeat offset
    r"L[123]:window:w[-+]\d:found",
    r"L\d+:\w+:row-cache:starts-in-this-block"))                                       # the row finder's next_to_update never passes the last searched position, 16 bytes before a block's end                                                   # fast / dfast: the window's low end comes from the block's end, the last search lies 8 bytes before it
