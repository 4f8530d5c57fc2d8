"""The shape catalogue of the streamed .zst encoder (fourmc_gpu_zst_compress / fourmc_gpu_zsts_compress; zstd_encode.hip, "streamed
frames"): the ext-dict parsers, the prefix-only parsers with a carried offset, the catch-up and the window bookkeeping.

  inputs()     name -> (source, level); a name ends in ":l<level>".  Built lazily, one at a time (source(name)).
  trace(name)  what the oracle's port of the streaming compressor (oracle.h: orc_zstd_stream_compress_ex) did on it
  ledger()     key -> the inputs that reach it, from the port's trace on the port's own run; a key ends in "@l<level>"
  REQUIRED     the keys the catalogue is there for;  UNREACHED  key -> the line that makes it unreachable
  MUTANTS      the deliberately wrong decisions of the port (oracle.h: ORC_ZMUT_*)
  fixture() / fixture_build()  tests/golden/zst_write_shapes.json: SHA-256 and length of the reference's image per input

Layout of a source (W the level's window, B = 128 KiB, R = W + B the input ring, m = R / B blocks per cycle): a prefix of R
incompressible bytes, shared by the inputs of a level, and one to three blocks behind the wrap at R.  Block m + j is an ext-dict
block with dictStartIndex at position (j + 2) B and prefixStartIndex at R.  Planted material lies where the parsers probe every
position: the first bytes of a block, or right behind a match.  A source of a copy lies where it was entered into the tables: the
first bytes of a block, or the last 100 bytes of block m - 1 after helper() (that block is one long match up to R - 100, so the
search behind it enters R - 100 .. R - 11).
"""
import functools
import hashlib
import json
import os

import numpy as np

import helpers
import zst_model as zm
import zst_write_model as wm
from zst_write_model import B, WINDOW, ring

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "zst_write_shapes.json")
LEVELS = (1, 2, 3, 4)
FAST, DFAST = (1, 2), (3, 4)
K = 4096                                                             # a planted copy
MUTANTS = {1: "catch-up ignores the low end, prefix source", 2: "catch-up ignores the low end, ext source", 3: "fast repcode rule >= 3",
           4: "behind-match repcode rule >= 4", 5: "fast candidate bound strict", 6: "dfast candidate bound non-strict",
           7: "max_rep compared with > at an ext block's start", 8: "saved repcodes not restored", 9: "hand-over block parsed by the ext parser",
           10: "dictStartIndex from the block's start", 11: "carried offset above dev_max dropped", 12: "dfast upgrade to a long match skipped"}
# oracle.h
MODE_SHORT, MODE_PREFIX, MODE_PREFIX_CARRY, MODE_EXT, MODE_HANDOVER, MODE_HANDOVER_CARRY = range(6)
ARMS = {1: "rep", 2: "ip0", 3: "ip1", 4: "long", 5: "short", 6: "short-then-long", 7: "rep-loop", 8: "pfx-rep", 9: "pfx-hit"}
STOPS = {1: "anchor", 2: "low-equal", 3: "low", 4: "mismatch"}
(ZB_NUMBER, ZB_START, ZB_LEN, ZB_MODE, ZB_DICT, ZB_PFX, ZB_REP_IN, _, ZB_REP_OUT, _, ZB_ZEROED, ZB_RESTORED, ZB_TYPE, ZB_NSEQ, ZB_IN_CYCLE, ZB_CYCLE,
 ZB_DEV_MAX, ZB_REF_MAX, ZB_MAX_REP, ZB_LAST) = range(20)


@functools.lru_cache(None)
def _base(level):
    """2 R + 3 B random bytes: every input of the level is a prefix of it with material planted"""
    return np.random.default_rng(0x2357 + level).integers(0, 256, 2 * ring(level) + 3 * B, dtype=np.uint8)


def _copy(s, dst, src, n):
    s[dst:dst + n] = s[src:src + n].copy()


def _differ(s, a, b):
    if s[a] == s[b]: s[a] ^= 0x55


def _helper(s, level):
    """block m - 1 becomes one match up to R - 100: positions R - 100 .. R - 11 are probed one by one and entered"""
    R = ring(level)
    _copy(s, R - B, R - 2 * B, B - 100); _differ(s, R - 100, R - B - 100)


def _generators(level):
    """name -> (length, function(s) that plants into the prefix s of the base)"""
    W, R = WINDOW[level], ring(level)
    m, S, D = R // B, R - B, R + B                                   # S: start of the last prefix block; D: start of block m + 1
    fast = level in FAST
    g = {}

    def add(name, n, f=None):
        g[name] = (n, f)
    # ---- window and driver: a copy from the first bytes of block m - 1 at the wrap, cut at the source's end
    for name, n in (("G:R", R), ("G:R+1", R + 1), ("G:R+6", R + 6), ("G:R+7", R + 7), ("G:R+8", R + 8), ("G:R+9", R + 9), ("G:R+4096", R + 4096),
                    ("G:R+B-1", R + B - 1), ("G:R+B", R + B), ("G:R+B+1", R + B + 1)):
        add(name, n, lambda s, n=n: _copy(s, R, S + 8, min(n - R, K)))

    def cycle(s):                                                    # a copy at the start of every block from the wrap on, from the block before it
        for k in range(m, len(s) // B + 1):
            if k * B + 64 <= len(s): _copy(s, k * B, (k - 1) * B + 8, min(K, len(s) - k * B))
    add("W:cycle", 2 * R + 2 * B + 5000, cycle)                      # both wraps, the hand-over block, blocks of the second cycle, a short last one
    add("W:handover-short", R + (m - 2) * B + 5000, cycle)           # the hand-over position holds a short last block: the ext parser's
    def text(s): s[:] = helpers.corpus(len(s), logs=True)             # log text through the ext parsers: dense sequences, full tables
    add("T:text", D + B, text)
    def rle(s): s[R:] = 0x5A
    add("W:rle", D + B + 1000, rle)
    def rawmid(s):
        _copy(s, R, S + 8, 60000); _copy(s, D + B, S + 8, 60000); _copy(s, D + B + 60000, S + 8, 60000)
    add("W:rawmid", D + 2 * B, rawmid)                               # compressed, raw, compressed (the repeat offsets and tables of block m serve block m + 2)
    # ---- search arms, ext source (from block m - 1) and prefix source (from block m)
    def ip0_ext(s): _copy(s, R, S + 8, K)
    def ip1_ext(s): _copy(s, R + 1, S + 8, K); _differ(s, R, S + 7)
    def ip0_pfx(s): _copy(s, D, R + 8, K)
    def ip1_pfx(s): _copy(s, D + 1, R + 8, K); _differ(s, D, R + 7)
    def rep_at(s, d, src):                                            # a copy with five other bytes in its middle: its second half is the repeat offset's
        _copy(s, d, src, K)
        for i in range(5): s[d + K // 2 + i] ^= 0xA5
    add("A:first:ext", D, ip0_ext); add("A:second:ext", D, ip1_ext); add("A:first:pfx", D + B, ip0_pfx); add("A:second:pfx", D + B, ip1_pfx)
    add("A:rep:ext", D, lambda s: rep_at(s, R, S + 8)); add("A:rep:pfx", D + B, lambda s: rep_at(s, D, R + 8))
    def run(s):                                                       # behind a match (the repeat offset is not 1) a run of one byte that no table knows: ip0 and ip1 share a slot, ip1 finds ip0
        _copy(s, R, S + 8, 62); s[R + 62:R + 8192] = 0xEE
    add("A:run", D, run)
    def short_at(s, d, src): _copy(s, d, src, 6); _differ(s, d + 6, src + 6); s[d + 4096:d + 12288] = 0x11      # (the run makes the block worth compressing)
    if not fast: add("A:short:ext", D, lambda s: short_at(s, R, S + 8)); add("A:short:pfx", D + B, lambda s: short_at(s, D, R + 8))
    def upgrade(s, d, src):                                           # five bytes of `src` at d, and from d + 1 a long copy of src + 40
        s[src + 40:src + 44] = s[src + 1:src + 5]
        s[d] = s[src]; _copy(s, d + 1, src + 40, K); _differ(s, d + 8, src + 8)
    if not fast: add("A:upgrade:ext", D, lambda s: upgrade(s, R, S + 8)); add("A:upgrade:pfx", D + B, lambda s: upgrade(s, D, R + 8))
    # ---- search length: the copy starts d bytes into the block
    def lengths(s):                                                   # each search starts behind the last copy, where every position is probed again
        at = R
        for d in (10, 64, 100, 200, 400, 700, 3000):
            _copy(s, at + d, S + 8, K); _differ(s, at + d - 1, S + 7); _differ(s, at + d + K, S + 8 + K)
            at += d + K
    add("L:all", D, lengths)
    # ---- two positions of one search with equal words: the second finds the first
    def twice(s, gap):
        s[R + 20 + gap:R + 32 + gap] = s[R + 20:R + 32]; s[R + 4096:R + 12288] = 0x11
        # certain sharing, from the bytes: the search starts at R with step 2 (fast: pairs of neighbours) or 1 (dfast) and holds this step for
        # 128 bytes, so R + 20 and R + 20 + gap are both probed, gap / 2 pairs or gap positions apart, with equal words: one table slot
        assert gap % 2 == 0 and 20 + gap + 12 < 128 and (gap // 2 if fast else gap) <= 15
        assert bytes(s[R + 20:R + 28]) == bytes(s[R + 20 + gap:R + 28 + gap]) and bytes(s[R + 20:R + 24]) not in bytes(s[R:R + 20 + gap + 3])[:20 + 3]
    add("S:own:12", D, lambda s: twice(s, 12))
    # ---- candidate bounds: the copy's source starts at dictStartIndex - 1, at it, one above it (block m: position 2 B; block m + 2: position 4 B)
    add("C:dict-1", D, lambda s: _copy(s, R, 2 * B - 1, K))

    def exact(s, r):
        # A last block of 76 bytes: dictStartIndex is position 2 B + 76, among the first bytes of block 2, where every position was
        # entered (a third of those entries is overwritten by the blocks between; 75, 76 and 77 survive at all four levels: the ledger says so).  The copy (from dictStartIndex + r) is as long as the hash reads and no longer, so no later position finds it: the
        # entry at dictStartIndex + r itself decides, and the lowest valid index is the one taken from the block's END (from its
        # start it would be 76 lower: all three would pass).  The run behind it makes the block worth compressing
        dct, w = 2 * B + 76 + r, (7, 6, 5, 5)[level - 1]
        _copy(s, D, dct, w); _differ(s, D + w, dct + w)
        s[D + 16:D + 76] = 0x11
    add("C:dict-1:exact", D + 76, lambda s: exact(s, -1)); add("C:dict:exact", D + 76, lambda s: exact(s, 0)); add("C:dict+1:exact", D + 76, lambda s: exact(s, 1))
    def handover_rep(s):
        # block 2 m - 3 leaves the offset W - B (fast) or W - B + 1 (dfast): the hand-over block's prefix parser keeps the first and drops
        # the second, the ext parser would do the opposite
        hs, d = R + (m - 2) * B, W - B + (0 if fast else 1)
        _copy(s, hs - B + 4, hs - B + 4 - d, K); _differ(s, hs - B + 3, hs - B + 3 - d); _differ(s, hs - B + 4 + K, hs - B + 4 + K - d)
        q = hs + (2 if fast else 1)
        _copy(s, q, q - d, K)
    add("W:handover-rep", R + (m - 1) * B, handover_rep)
    # ---- catch-up: L equal bytes in front of a source that the tables hold (the first byte of block m - 1)
    for L in (1, 63, 64, 65, 140):                                    # (the bytes in front of a block's start were not entered: the hit is the block's first byte)
        add(f"U:{L}:mismatch", D, lambda s, L=L: (_copy(s, R + 4, S - L, L + K), _differ(s, R + 3, S - L - 1)))
    add("U:pfx-start", D + B, lambda s: _copy(s, D + 4, R - 16, 16 + K))     # the source is the prefix's first byte, 16 equal bytes in front of it
    # ---- forward count
    add("F:wrap", D + B, lambda s: _copy(s, D, S + 8, B))            # the source runs across the wrap point, the match to the block's end
    add("F:end-5", D, lambda s: (_copy(s, D - K - 5, S + 8, K), _differ(s, D - 5, S + 8 + K)))
    # ---- repeat-offset tests that find equal bytes at prefixStartIndex + r (block m + 1, after helper())
    for r in (-4, -3, -1, 0, 1):
        def search_test(s, r=r):
            _helper(s, level)
            q = R + r - (70 if fast else 69)                         # the first match's source; its offset puts the first clean test on R + r
            _copy(s, D, q, 64); _differ(s, D + 64, q + 64)
            _copy(s, D + 69, q + 69, K)
            for i in range(64, 69): _differ(s, D + i, q + i)
        def behind_test(s, r=r):
            _helper(s, level)
            a = R + r - 64
            _copy(s, D, a, 32); _copy(s, D + 32, R - 95, 32); _differ(s, D + 32, a + 32); _differ(s, D + 64, R - 95 + 32)
            _copy(s, D + 64, a + 64, K)
        add(f"P:search:{r:+d}", D + B, search_test); add(f"P:behind:{r:+d}", D + B, behind_test)
    def loop2(s):
        _helper(s, level)
        a, b = R - 80, R - 40
        _copy(s, D, a, 24); _copy(s, D + 24, b, 16); _differ(s, D + 24, a + 24)
        _copy(s, D + 40, a + 40, 16); _differ(s, D + 40, b + 16)     # behind the second match: the first one's offset ...
        _copy(s, D + 56, b + 32, K); _differ(s, D + 56, a + 56)     # ... and behind that the second one's again
    add("P:loop2", D + B, loop2)
    # ---- repeat offsets at an ext block's start: block m leaves max_rep of block m + 1 (W - B), or one less
    for name, d in (("max", W - B), ("max-1", W - B - 1)) if fast else ():
        def rep1(s, d=d, use=True):
            _copy(s, R + 4, R + 4 - d, K); _differ(s, R + 3, R + 3 - d); _differ(s, R + 4 + K, R + 4 + K - d)
            if use: _copy(s, D + 2, D + 2 - d, K)
        def rep2(s, d=d, use=True):
            rep1(s, d, False)
            _copy(s, R + 2 * K, S + 8, 64); _differ(s, R + 2 * K - 1, S + 7)
            if use: _copy(s, D, S + 8 + 64, 32); _differ(s, D + 32, S + 8 + 96); _copy(s, D + 32, D + 32 - d, K)
        add(f"K:rep1={name}", D + B, rep1); add(f"K:rep2={name}", D + B, rep2)
        # block m + 1 finds nothing: what it put aside comes back, and the short block behind it (max_rep = W - 1000) uses it
        def idle(s):                                                  # 64 symbols: no match, and literals that Huffman makes smaller, so the block confirms its offsets
            s[D:D + B] = np.random.default_rng(77).integers(0, 64, B, dtype=np.uint8)
        add(f"K:rep1={name}:idle", D + B + 1000, lambda s, f=rep1, d=d: (f(s, use=False), idle(s), _copy(s, D + B + 2, D + B + 2 - d, 64)))
        add(f"K:rep2={name}:idle", D + B + 1000, lambda s, f=rep2, d=d: (f(s, use=False), idle(s), _copy(s, D + B, S + 72, 32), _differ(s, D + B + 32, S + 104),
                                                                          _copy(s, D + B + 32, D + B + 32 - d, 64)))
    # ---- the last block before the wrap with a carried offset: block m - 2 leaves dev_max (W - B), or one more
    for name, d in (("dev_max", W - B), ("dev_max+1", W - B + 1)):
        def carry(s, d=d):
            p = W - B + 40
            _copy(s, p, p - d, K); _differ(s, p - 1, p - d - 1); _differ(s, p + K, p - d + K)
            _copy(s, W + 2, W + 2 - d, K)                            # block m - 1: the offset's own match ...
            _copy(s, W + 2 * K, W - B + 8, 64)                         # ... and one that the table finds
        add(f"Y:{name}", R + 1, carry)
        def carry2(s, d=d):                                          # the same offset left as the SECOND one: a short match right behind the planted one
            p = W - B + 40
            _copy(s, p, p - d, K); _differ(s, p - 1, p - d - 1); _differ(s, p + K, p - d + K)
            _copy(s, p + K, W - B + 8, 64); _differ(s, p + K + 64, W - B + 72)
            q, d1 = W + (2 if fast else 1), p + K - (W - B + 8)      # block m - 1: the first offset's own match, which leaves both as they are ...
            _copy(s, q, q - d1, 64); _differ(s, q + 64, q + 64 - d1)
            _copy(s, q + 64, q + 64 - d, K)                          # ... and right behind it the second offset's own
        add(f"Y2:{name}", R + 1, carry2)
    return g


@functools.lru_cache(None)
def names():
    return tuple(f"{n}:l{lv}" for lv in LEVELS for n in _generators(lv))


def source(name):
    base, lv = name.rsplit(":l", 1)
    n, f = _generators(int(lv))[base]
    s = _base(int(lv))[:n].copy()
    if f: f(s)
    return s, int(lv)


class _Inputs:
    """name -> (source, level), built when asked for: the catalogue is never held as a whole"""
    def __getitem__(self, name): return source(name)
    def __iter__(self): return iter(names())
    def __len__(self): return len(names())
    def keys(self): return names()
    def items(self): return ((n, source(n)) for n in names())


def inputs():
    return _Inputs()


def total_bytes():
    return sum(_generators(lv)[n][0] for lv in LEVELS for n in _generators(lv))


def port(name, mutate=0):
    src, lv = source(name)
    return helpers.orc_zstd_stream_compress(src, lv, mutate=mutate)


def trace(name):
    src, lv = source(name)
    return helpers.orc_zstd_stream_compress(src, lv, trace=True)


def keys_of(name, tabs):
    """the ledger keys one input reaches (without the level suffix)"""
    search, blocks, seqs, reps = tabs
    src, lv = source(name)
    W, R = WINDOW[lv], ring(lv)
    m = R // B
    out = set()
    n = len(src)
    for d, label in ((0, "R"), (1, "R+1"), (B - 1, "R+B-1"), (B, "R+B"), (B + 1, "R+B+1")):
        if n == R + d: out.add("src:" + label)
    for t in (0, 1, 6, 7, 8, 9, 4096):
        if n == R + t: out.add(f"tail:{t}")
    mode = {int(b[ZB_NUMBER]): int(b[ZB_MODE]) for b in blocks}
    dict_of = {int(b[ZB_NUMBER]): int(b[ZB_DICT]) for b in blocks}
    for i, b in enumerate(blocks):
        md, ic, cy, ln, ty = int(b[ZB_MODE]), int(b[ZB_IN_CYCLE]), int(b[ZB_CYCLE]), int(b[ZB_LEN]), int(b[ZB_TYPE])
        if md == MODE_EXT:
            if ic == 0 and cy == 1: out.add("blk:first-ext")
            if ic == m - 3: out.add("blk:last-ext-of-cycle")
            if ic == m - 2 and ln < B: out.add("blk:handover-short-ext")
            if ty == 0 and b[ZB_NSEQ] == 0 and ln >= 7: out.add("blk:ext-raw-no-sequence")
            if ty == 1: out.add("blk:ext-rle")
            if ty == 0 and 0 < i < len(blocks) - 1 and blocks[i - 1][ZB_MODE] == MODE_EXT and blocks[i - 1][ZB_TYPE] == 2 \
                    and blocks[i + 1][ZB_MODE] == MODE_EXT and blocks[i + 1][ZB_TYPE] == 2: out.add("blk:raw-between-compressed-ext")
            if lv in FAST:
                for w, nm in ((0, "rep1"), (1, "rep2")):
                    if b[ZB_REP_IN + w] == b[ZB_MAX_REP] and b[ZB_ZEROED] >> w & 1: out.add(f"start:{nm}=max_rep:dropped")
                    if b[ZB_REP_IN + w] == b[ZB_MAX_REP] - 1 and not b[ZB_ZEROED] >> w & 1: out.add(f"start:{nm}=max_rep-1:kept")
                if b[ZB_RESTORED] & 1: out.add("restore:rep1")
                if b[ZB_RESTORED] & 2: out.add("restore:rep2")
                if b[ZB_RESTORED] & 4: out.add("restore:saved1-to-rep2")
                if b[ZB_ZEROED] & 1 and (search[:, 0] == b[ZB_NUMBER]).any(): out.add("search:rep1=0")
        if md in (MODE_HANDOVER, MODE_HANDOVER_CARRY) and ln == B: out.add("blk:handover-full")
        if ic == m - 1 and cy >= 1: out.add("blk:last-of-cycle")
        if cy >= 2: out.add("blk:second-cycle")
        if md in (MODE_PREFIX, MODE_PREFIX_CARRY, MODE_HANDOVER, MODE_HANDOVER_CARRY) and ic == m - 1:
            for w, nm in ((0, "rep1"), (1, "rep2")):
                v = int(b[ZB_REP_IN + w])
                if v == b[ZB_DEV_MAX] and md in (MODE_PREFIX, MODE_HANDOVER): out.add(f"carry:{nm}=dev_max:plain")
                if v == b[ZB_DEV_MAX] + 1 and md in (MODE_PREFIX_CARRY, MODE_HANDOVER_CARRY): out.add(f"carry:{nm}=dev_max+1:kept")
    for i, q in enumerate(seqs):
        blk, arm, ip, cand, seg, cross, back, stop, mlen, left, own, turn = (int(x) for x in q)
        md = mode[blk]
        if arm in (8, 9):
            if md in (MODE_PREFIX_CARRY, MODE_HANDOVER_CARRY): out.add("carry:uses-rep" if arm == 8 else "carry:hash-hit")
            continue
        where = "pfx" if seg else "ext"
        out.add(f"arm:{ARMS[arm]}:{where}")
        if cross: out.add("fwd:across-wrap")
        if left == 0: out.add("fwd:to-block-end")
        elif left < 8: out.add("fwd:within-8-of-end")
        if arm == 7: out.add("loop:1" if turn == 1 else "loop:2+")
        elif left >= 8 and not (i + 1 < len(seqs) and seqs[i + 1][1] == 7 and seqs[i + 1][0] == blk): out.add("loop:0")   # the loop behind this match ran and took nothing
        if stop and md == MODE_EXT:
            d = cand - dict_of[blk]
            if d in (0, 1): out.add(f"cand:dict+{d}")
        if stop:
            for L in (0, 1, 63, 64, 65):
                if back == L: out.add(f"catchup:{L}")
            if back >= 130: out.add("catchup:130+")
            out.add(f"stop:{STOPS[stop]}" + (f":{where}" if stop in (2, 3) else ""))
            if own: out.add("hit:entered-by-this-search")
    for s in search:
        blk, first, probes, step, arm, from_anchor, dist, equal, same, grew = (int(x) for x in s)
        if arm == 0: out.add("search:block-end")
        else:
            if lv in FAST:
                out.add("pairs:" + ("0" if probes == 0 else "1-15" if probes < 16 else "16-47" if probes < 48 else "48-111" if probes < 112 else "112+"))
                if arm == 3 and same and probes == 0: out.add("arm:ip1:one-slot")
            else: out.add("event:below-256" if from_anchor < 256 else "event:256-and-above")
            if grew:
                out.add("search:step-grew")
                # the kernel speculates the probes of a search in batches of 16, 32, 64, 64, ... (zstd_encode.hip, fast_block_ext /
                # dfast_block_ext): the batch that holds the first probe at the new step, and the event behind it, has the step change
                # inside (the general path of :3306-3314, and of :3422-3423 in dfast); a scoreboard cut can only shorten a batch
                lo, w = 0, 16
                while lo + w <= grew: lo, w = lo + w, min(64, 2 * w)
                if grew > lo and probes >= grew: out.add(f"search:step-grew:inside-batch-of-{w}")
        if equal: out.add("share:equal-words-within-15")
    for e in reps:
        blk, site, at, rel, ok = (int(x) for x in e)
        if site == 2:
            out.add(f"cand:dict{rel:+d}:refused")
            if rel < 0 and at == blocks[blk][ZB_START] and rel + blocks[blk][ZB_LEN] > 0: out.add("bound:from-block-end")   # valid by the block's start, refused by its end
        elif rel in (-4, -3, -1, 0, 1): out.add(f"rep:{'behind' if site else 'search'}:pfx{rel:+d}:{'accepted' if ok else 'refused'}")
    return out


@functools.lru_cache(None)
def ledger():
    out = {}
    for name in names():
        lv = name.rsplit(":l", 1)[1]
        for k in keys_of(name, trace(name)[1]): out.setdefault(f"{k}@l{lv}", []).append(name)
    return out


_BOTH = ["cand:dict+1", "blk:first-ext", "blk:last-ext-of-cycle", "blk:handover-full", "blk:handover-short-ext", "blk:last-of-cycle", "blk:second-cycle",
         "blk:ext-raw-no-sequence", "blk:ext-rle", "blk:raw-between-compressed-ext",
         "src:R", "src:R+1", "src:R+B-1", "src:R+B", "src:R+B+1", "tail:0", "tail:1", "tail:6", "tail:7", "tail:8", "tail:9", "tail:4096",
         "arm:rep:ext", "arm:rep:pfx", "arm:rep-loop:ext", "arm:rep-loop:pfx", "loop:0", "cand:dict-1:refused", "bound:from-block-end",
         "search:step-grew:inside-batch-of-64", "carry:rep2=dev_max:plain", "carry:rep2=dev_max+1:kept", "search:block-end", "search:step-grew", "share:equal-words-within-15", "hit:entered-by-this-search",
         "catchup:0", "catchup:1", "catchup:63", "catchup:64", "catchup:65", "catchup:130+",
         "stop:anchor", "stop:mismatch", "stop:low-equal:pfx", "stop:low-equal:ext", "fwd:across-wrap", "fwd:to-block-end", "fwd:within-8-of-end",
         "loop:1", "loop:2+", "carry:rep1=dev_max:plain", "carry:rep1=dev_max+1:kept", "carry:uses-rep", "carry:hash-hit",
         "rep:search:pfx-4:accepted", "rep:search:pfx-3:refused", "rep:search:pfx-1:refused", "rep:search:pfx+1:accepted",
         "rep:behind:pfx-4:accepted", "rep:behind:pfx-3:refused", "rep:behind:pfx-1:refused", "rep:behind:pfx+0:accepted", "rep:behind:pfx+1:accepted"]
_FAST = ["cand:dict+0", "arm:ip0:ext", "arm:ip0:pfx", "arm:ip1:ext", "arm:ip1:pfx", "arm:ip1:one-slot", "pairs:0", "pairs:1-15", "pairs:16-47", "pairs:48-111", "pairs:112+",
         "rep:search:pfx+0:refused", "start:rep1=max_rep:dropped", "start:rep1=max_rep-1:kept", "start:rep2=max_rep:dropped", "start:rep2=max_rep-1:kept",
         "restore:rep1", "restore:rep2", "restore:saved1-to-rep2", "search:rep1=0"]
_DFAST = ["cand:dict+0:refused", "arm:long:ext", "arm:long:pfx", "arm:short:ext", "arm:short:pfx", "arm:short-then-long:ext", "arm:short-then-long:pfx",
          "event:below-256", "event:256-and-above", "rep:search:pfx+0:accepted"]
REQUIRED = tuple(f"{k}@l{lv}" for lv in LEVELS for k in _BOTH + (_FAST if lv in FAST else _DFAST))
_WHY_FAST = "zstd_fast.c:684-935 has one table and the arms repcode / ip0 / ip1 only; the long and short tables are zstd_double_fast.c:627-635"
_WHY_DFAST = "zstd_double_fast.c:592-734 probes one position at a time (long, short, long at ip + 1); pairs are zstd_fast.c:766-857"
_WHY_NO_SAVE = "zstd_double_fast.c:617-623, :728-730: the ext-dict variant puts no repeat offset aside at a block's start; it bounds each test (:645, :713)"
UNREACHED = {}
for _lv in LEVELS:
    for _k in (_DFAST if _lv in FAST else _FAST):
        UNREACHED[f"{_k}@l{_lv}"] = _WHY_FAST if _lv in FAST else (_WHY_NO_SAVE if _k.startswith(("start:", "restore:", "search:rep1")) else _WHY_DFAST)
    UNREACHED[f"rep:search:pfx+0:{'accepted' if _lv in FAST else 'refused'}@l{_lv}"] = \
        "zstd_fast.c:772 refuses a repeat index equal to prefixStartIndex" if _lv in FAST else "zstd_double_fast.c:644 accepts a repeat index equal to prefixStartIndex"
    if _lv in DFAST: UNREACHED[f"cand:dict+0@l{_lv}"] = "zstd_double_fast.c:652, :663, :670: a candidate must lie above dictStartIndex"
    if _lv in FAST: UNREACHED[f"cand:dict+0:refused@l{_lv}"] = "zstd_fast.c:798, :826: a candidate at dictStartIndex itself is taken"
    for _nm in ("rep1", "rep2"):
        UNREACHED[f"carry:{_nm}=ref_max@l{_lv}"] = UNREACHED[f"carry:{_nm}=ref_max+1@l{_lv}"] = \
            ("ref_max of the last block of a cycle is the window; a match starts at least 8 bytes in front of its block's end (ilimit, zstd_fast.c:159, "
             "zstd_double_fast.c:115) and reaches back to that end - window at most (ZSTD_getLowestPrefixIndex), so no offset above window - 8 is carried: the upper half of the kernel's carry test, `<= ref_max` in zstd_stream_frame, is never false for a carried offset, "
             "and the ZEROED word of a prefix-only block stays 0")


def reference(name):
    src, lv = source(name)
    return zm.zstcodec(src, lv)


def fixture_build():
    out = {}
    for name in names():
        img = reference(name)
        out[name] = {"sha256": hashlib.sha256(img).hexdigest(), "bytes": len(img)}
    for name, (src, lv) in wm.inputs().items():
        img = wm.reference()[name]
        out["zst_write_model/" + name] = {"sha256": hashlib.sha256(img).hexdigest(), "bytes": len(img)}
    return out


@functools.lru_cache(None)
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


if __name__ == "__main__":
    with open(FIXTURE, "w") as f:
        json.dump(fixture_build(), f, indent=1, sort_keys=True)
        f.write("\n")
