"""Inputs that walk every search, pattern, swap and price shape of the LZ4 HC kernel at levels 9..12 (4mc_amd/csrc/lz4hc_opt_encode.hip
and lz4hc_opt_core.h), for the encoder tests (plain module, like hc_shapes.py; numpy + the oracle port's trace).

  cases()         the deterministic input set: named inputs, each as small as its key allows.  Level 9 runs hc_shapes.cases() as well:
                  ho_hash_chain is its own text of the level 1..8 arbitration.
  trace()         what the oracle port's search and parse did on one input (oracle.h: the ORC_HX_* rows), as numpy tables.
  ledger()        the keys a case set reaches, computed from that trace, the input's hashes and the kernel's constants below.
  REQUIRED        the keys the set must reach, per level.  A missing key is a test failure.
  UNREACHED       keys no input can reach (or none inside the caps), with the reason; the CPU test asserts that no case reaches one.
  caps()          the capacities one input runs at: bound, n-1, r, r-1, r-6, n/2 (r = the port's size of it at that level).
  expected()      every (input, capacity) pair of one level with the port's result and bytes: what the GPU test launches.

A key is read from the port's trace; what a builder meant to build is never taken on trust."""
import collections
import ctypes as C
import functools

import numpy as np

import helpers
import hc_shapes as hs

# ---- constants the kernel branches on (4mc_amd/csrc) ------------------------------------------------------------------------------
LEVELS = (9, 10, 11, 12)
ATTEMPTS = {9: 256, 10: 96, 11: 512, 12: 16384}        # lz4hc_opt_core.h:327-330 (lz4hc.c:827-830)
SUFFICIENT = {10: 64, 11: 128, 12: 4095}               # lz4hc_opt_core.h:328-330, :259
K_LANES = 64                    # lz4hc_opt_encode.hip:55-81   positions per insert step; :173 deltas per swap-scan read; :209 records per price step
K_SCORE = 1024                  # lz4hc_opt_encode.hip:33, :60 folded scoreboard of one insert step
K_WIDE = 1024                   # lz4hc_opt_encode.hip:92, :134   a + 1024 <= lim: 16 bytes per lane; below it 64 bytes per step (:101, :142)
K_LANE_BYTES = 16               # lz4hc_opt_encode.hip:93-96   two 8-byte halves, told apart by d0 / d1
K_RING = 65536                  # lz4hc_opt_encode.hip:272   chain deltas of the last 64 Ki positions
K_MAXDIST, K_IDX0 = 65535, 65536                       # lz4hc_opt_core.h:23-24
K_OPT_NUM, K_TRAIL = 4096, 3                           # lz4hc_opt_core.h:25-26
MFLIMIT, LASTLIT, MINMATCH = 12, 5, 4                  # lz4hc_opt_core.h:19-21
MAX_CASE, MAX_BIG, BIG, MAX_WALKED = 160 << 10, 4, 64 << 10, 1_000_000

END = {1: "attempts", 2: "lowest", 3: "chain", 5: "break"}                              # oracle.h ORC_END_*
SWAP = {0: "overlap", 1: "none", 2: "jump", 3: "break"}                                 # oracle.h ORC_HX_SWAP_*
PA = {0: "not-pattern", 1: "below-lowest", 2: "four-differ", 3: "to-end", 4: "to-start:lookback", 5: "to-start:taken",
      6: "to-start:not-longer", 7: "break:distance", 8: "break:delta", 9: "swapped"}   # oracle.h ORC_HX_PA_*
BASE = {0: "lit-inside", 1: "lit-from-start", 2: "match"}                               # oracle.h ORC_HX_BASE_*
SITE = {0: "chain", 1: "first", 2: "series"}                                            # oracle.h ORC_HX_SITE_*
EV_SWAP, EV_PA = 40, 41
EV_OPT = {50: "no-match", 51: "first-now", 52: "first", 53: "at-mflimit", 54: "skip", 55: "search-anyway", 56: "no-longer",
          57: "inner-now:enough", 58: "inner-now:4096", 59: "update", 60: "series"}     # oracle.h ORC_HX_EV_OPT_*
WIDTHS = (12, 8, 12, 3)                                                                 # oracle.h ORC_HX_*_WORDS

Case = hs.Case
Trace = hs.Trace
bound = hs.bound


# ---- the port and its trace -------------------------------------------------------------------------------------------------------
def trace(data, level, cap=None):
    L = hs._lib()
    data = np.ascontiguousarray(data, np.uint8)
    n = len(data)
    dst = np.zeros(bound(n) + 64, np.uint8)

    def run(t):
        return L.orc_lz4hc_compress_ex(data.ctypes.data, dst.ctypes.data, n, bound(n) if cap is None else cap, level, C.byref(t))
    t = hs._Trace()
    run(t)
    bufs = [np.zeros(max(t.n[k], 1), np.int32) for k in range(4)]
    t2 = hs._Trace()
    for k in range(4):
        t2.ev[k] = bufs[k].ctypes.data_as(C.POINTER(C.c_int32)); t2.cap[k] = len(bufs[k])
    r = run(t2)
    tabs = [bufs[k][:t2.n[k]].reshape(-1, WIDTHS[k]) for k in range(4)]
    return Trace(r, dst[:max(r, 0)].copy(), *tabs)


def port(data, level, cap):
    return helpers.orc_compress_hc(data, level, cap)


def caps(data, level):
    n = len(data)
    r = port(data, level, bound(n))[0]
    out = []
    for c in (bound(n), n - 1, r, r - 1, r - 6, n // 2):
        c = max(c, 0)
        if c not in out: out.append(c)
    return out


# ---- builders ---------------------------------------------------------------------------------------------------------------------
_Lay, _not, bucket, B0, B1 = hs._Lay, hs._not, hs.bucket, hs.B0, hs.B1


def _raw(name, *parts):
    return Case(name, np.frombuffer(b"".join(bytes(p) for p in parts), np.uint8).copy(), {})


def _rnd(seed, k):
    return np.random.default_rng(seed).integers(0, 256, k, dtype=np.uint8).tobytes()


def _wide(name, f, room, seed=1):
    """W + body, and again with the forward count of the second stopped after `f` bytes by a mismatch, or by ihigh `room` bytes behind
    the four (lim - a = room)"""
    L = _Lay(seed)
    W = bucket(B0, 1)[0]
    body = L.bytes(max(f, room) + 8)
    L.rnd(3)
    L.put(W + body[:f] + _not(body[f])); L.rnd(5)
    L.put(W + body[:room + LASTLIT])
    return Case(name, L.data(), {})


def _same_word(name, count, seed=2):
    """one word `count` times, a different byte behind each, then the word with four more bytes, twice: the nearest candidate is
    the longest, the older ones hold the four bytes and no more.  The bytes behind the word's first stand once more just before,
    so that the chain swap finds the word's own chain the longest and stays on it"""
    L = _Lay(seed)
    W = bucket(B0, 1)[0]
    T = L.bytes(4)
    for i in range(count):
        L.put(W + bytes([i & 0xFF, (i >> 8) | 0x80]))
    L.put(b"\xEE" + W[1:] + T + b"\xEF"); L.put(W + T + b"\xED"); L.rnd(3)
    L.put(W + T); L.rnd(13)
    return Case(name, L.data(), {})


def _clusters(name, seed=3):
    """a block S, filler, and S again: the copy is one long match and its positions enter the tables 64 per step.  S holds, a step
    apart from each other, groups of 2, 3, 8 equal words, two shared words, and two words that fold onto one scoreboard slot"""
    L = _Lay(seed)
    U, U2 = bucket(B0, 2)
    V = bucket(B0 ^ K_SCORE, 1)[0]
    X = bucket(B1, 1)[0]
    S = _Lay(seed + 100)
    S.put(V); S.rnd(70)
    for rep in range(3):
        for grp in ((U, U), (X, X, X), (U,) * 9, (U, X, U, X), (U2, V), (U, V, U)):
            for w in grp:
                S.put(w); S.rnd(1 + rep)
            S.rnd(66 + 7 * rep)
    s = S.data().tobytes()
    L.rnd(5); L.put(s); L.rnd(40); L.put(s); L.rnd(13)
    return Case(name, L.data(), {})


def _swap_late(name, seed=12):
    """A + B, a hundred copies of A's first 70 bytes, A alone, and A + B again.  The nearest candidate (A alone) has its longest
    chain delta behind offset 64: the swap jumps from there to the oldest, A + B; without it the copies use up the attempts"""
    L = _Lay(seed)
    A, Bt = L.bytes(100), L.bytes(20)
    L.rnd(5); L.put(A + Bt + b"\x01"); L.rnd(3)
    for i in range(100): L.put(A[:70] + _not(A[70]) + bytes([i]))
    L.put(A + _not(Bt[0])); L.rnd(3); L.put(A + Bt); L.rnd(13)
    return Case(name, L.data(), {})


def _ring_swap(name, seed=4):
    """a match whose source lies across position 65536: the chain-swap scan of that candidate reads either side of the ring's wrap"""
    L = _Lay(seed)
    T = L.bytes(60)
    L.rnd(K_RING - 30)
    L.put(T); L.rnd(200); L.put(T); L.rnd(13)
    return Case(name, L.data(), {})


def _far_run(name, seed=5):
    """a run of 100 equal bytes and, 65535 behind its last 40, 40 of the same: pattern analysis stands the walk on `lowest` itself,
    with the run going on below it"""
    L = _Lay(seed)
    L.rnd(3); L.put(b"\x07" * 100); L.rnd(K_MAXDIST - 40); L.put(b"\x07" * 40); L.rnd(13)
    return Case(name, L.data(), {})


def _runs(name, lens, gap=5, byte=b"r", seed=6):
    L = _Lay(seed)
    for k in lens:
        if gap: L.rnd(gap)
        L.put(byte * k)
    L.rnd(13)
    return Case(name, L.data(), {})


@functools.lru_cache(None)
def _run_collider():
    """five bytes whose two overlapping words both carry the hash of b b b b, and b.  (No word x b b b with x != b has the hash of
    b b b b, so the position before a run never does; two neighbouring words of that hash do, one in 2^22 five-byte strings.)"""
    runs = np.arange(256, dtype=np.uint64) * 0x01010101
    rh = hs.hash15(runs)
    v = np.arange(1 << 22, dtype=np.uint64) + 0x31000000
    v = v[np.isin(hs.hash15(v), rh)]
    for y4 in range(256):
        w2 = (v >> 8) | (np.uint64(y4) << 24)
        hit = np.flatnonzero(hs.hash15(w2) == hs.hash15(v))
        if len(hit):
            w = int(v[hit[0]])
            return w.to_bytes(4, "little") + bytes([y4]), bytes([int(np.flatnonzero(rh == hs.hash15(np.uint64(w)))[0])])
    raise AssertionError("no neighbouring colliders")


@functools.lru_cache(None)
def _neighbours(kind):
    """five bytes whose two overlapping words differ and share a hash, and a third word of that hash: 'plain' the second word
    itself, 'abab' a two-byte period, 'abca' a word whose first and last bytes alone are equal"""
    a, b, c = (np.repeat(np.arange(256, dtype=np.uint64), 256), np.tile(np.arange(256, dtype=np.uint64), 256), np.uint64(0x5C))
    cand = {"abab": (a | (b << 8) | (a << 16) | (b << 24))[a != b], "abca": (a | (b << 8) | (c << 16) | (a << 24))[(a != b) & (a != c) & (b != c)]}.get(kind)
    rng = np.random.default_rng(5)
    v = rng.integers(0, 256, (1 << 21, 5), dtype=np.uint8)
    w = v.astype(np.uint64)
    w0, w1 = w[:, 0] | (w[:, 1] << 8) | (w[:, 2] << 16) | (w[:, 3] << 24), w[:, 1] | (w[:, 2] << 8) | (w[:, 3] << 16) | (w[:, 4] << 24)
    ok = (hs.hash15(w0) == hs.hash15(w1)) & (w0 != w1)
    if cand is not None: ok &= np.isin(hs.hash15(w1), hs.hash15(cand))
    i = int(np.flatnonzero(ok)[0])
    third = int(w1[i]) if cand is None else int(cand[hs.hash15(cand) == hs.hash15(w1[i:i + 1])[0]][0])
    return v[i].tobytes(), third.to_bytes(4, "little")


def _not_pattern(name, kind):
    """two neighbouring words of one hash, then a third word of that hash: its walk starts on the second, whose chain delta is 1,
    and the repeat test refuses the word"""
    five, word = _neighbours(kind)
    L = _Lay(11)
    L.rnd(5); L.put(five); L.rnd(9); L.put(word + five[4:] * 2); L.rnd(13)
    return Case(name, L.data(), {})


@functools.lru_cache(None)
def _word_then_collider(kind):
    """w x with w = a b a b ('abab') or a b c a ('abca'): the word behind w's first byte has w's hash, so the position of w is the
    one before a chain delta of 1"""
    a, b = np.repeat(np.arange(256, dtype=np.uint64), 256), np.tile(np.arange(256, dtype=np.uint64), 256)
    c, d = (a, b) if kind == "abab" else (b ^ np.uint64(0x5C), a)
    keep = (a != b) & ((a != c) | (kind == "abab"))
    a, b, c, d = a[keep], b[keep], c[keep], d[keep]
    for x in range(256):
        hit = np.flatnonzero(hs.hash15(b | (c << 8) | (d << 16) | (np.uint64(x) << 24)) == hs.hash15(a | (b << 8) | (c << 16) | (d << 24)))
        hit = hit[(a[hit] != x)]
        if len(hit): return bytes([int(v[hit[0]]) for v in (a, b, c, d)] + [x])
    raise AssertionError("no such word")


def _holds_word(name, kind):
    """a, w x, and later w a: the candidate before the chain delta of 1 holds ip's word w.  A repeat test that kept one of its halves
    alone (the 16-bit one for a b a b, the byte one for a b c a) would count runs of a here (srcLen 5, one a before the candidate)
    and step over the only match"""
    five = _word_then_collider(kind)
    L = _Lay(13)
    L.rnd(5); L.put(five[:1] + five + _not(five[0])); L.rnd(9); L.put(five[:4] + five[:1] + _not(five[0])); L.rnd(13)
    return Case(name, L.data(), {})


def _four_differ(name):
    """two neighbouring words of the hash of b b b b, then a run of b: its walk starts on the second, whose chain delta is 1"""
    five, b = _run_collider()
    L = _Lay(7)
    L.rnd(5); L.put(five); L.rnd(9); L.put(b * 30); L.rnd(13)
    return Case(name, L.data(), {})


def _run_end(name, room, first=10):
    """a short run, other bytes, and the same byte to the end of the input: the source run is counted up to ihigh, `room` bytes
    behind its first four"""
    return _raw(name, _rnd(room, 5), b"e" * first, _rnd(room + 1, 7), b"e" * (MINMATCH + room + LASTLIT))


def _chunks(name, size, seed=10):
    """a text of more than 4096 bytes behind its own pieces: `size` bytes from every `stride`-th position, each stored once between
    other bytes.  Every position of the text has a match, none longer than `size`: one series of matches up to the price table's end"""
    L = _Lay(seed + size)
    stride = size // 4
    T = L.bytes(K_OPT_NUM + 300)
    for a in range(0, len(T) - size, stride):
        L.put(T[a:a + size]); L.rnd(3)
    L.put(T); L.rnd(13)
    return Case(name, L.data(), {})


def _text(seed, n, words=24):
    rng = np.random.default_rng([seed, n])
    ws = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(words)]
    return np.frombuffer(b" ".join(ws[i] for i in rng.integers(0, words, n)), np.uint8)[:n].copy()


def _long_first(name, first, second, at, seed=8):
    """a first match of `first` bytes, and at offset `at` inside it a match of `second`"""
    L = _Lay(seed)
    s, y = L.bytes(first), L.bytes(second)
    L.put(s); L.rnd(30); L.put(s[at:] + y); L.rnd(30); L.put(s[:at + 8] + _not(s[at + 8])); L.rnd(9); L.put(s + y[:0]); L.rnd(3)
    L.put(s[:at] + s[at:] + y); L.rnd(13)
    return Case(name, L.data(), {})


def _lit_ml(name, lits, ml, seed=9):
    """sequences with literal runs `lits` in front of matches of `ml` bytes"""
    L = _Lay(seed + sum(lits) + sum(ml))
    S = [L.bytes(m) + b"" for m in ml]
    for s in S:
        L.put(s); L.rnd(1)
    for i, (r, s) in enumerate(zip(lits, S)):
        L.rnd(max(r - (L.n if i == 0 else 0), 0)); L.put(s)
    L.rnd(7)
    return Case(name, L.data(), {})


# seeds of hs._mix and _text found by a bounded search for the keys of the optimal parser the built cases do not reach
MIX = ((116, 700, 2), (361, 700, 0), (59, 120, 2), (165, 700, 0), (85, 300, 1), (7, 1500, 1), (11, 2500, 2), (3, 3000, 0))
TEXT = ((1, 1200), (2, 5000), (5, 20000))


@functools.lru_cache(None)
def cases():
    by = {c.name: c for c in hs.cases()}
    out = [by[k] for k in ("n0", "n1", "n12", "n13", "n14", "n75", "n76", "n77", "run", "period2", "period3", "period4", "zeros2k",
                           "fold10", "fold10_twice", "tie_cached", "tie_cached3", "longer_is_older", "back_cand5", "back_cand20",
                           "back_lookback", "behind1", "behind8", "behind127", "behind128", "lits0", "lits14_15", "lits270_271", "flush",
                           "dist65535_lead17", "dist65536_lead17")]
    for v in (0, 1, 15, 16, 59, 60, 61, 62, 63, 64, 65, 124, 125, 270):
        out.append(hs._chain(f"fwd{v}", 0, fwd=v, lead=3))
    for b in (0, 1, 63, 64, 65, 130):
        out.append(hs._back(f"back{b}", b))
    out += [_wide("wide_room1023", 500, 1023), _wide("wide_lane0_lo", 5, 1024), _wide("wide_lane63_hi", 1019, 1024),
            _wide("wide_mid_hi", 520, 1025), _wide("wide_none", 1500, 2100), _wide("wide_end", 3000, 1024), _wide("wide_end_tail", 3000, 1400),
            _wide("narrow_end", 300, 100), _wide("wide_room1025_end", 3000, 1025)]
    out += [_same_word("same95", 95), _same_word("same96", 96), _same_word("same97", 97), _same_word("same255", 255), _same_word("same257", 257),
            _same_word("same511", 511), _same_word("same513", 513)]
    out += [_clusters("clusters"), _ring_swap("ring_swap"), _far_run("far_run"), _swap_late("swap_late")]
    out += [_runs("run_at_0", (300,), gap=0), _runs("runs_short", (4, 5, 6, 9, 20, 19, 68, 67, 69, 5)), _runs("runs_grow", (5, 9, 17, 40, 300, 60, 2000, 6)),
            _runs("runs_shrink", (1500, 200, 132, 68, 67, 20, 8)), _runs("runs_4100", (4100, 4200, 30), byte=b"\x00"),
            _runs("runs_nogap", (70, 1, 1100, 1, 1030), gap=1)]
    out += [_not_pattern("not_pattern_plain", "plain"), _not_pattern("not_pattern_abab", "abab"), _not_pattern("not_pattern_abca", "abca"),
            _holds_word("period2_holds_word", "abab"), _holds_word("abca_holds_word", "abca")]
    out += [_four_differ("four_differ"), _run_end("run_end1023", 1023), _run_end("run_end1024", 1024), _run_end("run_end1025", 1025), _run_end("run_end90", 90),
            _raw("run_lane63", _rnd(1, 5), b"e" * 10, _rnd(2, 7), b"e" * 1016, _rnd(3, 40)),
            _raw("run_from_0", b"e" * 10, _rnd(4, 7), b"e" * 30, _rnd(5, 13))]
    out += [_chunks(f"chunks{v}", v) for v in (63, 64, 65, 128)]
    out += [hs._chain("fwd187", 0, fwd=187, lead=3), hs._chain("fwd4091", 0, fwd=4091, lead=3), _same_word("same700", 700),
            _long_first("first200_5000", 200, 5000, 18), _lit_ml("lit268_ml20", (267, 268, 269, 268), (20, 21, 22, 23)),
            _lit_ml("ml19_between14", (30, 14, 14), (30, 19, 30)), _lit_ml("ml274_between14", (30, 14, 14), (30, 274, 30)),
            _long_first("first40_in128", 40, 106, 18)]
    out.append(_raw("period2_long", b"\x07\x09" * 700, _rnd(1, 13)))
    out += [_long_first("first63_in", 63, 20, 18), _long_first("first64_in", 64, 30, 18), _long_first("first128_in", 128, 40, 18),
            _long_first("first200_4082", 200, 4082 - 182, 18), _long_first("first65", 65, 10, 30), _long_first("first129", 129, 10, 30)]
    out += [_lit_ml("lit15_ml19", (60, 12, 13, 15, 16), (17, 18, 19, 20, 21)), _lit_ml("lit270_ml274", (267, 268, 270, 530), (272, 273, 274, 275)),
            _lit_ml("ml_kib", (40,), (5000,))]
    out += [Case(f"mix{k}_{s}_{n}", hs._mix(s, n, k), {}) for s, n, k in MIX]
    out += [Case(f"text{s}_{n}", _text(s, n), {}) for s, n in TEXT]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def cases_of(level):
    """level 9 runs the level 1..8 catalogue as well"""
    if level != 9: return cases()
    mine = {c.name for c in cases()}
    return cases() + tuple(c for c in hs.cases() if c.name not in mine)


# ---- ledger -----------------------------------------------------------------------------------------------------------------------
LENS = (0, 1, 15, 16, 63, 64, 65)
BACKS = (0, 1, 63, 64, 65)


def _count_keys(pre, room, f, ended):
    """the path of ho_count / ho_run for a count of `f` with lim - a = room (lz4hc_opt_encode.hip:86-108, :126-149)"""
    keys = set()
    if f in LENS: keys.add(f"{pre}={f}")
    if room in (K_WIDE - 1, K_WIDE, K_WIDE + 1): keys.add(f"{pre}:lim-a={room}")
    if room >= K_WIDE:
        if f >= K_WIDE: keys.add(f"{pre}:wide:no-mismatch")
        else:
            lane, byte = divmod(f, K_LANE_BYTES)
            keys.add(f"{pre}:wide:lane" + ("0" if lane == 0 else "63" if lane == K_LANES - 1 else "-mid"))
            keys.add(f"{pre}:wide:byte" + ("<8" if byte < 8 else ">=8"))
    if ended: keys.add(f"{pre}:end-ihigh:" + ("after-wide" if room >= K_WIDE else "narrow"))
    return keys


def _prev_same_hash(h):
    """for every position, the nearest earlier position with its hash (-1: none)"""
    order = np.argsort(h, kind="stable")
    prev = np.full(len(h), -1, np.int64)
    same = h[order][1:] == h[order][:-1]
    prev[order[1:][same]] = order[:-1][same]
    return prev


def _insert_keys(d, S):
    keys = set()
    h = hs.hashes(d)
    prev = _prev_same_hash(h)
    ntu, ip = S[:, 9].astype(np.int64), S[:, 1].astype(np.int64)
    if (ntu > ip).any(): keys.add("ins:ntu>ip")
    if (ntu == ip).any(): keys.add("ins:empty")
    span = ip - ntu
    if (span >= K_LANES).any(): keys.add("ins:full-step")
    for v in (1, 63):
        if ((span > 0) & (span % K_LANES == v)).any(): keys.add(f"ins:partial={v}")
    if (ip > K_RING).any(): keys.add("ins:pos>=65536")

    def first_of_hash(p, start):
        """p: positions that are the first of their hash in a step starting at `start`"""
        q = prev[p]
        dl = p - q
        if (q < 0).any(): keys.add("ins:delta:empty-head")
        if ((q >= 0) & (dl < K_LANES)).any(): keys.add("ins:delta<64")
        if ((q >= 0) & (dl == K_MAXDIST)).any(): keys.add("ins:delta=65535")
        if ((q >= 0) & (dl == K_MAXDIST + 1)).any(): keys.add("ins:delta=65536:clamped")
    one = span == 1
    first_of_hash(ntu[one], None)
    for a, b in zip(ntu[span > 1].tolist(), ip[span > 1].tolist()):
        for g in range(a, b, K_LANES):
            e = min(g + K_LANES, b)
            grp = h[g:e]
            vals, idx, cnt = np.unique(grp, return_index=True, return_counts=True)
            first_of_hash(g + idx, g)
            if (cnt == 2).any(): keys.add("ins:same=2")
            if (cnt == 3).any(): keys.add("ins:same=3")
            if (cnt >= 8).any(): keys.add("ins:same>=8")
            if (cnt == K_LANES).any(): keys.add("ins:same=64")
            if (cnt >= 2).sum() >= 2: keys.add("ins:two-shared")
            if e - g < K_LANES and (cnt >= 2).any(): keys.add("ins:same:in-partial-step")
            low = vals.astype(np.int64) & (K_SCORE - 1)
            for s in np.unique(low):
                m = np.flatnonzero(low == s)
                if len(m) < 2: continue
                keys.add("ins:fold10")
                later = m[np.argmax(idx[m])]                    # the hash whose first lane is the latest among those of the slot
                if cnt[later] == 1 and prev[g + idx[later]] >= 0 and idx[later] > idx[m].min(): keys.add("ins:fold10:later-alone-reads-head")
    return keys


def _keys(c, level, t):
    keys = set()
    d, n = c.data, len(c.data)
    S, Cd, E, M = t.search, t.cand, t.arm, t.emit
    high = n - LASTLIT
    if n <= 14: keys.add(f"n={n}")
    if len(S): keys |= _insert_keys(d, S)
    first = np.concatenate([[0], np.cumsum(S[:, 4])]) if len(S) else np.zeros(1, np.int64)
    for e in np.unique(S[:, 5]) if len(S) else (): keys.add(f"end:{END[int(e)]}")
    # candidates
    if len(Cd):
        probe, eq4 = Cd[:, 1] == 1, Cd[:, 2] == 1
        if (~probe).any(): keys.add("probe:failed")
        if (probe & ~eq4).any(): keys.add("probe:passed:four-differ")
        if (probe & eq4).any(): keys.add("probe:passed:match")
        owner = np.repeat(np.arange(len(S)), S[:, 4])
        ips, lows = S[owner, 1], S[owner, 2]
        used = probe & eq4
        for i in np.flatnonzero(used):
            ip, low = int(ips[i]), int(lows[i])
            pos, _, _, f, b, fs, bs, left = (int(x) for x in Cd[i])
            keys |= _count_keys("fwd", high - (ip + MINMATCH), f, fs == 1)
            if ip - pos == K_MAXDIST: keys.add("dist=65535:candidate")
            if ip > low:
                if b in BACKS: keys.add(f"back={b}")
                if b >= 128: keys.add("back>=128")
                keys.add("back-stop:" + ("mismatch", "lookback", "cand")[bs])
        for v in np.unique(Cd[:, 7]): keys.add("left:" + ("chain", "swap", "pattern", "break", "chain-at-matchChainPos")[int(v)])
    # winners, ties, distances
    for i in np.flatnonzero(S[:, 6] >= 0) if len(S) else ():
        _, ip, low, lin, walked, end, win, lout, nxt, _, by_pa, _ = (int(x) for x in S[i])
        cd = Cd[first[i]:first[i] + walked]
        if by_pa: continue
        ml = MINMATCH + cd[:, 3] + cd[:, 4]
        tied = np.flatnonzero((cd[:, 1] == 1) & (cd[:, 2] == 1) & (ml == lout))
        if len(tied) >= 2 and tied[0] == win: keys.add("tie:first-kept")
        if ip - int(cd[win, 0]) == K_MAXDIST: keys.add("dist=65535:taken")
    if "dist" in c.marks and c.marks["dist"] == K_MAXDIST + 1:
        p = c.marks["probe"]
        i = np.flatnonzero((S[:, 1] == p) & (S[:, 2] == p))
        if len(i):
            i = int(i[0]); cd = Cd[first[i]:first[i] + S[i, 4]]
            if not (p - cd[:, 0] == K_MAXDIST + 1).any() and S[i, 6] < 0: keys.add("dist=65536:out-of-reach")
    # events
    for row in E.tolist():
        k = row[0]
        if k < 32: keys.add(f"arm:{hs.ARMS[k]}")
        elif k < 40: keys.add(f"refuse:{hs.REFUSE[k]}@{SITE[row[2]]}")
        elif k == EV_SWAP:
            _, ip, m, end, seen, widest, far, at, outcome, last_at = row[:10]
            keys.add(f"swap:{SWAP[outcome]}")
            if outcome:
                keys.add("swap:end" + ("=1" if end == 1 else "=2..64" if end <= 64 else "=65..128" if end <= 128 else ">1024" if end > 1024 else "=129..1024"))
                if widest >= 2: keys.add("swap:step>=2")
                if (m & 0xFFFF) + last_at >= K_RING: keys.add("swap:crosses-ring-wrap")
        elif k == EV_PA:
            _, ip, cp, rep, src_run, fwd, back_all, back, arm, fresh, flags = row[:11]
            keys.add(f"pa:{PA[arm]}")
            if fresh: keys.add("pa:state:" + ("confirmed" if rep == 2 else "not-pattern"))
            if arm == 0 and fresh:                          # which half of the repeat test (lz4hc_opt_core.h:118) refused ip's word
                w = d[ip:ip + 4]
                halves, ends = bool(w[0] == w[2] and w[1] == w[3]), bool(w[0] == w[3])
                if halves and not ends:
                    keys.add("pa:not-pattern:two-byte-period")
                    if np.array_equal(d[cp:cp + 4], w): keys.add("pa:not-pattern:two-byte-period:candidate-holds-word")
                if ends and not halves:
                    keys.add("pa:not-pattern:outer-bytes-equal")
                    if np.array_equal(d[cp:cp + 4], w): keys.add("pa:not-pattern:outer-bytes-equal:candidate-holds-word")
                if not ends and not halves: keys.add("pa:not-pattern:plain")
            if arm in (3, 4, 5, 6, 7, 8):
                keys |= _count_keys("run", high - (ip + 4), src_run - 4, ip + src_run == high)
                keys |= _count_keys("run", high - (cp + 4), fwd - 4, cp + fwd == high)
                if back_all in BACKS: keys.add(f"runback={back_all}")
                if back_all >= 128: keys.add("runback>=128")
                if flags & 1: keys.add("runback:clamped-by-lowest")
                if flags & 2: keys.add("runback:to-position-0")
        elif k in EV_OPT:
            nm = EV_OPT[k]
            if nm == "first":
                keys.add("opt:first")
                if row[4]: keys.add("opt:first=sufficient")
                if row[2] >= 64: keys.add("opt:first>=64")
            elif nm == "skip":
                keys.add("opt:skip" + (":both" if row[4] == 1 else ""))
            elif nm == "update":
                _, ip, cur, base, ml, rose, beyond, cheaper, refused, lit_better = row[:10]
                keys.add(f"opt:update:base={BASE[base]}")
                if ml in (4, 63, 64, 65): keys.add(f"opt:update:ml={ml}")
                if ml >= 128: keys.add("opt:update:ml>=128")
                keys.add("opt:update:last-" + ("rose" if rose else "stayed"))
                if beyond: keys.add("opt:update:written:beyond-last+3")
                if cheaper: keys.add("opt:update:written:price<=")
                if refused: keys.add("opt:update:refused")
                if lit_better: keys.add("opt:update:literal-improved")
                if ml >= 19: keys.add("opt:ml-crosses-19")
                if ml >= 274: keys.add("opt:ml-crosses-274")
            elif nm == "series":
                _, ip, hops, between, starts_lit, last, matches, lit_lo, lit_hi = row[:9]
                if hops >= 3: keys.add("opt:series:hops>=3")
                if between: keys.add("opt:series:literals-between")
                if starts_lit: keys.add("opt:series:starts-with-literal")
                if lit_lo < 15 <= lit_hi: keys.add("opt:lit-crosses-15")
                if lit_lo < 270 <= lit_hi: keys.add("opt:lit-crosses-270")
            else: keys.add(f"opt:{nm}")
    # a matchChainPos in use: a chain step of a candidate walked after the swap that set it (oracle.h ORC_HX_LEFT_CHAIN_SWAPPED)
    if len(Cd) and (Cd[:, 7] == 4).any(): keys.add("swap:chain-step-at-matchChainPos")
    # emit
    seq = M[M[:, 1] > 0]
    for col, nm, base in ((0, "lit", 0), (1, "ml", MINMATCH)):
        v = seq[:, col] - base
        for lo, hi, tag in ((0, 0, "0"), (1, 14, "1..14"), (15, 15, "15"), (16, 269, "16..269"), (270, 270, "270"), (525, 1 << 30, ">=525")):
            if ((v >= lo) & (v <= hi)).any(): keys.add(f"emit:{nm}:{tag}")
    if (seq[:, 1] >= 4096).any(): keys.add("emit:ml:KiB")
    for v in (1, K_MAXDIST):
        if (seq[:, 2] == v).any(): keys.add(f"emit:off={v}")
    return keys


def _refusals(c, level):
    keys = set()
    for cap in caps(c.data, level)[1:]:
        a = trace(c.data, level, cap).arm
        for row in a[(a[:, 0] >= 32) & (a[:, 0] < 40)].tolist():
            keys.add(f"refuse:{hs.REFUSE[row[0]]}@{SITE[row[2]]}")
    return keys


def ledger(case_list=None, levels=LEVELS, refusals=True, walked=None):
    """key -> names of the cases that reach it.  case_list None: cases_of(level).  walked: a dict that receives candidates walked per
    (case, level)"""
    led = collections.defaultdict(list)
    for lv in levels:
        for c in (cases_of(lv) if case_list is None else case_list):
            t = trace(c.data, lv)
            if walked is not None: walked[c.name, lv] = int(t.search[:, 4].sum())
            keys = _keys(c, lv, t)
            if refusals and len(c.data) <= BIG: keys |= _refusals(c, lv)
            for k in keys: led[f"L{lv}:{k}"].append(c.name)
    return dict(led)


def _required():
    req = set()
    count = lambda pre: ({f"{pre}={v}" for v in LENS} | {f"{pre}:lim-a={v}" for v in (1023, 1024, 1025)} | {f"{pre}:wide:{k}" for k in ("lane0", "lane-mid", "lane63", "byte<8", "byte>=8", "no-mismatch")} |
                         {f"{pre}:end-ihigh:after-wide", f"{pre}:end-ihigh:narrow"})
    for lv in LEVELS:
        per = {f"n={n}" for n in (0, 1, 12, 13, 14)}
        per |= {"ins:full-step", "ins:partial=1", "ins:partial=63", "ins:empty", "ins:same=2", "ins:same=3", "ins:same>=8", "ins:same=64", "ins:two-shared",
                "ins:fold10:later-alone-reads-head", "ins:delta:empty-head", "ins:delta<64", "ins:delta=65535", "ins:delta=65536:clamped", "ins:pos>=65536"}
        per |= count("fwd") | count("run")
        per |= {f"runback={v}" for v in BACKS} | {"runback>=128", "runback:to-position-0", "runback:clamped-by-lowest"}
        per |= {"end:attempts", "end:lowest", "end:chain", "probe:failed", "probe:passed:four-differ", "probe:passed:match", "tie:first-kept",
                "dist=65535:taken", "dist=65536:out-of-reach"}
        per |= {f"pa:{v}" for v in PA.values() if v != "swapped"} | {"pa:state:confirmed", "pa:state:not-pattern", "pa:not-pattern:plain", "pa:not-pattern:two-byte-period",
                                                                         "pa:not-pattern:two-byte-period:candidate-holds-word", "pa:not-pattern:outer-bytes-equal",
                                                                         "pa:not-pattern:outer-bytes-equal:candidate-holds-word"}
        per |= {f"emit:{nm}:{tag}" for nm in ("lit", "ml") for tag in ("0", "1..14", "15", "16..269", "270", ">=525")} | {"emit:ml:KiB", "emit:off=1", "emit:off=65535"}
        if lv == 9:
            per |= {"ins:ntu>ip"} | {f"back={v}" for v in BACKS} | {"back>=128", "back-stop:mismatch", "back-stop:lookback", "back-stop:cand"}
            per |= {f"arm:{a}" for a in hs.ARMS.values()}
            per |= {f"refuse:{r}@chain" for r in ("literals", "matchlen", "last")}
        else:
            per |= {f"swap:{v}" for v in SWAP.values()} | {"swap:end=1", "swap:end=2..64", "swap:end=65..128", "swap:end>1024", "swap:step>=2",
                                                           "swap:chain-step-at-matchChainPos", "pa:swapped", "swap:crosses-ring-wrap"}
            per |= {f"opt:{v}" for v in ("no-match", "first-now", "first=sufficient", "at-mflimit", "no-longer", "inner-now:enough", "inner-now:4096",
                                         "first>=64", "series:hops>=3", "series:starts-with-literal", "series:literals-between",
                                         "lit-crosses-15", "lit-crosses-270", "ml-crosses-19", "ml-crosses-274")}
            per |= {f"opt:update:base={v}" for v in BASE.values()} | {f"opt:update:ml={v}" for v in (4, 63, 64, 65)} | {"opt:update:ml>=128"}
            per |= {"opt:update:last-rose", "opt:update:last-stayed", "opt:update:written:beyond-last+3", "opt:update:written:price<=", "opt:update:refused",
                    "opt:update:literal-improved"}
            per |= {"opt:skip:both", "opt:search-anyway"} if lv == 12 else {"opt:skip"}
            per |= {f"refuse:{r}@{s}" for r in ("literals", "matchlen") for s in ("first", "series")} | {"refuse:last@series"}
        req |= {f"L{lv}:{k}" for k in per}
    return req


# keys that no input reaches, or none inside the caps, with the reason; tests/test_hc_opt_shapes_cpu.py asserts that no case reaches one
_NO_DICT = "a table index is position + 65536 and a chain delta is at most 65535, so a delta never exceeds the index without a dictionary"
UNREACHED = {}
for _lv in LEVELS:
    UNREACHED[f"L{_lv}:pa:break:delta"] = _NO_DICT
    UNREACHED[f"L{_lv}:pa:break:distance"] = "the backward run is clamped at `lowest` (lz4hc.c:373), so the segment's start is never more than 65535 behind ip"
    UNREACHED[f"L{_lv}:end:break"] = "both breaks of the walk are unreachable (pa:break:*, swap:break)"
    if _lv >= 10: UNREACHED[f"L{_lv}:swap:break"] = _NO_DICT
    else:
        for _a in hs.UNREACHED_ARMS: UNREACHED[f"L{_lv}:arm:{_a}"] = "as at levels 1..8 (DESIGN_NOTES.md, the HC / Medium catalogue)"
    if _lv >= 10: UNREACHED[f"L{_lv}:pa:to-start:lookback"] = "the optimal parser searches forward only: the lookback is 0"
    if _lv >= 10: UNREACHED[f"L{_lv}:opt:update:literal-improved"] = ("not reached by this catalogue nor by 7500 seeded low-entropy inputs (hs._mix, seeds 0..1499, five shapes): "
                                                                        "a record is a literal dearer than its neighbour only behind last_match_pos, where the search never stands")
UNREACHED["L9:ins:ntu>ip"] = "search positions only grow at level 9 as at levels 1..8 (DESIGN_NOTES.md, stepping back); the same 7500 inputs reach none"
UNREACHED["L12:end:attempts"] = "16384 candidates of one hash inside 65535 bytes, each walked: beyond the candidates-walked cap"
UNREACHED["L10:opt:update:ml=65"] = UNREACHED["L10:opt:update:ml>=128"] = "a match above sufficient_len = 64 is encoded at once"
UNREACHED["L10:opt:ml-crosses-274"] = UNREACHED["L11:opt:ml-crosses-274"] = "a match above sufficient_len (64, 128) is encoded at once"
REQUIRED = frozenset(_required() - set(UNREACHED))


# ---- what the GPU test launches -----------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def expected(level):
    """[(label, data, cap, result, bytes)] for level 9..12"""
    out = []
    for c in cases_of(level):
        for cap in caps(c.data, level):
            r, b = port(c.data, level, cap)
            out.append((f"{c.name}|cap={cap}", c.data, cap, r, b))
    return tuple(out)
