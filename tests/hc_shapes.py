"""Inputs that walk every search and parse shape of the LZ4 HC kernel at levels 1..8 (4mc_amd/csrc/lz4hc_encode.hip) and of the
4mc Medium kernel (lz4mc_encode.hip), for the encoder tests (plain module, like lz4_shapes.py; numpy + the oracle port's trace).

  cases()         the deterministic HC input set: named inputs, each as small as its key allows.  mc_cases(): the same for Medium.
  trace()         what the oracle port's search and parse did on one input (oracle.h: orc_trace), as numpy tables.
  ledger()        the keys a case set reaches, computed from that trace, the input's hashes and the kernels' constants below.
  REQUIRED        the keys the set must reach, per level where the level changes the answer.  A missing key is a test failure.
  caps()          the capacities one input runs at: bound, n-1, r, r-1, r-6, n/2 (r = the port's size of it at that level).
  expected()      every (input, capacity) pair of one level with the port's result and bytes: what the GPU test launches.

Colliding words (same 15-bit hash, different bytes) come from enumerating 2^23 consecutive 32-bit values: 256 per bucket on average.
A builder places them so that the chain walked from a probe position holds exactly the words meant, and checks that itself by
hashing every position of the input; the ledger then reads the walk off the port's trace, so a key is never taken on trust."""
import collections
import ctypes as C
import functools

import numpy as np

import helpers

# ---- constants the kernels branch on (4mc_amd/csrc) -----------------------------------------------------------------------------
ATTEMPTS = {1: 2, 2: 2, 3: 4, 4: 8, 5: 16, 6: 32, 7: 64, 8: 128}       # lz4hc_encode.hip:616 (lz4hc.c:817-827)
LEVELS = tuple(ATTEMPTS)
K_WINK = 8                      # lz4hc_encode.hip:42   candidates cached per position of the look-ahead window
K_FWD, K_BACK = 32, 16          # lz4hc_encode.hip:62-63, 216-217   bytes measured ahead of time after the four / before
K_STEP = 64                     # lz4hc_encode.hip:333  candidates per rest-of-chain step
K_RFWD, K_RBACK = 32, 32        # lz4hc_encode.hip:340-358   bytes measured per candidate there before the wave-wide count
K_WIDE = 1024                   # lz4hc_encode.hip:158  the wide compare of wave_count_fwd; below it 64 bytes per step (:167)
K_SCORE = 1024                  # lz4hc_encode.hip:39   folded scoreboard of one 64-position insert step (:127)
K_CHAINMASK = 0x1FFFF           # lz4hc_encode.hip:40   chain deltas of the last 128 Ki positions
K_RING = 3                      # lz4hc_encode.hip:75   look-ahead windows in LDS
K_GROUP = 64                    # lz4hc_encode.hip:120-149, 442   positions per insert step and per window
K_WIDE_F = 36                   # lz4hc_encode.hip:214  q + 36 <= n: the 32 forward bytes are read as two 16-byte words
K_INS_END = 3                   # lz4hc_encode.hip:209  positions below n - 3 enter the tables
K_TABLES_ONLY = 192             # lz4hc_encode.hip:452  v + 1 < keep: a match that carries the parser K_RING windows on
K_MAXDIST, K_IDX0 = 65535, 65536       # lz4hc_encode.hip:36-37
MC_ATTEMPTS = 4                 # lz4mc_encode.hip:27
MC_STRIDE = 64                  # lz4mc_encode.hip:69, 120   step = tries++ >> 6 with tries = 64 after a match
MC_CHAIN = 65536                # lz4mc_encode.hip:28   chain deltas of the last 64 Ki positions
MFLIMIT, LASTLIT, MINMATCH = 12, 5, 4  # lz4hc_encode.hip:38

END_ATTEMPTS, END_LOWEST, END_CHAIN = 1, 2, 3                  # oracle.h ORC_END_*
ARMS = {1: "no-search2", 2: "ml1", 3: "restore0", 4: "drop1", 5: "s3-near", 6: "s3-clamp", 7: "s3-tail", 8: "s3-correct", 9: "s3-far",
        10: "no-search3", 11: "ml12", 12: "ml12-cut", 13: "seq3-is-1", 14: "seq3-is-1-cut2", 15: "seq3-is-1-2", 16: "drop2", 17: "three",
        18: "three-near", 19: "three-clamp", 20: "three-tail", 21: "three-correct", 22: "three-far"}       # oracle.h ORC_ARM_*
REFUSE = {32: "literals", 33: "matchlen", 34: "last"}          # oracle.h ORC_REFUSE_*
SHARE = {1 | 8: "ntu-prev", 2 | 16: "ntu-ip", 4 | 32: "prev-ip"}        # oracle.h ORC_SHARE_* | ORC_DIFF_*

Case = collections.namedtuple("Case", "name data marks")


# ---- the port and its trace -------------------------------------------------------------------------------------------------------
class _Trace(C.Structure):
    _fields_ = [("ev", C.POINTER(C.c_int32) * 4), ("cap", C.c_int * 4), ("n", C.c_int * 4)]


Trace = collections.namedtuple("Trace", "result out search cand arm emit")


def _lib():
    L = helpers.oracle()
    L.orc_lz4hc_compress_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]; L.orc_lz4hc_compress_ex.restype = C.c_int
    L.orc_lz4mc_compress_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]; L.orc_lz4mc_compress_ex.restype = C.c_int
    return L


def bound(n):
    return n + n // 255 + 16


def trace(data, level, cap=None, arm_rows=None):
    """level 1..8: orc_lz4hc_compress_ex; level 'mc': orc_lz4mc_compress_ex (cap None: LZ4_compressMC, no limit).
    arm_rows: one run that keeps the arm table alone, of at most that many rows."""
    L = _lib()
    data = np.ascontiguousarray(data, np.uint8)
    n = len(data)
    dst = np.zeros(bound(n) + 64, np.uint8)
    widths = (11 if level == "mc" else 9, 4, 2, 3)

    def run(t):
        if level == "mc":
            return L.orc_lz4mc_compress_ex(data.ctypes.data, dst.ctypes.data, n, -1 if cap is None else cap, C.byref(t))
        return L.orc_lz4hc_compress_ex(data.ctypes.data, dst.ctypes.data, n, bound(n) if cap is None else cap, level, C.byref(t))
    t = _Trace()
    if arm_rows is None: run(t)
    else: t.n[2] = 2 * arm_rows
    bufs = [np.zeros(max(t.n[k], 1), np.int32) for k in range(4)]
    t2 = _Trace()
    for k in range(4):
        t2.ev[k] = bufs[k].ctypes.data_as(C.POINTER(C.c_int32)); t2.cap[k] = len(bufs[k])
    r = run(t2)
    tabs = [bufs[k][:min(t2.n[k], t.n[k])].reshape(-1, widths[k]) for k in range(4)]
    return Trace(r, dst[:max(r, 0)].copy(), *tabs)


def port(data, level, cap):
    """(result, bytes) of the port: level 1..8 -> LZ4_compress_HC; 'mc' -> LZ4_compressMC (cap < 0) / _limitedOutput"""
    return helpers.orc_compress_mc(data, cap) if level == "mc" else helpers.orc_compress_hc(data, level, cap)


def caps(data, level):
    n = len(data)
    r = port(data, level, -1 if level == "mc" else bound(n))[0]
    want = [-1 if level == "mc" else bound(n), n - 1, r, r - 1, r - 6, n // 2]
    out = []
    for c in want:
        c = c if c == -1 and level == "mc" else max(c, 0)
        if c not in out: out.append(c)
    return out


# ---- words ------------------------------------------------------------------------------------------------------------------------
def hash15(words):
    return ((np.asarray(words).astype(np.uint64) * 2654435761) & 0xFFFFFFFF) >> 17       # lz4hc_encode.hip:56, lz4mc_encode.hip:30


def hashes(data):
    """hash of the four bytes at every position that has four"""
    if len(data) < 4: return np.zeros(0, np.uint64)
    d = np.asarray(data).astype(np.uint32)
    return hash15(d[:-3] | (d[1:-2] << 8) | (d[2:-1] << 16) | (d[3:] << 24))


@functools.lru_cache(None)
def _enumerated():
    v = np.arange(1 << 23, dtype=np.uint32) + np.uint32(0x61000000)
    b = v.view(np.uint8).reshape(-1, 4)
    s = np.sort(b, axis=1)
    v = v[(s[:, 1:] != s[:, :-1]).all(axis=1)]                 # four different bytes: a word never overlaps a copy of itself
    h = hash15(v)
    order = np.argsort(h, kind="stable")
    return v[order], np.searchsorted(h[order], np.arange(32769))


def bucket(b, count):
    """`count` different words of hash `b`, as bytes"""
    v, starts = _enumerated()
    w = v[starts[b]:starts[b + 1]]
    assert len(w) >= count, (b, len(w))
    return [int(x).to_bytes(4, "little") for x in w[:count]]


B0, B1 = 0x1234, 0x2A51          # two buckets of more than 129 words each; B0 ^ 1024 folds onto B0 in the scoreboard


class _Lay:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed); self.parts = []; self.n = 0

    def put(self, b):
        pos = self.n; self.parts.append(bytes(b)); self.n += len(b)
        return pos

    def bytes(self, k):
        return self.rng.integers(0, 256, k, dtype=np.uint8).tobytes()

    def rnd(self, k):
        return self.put(self.bytes(k))

    def data(self):
        return np.frombuffer(b"".join(self.parts), np.uint8).copy()


def _seeded(build, buckets=(B0,), tries=400, clean=True):
    """the first seed at which exactly the positions the builder names carry the buckets' hashes (clean = False: seed 0 as it
    comes - an input too large for that; the ledger reads its keys off the trace all the same)"""
    for seed in range(tries):
        data, marks, want = build(seed)
        if not clean: return data, marks
        h = hashes(data)
        got = sorted(np.flatnonzero(np.isin(h, list(buckets))).tolist())
        if got == sorted(want): return data, marks
    raise AssertionError("no clean seed")


def _not(b):
    return bytes([b ^ 0xFF])


# ---- builders ---------------------------------------------------------------------------------------------------------------------
def _chain(name, ncol, fwd=8, ahead=(), end=None, lead=0):
    """source W + `fwd` bytes [+ `ahead`: further sources (fwd, colliders before it)], `ncol` colliding words, then the probe: W + the
    same bytes.  end = k: the input ends so that the match stops at matchlimit after k bytes beyond the four."""
    def build(seed):
        L = _Lay(seed)
        words = bucket(B0, 130)
        W, cols = words[0], iter(words[1:])
        body = L.bytes(max([fwd] + [a[0] for a in ahead]) + 8)
        want = []
        if lead: L.rnd(lead)
        want.append(L.put(W + body[:fwd] + _not(body[fwd])))
        L.rnd(1)
        for f, nc in ahead:
            for _ in range(nc):
                want.append(L.put(next(cols))); L.rnd(1)
            want.append(L.put(W + body[:f] + _not(body[f]))); L.rnd(1)
        for _ in range(ncol):
            want.append(L.put(next(cols))); L.rnd(1)
        probe = L.put(W)
        want.append(probe)
        if end is None:
            L.put(body[:fwd + 1]); L.rnd(13)
        else:
            L.put(body[:end + LASTLIT])
        return L.data(), {"probe": probe}, want
    return Case(name, *_seeded(build))


def _back(name, back, rest=False, stop="mismatch"):
    """source 1 gives a match X at the probe; source 2 holds X from k bytes in and goes on with Y; the second search of the
    arbitration, at probe + |X| - 2, finds source 2 by the word W = X[-2:] + Y[:2] and walks back.  rest: words colliding with W that
    stand ahead of source 2 in that walk (True: K_WINK of them, so that source 2 lies on the rest-of-chain path)."""
    def build(seed):
        L = _Lay(seed)
        words = bucket(B0, 12)
        W, cols = words[0], words[1:]
        W0 = bucket(B1, 130)
        e = 40
        if stop == "mismatch":
            k = 1 if back else 6
            ml = back + 2 + k
        elif stop == "cand":
            ml, k = (30, 23) if back < 16 else (40, 18)
            assert ml - 2 - k == back
        else:
            ml, k = back + 2, 0
        X = (W0[0] if stop == "lookback" else b"") + L.bytes(ml - 2 - (4 if stop == "lookback" else 0)) + W[:2]
        Y = W[2:] + L.bytes(e - 2)
        want = []
        s2 = X[k:] + Y + _not(0)
        if stop == "cand":
            L.put(s2); want.append(len(X) - k - 2)
        else:
            L.rnd(20)
            if stop == "mismatch": L.put(_not(X[k - 1]))
            p = L.put(s2); want.append(p + len(X) - k - 2)
        L.rnd(3)
        if stop == "lookback":
            for c in W0[1:129]:
                L.put(c); L.rnd(1)
        L.put(X + _not(Y[0])); L.rnd(3)
        if rest:
            for c in cols[:K_WINK if rest is True else rest]:
                want.append(L.put(c)); L.rnd(1)
        probe = L.put(X + Y)
        want.append(probe + len(X) - 2)
        L.rnd(13)
        return L.data(), {"probe": probe + len(X) - 2}, want
    return Case(name, *_seeded(build))


def _dist(name, dist, lead, word=None):
    """W + 16 bytes, filler, and the same again `dist` further on, after `lead` bytes.  word = 'collide': the first holds a colliding word"""
    def build(seed):
        L = _Lay(seed)
        words = bucket(B0, 2)
        W = words[0]
        T = L.bytes(16)
        L.rnd(lead)
        a = L.put((words[1] if word == "collide" else W) + T + _not(0))
        L.rnd(dist - 21)
        probe = L.put(W + T + b"\x00")
        assert probe - a == dist
        L.rnd(13)
        return L.data(), {"probe": probe, "dist": dist, "lead": lead}, [a, probe]
    return Case(name, *_seeded(build, tries=4000))


def _far_lowest():
    def build(seed):
        L = _Lay(seed)
        W = bucket(B0, 1)[0]
        T = L.bytes(12)
        a = L.put(W + T[:6] + _not(T[6])); L.rnd(65600)
        b = L.put(W + T + _not(0)); L.rnd(3)
        probe = L.put(W + T + b"\x00"); L.rnd(13)
        return L.data(), {"probe": probe}, [a, b, probe]
    return Case("far_lowest", *_seeded(build))


def _wrap():
    """more than 128 Ki + 64 Ki positions; repeats whose chain entries lie either side of the 128 Ki chain table's wrap (table index =
    position + 64 Ki: positions 65536 and 196608)"""
    def build(seed):
        L = _Lay(seed)
        W = bucket(B0, 4)
        want = []
        L.rnd(65536 - 50)
        for w, at in ((W[0], 65536), (W[1], 196608)):
            L.rnd(at - 50 - L.n)
            T = L.bytes(24)
            want.append(L.put(w + T + _not(0))); L.rnd(80 - 29)
            want.append(L.put(w + T + b"\x00"))
        L.rnd(200 * 1024 - L.n)
        return L.data(), {}, want
    return Case("wrap200k", *_seeded(build, clean=False))


def _fold(name, twice):
    """U and V: different hashes, equal in their low 10 bits, inserted in one aligned group of 64 positions (and U twice when `twice`);
    the longest source of each is the oldest, reached through the deltas written in that group"""
    def build(seed):
        L = _Lay(seed)
        U, U2 = bucket(B0, 2)
        V = bucket(B0 ^ K_SCORE, 1)[0]
        tu, tv = L.bytes(30), L.bytes(30)
        want = []
        L.rnd(3)
        want.append(L.put(U + tu + _not(0))); want.append(L.put(V + tv + _not(0)))
        L.rnd(2 * K_GROUP + 4 - L.n)                           # the next aligned group
        want.append(L.put(U + tu[:6] + _not(tu[6]))); want.append(L.put(V + tv[:6] + _not(tv[6])))
        if twice:
            want.append(L.put(U2 + L.bytes(2))); want.append(L.put(U + tu[:5] + _not(tu[5])))
        assert L.n < 3 * K_GROUP
        L.rnd(4 * K_GROUP - L.n)
        want.append(L.put(U + tu + b"\x00")); want.append(L.put(V + tv + b"\x00"))
        L.rnd(13)
        return L.data(), {}, want
    return Case(name, *_seeded(build, buckets=(B0, B0 ^ K_SCORE)))


def _size(n):
    """a match found by the search at mflimit = n - 12 itself"""
    def build(seed):
        L = _Lay(seed)
        W = bucket(B0, 1)[0]
        T = L.bytes(8)
        a = L.put(W + T); L.rnd(n - 24)
        b = L.put(W + T)
        return L.data(), {}, [a, b]
    return Case(f"n{n}", *_seeded(build))


def _lits(name, runs):
    """sequences with the literal runs `runs` before matches of 12"""
    L = _Lay(len(name) + sum(runs))
    S = [L.bytes(12) for _ in range(len(runs) + 1)]
    for s in S:
        L.put(s); L.rnd(1)
    for i, r in enumerate(runs):
        if i == 0:
            assert r >= L.n
            L.rnd(r - L.n)
        else: L.rnd(r)
        L.put(S[i])
    L.rnd(7)
    return Case(name, L.data(), {})


def _mix(seed, n, kind):
    """low-entropy inputs for the lazy arbitration: matches that overlap, shorten and replace one another"""
    rng = np.random.default_rng([seed, n, kind])
    if kind == 0:
        d = rng.integers(0, int(rng.integers(2, 5)), n, dtype=np.uint8) + 97
    elif kind == 1:
        base = rng.integers(0, 256, int(rng.integers(20, 80)), dtype=np.uint8)
        parts = []
        while sum(map(len, parts)) < n:
            a = int(rng.integers(0, len(base) - 4)); parts.append(base[a:a + int(rng.integers(3, 40))])
            if rng.integers(0, 3) == 0: parts.append(rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8))
        d = np.concatenate(parts)[:n]
    else:
        parts = []
        while sum(map(len, parts)) < n:
            p = rng.integers(97, 100, int(rng.integers(1, 7)), dtype=np.uint8)
            parts.append(np.resize(p, int(rng.integers(4, 60))))
        d = np.concatenate(parts)[:n]
    return np.ascontiguousarray(d, np.uint8)


# seeds of _mix found by a bounded search for the parse arms, refusals and stop reasons the built cases above do not reach
MIX = ((116, 700, 2), (361, 700, 0), (59, 120, 2), (165, 700, 0), (85, 300, 1))


FWD = (0, 31, 32, 33, 95, 96, 97, 32 + 1023, 32 + 1024, 32 + 1025)
BACK_CACHED = (0, 1, 15, 16, 17, 79, 80, 81)
BACK_REST = (31, 32, 33, 95, 96)
WIDER_BEHIND = (1, 2, 3, 4, 7, 8)
BEHIND = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 71, 72, 127, 128)
LITS = (0, 14, 15, 64, 65, 15 + 255, 15 + 256)
MLS = (4, 18, 19, 19 + 254, 19 + 255)


@functools.lru_cache(None)
def cases():
    out = []
    for n in BEHIND:                                                    # attempts, walk lengths, the ninth candidate
        out.append(_chain(f"behind{n}", n))
    out += [_chain("tie_cached", 0, ahead=((8, 0),)), _chain("tie_cached3", 0, ahead=((8, 0), (8, 0))),
            _chain("tie_rest", K_WINK, ahead=((8, 0),)), _chain("tie_both", 0, ahead=((8, K_WINK),)),
            _chain("tie_across_steps", K_WINK + K_STEP - 1, ahead=((8, 0),)),
            _chain("longer_is_older", 0, fwd=20, ahead=((8, 0),)), _chain("longer_is_older_rest", K_WINK, fwd=20, ahead=((8, 0),))]
    for v in FWD + tuple(m - 4 for m in MLS[1:]):
        out.append(_chain(f"fwd{v}", 0, fwd=v, lead=3))
    for v in FWD:
        out.append(_chain(f"fwd{v}_rest", K_WINK, fwd=v, lead=3))
    for nm, v in (("scalar", 10), ("fcap", 29), ("steps64", 32 + 100), ("wide_tail", 32 + K_WIDE + 100), ("wide_exact", 32 + K_WIDE)):
        out.append(_chain(f"end_{nm}", 0, fwd=v + 8, end=v, lead=3))
        out.append(_chain(f"end_{nm}_rest", K_WINK, fwd=v + 8, end=v, lead=3))
    for b in BACK_CACHED:
        out.append(_back(f"back{b}", b))
    for b in BACK_REST:
        out.append(_back(f"back{b}_rest", b, rest=True))
    out += [_back("back_cand5", 5, stop="cand"), _back("back_cand20", 20, stop="cand"), _back("back_lookback", 18, stop="lookback"),
            _back("back_cand20_rest", 20, rest=True, stop="cand"), _back("back_cand5_rest", 5, rest=True, stop="cand")]
    for n in WIDER_BEHIND:                                              # the attempt count of a search that looks back: hc_wider itself at every level
        out.append(_back(f"wider_behind{n}", 17, rest=n))
    for lead in (0, 1, 17, 65600):
        for d in (65534, 65535, 65536):
            out.append(_dist(f"dist{d}_lead{lead}", d, lead))
    out += [_dist("dist65535_collide", 65535, 17, word="collide"), _far_lowest(), _wrap()]
    for nm, d in (("run", b"a"), ("period2", b"ab"), ("period3", b"abc"), ("period4", b"abcd")):
        out.append(Case(nm, np.frombuffer((d * 400)[:331] + b"0123456789xyz", np.uint8).copy(), {}))
    out += [_fold("fold10", False), _fold("fold10_twice", True)]
    for n in (0, 1, 12, 13, 14):
        out.append(Case(f"n{n}", np.frombuffer(b"abcdabcdabcdab"[:n], np.uint8).copy(), {}))
    out += [_size(n) for n in (12 + 63, 12 + 64, 12 + 65)]
    out += [_lits("lits0", (60, 0, 0)), _lits("lits14_15", (60, 14, 15)), _lits("lits64_65", (64, 65, 64)),
            _lits("lits270_271", (270, 271)), _lits("flush", (60, 3, 5))]
    out.append(Case("zeros2k", np.concatenate([np.zeros(2000, np.uint8), np.arange(1, 8, dtype=np.uint8)]), {}))
    out += [Case(f"mix{k}_{s}_{n}", _mix(s, n, k), {}) for s, n, k in MIX]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


# ---- ledger -----------------------------------------------------------------------------------------------------------------------
def _data_keys(c):
    """what the insert step meets, from the input's hashes (lz4hc_encode.hip:118-151)"""
    keys = set()
    d, n = c.data, len(c.data)
    keys.add(f"n={n}" if n <= 14 else "")
    if n < MFLIMIT + 1: return keys - {""}
    h = hashes(d)[:n - K_INS_END]
    for g in range(0, len(h), K_GROUP):
        grp = h[g:g + K_GROUP]
        vals, cnt = np.unique(grp, return_counts=True)
        last = g + K_GROUP >= len(h) and len(grp) < K_GROUP
        if (cnt == 2).any(): keys.add("ins:same-hash:2")
        if (cnt >= 8).any(): keys.add("ins:same-hash:many")
        low = vals & (K_SCORE - 1)
        lv, lc = np.unique(low, return_counts=True)
        if (lc >= 2).any():
            keys.add("ins:fold10")
            shared = lv[lc >= 2]
            if any((cnt[low == s] >= 2).any() for s in shared): keys.add("ins:same-hash+fold10")
        if last and (cnt >= 2).any(): keys.add("ins:partial-last-group")
        if len(grp) == K_GROUP and g + K_GROUP + 4 <= n:
            for p in (1, 2, 3, 4):
                seg = d[g:g + K_GROUP + 4]
                if (seg[p:] == seg[:-p]).all() and not any((seg[q:] == seg[:-q]).all() for q in range(1, p)): keys.add(f"ins:period{p}")
    return keys - {""}


def _search_keys(c, level, t):
    keys = set()
    A = ATTEMPTS[level]
    K = min(A, K_WINK)
    d, n = c.data, len(c.data)
    S, Cd = t.search, t.cand
    first = np.concatenate([[0], np.cumsum(S[:, 4])])
    matchlimit = n - LASTLIT
    # the largest step back of the search position, in windows (hc_acquire's private rebuild needs 2)
    if len(S):
        w = S[:, 1] >> 6
        keys.add(f"stepback:{int((np.maximum.accumulate(w) - w).max())}")
    for e in np.unique(S[S[:, 4] > 0, 5]):
        keys.add({END_ATTEMPTS: "end:attempts", END_LOWEST: "end:lowest", END_CHAIN: "end:chain"}[int(e)])
    # (a search that met no four-byte match, did not run out of attempts and walked no length of interest has no more to say)
    look = (S[:, 6] >= 0) | ((S[:, 5] == END_ATTEMPTS) & (S[:, 4] > 0)) | np.isin(S[:, 4], (8, 9, 72, 73))
    for i in np.flatnonzero(look):
        _, ip, low, lin, walked, end, win, lout, nxt = (int(x) for x in S[i])
        cd = Cd[first[i]:first[i] + walked]
        hit = cd[:, 1] == 1
        lead = int(np.argmax(hit)) if hit.any() else walked
        lookback = ip - low
        if end != END_ATTEMPTS and walked in (8, 9, 72, 73): keys.add(f"walk:exact={walked}")
        if win >= 0 and win == lead and lookback == 0: keys.add(f"att:found:behind={lead}")
        if win < 0 and not hit.any() and end == END_ATTEMPTS and lookback == 0 and bytes(d[nxt:nxt + 4]) == bytes(d[ip:ip + 4]):
            keys.add(f"att:missed:behind={walked}")
        # the same for a search that looks back: an opening search of levels 1..4 is answered when its window is built
        # (lz4hc_encode.hip:229-264, 487-489), these always run hc_wider
        if win >= 0 and win == lead and lookback: keys.add(f"att:wider:found:behind={lead}")
        if win < 0 and not hit.any() and end == END_ATTEMPTS and lookback and bytes(d[nxt:nxt + 4]) == bytes(d[ip:ip + 4]):
            keys.add(f"att:wider:missed:behind={walked}")
        if win >= K_WINK and not hit[:K_WINK].any(): keys.add("cached-all-collide-then-match")
        if win < 0: continue
        ml = MINMATCH + cd[:, 2] + cd[:, 3]
        tied = np.flatnonzero(hit & (ml == lout))
        if len(tied) >= 2:
            keys.add("tie:cached" if tied[-1] < K else "tie:rest" if tied[0] >= K else "tie:both")
            if len(tied) >= 3: keys.add("tie:three")
            if tied[0] >= K and (tied[0] - K) // K_STEP != (tied[-1] - K) // K_STEP: keys.add("tie:across-steps")
        pos, _, fwd, back = (int(x) for x in cd[win])
        path = "cached" if win < K else "rest"
        if pos == 0: keys.add("cand:pos0")
        if lookback == 0 or path == "rest":
            if fwd in FWD: keys.add(f"fwd:{path}={fwd}")
        if ip + MINMATCH + fwd == matchlimit:
            meas = K_FWD if path == "cached" else K_RFWD
            if ip + K_WIDE_F > n: keys.add(f"fwd-end:{path}:scalar")
            elif fwd < meas: keys.add(f"fwd-end:{path}:measured")
            elif fwd - meas < K_WIDE: keys.add(f"fwd-end:{path}:steps64")
            elif (fwd - meas) % K_WIDE: keys.add(f"fwd-end:{path}:wide+tail")
            else: keys.add(f"fwd-end:{path}:wide-exact")
        if lookback:
            if back in (BACK_CACHED if path == "cached" else BACK_REST): keys.add(f"back:{path}={back}")
            if back == lookback: keys.add(f"back-stop:{path}:lookback")
            elif back == pos: keys.add(f"back-stop:{path}:cand" + ("<16" if pos < K_BACK else ">=16"))
            else: keys.add(f"back-stop:{path}:mismatch")
        for bnd in (K_IDX0, K_IDX0 + K_CHAINMASK + 1):
            if pos < bnd <= ip: keys.add(f"chainwrap:{bnd}")
    if "probe" in c.marks and "dist" in c.marks:
        p, dist, lead = c.marks["probe"], c.marks["dist"], c.marks["lead"]
        i = np.flatnonzero((S[:, 1] == p) & (S[:, 2] == p))
        if len(i):
            i = int(i[0]); cd = Cd[first[i]:first[i] + S[i, 4]]
            found = bool(((p - cd[:, 0] == dist) & (cd[:, 1] == 1)).any())
            if found == (dist <= K_MAXDIST): keys.add(f"dist:{dist}:lead={lead if lead < 65536 else '>64K'}:{'found' if found else 'out-of-reach'}")
            h = hashes(d)
            near = np.flatnonzero(h[p - K_MAXDIST + 1:p] == h[p])
            if not len(near) and p >= K_MAXDIST:
                same = h[p - K_MAXDIST] == h[p]
                keys.add("delta65535:" + ("other-hash" if not same else "same-word" if bytes(d[p - K_MAXDIST:p - K_MAXDIST + 4]) == bytes(d[p:p + 4]) else "same-hash-other-word"))
    if n > MFLIMIT:
        i = np.flatnonzero((S[:, 1] == n - MFLIMIT) & (S[:, 6] >= 0))
        if len(i) and n - MFLIMIT in (63, 64, 65): keys.add(f"n-12={n - MFLIMIT}:match@mflimit")
    for a in np.unique(t.arm[:, 0]):
        keys.add(f"arm:{ARMS[int(a)]}")
    E = t.emit
    seq, fin = E[E[:, 1] > 0], E[E[:, 1] == 0]
    for v in LITS:
        if (seq[:, 0] == v).any(): keys.add(f"emit:lit={v}")
    for v in MLS:
        if (seq[:, 1] == v).any(): keys.add(f"emit:ml={v}")
    for v in (1, 2, 3):
        if (seq[:, 2] == v).any(): keys.add(f"emit:off={v}")
    if (E[:, 1] > K_TABLES_ONLY).any() and (S[:, 0] > np.flatnonzero(E[:, 1] > K_TABLES_ONLY)[0]).any():
        # (the input lets the builder take its tables-only path, `v + 1 < keep`; whether it does depends on how far it runs
        # ahead of the parser at run time, so this key says the shape is there, not that the path ran)
        keys.add("emit:ml>192-then-search")
    if len(seq) >= 2 and len(fin) and (seq[-2:, 0] > 0).all() and (seq[-2:, 0] <= 64).all(): keys.add("emit:deferred-flush")
    return keys


def _refusals(c, level, full):
    """which of the three output checks refuses at the capacities the case runs at (`full`: its trace without a limit, which has
    all the arms a limited run can have but the refusal)"""
    keys = set()
    for cap in caps(c.data, level):
        if cap < 0: continue
        a = trace(c.data, level, cap, arm_rows=len(full.arm) + 1).arm[:, 0]
        for r in a[a >= 32]:
            keys.add(f"refuse:{REFUSE[int(r)]}")
    return keys


def ledger(case_list, levels=LEVELS, refusals=True):
    """key -> names of the cases that reach it"""
    led = collections.defaultdict(list)
    for c in case_list:
        for k in _data_keys(c): led[k].append(c.name)
        if len(c.data) > 192 * 1024: led["n>192Ki"].append(c.name)
        for lv in levels:
            t = trace(c.data, lv)
            keys = _search_keys(c, lv, t)
            if refusals: keys |= _refusals(c, lv, t)
            for k in keys: led[f"L{lv}:{k}"].append(c.name)
    return dict(led)


def _required():
    req = {f"n={n}" for n in (0, 1, 12, 13, 14)} | {"n>192Ki", "ins:same-hash:2", "ins:same-hash:many", "ins:fold10", "ins:same-hash+fold10",
                                                    "ins:partial-last-group", "ins:period1", "ins:period2", "ins:period3", "ins:period4"}
    for lv, A in ATTEMPTS.items():
        per = {f"att:found:behind={A - 1}", f"att:missed:behind={A}", "end:attempts", "end:lowest", "end:chain", "tie:cached",
               "cand:pos0", "fwd-end:cached:scalar", "fwd-end:cached:measured", "fwd-end:cached:steps64", "fwd-end:cached:wide+tail",
               "fwd-end:cached:wide-exact", "back-stop:cached:lookback", "back-stop:cached:cand<16", "back-stop:cached:cand>=16",
               "back-stop:cached:mismatch", "chainwrap:65536", "chainwrap:196608", "delta65535:other-hash", "delta65535:same-word",
               "delta65535:same-hash-other-word", "emit:ml>192-then-search", "emit:deferred-flush", "stepback:0",
               "refuse:literals", "refuse:matchlen", "refuse:last"}
        per |= {f"fwd:cached={v}" for v in FWD} | {f"back:cached={v}" for v in BACK_CACHED}
        per |= {f"dist:{d}:lead={ld}:{'found' if d <= K_MAXDIST else 'out-of-reach'}" for d in (65534, 65535, 65536) for ld in (0, 1, 17, ">64K")}
        per |= {f"n-12={v}:match@mflimit" for v in (63, 64, 65)}
        per |= {f"emit:lit={v}" for v in LITS} | {f"emit:ml={v}" for v in MLS} | {f"emit:off={v}" for v in (1, 2, 3)}
        per |= {f"arm:{a}" for a in REQUIRED_ARMS}
        if A <= K_WINK: per |= {f"att:wider:found:behind={A - 1}", f"att:wider:missed:behind={A}"}
        if A >= 3: per.add("tie:three")         # (three candidates need three attempts)
        if A > K_WINK:                          # levels 5..8: the rest of the chain
            per |= {"cached-all-collide-then-match", "walk:exact=8", "walk:exact=9", "tie:rest", "tie:both", "back-stop:rest:mismatch",
                    "back-stop:rest:cand>=16", "back-stop:rest:cand<16", "back-stop:rest:lookback", "fwd-end:rest:scalar", "fwd-end:rest:measured", "fwd-end:rest:steps64", "fwd-end:rest:wide+tail", "fwd-end:rest:wide-exact"}
            per |= {f"fwd:rest={v}" for v in FWD} | {f"back:rest={v}" for v in BACK_REST}
        if A > 72: per |= {"walk:exact=72", "walk:exact=73", "tie:across-steps"}        # a walk that long needs 73 attempts: level 8 alone
        req |= {f"L{lv}:{k}" for k in per}
    return frozenset(req)


# every arm of the arbitration the port numbers (oracle.h ORC_ARM_*) that a bounded search reached at every level; DESIGN_NOTES.md
# names the ones it did not
UNREACHED_ARMS = tuple(ARMS[k] for k in (18, 19, 20, 21))
REQUIRED_ARMS = tuple(v for v in ARMS.values() if v not in UNREACHED_ARMS)
REQUIRED = _required()


# ---- what the GPU test launches -----------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def expected(level):
    """[(label, data, cap, result, bytes)] for level 1..8 or 'mc'"""
    out = []
    for c in (mc_cases() if level == "mc" else cases()):
        for cap in caps(c.data, level):
            r, b = port(c.data, level, cap)
            out.append((f"{c.name}|cap={cap}", c.data, cap, r, b))
    return tuple(out)


# ---- Medium -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def _adjacent_colliders():
    """five bytes whose two overlapping words differ and share a hash"""
    rng = np.random.default_rng(5)
    b = rng.integers(0, 256, (1 << 20, 5), dtype=np.uint8)
    w = b.astype(np.uint32)
    h0 = hash15(w[:, 0] | (w[:, 1] << 8) | (w[:, 2] << 16) | (w[:, 3] << 24))
    h1 = hash15(w[:, 1] | (w[:, 2] << 8) | (w[:, 3] << 16) | (w[:, 4] << 24))
    i = np.flatnonzero((h0 == h1) & (b[:, 0] != b[:, 4]))[0]
    return b[i].tobytes()


def _mc_behind(n):
    def build(seed):
        L = _Lay(seed)
        words = bucket(B0, 6)
        T = L.bytes(9)
        L.rnd(1)
        want = [L.put(words[0] + T[:8] + _not(T[8]))]
        for c in words[1:1 + n]:
            L.rnd(1); want.append(L.put(c))
        L.rnd(1)
        probe = L.put(words[0] + T); want.append(probe)
        L.rnd(13)
        return L.data(), {"probe": probe}, want
    return Case(f"mc_behind{n}", *_seeded(build))


def _mc_share(which):
    L = _Lay(11)
    five = _adjacent_colliders()
    T = L.bytes(8)
    L.rnd(1)
    if which == "ntu-ip":                     # probes one byte apart: position ip - 1 enters the bucket the probe at ip reads
        L.put(five[1:] + T); L.rnd(3); L.put(five + T)
    elif which == "prev-ip":                  # the probe behind a match: the match's last byte opens a word of the probe's bucket
        Z = L.bytes(8)
        L.put(five[1:] + T); L.rnd(3); L.put(Z + five[:1] + _not(five[1])); L.rnd(3); L.put(Z + five + T)
    else:                                     # ... and the match's first and last positions share one
        W, Cw = bucket(B0, 2)
        mid = L.bytes(4)
        L.put(W + mid + Cw[:1] + _not(Cw[1])); L.rnd(3); L.put(W + mid + Cw + T); L.rnd(3); L.put(W + mid + Cw + T)
    L.rnd(13)
    return Case(f"mc_share_{which}", L.data(), {})


def _mc_stride(name, n_rnd, at):
    """a repeat of the first twelve bytes at `at`, behind misses enough for the probe stride to have grown"""
    L = _Lay(n_rnd + at)
    L.rnd(1)
    S = L.bytes(12)
    L.put(S); L.rnd(at - L.n); L.put(S); L.rnd(n_rnd - L.n); L.rnd(13)
    return Case(name, L.data(), {})


def _mc_zeros(name, lead, gap):
    """W + 12 bytes, a run of zeros that one match covers, and the same again: the probe behind the match stands on it"""
    L = _Lay(7)
    W = bucket(B0, 1)[0]
    T = L.bytes(11) + b"\x55"
    L.put(b"\x01" + bytes(lead))
    a = L.put(W + T); L.put(bytes(gap - 16))
    probe = L.put(W + T); L.rnd(13)
    assert probe - a == gap
    return Case(name, L.data(), {"probe": probe, "dist": gap})


@functools.lru_cache(None)
def mc_cases():
    hc = {c.name: c for c in cases()}
    out = [Case("mc_" + k, hc[k].data, {}) for k in ("n0", "n1", "n12", "n13", "n14", "n75", "n76", "n77", "run", "period3", "zeros2k",
                                                     "lits270_271", "fwd1056", "end_wide_tail", "end_scalar")]
    out += [_mc_behind(3), _mc_behind(4)]
    out += [_mc_share(w) for w in ("ntu-prev", "ntu-ip", "prev-ip")]
    out += [_mc_stride("mc_stride2_probed", 300, 108), _mc_stride("mc_stride2_skipped", 300, 109), _mc_stride("mc_stride1_64", 300, 65), _mc_stride("mc_stride1_last", 300, 66),
            _mc_stride("mc_stride2_first", 300, 68), _mc_stride("mc_stride2_first_skipped", 300, 67), _mc_stride("mc_stride3", 400, 330)]
    out += [_mc_zeros("mc_dist65535", 0, 65535), _mc_zeros("mc_dist65536", 0, 65536), _mc_zeros("mc_wrap", 30000, 40012)]
    out += [Case(f"mc_mix{k}_{s}_{n}", _mix(s, n, k), {}) for s, n, k in MIX]
    return tuple(out)


def _mc_keys(c, t):
    keys = set()
    d, n = c.data, len(c.data)
    keys.add(f"n={n}" if n <= 14 else f"n-12={n - MFLIMIT}" if n - MFLIMIT in (63, 64, 65) else "")
    P = t.search
    for _, ip, step, tries, walked, hits, best, ml, share, win, nxt in P.tolist():
        if ml and hits == 1 and win >= 3: keys.add(f"att:found:behind={win}")
        if not ml and not hits and walked == MC_ATTEMPTS and nxt >= 0 and bytes(d[nxt:nxt + 4]) == bytes(d[ip:ip + 4]): keys.add(f"att:missed:behind={walked}")
        for bits, nm in SHARE.items():
            if share & bits == bits: keys |= {f"share:{nm}"} | ({f"share:{nm}:then-match"} if ml else set())
        if not ml and tries - 63 in (64, 65, 128): keys.add(f"miss={tries - 63}")
        if ml and step > 1: keys.add(f"match@step={step}")
        if ml and tries - 64 in (64, 65, 66): keys.add(f"match-after-misses={tries - 64}")      # 65: the last unit stride, 66: the first of two
        if ml and ip - best == K_MAXDIST: keys.add("dist:65535:found")
        if ml and best < MC_CHAIN <= ip: keys.add("chainwrap:65536")
        if ml and best == 0: keys.add("cand:pos0")
        if ip == c.marks.get("probe") and c.marks.get("dist") == K_MAXDIST + 1 and not walked: keys.add("dist:65536:out-of-reach")
    if len(P): keys.add(f"maxstep={int(P[:, 2].max())}")
    E = t.emit
    if len(E) > 1 and (E[:-1, 1] >= 19 + 255).any(): keys.add("emit:ml>=274")
    if (E[:, 0] >= 15 + 255).any(): keys.add("emit:lit>=270")
    for cap in caps(d, "mc"):
        if cap < 0: continue
        a = trace(d, "mc", cap, arm_rows=len(t.arm) + 1).arm[:, 0]
        for r in a[a >= 32]: keys.add(f"refuse:{REFUSE[int(r)]}")
    return keys - {""}


def mc_ledger(case_list):
    led = collections.defaultdict(list)
    for c in case_list:
        for k in _mc_keys(c, trace(c.data, "mc")): led[k].append(c.name)
    return dict(led)


MC_REQUIRED = frozenset(
    {f"n={n}" for n in (0, 1, 12, 13, 14)} | {f"n-12={v}" for v in (63, 64, 65)} |
    {"att:found:behind=3", "att:missed:behind=4", "share:ntu-prev", "share:ntu-ip", "share:prev-ip", "miss=64", "miss=65", "miss=128",
     "match@step=2", "match-after-misses=64", "match-after-misses=65", "match-after-misses=66", "dist:65535:found", "dist:65536:out-of-reach", "chainwrap:65536", "emit:ml>=274", "emit:lit>=270",
     "refuse:literals", "refuse:matchlen", "refuse:last"})
