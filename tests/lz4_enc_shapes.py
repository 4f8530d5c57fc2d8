"""Inputs that walk the arms of the exact LZ4 fast encoder (4mc_amd/csrc/lz4_encode.hip, K2) and of its emitter (lz4emit.h), for the
encoder tests (plain module, like hc_opt_shapes.py; numpy, the oracle port's trace and the lane-level model's trace).

  cases()         the deterministic input set: named inputs, built lazily and seeded.  The generators of the four encoder test files
                  (test_gpu_lz4_mode_changes / _window_permutes / _input_ring / _window_waits) are reused as they stand.
  port_trace()    what the oracle port's parse did on one input (oracle.h: the ORC_LF_* rows), in the reference's coordinates.
  model_trace()   what the lane-level model (tools/model/lz4_fast_model.c) did, in the KERNEL's coordinates: windows, lanes, masks,
                  sparse batches, sequence() calls, ring events, and the counters K2_PROF counts.
  ledger()        the keys a case set reaches, computed from the two traces.  Keys carry the table instance: T16 (blocks below 65547
                  bytes) or T32.
  REQUIRED        the keys the set must reach.  A missing key is a test failure.
  UNREACHED       keys no input can reach, with the reason and the kernel line; the CPU test asserts that no case reaches one.
  OPEN            keys wanted of this catalogue that it does not reach yet and that are not known to be unreachable (none at present).
  caps()          the capacities one input runs at: bound, n-1, r, r-1, and the largest failing capacity of one early and one late sequence.
  expected()      every (input, capacity) pair with the port's result and bytes: what the GPU test launches.

A key is read from a trace; what a builder meant to build is never taken on trust."""
import collections
import ctypes as C
import functools
import hashlib
import os
import subprocess

import numpy as np

import helpers
import test_gpu_lz4_input_ring as ring
import test_gpu_lz4_mode_changes as mc
import test_gpu_lz4_window_permutes as wp
import test_gpu_lz4_window_waits as ww

# ---- constants the kernel branches on (4mc_amd/csrc/lz4_encode.hip, lz4emit.h) -------------------------------------------------------
BIG = 65547                     # lz4_encode.hip:50, :774   the smallest block of the 32-bit table
LANES = 64                      # lz4_encode.hip:292        positions per dense window, probes per sparse batch
WINDOW_NEED = 132               # lz4_encode.hip:281        sp + 132 <= n
K0_MAX = 32                     # lz4_encode.hip:281        k0 <= 32
PIECE = 1024                    # lz4_encode.hip:57
MAXDIST = 65535                 # lz4_encode.hip:51
RECORDS = 300                   # FOURMC_LZ4_RECORDS of the small-area runs (lz4_encode.hip:787-791: at least 2 * kRecSlack)
MAX_TOTAL, MAX_ABOVE_1M, MAX_ABOVE_256K = 48 << 20, 2, 12

PORT_WORDS = (4, 12, 4, 3)      # oracle.h ORC_LF_*_WORDS: SEARCH, HIT, EVENT, EMIT
MODEL_WORDS = (29, 8, 11, 12)   # lz4_fast_model.c LF_*_WORDS: WIN, SEQ, BATCH, EV
COUNTERS = ("nwin", "nseq", "nslow", "none", "cross", "dcut", "scut", "nit", "nrel", "nrot", "nrst")   # lz4_fast_model.c LF_C_*, lz4_encode.hip:130
EXIT = {0: "none", 1: "cross", 2: "dirty-cut", 3: "stride-cut", 4: "last-literals", 5: "output-full"}  # LF_EXIT_*
HOW = {0: "walk", 1: "general-step", 2: "sequence:slow", 3: "sequence:capok", 4: "sequence:catch-up", 5: "sequence:run_rt",
       6: "sequence:second-visited", 7: "sequence:second-entry", 8: "sequence:sparse"}                  # LF_HOW_*
PRED = {0: "probe", 1: "outside", 2: "in-match", 3: "refill-lane", 4: "xint"}                          # LF_PRED_*
BSTOP = {1: "anchor", 2: "candidate", 3: "byte"}                                                       # LF_BSTOP_*
BK = {0: "0", 1: "1", 2: "2", 3: "3", 4: "4:c==4", 5: "4:c>4"}                                         # LF_BK_*
FW = {0: "0..23", 1: "24..55", 2: "56"}                                                                # LF_FW_*
EV_SECOND, EV_RUN_RT, EV_SEQUENCE, EV_RING, EV_DRAIN, EV_TERM, EV_LAND, EV_GENERAL5 = range(1, 9)      # LF_EV_*
PEV_REFUSE = {32: "literals", 33: "matchlen", 34: "last"}                                              # oracle.h ORC_REFUSE_*
PEV_TABLE, PEV_DIST, PEV_RETEST = 64, 65, 66                                                           # oracle.h ORC_LF_EV_*

Case = collections.namedtuple("Case", "name data ring drain")       # ring: run at every source alignment; drain: traced with RECORDS too
PortTrace = collections.namedtuple("PortTrace", "result out search hit event emit")
ModelTrace = collections.namedtuple("ModelTrace", "result out win seq batch ev counters")


def bound(n):
    return n + n // 255 + 16


# ---- the port and the model ---------------------------------------------------------------------------------------------------------
class _LfTrace(C.Structure):              # lf_trace (tools/model/lz4_fast_model.c)
    _fields_ = [("ev", C.POINTER(C.c_int32) * 4), ("cap", C.c_int * 4), ("n", C.c_int * 4), ("cnt", C.c_int64 * len(COUNTERS))]


def build_model(out_dir, mutant=0, flags=("-O2",)):
    """the model as a shared library, with every warning an error"""
    so = os.path.join(str(out_dir), f"liblz4_fast_model_{mutant}.so")
    subprocess.run(["gcc", *flags, "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", f"-DLF_MUTANT={mutant}", "-o", so,
                    os.path.join(helpers.ROOT, "tools", "model", "lz4_fast_model.c")], check=True)
    return load_model(so)


def load_model(so):
    f = C.CDLL(so).lz4_fast_model_compress
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    f.restype = C.c_int
    return f


@functools.lru_cache(None)
def _model():
    d = os.path.join(helpers.ROOT, "tools", "model")
    so, src = os.path.join(d, "liblz4_fast_model_0.so"), os.path.join(d, "lz4_fast_model.c")
    if not os.path.exists(so) or os.path.getmtime(src) > os.path.getmtime(so):
        return build_model(d)
    return load_model(so)


def run_model(fn, data, cap, align=0, reccap=0, trace=None):
    data = np.ascontiguousarray(data, np.uint8)
    dst = np.zeros(max(cap, 1) + 64, np.uint8)
    r = fn(data.ctypes.data, dst.ctypes.data, len(data), cap, align, reccap, None if trace is None else C.byref(trace))
    return r, dst[:max(r, 0)]


def _twice(run, T, widths):
    """two runs: the first with no room sizes the second"""
    t = T()
    run(t)
    bufs = [np.zeros(max(t.n[k], 1), np.int32) for k in range(4)]
    t2 = T()
    for k in range(4):
        t2.ev[k] = bufs[k].ctypes.data_as(C.POINTER(C.c_int32)); t2.cap[k] = len(bufs[k])
    r, out = run(t2)
    assert [t2.n[k] for k in range(4)] == [t.n[k] for k in range(4)]
    return r, out, [bufs[k][:t2.n[k]].reshape(-1, widths[k]) for k in range(4)], t2


def port(data, cap):
    return helpers.orc_compress(data, cap)


def port_trace(data, cap=None):
    L = helpers.oracle()
    f = L.orc_lz4_compress_fast_ex
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]; f.restype = C.c_int
    data = np.ascontiguousarray(data, np.uint8)
    cap = bound(len(data)) if cap is None else cap
    dst = np.zeros(max(cap, 1) + 64, np.uint8)

    def run(t):
        r = f(data.ctypes.data, dst.ctypes.data, len(data), cap, C.byref(t))
        return r, dst[:max(r, 0)].copy()
    r, out, tabs, _ = _twice(run, helpers.OrcTrace, PORT_WORDS)
    return PortTrace(r, out, *tabs)


def model_trace(data, cap=None, align=0, reccap=0, fn=None):
    cap = bound(len(data)) if cap is None else cap
    r, out, tabs, t = _twice(lambda t: run_model(fn or _model(), data, cap, align, reccap, t), _LfTrace, MODEL_WORDS)
    return ModelTrace(r, out.copy(), *tabs, dict(zip(COUNTERS, (int(v) for v in t.cnt))))


def _seqs(emit):
    """the port's EMIT rows in the form mc._fail_caps reads: (literals, start, match length, offset), the last (literals, n, None, None)"""
    out, pos = [], 0
    for lit, ml, off in emit.tolist():
        pos += lit
        out.append((lit, pos, ml, off) if ml else (lit, pos, None, None)); pos += ml
    return out


@functools.lru_cache(None)
def _caps(name):
    data = by_name()[name].data
    n = len(data)
    t = port_trace(data)
    out = []
    fails = mc._fail_caps(_seqs(t.emit))
    picks = [fails[min(2, len(fails) - 1)][1], fails[-1 - min(2, len(fails) - 1)][1]] if fails else []
    for c in [bound(n), n - 1, t.result, t.result - 1] + picks:
        c = max(c, 0)
        if c not in out: out.append(c)
    return tuple(out)


def caps(data):
    """bound, n - 1, r, r - 1 and the largest capacity that fails at one early and one late sequence (the third from either end)"""
    for c in cases():
        if c.data is data: return _caps(c.name)
    raise KeyError("not a catalogue input")


# ---- builders -----------------------------------------------------------------------------------------------------------------------
def _arr(b):
    return np.frombuffer(bytes(b), np.uint8).copy()


def _rnd(seed, k):
    return np.random.default_rng(seed).integers(0, 256, k, dtype=np.uint8)


def _collide(rng, five, small, prefix=b""):
    """five bytes (beginning with `prefix`) of the table slot of `five` that do not begin with its four bytes"""
    want = wp._slot(five, small)
    while True:
        cand = rng.integers(0, 256, (1 << 16, 5), dtype=np.uint8)
        cand[:, :len(prefix)] = np.frombuffer(bytes(prefix), np.uint8)
        h, _ = wp._hashes(cand.reshape(-1), small)
        for k in np.nonzero(h[::5] == want)[0]:
            c = bytes(cand[k])
            if c[:4] != bytes(five[:4]): return c


def _open_window(g, n_src=160):
    """mc's way to a window at a known place: a source area, text, and a copy of 100 bytes that leaves its window; returns the source and
    the copy's end, where the next dense window begins"""
    src = g.source(n_src)
    g.text(260)
    return src, g.copy(src, 100, 3) + 100


def _probe_counts(small):
    """searches that hit at their 1st, 2nd, 33rd, 34th, 64th .. 67th, 129th and 200th probe behind the re-test"""
    g = mc._Gen(301 + small, t=20000)
    g.text(2000)
    for P in (1, 2, 33, 34, 64, 65, 66, 67, 129, 200):
        src, e = _open_window(g)
        g.copy(src + 110, 12, 1 + mc._probe_offset(P - 1))
        g.noise(3); g.text(300)
    g.text_to(60000 if small else BIG + 2000)
    return g.data()


def _far(dist):
    """five bytes, a run of one byte that is one match, and the five bytes again `dist` behind their first: the re-test behind the run"""
    g = mc._Gen(310 + dist % 7, t=30000)
    g.text(1500)
    g.source(40)
    W = bytes([0xE1, 0x3C, 0x9A, 0x47, 0xB2])
    p0 = len(g.out)
    g._add(W, False); g.noise(3, last_not=0x6D)
    g._add(bytes([0x6D]) * (dist - 8), False)
    assert len(g.out) == p0 + dist
    g._add(W + bytes([0x11, 0x22, 0x33]), False)
    g.noise(5); g.text(1500)
    return g.data()


def _first_bytes(small):
    """the block's first bytes come again: candidates at positions 0 .. 4.  For position 4 with four equal bytes in front of it the slots
    of positions 0 .. 3 are given to other strings first (T32; the 16-bit table hashes four bytes, so only its own bytes own a slot)"""
    rng = np.random.default_rng(320 + small)
    text = ring._text()
    n = 40000 if small else BIG + 3000
    data = text[50000:50000 + n].copy()
    data[:16] = rng.integers(0x80, 256, 16, dtype=np.uint8)
    for k in range(5):
        data[3000 + 2500 * k:3000 + 2500 * k + 14] = data[k:k + 14]
        data[3000 + 2500 * k - 1] = 0x7F                   # (nothing equal in front of it)
    at = 20000
    if not small:
        for k in range(4):
            data[at + 9 * k:at + 9 * k + 5] = np.frombuffer(_collide(rng, bytes(data[k:k + 5]), small), np.uint8)
    data[at + 200:at + 218] = data[0:18]                   # positions 0 .. 3 fail (their slots went away), position 4 hits with four bytes before it
    data[at + 199] = 0x7F
    # an empty slot read as position 0 that matches: the first four bytes with another fifth (T32: five bytes are hashed)
    data[40:44] = data[0:4]; data[44] = data[4] ^ 0x55; data[39] = 0x7E
    return data


def _runs_twice(small):
    """a short run of a byte and later a longer one: the match of the second on the first ends inside the second, so the ip-2 refill and the
    re-test read one slot and the re-test hits at distance 2.  The second runs begin at every place of a window, and at lanes 0 .. 3."""
    g = mc._Gen(330 + small, t=60000)
    g.text(3000)
    for i in range(40):
        b = bytes([0x80 + i])
        g._add(b * 12, False)
        g.text(150 + i)
        g._add(b * (30 + 3 * i), False)
        g.text(200)
    g.text_to(50000 if small else BIG + 4000)
    return g.data()


def _back_in_memory(small, extra, stop):
    """_back_in_memory_once with the first seed whose strings leave A's slot alone (they are random, and some 400 positions of them enter the table)"""
    for attempt in range(10):
        d = _back_in_memory_once(small, extra, stop, 1000 * attempt)
        if (port_trace(d).hit[:, 5] == 4 + extra).any(): return d
    raise AssertionError((small, extra, stop))


def _back_in_memory_once(small, extra, stop, seed):
    """F, 45 fresh bytes; A = F[:40] and 60 fresh bytes (the match on F starts a search at A + 40, which enters A + 40 .. A + 105 one by
    one); behind it strings that take the table slots of A's first 4 + extra positions away; then A again right behind a match (stop =
    'anchor'), or behind bytes that differ ('byte'), placed so that the search probes its (4 + extra)-th position: that is the first one
    that finds A in the table, and sequence() walks 4 + extra bytes back - the window knows four of them"""
    rng = np.random.default_rng(340 + extra + 7 * small + seed)
    g = mc._Gen(341 + extra + 7 * small + seed, t=100000)
    g.text(3000)
    k = 4 + extra
    f = g.source(45)
    g.noise(3); g.text(200)
    g.noise(2, last_not=g.out[f - 1])
    a = len(g.out)
    g._add(bytes(g.out[f:f + 40]), False); g.noise(60, last_not=None)
    if g.out[a + 40] == g.out[f + 40]: g.out[a + 40] ^= 0x55
    A = bytes(g.out[a:a + 100])
    g.noise(3)
    for j in range(k):
        if j % 8 == 0:                                     # a match first: the search behind it probes every position
            g._add(mc.MARK, False); g.noise(1)
        g._add(_collide(rng, A[j:j + 5], small), False)
    g.noise(4); g.text(300)
    src, e = _open_window(g)
    if stop == "byte":
        g.noise(2 if extra == 64 else 1, last_not=g.out[a - 1])
    g._add(A[:k + 12], False)
    g.noise(3, last_not=A[k + 12]); g.text(300)
    g.text_to(30000 if small else BIG + 1000)
    return g.data()


def _back_to_start(small):
    """the block's first bytes again, behind strings that took the slots of positions 0 .. 5 away: the hit is at position 6 and the walk
    back ends at position 0, the candidate's"""
    rng = np.random.default_rng(345 + small)
    g = mc._Gen(346 + small, t=105000)
    g.noise(40); g.text(1500)
    head = bytes(g.out[:24])
    g._add(mc.MARK + mc.MARK, False); g.noise(1)
    for j in range(6): g._add(_collide(rng, head[j:j + 5], small), False)
    g.noise(4); g.text(300)
    src, e = _open_window(g)
    g.noise(20)
    g._add(head[:20], False)
    g.noise(3, last_not=head[20]); g.text(300)
    g.text_to(20000 if small else BIG + 1000)
    return g.data()


def _cut_at(small, lane):
    """a block whose first sparse batch (positions 1 .. 64, no hit) is cut at `lane`: that position is the first to fold onto the scoreboard
    entry of an earlier one (lz4_encode.hip:683-686)"""
    for seed in range(4000):
        head = _rnd([400 + small, seed], 80)
        h, _ = wp._hashes(head, small)
        fold = (h[1:65].astype(np.int64) & 1023).tolist()
        first = next((i for i in range(64) if fold[i] in fold[:i]), 64)
        if first == lane: break
    else: raise AssertionError(lane)
    g = mc._Gen(401 + small, t=160000)
    g._add(head.tobytes(), False); g.noise(200); g.text(1000)
    g.text_to(5000 if small else BIG + 500)
    return g.data()


class _RtShapes(wp._Shapes):
    """one more window shape on wp's machinery: the re-test lane L behind a chosen match is the third lane of its slot, the refill lane
    L - 2 is the second and holds other bytes - run_rt's byte compare fails (lz4_encode.hip:576)"""

    def _rt_miss(self, L):
        a = self.area(); o = self.g.out
        e = self.open(a)
        m01 = bytes(o[a + 66:a + 68])
        while True:
            x = self.fresh(3)
            if x[0] == o[a + 68]: continue
            X = m01 + x
            cand = np.zeros((65536, 5), np.uint8)
            cand[:, :3] = np.frombuffer(x, np.uint8)
            cand[:, 3] = np.arange(65536) & 255; cand[:, 4] = np.arange(65536) >> 8
            h, _ = wp._hashes(cand.reshape(-1), self.small)
            hit = np.flatnonzero(h[::5] == wp._slot(X, self.small))
            if len(hit): break
        Y = bytes(cand[hit[0]])
        Z = self.collide(X)
        self.m1(a, e, L, tokens=[(3, Z)])
        self.lits(e, L + 16, [(L, Y)])
        self.need(e + L, e + L - 2, e + 3)
        self.close()
        self.names.append(f"rt miss L={L}")
    rt_miss = wp._case(_rt_miss)


def _rt_misses():
    b = _RtShapes(204, 60000)
    for L in (30, 45, 61): b.rt_miss(L)
    return b.data(BIG + 300)


def _wide_match(first16, rounds, at_limit=False):
    """a match that goes through sequence()'s 16-bytes-per-lane loop `rounds` times and ends in the first or the last 16 bytes of a round"""
    g = mc._Gen(350 + rounds + 3 * first16, t=110000)
    g.text(2000)
    L = 124 + 1024 * (rounds - 1) + (5 if first16 else 1013)         # (4 + 56 the window knows, 64 by the narrow loop, then the wide one)
    src = g.source(L + 40)
    g.text(300)
    g.copy(src, L, 3)
    g.noise(3); g.text(1200)
    g.text_to(BIG + 3000)
    return g.data()


def _to_matchlimit(small, length):
    """the block ends with a copy that runs into the match limit"""
    g = mc._Gen(360 + small + length % 5, t=120000)
    g.text(50000 if small else BIG)
    src = g.source(length + 30)
    g.text(400)
    g.copy(src, length, 3)
    g.avoid = None
    g._add(bytes(g.out[src + length:src + length + 5]), False)
    return g.data()


def _lengths(small):
    """literal runs and matches at the lengths where their encodings change: 14, 15, 269, 270, 4095 and above; literal runs of 64 and 65"""
    g = mc._Gen(370 + small, t=130000)
    g.text(1500)
    lens = (14, 15, 269, 270, 64, 65)
    for v in lens:
        src, e = _open_window(g, 160)
        g.copy(src + 110, 12, v)
        g.noise(3); g.text(200)
    for v in (14, 15, 269, 270, 4200):
        src = g.source(v + 4 + 30)
        g.text(300)
        g.copy(src, v + 4, 3)
        g.noise(3); g.text(200)
    g.noise(4300)
    src, e = _open_window(g, 160)
    g.text_to(40000 if small else BIG + 3000)
    return g.data()


def _before_window(small):
    """a first sequence of a window that owns literals from before it: 0, 14, 15, 269, 270"""
    g = mc._Gen(380 + small, t=140000)
    g.text(1500)
    for v in (14, 15, 269, 270, 33, 34, 35):
        for lane in (3, 20):
            src, e = _open_window(g, 160)
            g.copy(src + 110, 12, v + lane)
            g.noise(3); g.text(200)
    g.text_to(30000 if small else BIG + 3000)
    return g.data()


def _many_records(k, small):
    """a block of exactly 64 k (+ 1) sequences: units of four fresh bytes and twelve known ones"""
    def build(units):
        g = mc._Gen(390 + small, t=150000)
        g.text(100)
        g.units(units)
        g.noise(20)
        if not small: g.noise(BIG)
        return g.data()
    for units in range(k - 40, k + 2):
        d = build(units)
        if len(port_trace(d).emit) == k: return d
    raise AssertionError(k)


@functools.lru_cache(None)
def cases():
    text = ring._text()
    big_text = helpers.corpus((4 << 20) + (1 << 20) + 1)
    out = []

    def add(name, data, ring_case=False, drain=False):
        data = np.ascontiguousarray(data, np.uint8)
        data.setflags(write=False)
        out.append(Case(name, data, ring_case, drain))
    for n in (0, 1, 12, 13, 14) + tuple(range(131, 141)) + (BIG - 1, BIG, 131072, 131073):
        add(f"n{n}", text[1000:1000 + n])
    add("n1m1", big_text[:(1 << 20) + 1])
    add("n4m", big_text[(1 << 20) + 1:])
    blocks = mc._blocks()
    for k in ("features", "end0", "end1", "end130", "end131", "end132", "end133", "start4", "start5", "tail_probe", "tail_match", "fill_dense", "fill_sparse", "size128k"):
        add(k, blocks[k], ring_case=k in ("features", "end131"))
    add("drain", blocks["drain"], drain=True)
    add("small_drain", blocks["drain"][:60000], drain=True)
    for k in ("small_text", "small_5000", "small_noise"):
        add(k, mc._small(k), drain=k == "small_text")
    for k, (d, _) in wp._built().items():
        add(k, d, ring_case=k == "slots")
    add("ring_runs", ring._runs_block(), ring_case=True)
    add("ring_alternating", ring._alternating_block())
    add("ring_literal_runs", ring._literal_runs_block())
    add("piece_end_runs", ww._runs_at_piece_ends(0), ring_case=True)
    add("noise_behind_pieces", ww._noise_behind_piece_starts(0))
    for p in (1, 2, 3, 4, 5, 63, 64, 65):
        add(f"period{p}", ww._periodic(p))
        add(f"small_period{p}", ww._periodic(p)[:3000 + p])
    add("shared_slots", ww._shared_slots())
    add("small_shared_slots", ww._shared_slots()[2000:2000 + 60000])
    for small in (0, 1):
        s = "small_" if small else ""
        add(s + "probe_counts", _probe_counts(small))
        add(s + "first_bytes", _first_bytes(small))
        add(s + "runs_twice", _runs_twice(small))
        for extra in (0, 1, 64, 65):
            add(f"{s}back{extra}_byte", _back_in_memory(small, extra, "byte"))
        add(s + "back64_anchor", _back_in_memory(small, 64, "anchor"))
        add(s + "back_to_start", _back_to_start(small))
        add(s + "cut1", _cut_at(small, 1)); add(s + "cut63", _cut_at(small, 63))
        add(s + "to_matchlimit_30", _to_matchlimit(small, 30))
        add(s + "to_matchlimit_300", _to_matchlimit(small, 300))
        add(s + "lengths", _lengths(small))
        add(s + "before_window", _before_window(small))
        add(s + "records128", _many_records(128, small))
        add(s + "records129", _many_records(129, small))
    add("rt_misses", _rt_misses())
    for dist in (65534, 65535, 65536):
        add(f"dist{dist}", _far(dist))
    add("wide1_first16", _wide_match(1, 1)); add("wide1_last16", _wide_match(0, 1)); add("wide2_last16", _wide_match(0, 2)); add("wide3_first16", _wide_match(1, 3))
    add("random_100k", _rnd(7, 100000))
    add("two_symbols", np.random.default_rng(8).integers(0, 2, 70000, dtype=np.uint8))
    add("small_two_symbols", np.random.default_rng(9).integers(0, 2, 20000, dtype=np.uint8))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


@functools.lru_cache(None)
def by_name():
    return {c.name: c for c in cases()}


# ---- ledger -------------------------------------------------------------------------------------------------------------------------
def _mask(win, col):
    return (win[:, col].astype(np.int64) & 0xFFFFFFFF) | ((win[:, col + 1].astype(np.int64) & 0xFFFFFFFF) << 32)


def _bit(m, b):
    return bool(((m >> b) & 1).any())


def _len_keys(pre, v):
    keys = set()
    for x in (14, 15, 269, 270):
        if (v == x).any(): keys.add(f"{pre}={x}")
    if (v >= 4095).any(): keys.add(f"{pre}>=4095")
    return keys


def _port_keys(d, t):
    keys = set()
    n = len(d)
    if n in (0, 1, 12, 13, 14) or 131 <= n <= 140 or n in (BIG - 1, BIG, 131072, 131073, (1 << 20) + 1, 4 << 20): keys.add(f"n={n}")
    S, H, E, M = t.search, t.hit, t.event, t.emit
    if len(S):
        pr = S[:, 1]
        for v in (1, 2, 33, 34, 64, 65, 66, 67):
            if ((pr == v) & (S[:, 2] == 0)).any(): keys.add(f"search:probes={v}")
        if ((pr >= 129) & (S[:, 2] == 0)).any(): keys.add("search:probes>=129")
        if (S[:, 2] == 1).any(): keys.add("search:ends-block")
        if (S[:, 3] > 0).any(): keys.add("search:empty-slot:position-0-differs" if (S[:, 3] > 1).any() or not len(H) or not (H[:, 2] == 1).any() else "search:empty-slot")
    if len(H):
        dist = H[:, 0] - H[:, 1]
        for v in (65534, 65535):
            if (dist == v).any(): keys.add(f"search:dist={v}:accepted")
        if (H[:, 2] == 1).any(): keys.add("search:empty-slot:position-0-matches")
        for v in (1, 2, 3, 4):
            if ((H[:, 1] == v) & (H[:, 10] == 0)).any(): keys.add(f"search:cand={v}")
        if (H[:, 1] == 0).any(): keys.add("search:cand=0")
        for v in (0, 1, 2, 3, 4, 5, 68, 69):
            if ((H[:, 5] == v) & (H[:, 10] == 0)).any(): keys.add(f"hit:back={v}")
        for k, nm in ((0, "anchor"), (1, "candidate-0"), (2, "byte")):
            if ((H[:, 6] == k) & (H[:, 10] == 0)).any(): keys.add(f"hit:back-stop:{nm}")
        if (H[:, 9] == 1).any(): keys.add("hit:ends-at-matchlimit")
        if ((H[:, 10] == 1) & (H[:, 11] == 1)).any(): keys.add("retest:hit:refill-in-its-slot")
    for row in E.tolist():
        k = row[0]
        if k in PEV_REFUSE: keys.add(f"refuse:{PEV_REFUSE[k]}")
        elif k == PEV_DIST:
            if row[2] == MAXDIST + 1: keys.add("search:dist=65536:refused" + (":four-bytes-equal" if row[3] else ""))
            keys.add("search:dist:refused")
        elif k == PEV_RETEST:
            keys.add("retest:" + ("hit" if row[2] else "miss"))
            if row[3]: keys.add("retest:refill-in-its-slot")
    seq = M[M[:, 1] > 0]
    keys |= _len_keys("emit:lit", M[:, 0]) | _len_keys("emit:mcode", seq[:, 1] - 4)
    for v in (64, 65):
        if (M[:, 0] == v).any(): keys.add(f"emit:lit={v}")
    if len(M) % 64 == 0: keys.add("emit:records=64k")
    if len(M) % 64 == 1 and len(M) > 1: keys.add("emit:records=64k+1")
    return keys


def _model_keys(t):
    keys = set()
    W, Q, Bt, E = t.win, t.seq, t.batch, t.ev
    if len(W):
        m_hit, m_cond, m_dirty, m_slow, m_sat, m_second, m_nodist, m_nochk = (_mask(W, c) for c in range(10, 26, 2))
        hits = m_hit | m_cond
        for b, nm in BK.items():
            if ((W[:, 26] >> b) & 1).any(): keys.add(f"lane:bk={nm}")
        for b, nm in FW.items():
            if ((W[:, 27] >> b) & 1).any(): keys.add(f"lane:fw={nm}")
        if _bit(hits, 0): keys.add("lane:hit-at-0")
        if _bit(hits, 63): keys.add("lane:hit-at-63")
        if m_nodist.any(): keys.add("lane:pass-false:distance")
        if m_nochk.any(): keys.add("lane:pass-false:check-bits")
        if m_sat.any(): keys.add("lane:saturated")
        if (W[:, 28] == 1).any(): keys.add("slot:first-only")
        if (W[:, 28] == 2).any(): keys.add("slot:second")
        if (W[:, 28] >= 3).any(): keys.add("slot:third")
        if (m_second & ~m_cond).any(): keys.add("second:neither")
        for v in np.unique(W[:, 3]): keys.add(f"exit:{EXIT[int(v)]}")
        if (W[:, 4] == 1).any(): keys.add("exit:record-limit")
        if (W[:, 2] == 1).any(): keys.add("entry:retest")
        for v in (0, 1, 2, 32):
            if ((W[:, 2] == 0) & (W[:, 1] == v)).any(): keys.add(f"entry:k0={v}")
        for v in (0, 1):
            if (W[:, 6] == v).any(): keys.add(f"walk:rounds={v}")
        if (W[:, 6] >= 2).any(): keys.add("walk:rounds>=2")
        if (W[:, 8] == 0).any(): keys.add("walk:capok-false")
        first = W[W[:, 6] >= 1]
        for v in (0, 14, 15, 33):
            if (first[:, 9] == v).any(): keys.add(f"walk:before={v}")
        if len(Q):
            inwin = Q[(Q[:, 0] >= 0) & (Q[:, 6] == 0)]
            cnt = np.bincount(inwin[:, 0]) if len(inwin) else np.zeros(1, np.int64)
            for v in (1, 2, 6, 7):
                if (cnt == v).any(): keys.add(f"walk:chain={v}")
            if (cnt >= 10).any(): keys.add("walk:chain>=10")
    for v in np.unique(Q[:, 6]) if len(Q) else (): keys.add(f"chosen:{HOW[int(v)]}")
    if len(Bt):
        keys.add("batch")
        if (Bt[:, 1] == 0).any(): keys.add("batch:k0=0")
        if (Bt[:, 1] > 0).any(): keys.add("batch:k0>0")
        if (Bt[:, 1] == 33).any(): keys.add("batch:k0=33")
        if (Bt[:, 2] == 1).any(): keys.add("batch:rt")
        keys |= {"batch:wide" if w else "batch:narrow" for w in np.unique(Bt[:, 3])}
        for v in (1, 63):
            if ((Bt[:, 4] == v) & (Bt[:, 5] == 64)).any(): keys.add(f"batch:cut={v}")
        for v, nm in ((0, "none"), (1, "hit"), (2, "term")):
            if (Bt[:, 6] == v).any(): keys.add(f"batch:event:{nm}")
        if (Bt[:, 7] == 1).any(): keys.add("batch:h==h2")
        cr = Bt[Bt[:, 8] == 1]
        if (cr[:, 9] <= 8).any(): keys.add("batch:cregs:room<=8")
        if (cr[:, 10] < 8).any(): keys.add("batch:cregs:eq<8")
        if ((cr[:, 10] == 8) & (cr[:, 9] > 8)).any(): keys.add("batch:cregs:fwd_more")
        if ((Bt[:, 6] == 1) & (Bt[:, 8] == 0)).any(): keys.add("batch:hit-without-cregs")
    for row in E.tolist():
        k = row[0]
        if k == EV_SECOND:
            _, sp0, lane, j, visited, hitA, hit, place, gen = row[:9]
            keys.add(f"second:{'visited' if visited else 'not-visited'}:" + ("hitA+hit" if hitA and hit else "hitA" if hitA else "hit"))
            keys.add(f"second:pred:{PRED[place]}")
            if gen: keys.add("second:back-to-the-walk")
        elif k == EV_RUN_RT: keys.add("run_rt:" + ("miss", "hit", "e<2")[row[3]])
        elif k == EV_SEQUENCE:
            _, ip, rt, br, badd, bstop, wr, wp_, nr, atlim, ret, site = row
            if br:
                if badd in (0, 1, 64, 65): keys.add(f"sequence:back-loop:+{badd}")
                keys.add(f"sequence:back-loop:stop:{BSTOP[bstop]}")
            keys.add("sequence:wide-rounds=" + ("0" if wr == 0 else "1" if wr == 1 else ">=2"))
            if wp_ == 0: keys.add("sequence:wide:mismatch-in-first-16")
            if wp_ == 63: keys.add("sequence:wide:mismatch-in-last-16")
            if nr and atlim: keys.add("sequence:narrow:ends-at-matchlimit")
            keys.add(f"sequence:return={ret}" + (f":check{site}" if ret == 2 else ""))
            if rt: keys.add("sequence:rt_hit")
        elif k == EV_RING:
            _, sp0, kind, ralign, at_rend, jump, pos, neg, far = row[:9]
            keys.add("ring:" + ("reload", "rotate", "reset")[kind])
            if kind == 0 and jump: keys.add("ring:jump-past-rend")
            if at_rend: keys.add("ring:c_hi==rend")
            if pos: keys.add("ring:piece_store:sh>0")
            if neg: keys.add("ring:piece_store:sh<0")
            if far: keys.add("ring:piece_store:|sh|>=16")
        elif k == EV_DRAIN: keys.add("drain:" + ("behind-sequence()" if row[2] else "between-windows"))
        elif k == EV_TERM:
            if 1 <= row[3] <= 6: keys.add(f"walk:term:d={row[3]}:" + ("ends-chain" if row[4] else "goes-on"))
        elif k == EV_LAND:
            if 59 <= row[2] <= 65: keys.add(f"walk:landing={row[2]}")
        elif k == EV_GENERAL5: keys.add("walk:first-general-step:catch-up-5")
    return keys


def _ring_end_keys(c):
    """every ralign at the block's two ends: the shifts piece_store makes there (32-bit table)"""
    keys = set()
    for a in range(16):
        t = model_trace(c.data, align=a)
        r = t.ev[t.ev[:, 0] == EV_RING]
        first, last = r[0], r[r[:, 2] != 2][-1]
        if a == 0 or first[7]: keys.add(f"ring:ralign={a}:block-start")
        if first[7]: keys.add("ring:piece_store:sh<0")
        if last[6] or last[8]: keys.add(f"ring:ralign={a}:block-end")
    return keys


def keys_of(c, refusals=True):
    d = c.data
    tab = "T16" if len(d) < BIG else "T32"
    pt = port_trace(d)
    keys = _port_keys(d, pt)
    if len(d) == 0: return {f"{tab}:{k}" for k in keys}
    mt = model_trace(d)
    assert mt.result == pt.result and np.array_equal(mt.out, pt.out), c.name
    keys |= _model_keys(mt)
    if refusals and len(d) <= (1 << 20):
        for cap in _caps(c.name)[1:]:
            keys |= {k for k in _port_keys(d, port_trace(d, cap)) if k.startswith("refuse:")}
            keys |= {k for k in _model_keys(model_trace(d, cap)) if k.startswith(("sequence:return", "walk:capok", "exit:output-full", "chosen:sequence:capok"))}
    if c.drain: keys |= {k for k in _model_keys(model_trace(d, reccap=RECORDS)) if k.startswith(("drain:", "exit:record-limit"))}
    if c.ring and tab == "T32": keys |= _ring_end_keys(c)
    return {f"{tab}:{k}" for k in keys}


def ledger(case_list=None, refusals=True):
    """key -> names of the cases that reach it"""
    led = collections.defaultdict(list)
    for c in (cases() if case_list is None else case_list):
        for k in keys_of(c, refusals): led[k].append(c.name)
    return dict(led)


def _required():
    both = {f"search:probes={v}" for v in (1, 2, 33, 34, 64, 65, 66, 67)} | {"search:probes>=129", "search:ends-block", "retest:hit", "retest:miss",
            "retest:refill-in-its-slot", "retest:hit:refill-in-its-slot", "search:empty-slot:position-0-differs", "search:cand=0"}
    both |= {f"search:cand={v}" for v in (1, 2, 3, 4)}
    both |= {f"hit:back={v}" for v in (0, 1, 2, 3, 4, 5, 68, 69)} | {f"hit:back-stop:{v}" for v in ("anchor", "candidate-0", "byte")} | {"hit:ends-at-matchlimit"}
    both |= {f"lane:bk={v}" for v in BK.values()} | {f"lane:fw={v}" for v in FW.values()} | {"lane:hit-at-0", "lane:hit-at-63", "lane:saturated"}
    both |= {"slot:first-only", "slot:second", "slot:third", "run_rt:hit", "run_rt:miss"}
    both |= {f"walk:chain={v}" for v in (1, 2, 6, 7)} | {"walk:chain>=10"} | {f"walk:landing={v}" for v in range(59, 66)}
    both |= {f"walk:term:d={v}:goes-on" for v in (1, 2, 3, 4)} | {f"walk:term:d={v}:ends-chain" for v in (5, 6)}
    both |= {"walk:rounds=0", "walk:rounds=1", "walk:rounds>=2", "walk:first-general-step:catch-up-5", "walk:capok-false"} | {f"walk:before={v}" for v in (0, 14, 15, 33)}
    both |= {f"exit:{v}" for v in EXIT.values()} | {"exit:record-limit", "entry:retest"} | {f"entry:k0={v}" for v in (0, 1, 2, 32)}
    both |= {"batch:k0=0", "batch:k0>0", "batch:k0=33", "batch:rt", "batch:narrow", "batch:wide", "batch:cut=1", "batch:cut=63", "batch:event:hit", "batch:event:term",
             "batch:event:none", "batch:h==h2", "batch:cregs:room<=8", "batch:cregs:eq<8", "batch:cregs:fwd_more", "batch:hit-without-cregs"}
    both |= {f"sequence:back-loop:+{v}" for v in (0, 1, 64, 65)} | {f"sequence:back-loop:stop:{v}" for v in BSTOP.values()}
    both |= {"sequence:wide-rounds=0", "sequence:wide-rounds=1", "sequence:wide-rounds=>=2", "sequence:wide:mismatch-in-first-16", "sequence:wide:mismatch-in-last-16",
             "sequence:narrow:ends-at-matchlimit", "sequence:return=0", "sequence:return=1", "sequence:return=2:check1", "sequence:return=2:check2", "sequence:rt_hit"}
    both |= {f"emit:{a}={v}" for a in ("lit", "mcode") for v in (14, 15, 269, 270)} | {"emit:lit>=4095", "emit:mcode>=4095", "emit:lit=64", "emit:lit=65",
                                                                                        "emit:records=64k", "emit:records=64k+1"}
    both |= {"drain:behind-sequence()", "drain:between-windows", "refuse:literals", "refuse:matchlen", "refuse:last"}
    both |= {f"chosen:{v}" for v in HOW.values()}
    t32 = {"search:dist=65534:accepted", "search:dist=65535:accepted", "search:dist=65536:refused:four-bytes-equal", "search:empty-slot:position-0-matches",
           "lane:pass-false:distance", "lane:pass-false:check-bits", "second:neither", "second:back-to-the-walk"}
    t32 |= {f"second:{a}:{b}" for a in ("visited", "not-visited") for b in ("hitA", "hit", "hitA+hit")} | {f"second:pred:{v}" for v in PRED.values()}
    t32 |= {"ring:reload", "ring:rotate", "ring:reset", "ring:jump-past-rend", "ring:c_hi==rend", "ring:piece_store:sh>0", "ring:piece_store:sh<0", "ring:piece_store:|sh|>=16"}
    t32 |= {f"ring:ralign={a}:block-{e}" for a in range(16) for e in ("start", "end")}
    req = {f"T16:{k}" for k in both} | {f"T32:{k}" for k in both | t32}
    req |= {f"T16:n={n}" for n in (0, 1, 12, 13, 14, BIG - 1) + tuple(range(131, 141))} | {f"T32:n={n}" for n in (BIG, 131072, 131073, (1 << 20) + 1, 4 << 20)}
    return req


# keys that no input reaches, with the reason and the kernel line; tests/test_lz4_enc_shapes_cpu.py asserts that no case reaches one
UNREACHED = {}
for _k in ("search:dist=65534:accepted", "search:dist=65535:accepted", "search:dist=65536:refused:four-bytes-equal", "search:dist=65536:refused", "search:dist:refused", "lane:pass-false:distance"):
    UNREACHED[f"T16:{_k}"] = "a block of the 16-bit table is shorter than 65547 bytes and its distance test is compiled out (lz4_encode.hip:335 `!U32TAB ||`, :682)"
UNREACHED["T16:lane:pass-false:check-bits"] = "entries of the 16-bit table carry no check bits (lz4_encode.hip:149 cbits = 0 for !U32TAB)"
UNREACHED["T16:search:empty-slot:position-0-matches"] = ("the 16-bit table hashes the four bytes that are compared (lz4_encode.hip:63): a position with the four bytes of position 0 "
                                                         "reads position 0's slot, which is filled (:195)")
for _k in ["second:neither", "second:back-to-the-walk", "chosen:sequence:second-visited", "chosen:sequence:second-entry"] + [f"second:{a}:{b}" for a in ("visited", "not-visited") for b in ("hitA", "hit", "hitA+hit")] + [f"second:pred:{v}" for v in PRED.values()]:
    UNREACHED[f"T16:{_k}"] = "the 16-bit table's scoreboard tells the first lane of a slot from all others, which are dirty: no second lanes (lz4_encode.hip:367-372)"
for _k in ["ring:reload", "ring:rotate", "ring:reset", "ring:jump-past-rend", "ring:c_hi==rend", "ring:piece_store:sh>0", "ring:piece_store:sh<0", "ring:piece_store:|sh|>=16"] + [f"ring:ralign={a}:block-{e}" for a in range(16) for e in ("start", "end")]:
    UNREACHED[f"T16:{_k}"] = "the input ring belongs to the 32-bit-table instance (lz4_encode.hip:297, :318)"
for _t in ("T16", "T32"):
    UNREACHED[f"{_t}:run_rt:e<2"] = ("run_rt needs e == anc and a dirty lane e; the anchor lane of a window is 0 on entry with a re-test, and lane 0 is the first of its slot, or the end "
                                     "of a match chosen in the window, which is lane 4 or later (lz4_encode.hip:565): `e >= 2` never decides")
    for _v in (269, 270):
        UNREACHED[f"{_t}:walk:before={_v}"] = ("a window begins with k0 <= 32 (lz4_encode.hip:281), so its first position is at most 1 + probe_offset(32) = 33 bytes behind the anchor: "
                                               "longer literal runs reach their match through the sparse batch (emit:lit=269 / 270 are required)")
# keys wanted of this catalogue that it does not reach yet and that are not known to be unreachable
OPEN = {}
REQUIRED = frozenset(_required() - set(UNREACHED) - set(OPEN))


@functools.lru_cache(None)
def expected():
    """[(label, data, cap, result, bytes, ring)]"""
    out = []
    for c in cases():
        for cap in _caps(c.name):
            r, b = port(c.data, cap)
            out.append((f"{c.name}|cap={cap}", c.data, cap, r, b, c.ring))
    return tuple(out)


FIXTURE = os.path.join(helpers.ROOT, "tests", "golden", "lz4_enc_shapes.json")


def digest(r, comp):
    return hashlib.sha256(str(int(r)).encode() + b":" + bytes(comp)).hexdigest()


def reference_digests(ref):
    """label -> SHA-256 of the result and bytes of the reference's own LZ4_compress_default (helpers.ref()) for every pair of expected(): what
    tests/golden/make_golden.py records in FIXTURE, for the machines that have no reference library"""
    out = {}
    for label, d, cap, _, _, _ in expected():
        dst = np.zeros(max(cap, 1) + 8, np.uint8)
        r = ref.LZ4_compress_default(d.ctypes.data, dst.ctypes.data, len(d), cap)
        out[label] = digest(r, dst[:max(r, 0)])
    return out
