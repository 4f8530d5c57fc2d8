"""The exact LZ4 fast encoder (lz4_encode.hip) runs its dense windows in a loop of their own; the sparse batch, the general
sequence routine, the last literals, a full output and the drain of a full record area are reached from that loop and lead
back into it.  Every hand-over, byte for byte against the reference's LZ4_compress_default (the reference library where it is
built, else the oracle), in raw mode (guard bytes behind the result) and in container mode: block sizes at which the last
window is and is not a dense one, searches that pass 32 probes at a window's start, matches that the window sizes itself (59
bytes) and that go through the general routine (60, 61, 1250 bytes, a catch-up in memory, a re-test hit) inside a window and
across its end, each way into the last literals, outputs that fill in a dense window and behind a sparse batch, and a record
area that fills right behind a general sequence and in the middle of dense windows.  Every generator asserts, from the
reference's compressed bytes (sequences, literal runs, match lengths, the probes of the search in front of a match), that its
block holds what it was built for; those assertions need no GPU and run in a test of their own."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers

gpu_test = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A
BIG = 65547                                     # the smallest block of the 32-bit table
MARK = bytes([0xF1, 0x07, 0xE2, 0x18, 0xD3, 0x29, 0xC4, 0x3A])
C12 = bytes([0x91, 0x13, 0xA2, 0x24, 0xB3, 0x35, 0xC4, 0x46, 0xD5, 0x57, 0xE6, 0x68])
RECORDS = 300                                   # FOURMC_LZ4_RECORDS of the drain case
REC_LIMIT = RECORDS - 128                       # the area is drained when it holds more (kRecSlack of lz4emit.h)


# ------------------------------------------------------------------------------------------------ the reference and its parse
def _bound(n):
    return helpers.oracle().orc_lz4_compress_bound(n)


def _compress(src, cap):
    """LZ4_compress_default of the reference's own sources where they are built, else the oracle's restatement"""
    L = helpers.ref()
    if L is None:
        return helpers.orc_compress(src, cap)
    src = np.ascontiguousarray(src, dtype=np.uint8)
    dst = np.empty(max(cap, 1) + 8, dtype=np.uint8)
    r = L.LZ4_compress_default(src.ctypes.data, dst.ctypes.data, len(src), cap)
    return r, dst[:max(r, 0)].copy()


_want_cache = {}


def _want(name, cap=None):
    """the reference's result for a named block (computed once per capacity)"""
    key = (name, cap)
    if key not in _want_cache:
        data = _blocks()[name]
        _want_cache[key] = _compress(data, _bound(len(data)) if cap is None else cap)
    return _want_cache[key]


def _parse(comp):
    """sequences of an LZ4 block as (literal length, match start, match length, offset); the last is (literals, n, None, None)"""
    out, i, n, pos = [], 0, len(comp), 0
    while i < n:
        tok = int(comp[i]); i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = int(comp[i]); i += 1; lit += b
                if b != 255:
                    break
        i += lit; pos += lit
        if i >= n:
            out.append((lit, pos, None, None)); break
        off = int(comp[i]) | int(comp[i + 1]) << 8; i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = int(comp[i]); i += 1; ml += b
                if b != 255:
                    break
        out.append((lit, pos, ml + 4, off)); pos += ml + 4
    return out


def _probe_offset(k):
    """distance of probe k of a search from its first probe: steps of 1 for 65 probes, one more every 64 (lz4.c:1014-1023)"""
    if k == 0:
        return 0
    t = k - 1
    m, r = t >> 6, t & 63
    return 1 + t + 32 * m * (m - 1) + m * r


def _probes(lit):
    """probes of the search in front of a match that has `lit` literals, at least (the hit lies at the match's first byte or
    behind it); 0: the re-test right behind the previous match hit"""
    if lit == 0:
        return 0
    k = 0
    while _probe_offset(k) < lit - 1:
        k += 1
    return k + 1


def _probed(lit):
    """distances from the previous match's end of the positions a search over `lit` literals put into the table"""
    out, k = set(), 0
    while 1 + _probe_offset(k) <= lit:
        out.add(1 + _probe_offset(k)); k += 1
    return out


def _first_overflow(seqs, cap):
    """index of the sequence at which LZ4_compress_generic gives up with this capacity (lz4.c:1096, 1183, 1270), and whether the
    literals (True) or the match length (False) did not fit; None when everything fits"""
    op = 0
    for i, (lit, _, ml, _) in enumerate(seqs):
        if ml is None:
            return (i, True) if op + lit + 1 + (lit + 255 - 15) // 255 > cap else None
        op += 1
        if op + lit + (2 + 1 + 5) + lit // 255 > cap:
            return i, True
        op += lit + (1 + (lit - 15) // 255 if lit >= 15 else 0) + 2
        if op + (1 + 5) + (ml - 4 + 240) // 255 > cap:
            return i, False
        op += 1 + (ml - 4 - 15) // 255 if ml - 4 >= 15 else 0
    return None


def _fail_caps(seqs):
    """(i, capacity) for every sequence i at which some capacity gives up first: the largest such capacity"""
    out, op, worst = [], 0, 0
    for i, (lit, _, ml, _) in enumerate(seqs):
        if ml is None:
            break
        need = op + 1 + lit + (2 + 1 + 5) + lit // 255
        op += 1 + lit + (1 + (lit - 15) // 255 if lit >= 15 else 0) + 2
        need = max(need, op + (1 + 5) + (ml - 4 + 240) // 255)
        op += 1 + (ml - 4 - 15) // 255 if ml - 4 >= 15 else 0
        if need > worst:
            if i:
                out.append((i, need - 1))
            worst = need
    return out


@functools.lru_cache(maxsize=None)
def _text():
    t = helpers.corpus(400000)                  # the corpus begins with its text class
    t.setflags(write=False)
    assert t[:330000].max() < 0x80
    return t


class _Gen:
    """A block put together from text, fresh random bytes and copies of earlier bytes.  `planted` lists the copies as the
    matches the parse has to find: (start, length, offset)."""

    def __init__(self, seed, t=0):
        self.rng = np.random.default_rng(seed)
        self.out = bytearray()
        self.t = t
        self.avoid = None                       # what the next byte must not be: the byte behind the last copy's source
        self.planted = []

    def _add(self, b, fresh):
        b = bytearray(b)
        if b and self.avoid is not None and b[0] == self.avoid:
            assert fresh, "a copy would go on into what follows it"
            b[0] ^= 0x55
        if b:
            self.avoid = None
        self.out += b

    def text(self, k):
        self._add(_text()[self.t:self.t + k].tobytes(), False); self.t += k

    def text_to(self, size):
        self.text(size - len(self.out))

    def noise(self, k, last_not=None):
        b = bytearray(self.rng.integers(0, 256, k, dtype=np.uint8).tobytes())
        if k and last_not is not None and b[-1] == last_not:
            b[-1] ^= 0x2B
        self._add(b, True)

    def source(self, k):
        """the marker twice (the second is a match of the first, if of nothing else: a search begins behind it), k fresh bytes, the
        marker: the search that runs over the bytes puts the first 66 of them into the table one by one and the rest at its
        growing steps; returns where they begin"""
        self._add(MARK + MARK, False); p = len(self.out); self.noise(k); self._add(MARK, False)
        return p

    def copy(self, src, length, lits):
        """`lits` fresh bytes and a copy of [src, src + length) that matches neither a byte earlier nor a byte longer"""
        if lits:
            self.noise(lits, last_not=self.out[src - 1])
        else:
            assert self.out[-1] != self.out[src - 1]
        p = len(self.out)
        self._add(bytes(self.out[src:src + length]), False)
        self.avoid = self.out[src + length]
        self.planted.append((p, length, p - src))
        return p

    def units(self, k):
        """k times four fresh bytes and the same twelve: one sequence each (but the first), a match of 12 at offset 16"""
        for _ in range(k):
            self.noise(4, last_not=C12[-1]); self._add(C12, False)

    def data(self):
        return np.frombuffer(bytes(self.out), np.uint8).copy()


def _has(seqs, planted):
    """every planted copy is a match of the parse, with its start, length and offset"""
    found = {(s, ml, off) for _, s, ml, off in seqs}
    for p in planted:
        assert p in found, (p, [q for q in sorted(found) if abs(q[0] - p[0]) < 80])
    return {s: i for i, (_, s, _, _) in enumerate(seqs)}


# ------------------------------------------------------------------------------------------------ the blocks
@functools.lru_cache(maxsize=None)
def _features():
    """About 128 KiB: every hand-over between the dense windows, the sparse batch and the general routine.  A long match (100
    bytes: the general routine) ends a window, so the next window begins at its end E; what follows is placed against E."""
    g = _Gen(101)
    g.text(3000)
    at = {}

    def window(tag, n_src=160):
        src = g.source(n_src)
        g.text(260)
        e = g.copy(src, 100, 3) + 100
        at[tag] = (src, e)
        return src, e

    # a search that passes 32 probes where a window begins: the match before it ends at lane 31 (32 probes made when the next
    # window begins: it is a dense one and ends at the first probe two bytes on) and at lane 30 (33: the sparse batch)
    for tag, lits in (("k32", 19), ("k33", 18)):
        src, e = window(tag)
        g.copy(src + 20, 12, lits)
        assert len(g.out) == e + (31 if tag == "k32" else 30)
        g.noise(700); g.text(600)
    # matches of 59 bytes (sized by the window), 60 and 61 (the general routine) that end inside the window they begin in ...
    for tag, length, lits in (("in59", 59, 1), ("in60", 60, 1), ("in61", 61, 2)):
        src, e = window(tag)
        g.copy(src + 10, length, lits)
        assert len(g.out) <= e + 63
        g.noise(3); g.text(300)
    # ... and that cross its end
    for tag, length, lits in (("x59", 59, 10), ("x60", 60, 10), ("x61", 61, 40)):
        src, e = window(tag)
        g.copy(src + 10, length, lits)
        assert len(g.out) > e + 64
        g.noise(3); g.text(300)
    # over 1100 bytes, out of a dense window
    src, e = window("long", 1400)
    g.copy(src + 30, 1250, 6)
    g.noise(3); g.text(300)
    # the re-test right behind a match hits: no literals, a short match and one for the general routine
    src, e = window("rt")
    g.copy(src + 5, 20, 0); g.copy(src + 40, 70, 0)
    g.noise(3); g.text(300)
    # a catch-up of five bytes in memory behind eight literals: the search over the source's bytes stepped by six where the copy's
    # source begins, so the first position of the copy that finds its source in the table is the sixth
    src = g.source(1100)
    g.text(260)
    at["catch"] = (src, g.copy(src + 963, 24, 8))
    g.noise(3); g.text(300)
    # sparse -> dense -> sparse: random bytes and text in turn
    for _ in range(6):
        g.noise(1500); g.text(1500)
    g.text_to(131072 + 77)
    return g, at


def _check_features(g, at, seqs):
    idx = _has(seqs, g.planted)
    n = len(g.out)
    assert n >= 2 * BIG - 100
    for tag in ("k32", "k33"):
        src, e = at[tag]
        i = next(i for i, (_, s, ml, _) in enumerate(seqs) if ml and s + ml == e)
        assert seqs[i][2] == 100                                    # leaves its window: the next begins at e
        lit, s, ml, _ = seqs[i + 1]
        assert s + ml == e + (31 if tag == "k32" else 30) and lit >= 1 and ml < 60
        assert seqs[i + 2][0] >= 700 and _probes(seqs[i + 2][0]) > 64   # the search behind it: well past 32 probes, strided
        assert any(ml is not None and lit < 32 for lit, _, ml, _ in seqs[i + 3:i + 8])   # and the text brings the dense windows back
    for tag in ("in59", "in60", "in61", "x59", "x60", "x61"):
        src, e = at[tag]
        i = next(i for i, (_, s, ml, _) in enumerate(seqs) if ml and s + ml == e)
        lit, s, ml, _ = seqs[i + 1]
        assert ml == int(tag[-2:]) and _probes(lit) <= 64
        assert (s + ml <= e + 63) == tag.startswith("in"), (tag, s - e, ml)
    assert any(ml and ml == 1250 for _, _, ml, _ in seqs)
    src, e = at["rt"]
    i = next(i for i, (_, s, ml, _) in enumerate(seqs) if ml and s + ml == e)
    assert seqs[i + 1][0] == 0 and seqs[i + 1][2] == 20 and seqs[i + 2][0] == 0 and seqs[i + 2][2] == 70
    # the catch-up: the source's bytes are one literal run whose search put position src + 968 into the table and none of the
    # five before it, so the hit was at the copy's sixth byte and five bytes were caught up, with eight literals in front
    src, p = at["catch"]
    run = next((lit, s) for lit, s, ml, _ in seqs if s - lit <= src < s and lit >= 1100)
    start = run[1] - run[0]                                          # the previous match's end
    probed = _probed(run[0])
    assert start == src and src + 968 - start in probed and not any(src + 963 + j - start in probed for j in range(5))
    lit, s, ml, off = seqs[idx[p]]
    assert (lit, ml, off) == (8, 24, p - (src + 963))
    assert sum(1 for lit, _, _, _ in seqs if lit >= 1400) >= 6         # the sparse stretches at the end


@functools.lru_cache(maxsize=None)
def _ends():
    """Blocks of 65547 + d bytes in which a match of 100 bytes ends at E = 65546.  d = 0, 1: the match runs into the block's end
    (last literals out of the general routine).  d = 130: no window can begin at E (E + 132 > n): the sparse batch runs to the
    end.  d = 131, 132: the last window begins at E with E + 132 = n and n - 1; 63 bytes on, a match of 59 bytes - the longest
    the window sizes itself - ends at E + 122 >= n - 11: last literals out of the window itself.  d = 133: the same match ends
    in front of the limit, and the sparse batch that follows reaches the end."""
    g = _Gen(102, t=40000)
    E = BIG - 1
    g.text(E - 100 - 3 - 260 - 160 - 24)
    src = g.source(160)
    g.text(260)
    assert g.copy(src, 100, 3) + 100 == E
    cut = g.data()                                                  # (the copy goes on for d = 0, 1: its source does)
    g.copy(src + 30, 59, 63)
    assert len(g.out) == E + 122
    g.noise(40)
    full = g.data()
    out = {}
    for d in (0, 1):
        out[f"end{d}"] = np.concatenate([cut, np.frombuffer(bytes(g.out[src + 100:src + 101 + d]), np.uint8)])
    for d in (130, 131, 132, 133):
        out[f"end{d}"] = full[:BIG + d].copy()
    return out, E


def _check_ends(blocks, E, parses):
    for d in (0, 1):
        seqs = parses[f"end{d}"]
        n = BIG + d
        assert len(blocks[f"end{d}"]) == n
        lit, s, ml, _ = seqs[-2]
        assert s == E - 100 and s + ml == n - 5 and ml >= 60 and seqs[-1][0] == 5   # ends at the match limit: the general routine
    for d in (130, 131, 132, 133):
        seqs = parses[f"end{d}"]
        n = BIG + d
        assert len(blocks[f"end{d}"]) == n
        i = next(i for i, (_, s, ml, _) in enumerate(seqs) if ml and s + ml == E)
        assert seqs[i][2] == 100
        lit, s, ml, _ = seqs[i + 1]
        assert (lit, s, ml) == (63, E + 63, 59) and _probes(lit) == 63 and seqs[i + 2][2] is None
        assert (E + 132 <= n) == (d >= 131) and (E + 122 >= n - 11) == (d <= 132)


@functools.lru_cache(maxsize=None)
def _starts():
    """The first dense window begins at position 4 (and at 5): the block's first bytes have a period of three (four), so the
    sparse batch that begins every block is cut where position 4 (5) meets the table slot of position 1, and that position is the
    first match"""
    out = {}
    for period in (3, 4):
        g = _Gen(110 + period)
        unit = bytes(range(0xA0, 0xA0 + period))
        g._add(bytes([0x11]) + (unit * 20)[:41], False)
        g.noise(5); g.text_to(BIG + 500 + period)
        out[f"start{period + 1}"] = g.data()
    return out


def _check_starts(parses):
    for period in (3, 4):
        lit, s, ml, off = parses[f"start{period + 1}"][0]
        assert (lit, s, off) == (period + 1, period + 1, period) and ml == 41 - period, (lit, s, ml, off)
        assert _probes(lit) == period + 1


@functools.lru_cache(maxsize=None)
def _tails():
    """the sparse batch reaches the end: with a probe past the limit, and with a match that runs into it"""
    g = _Gen(120, t=90000)
    g.text(BIG); g.noise(400)
    a = g.data()
    g = _Gen(121, t=95000)
    g.text(BIG - 300)
    src = g.source(50)
    g.noise(400); g.copy(src, 40, 30)
    g.avoid = None
    g._add(bytes(g.out[src + 40:src + 50]), False)                   # the match goes on to the match limit
    return {"tail_probe": a, "tail_match": g.data()}


def _check_tails(blocks, parses):
    seqs = parses["tail_probe"]
    assert seqs[-1][0] >= 400 and _probes(seqs[-1][0]) > 64
    seqs, n = parses["tail_match"], len(blocks["tail_match"])
    lit, s, ml, _ = seqs[-2]
    assert lit >= 400 and _probes(lit) > 64 and s + ml == n - 5 and seqs[-1][0] == 5


@functools.lru_cache(maxsize=None)
def _fills():
    """Blocks that do not fit into n - 1 bytes (container mode stores them).  `fill_dense`: 125 000 random bytes, a run of one
    byte (the search, by then in steps of some sixty bytes, finds it), then 18 short sequences - the output fills at one of
    them, a few sequences behind the long literal run and 200 bytes in front of the end; the run's length is chosen for that.
    `fill_sparse`: the match that ends the random bytes is found by the sparse batch and its literals do not fit."""
    dense = None
    for run in range(200, 330):
        g = _Gen(130)
        g.noise(125000, last_not=0x77); g._add(bytes([0x77]) * run, False)
        g.units(18)
        d = g.data()
        seqs = _parse(_compress(d, _bound(len(d)))[1])
        hit = _first_overflow(seqs, len(d) - 1)
        if hit and hit[0] >= 5 and seqs[hit[0]][1] + 200 <= len(d):
            dense = d
            break
    assert dense is not None
    g = _Gen(131)
    src = g.source(40)
    g.noise(70000); g.copy(src, 24, 1); g.noise(100)
    return {"fill_dense": dense, "fill_sparse": g.data()}


def _check_fills(blocks, parses):
    seqs, n = parses["fill_dense"], len(blocks["fill_dense"])
    i, literals = _first_overflow(seqs, n - 1)
    assert i >= 5 and all(lit == 4 and ml == 12 for lit, _, ml, _ in seqs[2:i + 1]), (i, seqs[:i + 2])
    assert seqs[0][0] >= 125000 and seqs[0][2] >= 200 and seqs[i][1] + 200 <= n   # a dense window is where it happens
    assert _want("fill_dense", n - 1)[0] == 0
    seqs, n = parses["fill_sparse"], len(blocks["fill_sparse"])
    i, literals = _first_overflow(seqs, n - 1)
    assert literals and seqs[i][0] >= 70000 and _probes(seqs[i][0]) > 64
    assert _want("fill_sparse", n - 1)[0] == 0


@functools.lru_cache(maxsize=None)
def _drain():
    """With record areas of RECORDS records the area is drained when it holds more than REC_LIMIT.  The block's first
    REC_LIMIT sequences are short ones and the next is a match of 200 bytes: the area fills right behind a general sequence.
    Text follows: it fills many more times in the middle of dense windows."""
    def build(units):
        g = _Gen(140, t=150000)
        src = g.source(230)
        g.units(units)
        long_at = g.copy(src, 200, 3)
        g.noise(3); g.text_to(BIG + 3000)
        return g, long_at
    g, long_at = build(REC_LIMIT)
    seqs = _parse(_compress(g.data(), _bound(len(g.out)))[1])
    first = next(i for i, (_, s, _, _) in enumerate(seqs) if s == long_at)
    g, long_at = build(REC_LIMIT - (first - REC_LIMIT))
    return g, long_at


def _check_drain(g, long_at, seqs):
    idx = _has(seqs, g.planted)
    i = idx[long_at]
    assert i == REC_LIMIT and seqs[i][2] == 200                      # record REC_LIMIT + 1 is the general sequence's
    assert all(ml is not None and ml < 60 for _, _, ml, _ in seqs[:i])
    assert len(seqs) > 10 * REC_LIMIT                                # and the text fills it again and again
    dense = sum(1 for lit, _, ml, _ in seqs[i + 1:] if ml is not None and lit < 32 and ml < 60)
    assert dense > 0.8 * (len(seqs) - i)


@functools.lru_cache(maxsize=None)
def _blocks():
    blocks = {}
    blocks["features"] = _features()[0].data()
    blocks.update(_ends()[0])
    blocks.update(_starts())
    blocks.update(_tails())
    blocks.update(_fills())
    blocks["drain"] = _drain()[0].data()
    text = _text()
    blocks["size128k"] = text[200000:200000 + 131072].copy()
    for b in blocks.values():
        assert len(b) >= BIG
        b.setflags(write=False)
    return blocks


@functools.lru_cache(maxsize=None)
def _checked():
    """every generator's assertions, from the reference's parse of its blocks; returns the blocks"""
    blocks = _blocks()
    parses = {k: _parse(_want(k)[1]) for k in blocks}
    for k, b in blocks.items():                                      # the parse is one of the block: it covers every byte
        assert parses[k][-1][1] == len(b), k
    g, at = _features()
    assert np.array_equal(g.data(), blocks["features"])
    _check_features(g, at, parses["features"])
    _check_ends(blocks, _ends()[1], parses)
    _check_starts(parses)
    _check_tails(blocks, parses)
    _check_fills(blocks, parses)
    g, long_at = _drain()
    _check_drain(g, long_at, parses["drain"])
    return blocks


def test_generators_hold_their_features():
    """needs no GPU: the reference's own parse of every block contains what the block was built for"""
    blocks = _checked()
    assert {len(blocks[f"end{d}"]) - BIG for d in (0, 1, 131, 132, 133)} == {0, 1, 131, 132, 133}
    assert abs(len(blocks["size128k"]) - (128 << 10)) < 1024 and abs(len(blocks["features"]) - (128 << 10)) < 1024


# ------------------------------------------------------------------------------------------------ the device against the reference
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _layout(srcs, align):
    offs, pos = [], 0
    for s, a in zip(srcs, align):
        pos += (a - pos) % 16
        offs.append(pos); pos += len(s)
    buf = np.zeros(pos + 16, np.uint8)
    for s, o in zip(srcs, offs):
        buf[o:o + len(s)] = s
    return buf, offs


def _check_raw(gpu, srcs, wants, caps, align):
    buf, offs = _layout(srcs, align)
    dsts, dpos = [], 5
    for c in caps:
        dsts.append(dpos); dpos += c + 40
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, [len(s) for s in srcs], caps))
    d_out = torch.full((dpos,), GUARD, dtype=torch.uint8, device="cuda")
    gpu.lz4_compress_fast(_dev(buf), d_out, batch)
    res = [int(r) for r in batch.download()["result"]]
    out = d_out.cpu().numpy()
    for i, (s, c, d, (want_r, want)) in enumerate(zip(srcs, caps, dsts, wants)):
        assert res[i] == want_r, (i, len(s), c, res[i], want_r)
        if want_r > 0:
            assert np.array_equal(out[d:d + want_r], want), (i, len(s), c)
        assert (out[d + max(want_r, 0):d + c + 40] == GUARD).all(), (i, len(s), c, "bytes written past the result")


def _check_container(gpu, srcs, wants, align):
    """container mode: capacity n - 1, stored when it does not fit (`wants`: the reference's results at that capacity)"""
    buf, offs = _layout(srcs, align)
    lens = [len(s) for s in srcs]
    dsts, dpos = [], 0
    for n in lens:
        dsts.append(dpos); dpos += n + 64
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, lens, lens))
    d_out = torch.full((dpos,), GUARD, dtype=torch.uint8, device="cuda")
    gpu.encode_blocks(_dev(buf), d_out, batch)
    enc = batch.download()
    out = d_out.cpu().numpy()
    for i, (s, (want_r, want)) in enumerate(zip(srcs, wants)):
        if want_r <= 0:
            want_r, want = len(s), s
        r = int(enc["result"][i])
        assert r == want_r, (i, len(s), r, want_r)
        assert np.array_equal(out[dsts[i]:dsts[i] + r], want), i
        assert (out[dsts[i] + r:dsts[i] + lens[i] + 64] == GUARD).all(), (i, "bytes written past the result")
        assert int(enc["xxh32"][i]) == helpers.orc_xxh32(want), i


def _small(name):
    """blocks of the 16-bit table, an empty one and one of 12 bytes: not from _blocks(), compressed where they are used"""
    text = _text()
    return {"empty": np.zeros(0, np.uint8), "twelve": text[7:19].copy(), "small_text": text[:BIG - 1].copy(),
            "small_5000": text[300000:305000].copy(),
            "small_noise": np.random.default_rng(150).integers(0, 256, 3000, dtype=np.uint8)}[name]


def _both(gpu, names, align=None):
    """raw mode at the compress bound and container mode, for named blocks in one launch each"""
    blocks = _checked()
    srcs, bound, cont = [], [], []
    for k in names:
        if k in blocks:
            s = blocks[k]; srcs.append(s); bound.append(_want(k)); cont.append(_want(k, max(len(s) - 1, 0)))
        else:
            s = _small(k); srcs.append(s); bound.append(_compress(s, _bound(len(s)))); cont.append(_compress(s, max(len(s) - 1, 0)))
    align = align or [(5 * i) % 16 for i in range(len(srcs))]
    _check_raw(gpu, srcs, bound, [_bound(len(s)) for s in srcs], align)
    _check_container(gpu, srcs, cont, align)


@gpu_test
def test_block_sizes_around_the_last_window(gpu):
    _both(gpu, ["end0", "end1", "end130", "end131", "end132", "end133", "size128k"])


@gpu_test
def test_hand_overs_between_the_loops(gpu):
    _both(gpu, ["features", "start4", "start5"], [0, 0, 7])


@gpu_test
def test_ways_into_the_last_literals(gpu):
    _both(gpu, ["end0", "end131", "end132", "end133", "tail_probe", "tail_match"])


@gpu_test
def test_output_full(gpu):
    """container mode stores both blocks; raw mode gives up (result 0) at capacities at which the features block fills in a
    sequence the window sizes, in a match of the general routine and in the literals behind a sparse batch - and fits exactly"""
    blocks = _checked()
    _both(gpu, ["fill_dense", "fill_sparse"])
    data, seqs = blocks["features"], _parse(_want("features")[1])
    csz = _want("features")[0]
    picks = {}
    for i, cap in _fail_caps(seqs):
        lit, _, ml, _ = seqs[i]
        kind = "sparse" if lit >= 700 else "general" if ml is not None and ml >= 60 and lit < 64 else "window" if ml is not None and lit < 32 else None
        if kind and len([c for c, k in picks.items() if k == kind]) < 3:
            assert _first_overflow(seqs, cap)[0] == i
            picks[cap] = kind
    assert sorted(set(picks.values())) == ["general", "sparse", "window"], picks
    caps = sorted(picks) + [csz - 1, csz, csz + 1]
    wants = [_want("features", c) for c in caps]
    assert [w[0] for w in wants] == [0] * (len(caps) - 2) + [csz, csz]
    _check_raw(gpu, [data] * len(caps), wants, caps, [3 * i % 16 for i in range(len(caps))])


@gpu_test
def test_mixed_launch(gpu):
    names = ["small_text", "features", "empty", "end131", "small_noise", "start4", "fill_sparse", "twelve", "tail_match", "end0",
             "small_5000", "drain", "fill_dense", "empty", "end133", "tail_probe"]
    _both(gpu, names, [3, 5, 1, 14, 0, 7, 15, 4, 0, 11, 6, 9, 2, 13, 8, 10])


_CHILD = """
import helpers
import test_gpu_lz4_mode_changes as t
p = helpers.pkg(); p.gpu_init(0)
t._both(p, ["drain", "features", "small_text", "end131"])
print("ok")
"""


@gpu_test
def test_drain_behind_a_general_sequence_and_between_windows(gpu):
    """record areas of RECORDS records (the way tests/test_gpu_lz4_emit.py runs its drain cases: a child process with
    FOURMC_LZ4_RECORDS set): the area fills right behind the general sequence that is record REC_LIMIT + 1 of the block, and
    then in the middle of the text's dense windows"""
    _checked()
    env = dict(os.environ)
    env["FOURMC_LZ4_RECORDS"] = str(RECORDS)
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout, r.stdout + r.stderr
