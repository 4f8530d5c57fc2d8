"""The dense window of the exact LZ4 fast encoder (lz4_encode.hip) works out, for every lane at once, where the walk goes behind
a chosen match (`nextE` / `fin`: the first event at or after the lane the match lands on) and whether a second lane of a table
slot has its predecessor's four bytes (`wpred`).  Both come from wave permutes that the window asks for early and waits for
once.  Every shape those values decide, byte for byte against the reference's LZ4_compress_default (the reference library
where it is built, else the oracle), in raw mode (guard bytes behind the result) and in container mode:

* landing shapes - a match chosen in a window ends at lane L of the same window, and at L there is: a hit (the re-test, no
  literals); the next hit d = 1 .. 6 bytes on, with a candidate that matches four bytes and more backwards (from d = 5 on the
  catch-up goes through memory and ends the chain); as the first event a stop lane - the third lane of a slot, a match of 60
  bytes and more, a second lane of a slot; nothing at all; for L in the middle of the window and at 59 .. 63, matches that end
  at lanes 64 and 65, and a chain of ten hits in one window;
* slot sharing - two positions of one window in one table slot, the first one a probe, inside a chosen match or the refill
  lane two bytes in front of a match's end, the second one with the first one's four bytes or others, with the table entry's
  four bytes or others, at lanes 0/1, 0/63, 62/63 and in the middle, as the landing point of an earlier match, and three in a
  slot.

Positions are kept out of the table, and put into one slot, with five-byte strings chosen for their hash.  A model of the
parse written here (the table, the probes, the refill, the re-test) must give the reference's sequences for every block, and
every generator asserts on that model's record - which probe hit, which candidate it saw, what was never a probe - that its
block holds what it was built for; those assertions need no GPU and run in a test of their own."""
import functools

import numpy as np
import pytest

import test_gpu_lz4_mode_changes as mc

gpu_test = pytest.mark.gpu
BIG = mc.BIG                                    # the smallest block of the 32-bit table
MARK = mc.MARK
EDGES = (59, 60, 61, 62, 63)


# ------------------------------------------------------------------------------------------------ hashes and a model of the parse
def _hashes(data, small):
    """the table slot of every position (lz4.c:758-769: four bytes into 13 bits below 65547 bytes, else five into 12) and its
    four bytes as a number"""
    n = len(data)
    pad = np.concatenate([np.asarray(data, np.uint8), np.zeros(8, np.uint8)])
    w = np.zeros(n, np.uint64)
    for i in range(5):
        w |= pad[i:i + n].astype(np.uint64) << np.uint64(8 * i)
    w4 = w & np.uint64(0xFFFFFFFF)
    if small:
        h = ((w4 * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)
    else:
        h = ((w << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(52)
    return h, w4


def _slot(five, small):
    return int(_hashes(np.frombuffer(bytes(five[:5]), np.uint8), small)[0][0])


class _Model:
    """LZ4_compress_generic at acceleration 1 (lz4.c:981-1264), with a record: `matches` (probe that hit, candidate it saw, start,
    length), `seen` (position -> the candidate a probe or re-test there read), `refill` (positions entered two bytes in front of
    a match's end)"""

    def __init__(self, data):
        b = bytes(np.asarray(data, np.uint8)); n = len(b)
        small = n < BIG
        self.matches, self.seen, self.refill, self.seqs = [], {}, set(), []
        if n < 13:
            self.seqs.append((n, n, None, None))
            return
        h, w4 = _hashes(data, small)
        H, W = h.tolist(), w4.tolist()
        last_probe, mlimit = n - 11, n - 5
        tab = {H[0]: 0}
        ip, anchor, done = 1, 0, False
        while not done:
            fip, step, nb = ip, 1, 64
            while True:
                ip = fip; fip += step; step = nb >> 6; nb += 1
                if fip > last_probe:
                    done = True
                    break
                m = tab.get(H[ip], 0); tab[H[ip]] = ip; self.seen[ip] = m
                if (small or m + 65535 >= ip) and W[m] == W[ip]:
                    break
            while not done:
                s, ms = ip, m
                while s > anchor and ms > 0 and b[s - 1] == b[ms - 1]:
                    s -= 1; ms -= 1
                i, j = ip + 4, m + 4
                while i < mlimit and b[i] == b[j]:
                    i += 1; j += 1
                self.matches.append((ip, m, s, i - s))
                self.seqs.append((s - anchor, s, i - s, s - ms))
                ip = anchor = i
                if ip >= last_probe:
                    done = True
                    break
                tab[H[ip - 2]] = ip - 2; self.refill.add(ip - 2)
                m = tab.get(H[ip], 0); tab[H[ip]] = ip; self.seen[ip] = m
                if not ((small or m + 65535 >= ip) and W[m] == W[ip]):
                    ip += 1
                    break
        self.seqs.append((n - anchor, n, None, None))
        self.at = {s: (hit, cand, ln) for hit, cand, s, ln in self.matches}

    def none_from(self, lo, hi):
        """no match begins in [lo, hi)"""
        assert not [s for s in self.at if lo <= s < hi], (lo, hi, [s for s in self.at if lo <= s < hi])


# ------------------------------------------------------------------------------------------------ the generators
class _Block:
    """Windows at chosen places: a source area A of 160 fresh bytes (the search that runs over them enters the first 66 into the
    table one by one) and, three fresh bytes on, a copy of A[60:160] - a match of 100 bytes, which leaves its window, so the next
    dense window begins at its end e and lane l of it is position e + l.  `checks` are the assertions on the model's record."""

    def __init__(self, seed, t, small=False):
        self.g = mc._Gen(seed, t)
        self.small = small
        self.checks = []
        self.names = []
        self.needs = []
        self.g.text(1500)

    def need(self, pos, *others):
        """among this window's bytes (A to the window's end) the table slot of `pos` belongs to copies of its bytes and to `others`
        alone: nothing else there can take the slot away from the position that is meant to hold it.  A window that does not
        meet this is built again"""
        self.needs.append((pos, others))

    def collide(self, five, prefix=b""):
        """five bytes (beginning with `prefix`) of the table slot of `five`, and not its four bytes"""
        want = _slot(five, self.small)
        while True:
            cand = self.g.rng.integers(0, 256, (1 << 16, 5), dtype=np.uint8)
            cand[:, :len(prefix)] = np.frombuffer(bytes(prefix), np.uint8)
            h, _ = _hashes(cand.reshape(-1), self.small)
            for k in np.nonzero(h[::5] == want)[0]:
                c = bytes(cand[k])
                if c[:4] != bytes(five[:4]):
                    return c

    def area(self):
        return self.g.source(160)

    def fresh(self, k):
        """k fresh bytes that may stand right behind a copy of A's end"""
        while True:
            t = bytes(self.g.rng.integers(0, 256, k, dtype=np.uint8))
            if t[0] != MARK[0]:
                return t

    def open(self, a):
        g = self.g
        e = g.copy(a + 60, 100, 3) + 100
        self.need(a + 60)
        self.checks.append(lambda m, e=e: self._long_ends(m, e))
        return e

    @staticmethod
    def _long_ends(m, e):
        assert any(s + ln == e and ln == 100 for s, (_, _, ln) in m.at.items()), e

    def lits(self, e, upto, tokens=(), last_not=None):
        """fresh bytes up to lane `upto` of the window at e, with (lane, bytes) tokens written into them"""
        g = self.g
        start = len(g.out)
        k = e + upto - start
        assert k >= 0, (upto, start - e)
        avoid = g.avoid
        g.noise(k, last_not=last_not)
        for lane, tok in tokens:
            assert start <= e + lane and e + lane + len(tok) <= start + k, (lane, len(tok), start - e, k)
            g.out[e + lane:e + lane + len(tok)] = tok
        if k:
            assert avoid is None or g.out[start] != avoid
            assert last_not is None or g.out[-1] != last_not

    def differ(self, p, q):
        """make the byte at p another one than the byte at q (p is a fresh byte that nothing has copied yet)"""
        if self.g.out[p] == self.g.out[q]:
            self.g.out[p] ^= 0x3C

    def plant(self, src, length):
        g = self.g
        p = len(g.out)
        g._add(bytes(g.out[src:src + length]), False)
        g.avoid = g.out[src + length]
        return p

    def close(self, k=150):
        self.g.noise(3); self.g.text(k)


def _case(build):
    """build a window; again, with other fresh bytes, until its slots are its own (`need`)"""
    def again(self, *args):
        g = self.g
        for _ in range(40):
            keep = (len(g.out), g.t, len(g.planted), g.avoid, len(self.checks), len(self.names))
            self.needs = []
            build(self, *args)
            base, k = keep[0], 4 if self.small else 5
            h, _ = _hashes(np.frombuffer(bytes(g.out[base:]), np.uint8), self.small)
            if all(bytes(g.out[base + q:base + q + k]) == bytes(g.out[pos:pos + k]) or base + q in others
                   for pos, others in self.needs for q in np.nonzero(h[:-8] == h[pos - base])[0].tolist()):
                return
            del g.out[keep[0]:], g.planted[keep[2]:], self.checks[keep[4]:], self.names[keep[5]:]
            g.t, g.avoid = keep[1], keep[3]
        raise AssertionError(build.__name__)
    return again


class _Shapes(_Block):
    """one method per shape; each builds one window and says, in `checks`, what the model's record must show for it"""

    def m1(self, a, e, L, off=48, tokens=()):
        """the chosen match of the window at e: 20 bytes of A[off:], ending at lane L"""
        assert L >= 21 and off < 60
        self.lits(e, L - 20, tokens, last_not=self.g.out[a + off - 1])
        p = self.plant(a + off, 20)
        assert p == e + L - 20
        self.need(a + off)
        self.checks.append(lambda m, p=p, c=a + off: self._is(m, p, p, c, 20))
        return p

    @staticmethod
    def _is(m, start, hit, cand, length):
        assert m.at.get(start) == (hit, cand, length), (start, m.at.get(start), (hit, cand, length))

    # ---------------------------------------------------------------- landing shapes
    @_case
    def retest_hit(self, L):
        a = self.area(); o = self.g.out
        self.differ(a + 29, a + 67); self.differ(a + 68, a + 30)
        e = self.open(a)
        self.m1(a, e, L)
        p = self.plant(a + 30, 10)
        self.need(a + 30)
        self.close()
        self.checks.append(lambda m: self._is(m, p, p, a + 30, 10))
        self.names.append(f"retest L={L}")

    @_case
    def back(self, L, d):
        """the bytes behind the match are A[0:d + 12]; strings of the slots of A[0], .. A[d - 1] stand later in A and own those
        slots, so the first position that finds its source in the table is lane L + d, and the d bytes (and, in front of them, the
        match's last bytes: they are the bytes in front of A) match backwards"""
        a = self.area(); o = self.g.out
        o[a + 64:a + 68] = MARK[4:8]
        for i in range(d):
            o[a + 18 + 5 * i:a + 23 + 5 * i] = self.collide(o[a + i:a + i + 5])
        self.differ(a + 68, a)
        e = self.open(a)
        self.m1(a, e, L)
        p = self.plant(a, d + 12)
        for i in range(d):
            self.need(a + i, a + 18 + 5 * i)
        self.need(a + d)
        self.close()

        def check(m):
            self._is(m, p, p + d, a + d, d + 12)
            for i in range(d):
                assert m.seen[p + i] == a + 18 + 5 * i, (L, d, i, m.seen[p + i] - a)
            assert bytes(o[p - 4:p]) == bytes(o[a - 4:a])
        self.checks.append(check)
        self.names.append(f"back L={L} d={d}")

    @_case
    def dirty(self, L, k):
        """three strings of one slot at lanes 0, 5 and L + k"""
        a = self.area(); o = self.g.out
        c1 = self.fresh(5)
        c2 = self.collide(c1); c3 = self.collide(c1)
        assert len({c1[:4], c2[:4], c3[:4]}) == 3
        if k == 0 and o[a + 68] == c3[0]:
            o[a + 68] ^= 0x3C
        if o[a + 47] == c2[4]:
            o[a + 47] ^= 0x3C
        e = self.open(a)
        self.m1(a, e, L, tokens=[(0, c1), (5, c2)])
        self.lits(e, L + k + 10, [(L + k, c3)])
        self.need(e, e + 5, e + L + k)
        self.close()

        def check(m):
            assert m.seen[e + 5] == e and m.seen[e + L + k] == e + 5
            m.none_from(e + L, e + L + k + 10)
        self.checks.append(check)
        self.names.append(f"dirty L={L} k={k}")

    @_case
    def slow(self, L, k):
        a = self.area(); o = self.g.out
        if k == 0:
            self.differ(a + 1, a + 67)
        self.differ(a + 68, a + 2)
        e = self.open(a)
        self.m1(a, e, L)
        self.lits(e, L + k, last_not=o[a + 1])
        p = self.plant(a + 2, 70)
        self.need(a + 2)
        self.close()
        self.checks.append(lambda m: self._is(m, p, p, a + 2, 70))
        self.names.append(f"slow L={L} k={k}")

    @_case
    def second(self, L, k):
        """five bytes at lane 2 and again at L + k"""
        a = self.area(); o = self.g.out
        T = self.fresh(5)
        if k == 0 and o[a + 68] == T[0]:
            o[a + 68] ^= 0x3C
        e = self.open(a)
        self.m1(a, e, L, tokens=[(2, T)])
        self.lits(e, L + k + 10, [(L + k, T)])
        p = e + L + k
        self.differ(p + 5, e + 7)
        if k:
            self.differ(p - 1, e + 1)
        self.need(e + 2)
        self.close()
        self.checks.append(lambda m: self._is(m, p, p, e + 2, 5))
        self.names.append(f"second L={L} k={k}")

    @_case
    def nothing(self, L):
        a = self.area()
        e = self.open(a)
        self.m1(a, e, L)
        self.lits(e, L + 70)
        self.close()
        self.checks.append(lambda m: m.none_from(e + L, e + L + 70))
        self.names.append(f"nothing L={L}")

    @_case
    def chain(self):
        a = self.area()
        e = self.open(a)
        ps = [self.g.copy(a + 6 * i, 6, 1) for i in range(10)]
        assert ps[8] + 6 <= e + 64
        for i in range(10):
            self.need(a + 6 * i)
        self.close()
        self.checks.append(lambda m: [self._is(m, p, p, a + 6 * i, 6) for i, p in enumerate(ps)])
        self.names.append("chain")

    # ---------------------------------------------------------------- slot sharing
    @_case
    def probe_pair(self, p1, p2, equal, entry):
        """the first one a probe.  equal: five fresh bytes at both lanes (the second finds the first) - else a string of the same
        slot at the first; entry: the second one's bytes stand in A, which owns the slot when the window begins"""
        a = self.area(); o = self.g.out
        T = self.fresh(5)
        first = T if equal else self.collide(T)
        while first[0] == MARK[0]:
            first = self.collide(T)
        if entry:
            o[a + 30:a + 35] = T
        e = self.open(a)
        assert o[a + 160] != first[0]
        self.lits(e, 80, [(p1, first), (p2, T)])
        q1, q2 = e + p1, e + p2
        if equal:
            self.differ(q2 + 5, q1 + 5); self.differ(q2 - 1, q1 - 1)
        self.need(q2, q1, a + 30)
        self.close()

        def check(m):
            assert _slot(first, self.small) == _slot(T, self.small)
            assert q1 not in m.at and m.seen[q1] == (a + 30 if entry else m.seen[q1]) and m.seen[q2] == q1
            if equal:
                self._is(m, q2, q2, q1, 5)
            else:
                assert q2 not in m.at
        self.checks.append(check)
        self.names.append(f"probe pair {p1}/{p2} equal={equal} entry={entry}")

    @_case
    def run_pair(self, p):
        """six equal bytes at lanes p .. p + 5: lanes p and p + 1 hold the same five"""
        a = self.area(); o = self.g.out
        r = next(r for r in range(0xB7, 0x100) if r not in (o[a + 159], o[a + 160]) and bytes([r]) * 4 not in o)
        e = self.open(a)
        self.lits(e, 80, [(p, bytes([r]) * 6)])
        for q in (e + p - 1, e + p + 6):
            if q >= e and o[q] == r:
                o[q] ^= 0x3C
        self.need(e + p)
        self.close()
        self.checks.append(lambda m: self._is(m, e + p + 1, e + p + 1, e + p, 5))
        self.names.append(f"run pair {p}/{p + 1}")

    @_case
    def inside_pair(self, equal, entry):
        """the first one inside the chosen match (A[10:30], at A[16:21]), the second one three bytes behind the match"""
        a = self.area(); o = self.g.out
        L = 34
        if equal:
            T = bytes(o[a + 16:a + 21])
            if not entry:
                o[a + 40:a + 45] = self.collide(T)                     # owns the slot instead of A + 16
        else:
            T = self.fresh(5)
            o[a + 16:a + 21] = self.collide(T)
            if entry:
                o[a + 40:a + 45] = T
        e = self.open(a)
        self.m1(a, e, L, off=10)
        self.lits(e, L + 12, [(L + 3, T)])
        p = e + L + 3
        z = a + 16 if equal else a + 40
        self.differ(p + 5, z + 5); self.differ(p - 1, z - 1)
        self.need(p, a + 16, a + 40, e + L - 14)
        self.close()

        def check(m):
            q1 = e + L - 14
            assert q1 not in m.seen and q1 not in m.refill and _slot(o[q1:q1 + 5], self.small) == _slot(T, self.small)
            if entry:
                self._is(m, p, p, z, 5)
            else:
                assert p not in m.at and (m.seen[p] == a + 40 if equal else bytes(o[m.seen[p]:m.seen[p] + 4]) != T[:4])
        self.checks.append(check)
        self.names.append(f"inside pair equal={equal} entry={entry}")

    @_case
    def refill_pair(self, equal, entry):
        """the first one the refill lane L - 2 (the match's last two bytes and the three behind it), the second one at L + 6.
        entry: the second one's five bytes stand at A + 30, which owns the slot when the window begins - with equal bytes they are
        the refill lane's too, and the match has to go to the refill lane, not to A + 30"""
        a = self.area(); o = self.g.out
        L = 30
        T = self.fresh(5)
        while True:
            three = self.fresh(3) if equal else self.collide(T, prefix=bytes(o[a + 66:a + 68]))[2:]
            if three[0] != o[a + 68]:
                break
        if entry:
            o[a + 30:a + 35] = bytes(o[a + 66:a + 68]) + three if equal else T
        e = self.open(a)
        self.m1(a, e, L)
        self.lits(e, L + 16, [(L, three)])
        X = bytes(o[e + L - 2:e + L + 3])
        p = e + L + 6
        o[p:p + 5] = X if equal else T
        if equal:
            self.differ(p + 5, e + L + 3); self.differ(p - 1, e + L - 3)
        self.need(p, e + L - 2, a + 30)
        self.close()

        def check(m):
            assert e + L - 2 in m.refill and m.seen[p] == e + L - 2
            if entry:
                assert m.seen[a + 30] is not None and bytes(o[a + 30:a + 35]) == bytes(o[p:p + 5])
            if equal:
                self._is(m, p, p, e + L - 2, 5)
            else:
                assert p not in m.at and _slot(X, self.small) == _slot(T, self.small)
        self.checks.append(check)
        self.names.append(f"refill pair equal={equal} entry={entry}")

    @_case
    def triple(self):
        """the same five bytes at lanes 2, 12 and 22"""
        a = self.area(); o = self.g.out
        T = self.fresh(5)
        e = self.open(a)
        self.lits(e, 80, [(2, T), (12, T), (22, T)])
        for q in (12, 22):
            self.differ(e + q + 5, e + q - 5); self.differ(e + q - 1, e + q - 11)
        self.need(e + 2)
        self.close()
        self.checks.append(lambda m: (self._is(m, e + 12, e + 12, e + 2, 5), self._is(m, e + 22, e + 22, e + 12, 5)))
        self.names.append("triple")

    def data(self, size=None):
        if size:
            self.g.text_to(size)
        return self.g.data()


def _landing(b, Ls, ds):
    for L in Ls:
        b.retest_hit(L)
        for d in ds:
            b.back(L, d)
        b.slow(L, 0); b.second(L, 0); b.nothing(L)
        if not b.small:
            b.dirty(L, 0)
    b.slow(30, 2); b.second(30, 2)
    if not b.small:
        b.dirty(30, 2)
    b.nothing(64); b.nothing(65)
    b.chain()


@functools.lru_cache(maxsize=None)
def _built():
    """name -> (block, generator)"""
    out = {}
    b = _Shapes(201, 10000)
    _landing(b, (30,) + EDGES, (1, 2, 3, 4, 5, 6))
    out["landing"] = (b.data(BIG + 900), b)
    b = _Shapes(202, 120000)
    for p1, p2 in ((0, 63), (20, 41)):
        b.probe_pair(p1, p2, True, False)
        b.probe_pair(p1, p2, False, True)
        b.probe_pair(p1, p2, False, False)
    b.run_pair(0); b.run_pair(62); b.run_pair(31)
    for equal in (True, False):
        for entry in (True, False):
            b.inside_pair(equal, entry)
    b.refill_pair(True, True); b.refill_pair(True, False); b.refill_pair(False, True); b.refill_pair(False, False)
    b.second(30, 0); b.second(63, 0)
    b.triple()
    b.dirty(30, 2)
    out["slots"] = (b.data(BIG + 17), b)
    b = _Shapes(203, 200000, small=True)
    _landing(b, (30, 61), (4, 5, 6))
    out["small_landing"] = (b.data(), b)
    for name, (d, _) in out.items():
        assert (len(d) < BIG) == name.startswith("small") and len(d) <= 128 << 10, (name, len(d))
        d.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(name, container):
    d = _source(name)
    return mc._compress(d, max(len(d) - 1, 0) if container else mc._bound(len(d)))


def _source(name):
    if name in _built():
        return _built()[name][0]
    return mc._small(name)


@functools.lru_cache(maxsize=None)
def _checked():
    """the model gives the reference's sequences for every block, and its record holds what every window was built for"""
    for name, (d, b) in _built().items():
        m = _Model(d)
        assert m.seqs == mc._parse(_want(name, False)[1]), name
        for check in b.checks:
            check(m)
    return True


def test_generators_hold_their_shapes():
    """needs no GPU"""
    assert _checked()
    names = sum((b.names for _, b in _built().values()), [])
    for d in range(1, 7):
        for L in (30,) + EDGES:
            assert f"back L={L} d={d}" in names
    for equal in (True, False):
        for entry in (True, False):
            assert f"refill pair equal={equal} entry={entry}" in names and f"inside pair equal={equal} entry={entry}" in names
    for L in (30,) + EDGES:
        for kind in ("retest", "dirty", "slow", "second", "nothing"):
            assert f"{kind} L={L}" + ("" if kind in ("retest", "nothing") else " k=0") in names
    assert _Model(mc._small("twelve")).seqs == [(12, 12, None, None)]


# ------------------------------------------------------------------------------------------------ the device against the reference
def _both(gpu, names, align=None):
    assert _checked()
    srcs = [_source(k) for k in names]
    align = align or [(7 * i + 3) % 16 for i in range(len(srcs))]
    mc._check_raw(gpu, srcs, [_want(k, False) for k in names], [mc._bound(len(s)) for s in srcs], align)
    mc._check_container(gpu, srcs, [_want(k, True) for k in names], align)


@gpu_test
def test_landing_shapes(gpu):
    _both(gpu, ["landing"], [0])
    _both(gpu, ["landing"], [11])


@gpu_test
def test_slot_sharing(gpu):
    _both(gpu, ["slots"], [0])
    _both(gpu, ["slots"], [5])


@gpu_test
def test_mixed_launch(gpu):
    _both(gpu, ["small_landing", "landing", "empty", "slots", "twelve", "small_landing", "small_noise", "slots", "landing", "empty"])
