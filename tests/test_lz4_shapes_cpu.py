"""CPU side of the LZ4 shape catalogue (tests/lz4_shapes.py): the ledger, the builder against the oracle, the oracle against the
reference's own LZ4_decompress_safe on every stream and capacity the GPU test launches, and the inspector against a sequence
list derived without it."""
import ctypes as C

import numpy as np
import pytest

import helpers
import lz4_shapes as ls

NO_REF = "oracle/_ref/libref4mc.so is missing (__graft_entry__.build() makes it)"      # (as test_gpu_pieces.py)


def test_ledger_reaches_every_required_key():
    fr = ls.frames()
    led = ls.ledger(fr)
    missing = sorted(ls.REQUIRED - set(led))
    assert not missing, missing
    # ... and, but for the keys only a block outside the fast paths' sizes has, by blocks the fast paths are eligible for
    missing = sorted(ls.REQUIRED - ls.ELIGIBILITY - set(ls.ledger(fr, only_eligible=True)))
    assert not missing, missing
    # dropping a frame loses its key
    assert "chunk:ntok=385" not in ls.ledger([f for f in fr if f.name != "chunk385"])
    assert "extreme:dense4M" not in ls.ledger([f for f in fr if f.name != "dense4m"])


def test_builder_agrees_with_oracle():
    for f in ls.frames():
        r, d = helpers.orc_decompress(f.stream, len(f.decoded))
        assert r == len(f.decoded), (f.name, r)
        assert np.array_equal(d, f.decoded), f.name


def test_builder_vectorised_form_equals_the_plain_one():
    rng = np.random.default_rng(3)
    lead = (rng.integers(0, 256, 40, dtype=np.uint8).tobytes(), 40, 4)
    a = ls.build([lead, (b"", 7, 5, 300), (b"xy", 3, 4, 50)], b"0123456789ab")
    b = ls.build([lead] + [(b"", 7, 5)] * 300 + [(b"xy", 3, 4)] * 50, b"0123456789ab")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_oracle_pinned_to_reference_on_every_case():
    ref = helpers.ref()
    assert ref is not None, NO_REF
    cases = ls.cases()
    assert len(cases) > 2000
    accepted = 0
    for label, st, cap, _ in cases:
        wr, want = helpers.orc_decompress(st, cap)
        dst = np.zeros(max(cap, 1), np.uint8)
        rr = ref.LZ4_decompress_safe(st.ctypes.data, dst.ctypes.data, len(st), cap)
        if wr == -(2 ** 31): continue                  # offset 0: undefined in the reference (it may even accept); the oracle and the
        assert rr == wr, (label, rr, wr)               # GPU reject with a code of their own (test_gpu_parity.py)
        if wr >= 0:
            accepted += 1
            assert np.array_equal(dst[:rr], want), label
    assert accepted > sum(len(f.caps) for f in ls.frames())                     # some damage is harmless; the oracle says which


def _oracle_sequences(st, cap):
    L = helpers.oracle()
    L.orc_lz4_sequences_ex.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.orc_lz4_sequences_ex.restype = C.c_int
    mx = len(st) // 3 + 8
    tp, op, fl = np.zeros(mx, np.uint32), np.zeros(mx, np.uint32), np.zeros(4 * mx, np.uint32)
    total = C.c_int(0)
    n = L.orc_lz4_sequences_ex(st.ctypes.data, len(st), cap, tp.ctypes.data, op.ctypes.data, fl.ctypes.data, mx, C.byref(total))
    assert n > 0, n
    return tp[:n], op[:n], fl[:4 * n].reshape(n, 4), total.value


def test_inspector_sequence_list_equals_the_oracles():
    for f in ls.frames():
        tp, op, fl, total = _oracle_sequences(f.stream, len(f.decoded) + 64)
        w = ls.walk(f.stream)
        assert total == w.n == len(f.decoded), f.name
        assert np.array_equal(tp, np.append(w.tp, w.ftp)), f.name
        assert np.array_equal(op, np.append(w.out, w.n - w.fll)), f.name
        assert np.array_equal(fl[:, 0], np.append(w.lp, w.flp)) and np.array_equal(fl[:, 1], np.append(w.ll, w.fll)), f.name
        assert np.array_equal(fl[:-1, 2], w.ml) and np.array_equal(fl[:-1, 3], w.off), f.name
        # the fields tile the stream: offset position = literal start + literal length, and a sequence ends where the next begins
        assert np.array_equal(w.mp, w.lp + w.ll), f.name


def test_inspector_on_three_frames_checked_by_hand():
    st, dec = ls.build([(b"abcd", 4, 4)], b"12345")
    assert st.tobytes() == bytes.fromhex("40 61626364 0400 50 3132333435") and dec.tobytes() == b"abcdabcd12345"
    assert ls.sequences(st) == ([(0, 4, 4, 4, 0)], (7, 5, 8))
    assert ls.inspect(st, 13) == {"ll:4", "ll:5", "ml:4", "off:4", "off=out", "slack:0", "end:final:5"}
    assert ls.inspect(st, 141) == {"ll:4", "ll:5", "ml:4", "off:4", "off=out", "slack:128", "end:final:5"}

    st, dec = ls.build([(b"x" * 15, 1, 19)], b"vwxyz")
    assert st.tobytes() == b"\xff\x00" + b"x" * 15 + b"\x01\x00\x00" + b"\x50vwxyz" and dec.tobytes() == b"x" * 34 + b"vwxyz"
    assert ls.sequences(st) == ([(0, 15, 1, 19, 0)], (20, 5, 34))
    assert ls.inspect(st, 40) == {"ll:15", "ll:5", "ml:19", "off:1", "slack:1", "end:final:5"}

    st, dec = ls.build([(b"ab", 2, 4), (b"", 3, 5)], b"hello!")
    assert st.tobytes() == b"\x20ab\x02\x00" + b"\x01\x03\x00" + b"\x60hello!" and dec.tobytes() == b"ababab" + b"babba" + b"hello!"
    assert ls.sequences(st) == ([(0, 2, 2, 4, 0), (5, 0, 3, 5, 6)], (8, 6, 11))
    assert ls.inspect(st, 17) == {"ll:0", "ll:2", "ll:6", "ml:4", "off:2", "off:3", "off=out", "slack:0", "end:final:6"}


def test_false_chain_is_simulated_not_assumed():
    """`falsechain`: in every segment behind the first the true chain takes more than kFixCap hops without ever meeting the chain
    walked from the segment's first byte; `falsechain_met`: it meets it after 16 .. kFixCap hops somewhere."""
    f = {x.name: x for x in ls.frames()}
    s = f["falsechain"].stream.tobytes()
    fx = ls.fix_hops(s, ls.walk(s))
    assert len(fx) == ls.K_SEGS_SEG - 1 and all(not met and h > ls.K_FIXCAP for met, h in fx.values()), fx
    s = f["falsechain_met"].stream.tobytes()
    assert any(met and 16 <= h <= ls.K_FIXCAP for met, h in ls.fix_hops(s, ls.walk(s)).values())


def test_damage_is_placed_at_the_fields():
    f = {x.name: x for x in ls.frames()}["bounds"]
    w = ls.walk(f.stream)
    got = {lab.split("|")[1]: (st, cap) for lab, st, cap in ls.damaged(f)}
    for where in ("first", "mid", "front-of-margin", "in-margin", "last"):
        assert f"off=0@{where}" in got and f"cut-in-offset@{where}" in got, where
    st, _ = got["off=0@in-margin"]
    diff = np.flatnonzero(st != f.stream)
    assert len(diff) and diff.min() >= w.csize - ls.K_MARGIN and set(diff.tolist()) <= set((w.mp[:, None] + [0, 1]).ravel().tolist())
    st, _ = got["off=0@front-of-margin"]
    assert np.flatnonzero(st != f.stream).max() < w.csize - ls.K_MARGIN
    assert helpers.orc_decompress(*got["final-literals-4/cap+0"])[0] < 0        # lz4.c LASTLITERALS
