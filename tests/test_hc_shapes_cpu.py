"""CPU side of the HC / Medium search-and-parse catalogue (tests/hc_shapes.py): the ledger, and the oracle port against the
reference's own LZ4_compress_HC (levels 1..8) and LZ4_compressMC[_limitedOutput] on every (input, capacity) pair the GPU test
launches."""
import ctypes as C

import numpy as np
import pytest

import helpers
import hc_shapes as hs

NO_REF = "oracle/_ref/libref4mc.so is missing (__graft_entry__.build() makes it)"      # (as test_lz4_shapes_cpu.py)


def test_ledger_reaches_every_required_key():
    cs = hs.cases()
    led = hs.ledger(cs)
    missing = sorted(hs.REQUIRED - set(led))
    assert not missing, missing
    assert sum(len(c.data) for c in cs) < 8 << 20
    # no search position ever lies a window behind an earlier one: hc_acquire's private rebuild stays out of REQUIRED (DESIGN_NOTES.md)
    assert not [k for k in led if ":stepback:" in k and not k.endswith(":0")]
    # ... and no case reaches one of the four arms the parse cannot take (DESIGN_NOTES.md): the day one does, its key joins REQUIRED
    assert not [k for k in led if k.split(":arm:")[-1] in hs.UNREACHED_ARMS]
    # dropping a case loses its key
    lv8 = hs.ledger([c for c in cs if c.name != "behind127"], levels=(8,), refusals=False)
    assert "L8:att:found:behind=127" not in lv8 and "L8:att:missed:behind=128" in lv8
    lv5 = hs.ledger([c for c in cs if c.name != "back95_rest"], levels=(5,), refusals=False)
    assert "L5:back:rest=95" not in lv5 and "L5:back:rest=96" in lv5


def test_medium_ledger_reaches_every_required_key():
    cs = hs.mc_cases()
    led = hs.mc_ledger(cs)
    missing = sorted(hs.MC_REQUIRED - set(led))
    assert not missing, missing
    assert "att:missed:behind=4" not in hs.mc_ledger([c for c in cs if c.name != "mc_behind4"])
    assert "share:ntu-prev" not in hs.mc_ledger([c for c in cs if c.name != "mc_share_ntu-prev"])


def test_the_shapes_tell_the_levels_apart():
    """the winner behind N colliding words is found with more than N attempts and not below, and the output shows it: a kernel that
    miscounts attempts by one differs in the bytes"""
    by = {c.name: c for c in hs.cases()}
    for n in hs.BEHIND:
        d = by[f"behind{n}"].data
        sizes = {lv: hs.port(d, lv, hs.bound(len(d)))[0] for lv in hs.LEVELS}
        found = {sizes[lv] for lv, a in hs.ATTEMPTS.items() if a > n}
        missed = {sizes[lv] for lv, a in hs.ATTEMPTS.items() if a <= n}
        assert len(found) <= 1 and len(missed) <= 1, (n, sizes)
        if found and missed: assert max(found) < min(missed), (n, sizes)
        assert found or n >= 128


@pytest.mark.parametrize("level", hs.LEVELS)
def test_port_pinned_to_reference_on_every_pair(level):
    ref = helpers.ref()
    assert ref is not None, NO_REF
    pairs = hs.expected(level)
    assert len(pairs) > 5 * len(hs.cases())
    for label, d, cap, r, comp in pairs:
        out = np.zeros(hs.bound(len(d)) + 64, np.uint8)
        rr = ref.LZ4_compress_HC(d.ctypes.data, out.ctypes.data, len(d), cap, level)
        assert rr == r, (level, label, rr, r)
        assert np.array_equal(out[:max(rr, 0)], comp), (level, label)


def test_medium_port_pinned_to_reference_on_every_pair():
    ref = helpers.ref()
    assert ref is not None, NO_REF
    ref.LZ4_compressMC.argtypes = [C.c_void_p, C.c_void_p, C.c_int]; ref.LZ4_compressMC.restype = C.c_int
    ref.LZ4_compressMC_limitedOutput.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]; ref.LZ4_compressMC_limitedOutput.restype = C.c_int
    pairs = hs.expected("mc")
    assert len(pairs) > 5 * len(hs.mc_cases())
    for label, d, cap, r, comp in pairs:
        out = np.zeros(hs.bound(len(d)) + 80, np.uint8)
        rr = (ref.LZ4_compressMC(d.ctypes.data, out.ctypes.data, len(d)) if cap < 0
              else ref.LZ4_compressMC_limitedOutput(d.ctypes.data, out.ctypes.data, len(d), cap))
        assert rr == r, (label, rr, r)
        assert np.array_equal(out[:max(rr, 0)], comp), label


def test_trace_leaves_the_ports_output_alone():
    for c in hs.cases()[::7]:
        for lv in (1, 5, 8):
            t = hs.trace(c.data, lv)
            r, comp = hs.port(c.data, lv, hs.bound(len(c.data)))
            assert t.result == r and np.array_equal(t.out, comp), (c.name, lv)
            assert int(t.emit[:, 0].sum() + t.emit[:, 1].sum()) == len(c.data), (c.name, lv)        # the sequences tile the input
    for c in hs.mc_cases()[::3]:
        t = hs.trace(c.data, "mc")
        r, comp = hs.port(c.data, "mc", -1)
        assert t.result == r and np.array_equal(t.out, comp), c.name
