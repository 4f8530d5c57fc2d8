"""CPU side of the LZ4 HC level 9..12 catalogue (tests/hc_opt_shapes.py): the ledger and its caps, the oracle port against the
reference's own LZ4_compress_HC on every (input, capacity, level) triple the GPU test launches, the CPU model of the kernel's serial
text (tools/model/lz4hc_opt_model.c) on the same triples, and mutants of that model that the catalogue must tell from the port."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import helpers
import hc_opt_inputs
import hc_opt_shapes as ho
from helpers import B, ROOT

NO_REF = "oracle/_ref/libref4mc.so is missing (__graft_entry__.build() makes it)"
MUTANTS = {1: "insert without the 65535 clamp", 2: "insert: first lane of a hash becomes the head", 3: "swap scan never reloads after 64 positions",
           4: "swap scan drops matchChainPos", 5: "ho_opt_match returns the old last when matchML > 64", 6: "ho_count_back ignores maxn"}
# a mutant no case of the catalogue tells from the model by its bytes (DESIGN_NOTES.md says why none can): the test asserts that none
# does, so that the entry cannot rot
EQUIVALENT = {1: "a delta is clamped where the hash has no earlier position or one more than 65535 back; a walk that reads it is that of a "
                 "later position, for which 65535 steps back and any other number both lead to no position that holds the word within reach"}
# the repeat test of pattern analysis stands in lz4hc_opt_core.h, which takes no switch: these two are built from a copy of it
REPEAT_TEST = "if (((pattern & 0xFFFF) == (pattern >> 16)) && ((pattern & 0xFF) == (pattern >> 24)))"
HEADER_MUTANTS = {"repeat test keeps its 16-bit half alone": "if ((pattern & 0xFFFF) == (pattern >> 16))",
                  "repeat test keeps its byte half alone": "if ((pattern & 0xFF) == (pattern >> 24))"}


def _model(tmp, mutant=0, repeat_test=None):
    so = str(tmp / f"liblz4hc_opt_model_{mutant}.so")
    inc = os.path.join(ROOT, "4mc_amd", "csrc")
    if repeat_test is not None:                                    # a copy of the kernel's serial text with that one line changed
        text = open(os.path.join(inc, "lz4hc_opt_core.h")).read()
        assert text.count(REPEAT_TEST) == 1
        (tmp / "lz4hc_opt_core.h").write_text(text.replace(REPEAT_TEST, repeat_test))
        inc = str(tmp)
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", f"-DHO_MUTANT={mutant}",
                    "-I", inc, "-o", so, os.path.join(ROOT, "tools", "model", "lz4hc_opt_model.c")], check=True)
    L = C.CDLL(so)
    L.lz4hc_opt_model_compress.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.lz4hc_opt_model_compress.restype = C.c_int
    return L.lz4hc_opt_model_compress


def _run(fn, s, cap, level):
    s = np.ascontiguousarray(s, dtype=np.uint8)
    d = np.zeros(max(cap, 1) + 64, np.uint8)
    r = fn(s.ctypes.data, d.ctypes.data, len(s), cap, level)
    return r, d[:max(r, 0)].tobytes()


@pytest.fixture(scope="module")
def ref():
    r = helpers.ref()
    assert r is not None, NO_REF
    return r


def test_ledger_reaches_every_required_key_inside_the_caps():
    walked = {}
    led = ho.ledger(walked=walked)
    missing = sorted(ho.REQUIRED - set(led))
    reached = sorted(ho.REQUIRED & set(led))
    print(f"keys reached: {len(reached)} of {len(ho.REQUIRED)} required")
    for k, why in sorted(ho.UNREACHED.items()): print(f"UNREACHED {k}: {why}")
    assert not missing, missing
    rotten = sorted(k for k in ho.UNREACHED if k in led)
    assert not rotten, [(k, led[k][:3]) for k in rotten]
    # the size caps hold for the cases this catalogue adds; level 9 also runs hc_shapes.cases() whole, wrap200k (200 KiB) included,
    # and those count towards the candidates-walked cap alone
    cs = ho.cases()
    assert max(len(c.data) for c in cs) <= ho.MAX_CASE
    big = [c.name for c in cs if len(c.data) > ho.BIG]
    assert len(big) <= ho.MAX_BIG, big
    heavy = max((v, k) for k, v in walked.items())
    print(f"most candidates walked: {heavy[0]} on {heavy[1]}")
    assert heavy[0] <= ho.MAX_WALKED, heavy
    # dropping a case loses its key
    l10 = ho.ledger([c for c in cs if c.name != "far_run"], levels=(10,), refusals=False)
    assert "L10:pa:below-lowest" not in l10 and "L10:pa:to-end" in l10
    l9 = ho.ledger([c for c in ho.cases_of(9) if c.name != "four_differ"], levels=(9,), refusals=False)
    assert "L9:pa:four-differ" not in l9 and "L9:pa:to-end" in l9


@pytest.mark.parametrize("level", ho.LEVELS)
def test_port_pinned_to_reference_on_every_triple(ref, level):
    pairs = ho.expected(level)
    assert len(pairs) > 4 * len(ho.cases_of(level))
    for label, d, cap, r, comp in pairs:
        assert _run(ref.LZ4_compress_HC, d, cap, level) == (r, comp.tobytes()), (level, label)


@pytest.mark.parametrize("level", ho.LEVELS)
def test_port_pinned_to_reference_on_the_older_inputs(ref, level):
    """the hand-picked inputs of hc_opt_inputs.py and the corpus blocks of test_lz4hc_opt_model_cpu.py"""
    for k, s in hc_opt_inputs.shapes().items():
        if level == 12: s = s[: 256 << 10]
        n = len(s)
        for cap in (ho.bound(n), max(n - 1, 0), n // 2):
            r, comp = ho.port(s, level, cap)
            assert _run(ref.LZ4_compress_HC, s, cap, level) == (r, comp.tobytes()), (level, k, cap)
    for k in ((0, 5, 8) if level < 12 else (3,)):
        s = helpers.corpus(B, first_block=k)
        r, comp = ho.port(s, level, B - 1)
        assert _run(ref.LZ4_compress_HC, s, B - 1, level) == (r, comp.tobytes()), (level, k)


def test_port_maps_levels_like_the_reference(ref):
    by = {c.name: c for c in ho.cases()}
    for name in ("runs_grow", "text1_1200", "chunks64", "n13"):
        d = by[name].data
        for level, same_as in ((0, 9), (-7, 9), (13, 12), (1000, 12)):
            r, comp = ho.port(d, level, ho.bound(len(d)))
            assert _run(ref.LZ4_compress_HC, d, ho.bound(len(d)), level) == (r, comp.tobytes()), (name, level)
            r2, comp2 = ho.port(d, same_as, ho.bound(len(d)))
            assert r2 == r and np.array_equal(comp2, comp), (name, level)


def test_trace_leaves_the_ports_output_alone():
    for lv in ho.LEVELS:
        for c in ho.cases_of(lv)[::5]:
            for cap in ho.caps(c.data, lv)[::2]:
                t = ho.trace(c.data, lv, cap)
                r, comp = ho.port(c.data, lv, cap)
                assert t.result == r and np.array_equal(t.out, comp), (c.name, lv, cap)
                if r > 0: assert int(t.emit[:, 0].sum() + t.emit[:, 1].sum()) == len(c.data), (c.name, lv)      # the sequences tile the input


def test_the_shapes_tell_neighbouring_levels_apart():
    for a, b in ((9, 10), (10, 11), (11, 12)):
        differ = [c.name for c in ho.cases() if not np.array_equal(ho.port(c.data, a, ho.bound(len(c.data)))[1], ho.port(c.data, b, ho.bound(len(c.data)))[1])]
        print(f"levels {a} / {b} differ on {len(differ)} cases: {differ[:6]}")
        assert differ, (a, b)


@pytest.mark.parametrize("level", ho.LEVELS)
def test_model_equals_port_on_every_triple(tmp_path_factory, level):
    model = _model(tmp_path_factory.mktemp("hcopt"))
    for label, d, cap, r, comp in ho.expected(level):
        assert _run(model, d, cap, level) == (r, comp.tobytes()), (level, label)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_catalogue_catches_the_mutant(tmp_path_factory, mutant):
    fn = _model(tmp_path_factory.mktemp("hcopt"), mutant)
    caught = []
    for level in ho.LEVELS:
        for label, d, cap, r, comp in ho.expected(level):
            if len(caught) >= 8: break
            if mutant in EQUIVALENT and cap != ho.bound(len(d)): continue     # (every case at its bound alone: run time; its wandering walks are long)
            if _run(fn, d, cap, level) != (r, comp.tobytes()): caught.append(f"L{level}:{label}")
    print(f"mutant {mutant} ({MUTANTS[mutant]}): caught by {caught}")
    if mutant in EQUIVALENT:
        print(f"mutant {mutant} changes no byte: {EQUIVALENT[mutant]}")
        assert not caught, (mutant, caught)
    else: assert caught, (mutant, MUTANTS[mutant])


@pytest.mark.parametrize("what", sorted(HEADER_MUTANTS))
def test_catalogue_catches_half_a_repeat_test(tmp_path_factory, what):
    fn = _model(tmp_path_factory.mktemp("hcopt"), repeat_test=HEADER_MUTANTS[what])
    caught = []
    for level in ho.LEVELS:
        caught += [f"L{level}:{label}" for label, d, cap, r, comp in ho.expected(level) if cap == ho.bound(len(d)) and _run(fn, d, cap, level) != (r, comp.tobytes())]
    print(f"{what}: caught by {caught}")
    assert all(any(c.startswith(f"L{lv}:") for c in caught) for lv in ho.LEVELS), (what, caught)
