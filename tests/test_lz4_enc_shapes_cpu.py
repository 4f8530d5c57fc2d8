"""CPU side of the exact LZ4 fast encoder's catalogue (tests/lz4_enc_shapes.py): the ledger and its caps, the oracle port against the
reference's own LZ4_compress_default on every (input, capacity) pair the GPU test launches, the trace against the untraced port, the
lane-level model of the kernel (tools/model/lz4_fast_model.c) on the same pairs - at every source alignment for the ring cases, with
the default record area and with one of 300 records -, the model's sequence list against the port's hit rows, mutants of the model that
the catalogue must tell from the port, and the model under a sanitizer in a program of its own."""
import json
import os
import subprocess

import numpy as np
import pytest

import helpers
import lz4_enc_shapes as ls
from helpers import ROOT

MUTANTS = {1: "a third lane of a slot is taken for a second one", 2: "run_rt is never taken", 3: "run_rt is taken without the rl(h, e-2) == rl(h, e) test",
           4: "the commit (and `inside`) includes lane endP - 2 of a chosen match", 5: "the commit keeps the earliest position of a slot", 6: "scut is off by one",
           7: "`visited` ignores xint", 8: "a second lane that is not visited uses hitA", 9: "the check-bit test also refuses c == 0",
           10: "the distance test uses > where the kernel has >=", 11: "the term rule fires at d >= 4", 12: "saturation is declared slow at fw == 24, the 32 further bytes unread",
           13: "the sparse batch commits the event lane when it is a term lane", 14: "the sparse batch reads the table before the ip-2 refill (h == h2)",
           15: "capok uses 256 where the kernel has 320", 16: "sequence()'s wide forward loop is entered with mcode < 64", 17: "the drain passes tail = 0",
           18: "the first general step ignores the catch-up limit 5", 19: "the sparse batch is never cut at a shared scoreboard entry",
           20: "a window without an event left counts the anchor lane as a probe (k0 one too large)", 21: "xint includes the refill lane of a sequence() match",
           22: "the commit takes `inside` from the first record round when there were more"}
# mutants that change no byte of any input (the test asserts that none of the catalogue's does, so that an entry cannot rot)
EQUIVALENT = {
    2: "run_rt is a short cut: without it the window ends in front of the lane with `retest` set, and lane 0 of the next window is the first of its slot and reads the "
       "refill's entry from the table itself (lz4_encode.hip:569, :330)",
    11: "a chain that ends early hands the hit to sequence(), which sizes the same match from memory (lz4_encode.hip:605-610); the rule only has to fire by d = 5",
    12: "`slow` sends the hit to sequence() with fwd = 24 and fwd_more, which compares the same bytes in memory (lz4_encode.hip:231-254)",
    13: "a term event ends the block (lz4_encode.hip:703): no probe reads the table after it",
    15: "a window adds at most 64 literals and 16 sequences of 4 bytes to `before` and its length bytes, and the reference's checks ask for 8 more: 136 < 256 "
        "(lz4_encode.hip:439 keeps a margin)",
    16: "the wide loop compares the same bytes sixteen per lane; a + 1024 <= matchlimit keeps its reads inside the block (lz4_encode.hip:234)"}


def _same(got, r, comp):
    return got[0] == r and np.array_equal(got[1], comp)


def test_ledger_reaches_every_required_key_inside_the_caps():
    cs = ls.cases()
    led = ls.ledger()
    missing = sorted(ls.REQUIRED - set(led))
    print(f"keys reached: {len(ls.REQUIRED & set(led))} of {len(ls.REQUIRED)} required, {len(led)} in all, by {len(cs)} cases")
    for k, why in sorted(ls.UNREACHED.items()): print(f"UNREACHED {k}: {why}")
    for k, why in sorted(ls.OPEN.items()): print(f"OPEN {k}: {why}")
    assert not missing, missing
    rotten = sorted(k for k in ls.UNREACHED if k in led)
    assert not rotten, [(k, led[k][:3]) for k in rotten]
    stale = sorted(k for k in ls.OPEN if k in led)
    assert not stale, stale
    # the caps
    sizes = [len(c.data) for c in cs]
    assert sum(sizes) <= ls.MAX_TOTAL, sum(sizes)
    assert sum(1 for v in sizes if v > 1 << 20) <= ls.MAX_ABOVE_1M and sum(1 for v in sizes if v > 256 << 10) <= ls.MAX_ABOVE_256K
    print(f"{sum(sizes) / 2 ** 20:.1f} MiB in all inputs, {sum(1 for v in sizes if v > 256 << 10)} above 256 KiB, {len(ls.expected())} (input, capacity) pairs")
    # dropping a named case loses its key
    for name, key, kept in (("rt_misses", "T32:run_rt:miss", "T32:run_rt:hit"), ("dist65535", "T32:search:dist=65535:accepted", "T32:search:dist=65534:accepted")):
        assert led[key] == [name], (key, led[key])
        small = ls.ledger([c for c in cs if c.name in set(led[kept][-2:]) | {"dist65534"}], refusals=False)
        assert key not in small and kept in small, (key, kept)


def test_every_case_runs_at_its_six_capacities():
    for c in ls.cases():
        n, cp = len(c.data), ls.caps(c.data)
        r = ls.port(c.data, ls.bound(n))[0]
        assert cp[0] == ls.bound(n) and max(n - 1, 0) in cp and r in cp and max(r - 1, 0) in cp, (c.name, cp)
        if len(ls.port_trace(c.data).emit) >= 8 and n <= 1 << 20: assert len(cp) == 6, (c.name, cp)      # an early and a late failing capacity of their own
        for cap in cp[4:]: assert 0 < cap < r and ls.port(c.data, cap)[0] == 0, (c.name, cap)


def test_port_pinned_to_reference_on_every_pair():
    """LZ4_compress_default of the reference's own sources where they are built (oracle/_ref); else the SHA-256 of every pair's result and bytes
    that tests/golden/make_golden.py recorded from it (tests/golden/lz4_enc_shapes.json: recorded results only)"""
    ref = helpers.ref()
    pairs = ls.expected()
    assert len(pairs) > 4 * len(ls.cases())
    gold = ls.reference_digests(ref) if ref is not None else json.load(open(ls.FIXTURE))
    print("against " + ("the reference library" if ref is not None else "the recorded digests"))
    assert set(gold) == {p[0] for p in pairs}
    for label, d, cap, r, comp, _ in pairs: assert gold[label] == ls.digest(r, comp), label


def test_recorded_digests_are_the_ports():
    """the fixture itself, also where the reference library is built: it names every pair and holds the port's digests"""
    gold = json.load(open(ls.FIXTURE))
    assert gold == {label: ls.digest(r, comp) for label, d, cap, r, comp, _ in ls.expected()}


def test_trace_leaves_the_ports_output_alone():
    for label, d, cap, r, comp, _ in ls.expected():
        if len(d) > 1 << 20 and cap != ls.bound(len(d)): continue
        t = ls.port_trace(d, cap)
        assert t.result == r and np.array_equal(t.out, comp), label
        if r > 0 and len(d): assert int(t.emit[:, 0].sum() + t.emit[:, 1].sum()) == len(d), label      # the sequences tile the input
        if r > 0 and len(d): assert len(t.hit) + 1 == len(t.emit) and (t.search[:, 2] == 0).sum() + t.hit[:, 10].sum() == len(t.hit), label


def test_model_equals_port_on_every_pair():
    fn = ls._model()
    runs = 0
    for label, d, cap, r, comp, ring in ls.expected():
        for align in (range(16) if ring and len(d) >= ls.BIG else (len(label) % 16,)):
            for reccap in (0, ls.RECORDS):
                if reccap and len(d) > 1 << 20 and cap != ls.bound(len(d)): continue
                assert _same(ls.run_model(fn, d, cap, align, reccap), r, comp), (label, align, reccap)
                runs += 1
    print(f"{runs} model runs")


def test_models_sequence_list_is_the_ports_hit_list():
    """position that hit, its candidate, literals, mcode and the re-test flag of every sequence, in order; and the alignment changes no row but the ring's"""
    for c in ls.cases():
        if not len(c.data): continue
        for cap in ls.caps(c.data)[:2 if len(c.data) > 1 << 20 else 6]:
            pt, mt = ls.port_trace(c.data, cap), ls.model_trace(c.data, cap, align=5)
            if pt.result <= 0:
                k = min(len(pt.hit), len(mt.seq))                                           # up to the refusal, which the two reach at different places of a window
                assert len(mt.seq) <= len(pt.hit) + 64 and np.array_equal(mt.seq[:k, 2:6], pt.hit[:k][:, [0, 1, 7, 8]]), (c.name, cap)
                continue
            assert np.array_equal(mt.seq[:, 2:6], pt.hit[:, [0, 1, 7, 8]]) and np.array_equal(mt.seq[:, 7], pt.hit[:, 10]), (c.name, cap)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_catalogue_catches_the_mutant(tmp_path_factory, mutant):
    fn = ls.build_model(tmp_path_factory.mktemp("lz4fast"), mutant)
    drains = {c.name for c in ls.cases() if c.drain}
    caught = []
    for label, d, cap, r, comp, _ in ls.expected():
        if len(caught) >= 8 and mutant not in EQUIVALENT: break
        if len(d) > (1 << 20) + 1: continue                                                # (the 4 MiB text adds time and no arm)
        for reccap in ((0, ls.RECORDS) if label.split("|")[0] in drains else (0,)):
            if not _same(ls.run_model(fn, d, cap, len(label) % 16, reccap), r, comp): caught.append(label + (f"|records={reccap}" if reccap else ""))
    print(f"mutant {mutant} ({MUTANTS[mutant]}): caught by {caught}")
    if mutant in EQUIVALENT:
        print(f"mutant {mutant} changes no byte: {EQUIVALENT[mutant]}")
        assert not caught, (mutant, caught)
    else: assert caught, (mutant, MUTANTS[mutant])


def test_model_under_a_sanitizer_in_a_program_of_its_own(tmp_path):
    """the model and the port in one program with its own main, -fsanitize=address,undefined: every input at its capacities, the ring cases at two
    alignments, the drain cases with 300 records too; inputs are dumped to a temporary directory, each read into a block of exactly its size"""
    exe = str(tmp_path / "lz4_fast_model_asan")
    subprocess.run(["gcc", "-O1", "-g", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DLF_MAIN",
                    "-I", os.path.join(ROOT, "oracle"), "-o", exe, os.path.join(ROOT, "tools", "model", "lz4_fast_model.c"),
                    os.path.join(ROOT, "oracle", "lz4_port.c")], check=True)
    lines = []
    for c in ls.cases():
        if len(c.data) > 1 << 20: continue
        path = str(tmp_path / f"{c.name}.bin")
        c.data.tofile(path)
        for cap in ls.caps(c.data):
            for align in ((0, 11) if c.ring else (3,)):
                for reccap in ((0, ls.RECORDS) if c.drain else (0,)): lines.append(f"{path} {cap} {align} {reccap}")
    manifest = tmp_path / "manifest.txt"
    manifest.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(manifest)], capture_output=True, text=True, timeout=600)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{len(lines)} runs, 0 differ" in r.stdout
