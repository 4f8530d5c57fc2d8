"""CPU side of the zstd encoder catalogue (tests/zstd_enc_shapes.py): the ledger, the oracle port against the reference's own
ZSTD_compress on every (input, capacity, level) triple the GPU test launches, the trace's neutrality, and the shapes that tell
neighbouring levels apart."""
import numpy as np
import pytest

import helpers
import zstd_enc_shapes as zs

NO_REF = "oracle/_ref/libref4mc.so is missing (__graft_entry__.build() makes it)"      # (as test_hc_shapes_cpu.py)


def test_ledger_reaches_every_required_key():
    cs = zs.cases()
    led = zs.ledger(cs)
    missing = sorted(zs.REQUIRED - set(led))
    assert not missing, missing
    # the catalogue's size limits: all of it, one input, and where the large ones run
    assert sum(len(c.data) for c in cs) < 24 << 20
    for c in cs:
        if len(c.data) > 300000:
            assert c.levels is not None and (c.name.startswith("window_L") and len(c.data) <= (1 << zs.ROWS[c.levels[0] - 1][0][0]) + zs.BLOCK
                                             or c.name == "blocks32" and len(c.data) == 4 << 20), c.name
    # no case reaches what the reference cannot reach (DESIGN_NOTES.md): the day one does, its key joins REQUIRED
    reached = sorted(k for k in led if any(u.fullmatch(k) for u in zs.UNREACHED))
    assert not reached, reached
    # dropping a case loses its key
    lv7 = zs.ledger([c for c in cs if c.name != "behind63"], levels=(7,), capacities=False)
    assert "L7:hc:found:behind=63" not in lv7 and "L7:hc:missed:behind=64" in lv7
    lv1 = zs.ledger([c for c in cs if c.name != "window_L1"], levels=(1,), capacities=False)
    assert "L1:window:edge+0:found" not in lv1 and "L1:fast:arm:hit-ip0" in lv1
    lv5 = zs.ledger([c for c in cs if not c.name.startswith("nseq_words")], levels=(5,), capacities=False)
    assert "lt-lazy:fmt:nseq:3B" not in lv5 and "lt-lazy:fmt:nseq:2B" in lv5
    rle = [c for c in cs if c.name in ("lit_rle", "lit_rle_zeros")]
    assert len(rle) == 2
    for lv, key in ((1, "lt-lazy:fmt:lit:rle:sz2"), (6, "ge-lazy:fmt:lit:rle:sz2")):
        assert key in zs.ledger(rle, levels=(lv,), capacities=False)
        g = zs.ledger([c for c in cs if c not in rle and len(c.data) <= 300000], levels=(lv,), capacities=False)
        assert key not in g and key.replace(":rle:", ":raw:") in g


@pytest.mark.parametrize("level", zs.LEVELS)
def test_port_pinned_to_reference_on_every_triple(level):
    ref = helpers.ref()
    assert ref is not None, NO_REF
    pairs = zs.expected(level)
    assert len(pairs) > 4 * sum(zs.runs_at(c, level) for c in zs.cases())
    bad = []
    for label, d, cap, r, frame in pairs:
        out = np.zeros(max(cap, 1) + 64, np.uint8)
        rr = ref.ZSTD_compress(out.ctypes.data, cap, d.ctypes.data, len(d), level)
        rr = rr - (1 << 64) if ref.ZSTD_isError(rr) else rr
        if rr != r: bad.append((label, "result", rr, r))
        elif not np.array_equal(out[:max(rr, 0)], frame): bad.append((label, "bytes"))
    assert not bad, (level, len(bad), bad[:12])


def test_trace_leaves_the_ports_output_alone():
    for i, c in enumerate(zs.cases()):
        for lv in zs.LEVELS:
            if not zs.runs_at(c, lv) or (i + lv) % 3: continue     # a third of the (case, level) pairs, every level and every case among them
            for cap in (None, len(c.data) // 3):
                t = zs.trace(c.data, lv, cap)
                r, frame = zs.port(c.data, lv, cap)
                assert t.result == r and np.array_equal(t.out, frame), (c.name, lv, cap)
            t = zs.trace(c.data, lv)
            # the rows of every inner block tile it
            for b, start, ln in t.block[:, :3].tolist():
                e = t.emit[t.emit[:, 0] == b]
                assert int(e[:, 2].sum() + e[:, 4].sum()) == ln and (not len(e) or int(e[0, 1]) == start), (c.name, lv, b)
            assert int(t.block[:, 2].sum()) == len(c.data), (c.name, lv)


def test_the_shapes_tell_the_levels_apart():
    """the source behind k words of its hash is found with more than k attempts and not with k, and the frame shows it: a kernel
    that miscounts attempts by one writes other sequences.  Levels 4..8 walk a hash chain at this size with 2^searchLog attempts.
    (Their parsers differ - greedy, lazy, lazy2 - and so do their frames' sizes for reasons of their own, so the sequence at the probe
    is what is compared, and whole frames only between levels of one parser.)"""
    by = {c.name: c for c in zs.cases()}
    chain_levels = [lv for lv in zs.LEVELS if 3 <= zs.params(lv, 10000)["strat"] <= 5]
    assert chain_levels == [4, 5, 6, 7, 8]
    for k in zs.BEHIND:
        c = by[f"behind{k}"]
        d, probe, source = c.data, c.marks["probe"], c.marks["source"]
        frames = {}
        for lv in chain_levels:
            p = zs.params(lv, len(d))
            assert p["wlog"] == 14 and p["hlog"] == 14 and p["mml"] == 4
            t = zs.trace(d, lv)
            frames[lv] = t.out.tobytes()
            e = t.emit
            near = e[(e[:, 1] + e[:, 2] >= probe - 2) & (e[:, 1] + e[:, 2] <= probe + 4) & (e[:, 4] > 0)]      # a sequence whose match starts at the probe or just beside it
            found = len(near) == 1 and int(near[0, 1] + near[0, 2]) == probe and int(near[0, 3]) == probe - source + 3 and int(near[0, 4]) == 4
            assert found == ((1 << p["slog"]) > k) and (found or not len(near)), (k, lv, near.tolist())
        for a, b in ((6, 7), (7, 8)):                              # lazy2 with 16, 64 and 256 attempts
            sa, sb = zs.params(a, len(d))["slog"], zs.params(b, len(d))["slog"]
            if (1 << sa) <= k < (1 << sb): assert frames[a] != frames[b], (k, a, b)      # four literals here, a sequence there (the sizes may agree)
    # the row finder (16 KiB < n <= 128 KiB, levels 5..10): min(2^searchLog, entries of a row) attempts, the words share row and tag
    row_levels = [lv for lv in zs.LEVELS if 3 <= zs.params(lv, 20000)["strat"] <= 5 and zs.params(lv, 20000)["mml"] == 4]
    assert row_levels == [5, 6, 7, 8, 9, 10]
    for k in zs.ROW_BEHIND:
        c = by[f"row_behind{k}"]
        d, probe, source = c.data, c.marks["probe"], c.marks["source"]
        frames = {}
        for lv in row_levels:
            p = zs.params(lv, len(d))
            assert p["wlog"] == 15 and p["hlog"] == 16
            t = zs.trace(d, lv)
            frames[lv] = t.out.tobytes()
            e = t.emit
            near = e[(e[:, 1] + e[:, 2] >= probe - 2) & (e[:, 1] + e[:, 2] <= probe + 4) & (e[:, 4] > 0)]
            found = len(near) == 1 and int(near[0, 1] + near[0, 2]) == probe and int(near[0, 3]) == probe - source + 3 and int(near[0, 4]) == 4
            assert found == ((1 << min(p["slog"], 6)) > k) and (found or not len(near)), (k, lv, near.tolist())
        for a, b in ((7, 8), (8, 9), (9, 10)):                     # lazy2 with 8, 16, 32 and 64 attempts
            sa, sb = zs.params(a, len(d))["slog"], zs.params(b, len(d))["slog"]
            if (1 << sa) <= k < (1 << sb): assert frames[a] != frames[b], (k, a, b)
    # the binary trees of btlazy2 (levels 9 and 10 at 16 KiB and less, 11 and 12 above) and the row finder's rows with minMatch 5
    # (level 4 above 128 KiB, levels 11 and 12 above 256 KiB): the same rule, told from the sequence at the probe
    def probe_found(c, lv):
        e = zs.trace(c.data, lv).emit
        probe, source, wlen = c.marks["probe"], c.marks["source"], c.marks.get("wlen", 4)
        near = e[(e[:, 1] + e[:, 2] >= probe - 2) & (e[:, 1] + e[:, 2] <= probe + 4) & (e[:, 4] > 0)]
        found = len(near) == 1 and int(near[0, 1] + near[0, 2]) == probe and int(near[0, 3]) == probe - source + 3 and int(near[0, 4]) == wlen
        assert found or not len(near), (c.name, lv, near.tolist())
        return found
    for k, hlog, _ in zs.BT_BEHIND:
        c = by[f"bt_behind{k}_h{hlog}"]
        for lv in ((9, 10) if hlog == 14 else (11, 12)):
            p = zs.params(lv, len(c.data))
            assert p["strat"] == 6 and p["hlog"] == hlog and p["mml"] == 4
            assert probe_found(c, lv) == ((1 << p["slog"]) > k), (k, lv)
    for k, _, levels, rowbits in zs.ROW5_BEHIND:
        c = by[f"row5_behind{k}"]
        for lv in levels:
            p = zs.params(lv, len(c.data))
            rowlog = min(max(p["slog"], 4), 6)
            assert 3 <= p["strat"] <= 5 and p["mml"] == 5 and p["hlog"] - rowlog == rowbits
            assert probe_found(c, lv) == ((1 << min(p["slog"], rowlog)) > k), (k, lv)
    # targetLength: only the optimal parser reads it among these levels' finders (the fast rows of levels 1..12 all carry 0, the lazy
    # parsers do not use it): level 11 takes a match above 12 bytes at once, level 12 one above 24.  On matches of 13 .. 24 bytes
    # level 11 takes some at once and level 12 none, and their frames differ.
    d = by["tlen_opt"].data
    assert zs.params(11, len(d))["tlen"] == 12 and zs.params(12, len(d))["tlen"] == 24
    t11, t12 = zs.trace(d, 11), zs.trace(d, 12)
    at_once = lambda t: [int(v) for a, _, v in t.arm.tolist() if a == 42]
    assert at_once(t11) and all(12 < v <= 24 for v in at_once(t11)) and not at_once(t12), (at_once(t11), at_once(t12))
    assert t11.out.tobytes() != t12.out.tobytes()
    # minMatch: a 3-byte match is worth a sequence to level 12's optimal parser (minMatch 3) and to no other
    d = by["match3"].data
    sizes = {lv: zs.port(d, lv, None)[0] for lv in zs.LEVELS}
    assert all(sizes[12] < sizes[lv] for lv in zs.LEVELS if lv != 12), sizes
