"""CPU: the zstd frame shapes of tests/zstd_shapes.py against the reference's ZSTD_decompress and the oracle port
(orc_zstd_decompress), which the GPU tests lean on.  The committed fixture subset always runs; the generated set and the damaged
set need oracle/_ref."""
import hashlib

import numpy as np
import pytest

import helpers
import zstd_shapes as zs

needs_ref = pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not present")

# What the reference alone makes of damaged_set() (seed 0xDA, 26 copies per frame class up to 600 KB of output and 8 above):
# ZSTD_decompress accepts 248 and rejects 2363 of the 2611 damaged frames.  The floors are those counts.
ACCEPTED_FLOOR, REJECTED_FLOOR = 248, 2363


def _oracle_gives(frame, want_len, want_sha, name):
    for slack in (0, 300):
        r, out = helpers.orc_zstd_decompress(frame, want_len + slack)
        assert r == want_len, (name, slack, r)
        assert hashlib.sha256(out.tobytes()).hexdigest() == want_sha, (name, slack)


def test_fixture_frames_decode_and_cover_the_ledger():
    """Every committed frame decodes to its recorded output through the oracle at exact capacity and at capacity + 300 (the two
    classes rejected by design are rejected), and the fixture alone reaches every key of REQUIRED."""
    fx = zs.fixture_frames()
    for name, f, n, sha in fx:
        if zs.rejected_by_design(f):
            assert helpers.orc_zstd_decompress(f, n)[0] < 0 and helpers.orc_zstd_decompress(f, n + 300)[0] < 0, name
        else:
            _oracle_gives(f, n, sha, name)
    led = zs.ledger([(n, f, None) for n, f, _, _ in fx])
    missing = [k for k in zs.REQUIRED if not led[k]]
    assert not missing, f"ledger keys the fixture does not reach: {missing}"


@needs_ref
def test_fixture_is_what_the_generator_selects():
    """tests/golden/zstd_shapes.json is fixture_select(frames()): the reference still writes these bytes."""
    sel = zs.fixture_select(zs.frames())
    got = {n: (f.hex(), ln, sha) for n, f, ln, sha in zs.fixture_frames()}
    assert got == {n: (e["frame"], e["output_bytes"], e["output_sha256"]) for n, e in sel.items()}


@needs_ref
def test_generated_frames_reference_and_oracle_agree():
    names = [n for n, _, _ in zs.frames()]
    assert len(set(names)) == len(names)
    for name, f, e in zs.frames():
        for slack in (0, 300):
            r, out = zs.ref_decode(f, len(e) + slack)
            wr, w = helpers.orc_zstd_decompress(f, len(e) + slack)
            if name == "hdr_dictid5_w1_30k":
                assert r < 0 and wr < 0, name                  # a dictionary this decoder does not have: both reject
            elif zs.rejected_by_design(f):
                assert r == len(e) and out == e and wr < 0, (name, r, wr)     # pinned deviation: the oracle (and the device) reject
            else:
                assert r == len(e) and out == e, (name, slack, r)
                assert wr == r and w.tobytes() == e, (name, slack, wr)
        if len(e) and not zs.rejected_by_design(f):            # one byte short: dstSize_tooSmall for both
            assert zs.ref_decode(f, len(e) - 1)[0] < 0 and helpers.orc_zstd_decompress(f, len(e) - 1)[0] < 0, name


@needs_ref
def test_ledger_covers_every_required_key():
    led = zs.ledger(zs.frames())
    print({k: led[k] for k in zs.REQUIRED})
    missing = [k for k in zs.REQUIRED if not led[k]]
    assert not missing, f"ledger keys no generated frame reaches: {missing}"


@needs_ref
def test_decline_rules_see_both_sides_of_each_limit():
    """The frames meant for the limits sit where they should: the split path's rules name one of each pair and not the other."""
    d = {n: zs.declines(f, len(e)) for n, f, e in zs.frames()}
    L = zs.limits()
    assert not d[f"stream_{L['inner']}_blocks"] and d[f"stream_{L['inner'] + 1}_blocks"]
    assert not d[f"seq_area_{L['seq']}"] and d[f"seq_area_{L['seq'] + 1}"]
    assert max(fr["lit_need"] for _, f, _ in zs.frames() for fr in zs.inspect(f)[2]) <= 4194304 + 64 * 63 < L["lit"]


@needs_ref
def test_damaged_frames_oracle_agrees_with_reference():
    """Structure-aware damage (header bytes, block headers, literals headers, jump tables, weight headers, sequence counts, mode
    bytes, the ends of every bitstream, cuts at section boundaries): the oracle gives the reference's verdict on every one, and the
    reference's bytes where it accepts.  Nothing is excluded; no frame may be one the reference accepts and the oracle does not."""
    accepted = rejected = lenient = 0
    for label, m, cap in zs.damaged_set():
        r, out = zs.ref_decode(m, cap)
        wr, w = helpers.orc_zstd_decompress(m, cap)
        if r < 0:
            rejected += 1
            assert wr < 0, (label, wr)
        elif wr < 0:
            lenient += 1; print("lenient:", label, r)
        else:
            accepted += 1
            assert wr == r and w.tobytes() == out, (label, r, wr)
    print(f"damaged frames: {accepted + rejected + lenient}, reference accepts {accepted + lenient}, rejects {rejected}")
    assert lenient == 0
    assert accepted >= ACCEPTED_FLOOR and rejected >= REJECTED_FLOOR, (accepted, rejected)
