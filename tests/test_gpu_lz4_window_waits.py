"""The dense window of the exact LZ4 fast encoder's 32-bit-table instance (lz4_encode.hip, blocks of 65 547 bytes and above) asks
for the ring's next piece behind its candidate gather and moves the bytes at a block's two ends to their place when the piece
is stored, a piece later; the gather itself is issued from the table entry, ahead of the slot-tag rounds, by every lane.
Results and bytes against the oracle, in raw mode (guard bytes behind the result) and in container mode: block ends at every
source alignment, windows that leave early or are followed by a sparse batch while a piece is on its way, and lanes that share
a table slot while their candidates pass and fail.  Every generator asserts, from the oracle's own output or the encoder's hash,
that its input is what it claims."""
import functools

import numpy as np
import pytest

import helpers
import test_gpu_lz4_input_ring as ring       # its layout, comparison and parse helpers

pytestmark = pytest.mark.gpu
PIECE, BIG = ring.PIECE, ring.BIG


def _matches(comp):
    """(start, length, offset) of every match of an LZ4 block, and the literal run lengths"""
    out, lits, i, n, pos = [], [], 0, len(comp), 0
    while i < n:
        tok = int(comp[i]); i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = int(comp[i]); i += 1; lit += b
                if b != 255:
                    break
        i += lit; pos += lit; lits.append(lit)
        if i >= n:
            break
        off = int(comp[i]) | int(comp[i + 1]) << 8; i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = int(comp[i]); i += 1; ml += b
                if b != 255:
                    break
        out.append((pos, ml + 4, off)); pos += ml + 4
    return out, lits


def _slot(data, pos):
    """table slot of the position in a block of the 32-bit table: LZ4_hash5 (lz4.c:764-769) of the five bytes there"""
    v = int.from_bytes(bytes(data[pos:pos + 8]), "little")
    return ((v << 24) * 889523592379 & (1 << 64) - 1) >> 52


def _pad_to(parts, size, text, t, coord):
    """text appended so that the next byte's coordinate is `coord` (mod PIECE), at least 1500 bytes of it"""
    k = 1500 + (coord - (size + 1500)) % PIECE
    parts.append(text[t:t + k])
    return size + k, t + k


# ------------------------------------------------------------------------------------------------ block ends
@functools.lru_cache(maxsize=None)
def _block_ends():
    text = ring._text()
    srcs, align = [], []
    for a in range(16):
        for d in range(41):
            i = len(srcs)
            srcs.append(text[(i * 389) % 300000:(i * 389) % 300000 + BIG + d]); align.append(a)
    assert len(srcs) == 656 and all(len(s) == BIG + i % 41 for i, s in enumerate(srcs))
    buf, offs = ring._layout(srcs, align)
    assert offs[0] == 0 and [o % 16 for o in offs] == align and offs[-1] + len(srcs[-1]) == len(buf)
    assert 42e6 < len(buf) < 44e6
    return srcs, align


def test_block_ends_at_every_alignment(gpu):
    """sizes 65547 + 0..40 at each source alignment: the last piece's bytes are loaded from inside the block and shifted when
    they are stored; the first block begins at byte 0 of its tensor, the last ends at the tensor's last byte"""
    srcs, align = _block_ends()
    ring._check_both(gpu, srcs, align)


# ------------------------------------------------------------------------------------------------ a refill that is due
RUN_OFFSETS = tuple(range(0, 64, 7))


@functools.lru_cache(maxsize=None)
def _runs_at_piece_ends(a):
    """text with runs of one byte and of a period of three, 1, 2 and 3 pieces long, each beginning 0, 7, .. 63 bytes in front of
    a piece boundary of a block that lies `a` bytes behind a multiple of 16"""
    text = ring._text()
    assert text[:330000].max() < 0x80
    parts, size, t, fresh, starts = [text[:20000]], 20000, 20000, 0x80, []
    for plen in (1, 3):
        for pieces in (1, 2, 3):
            for off in RUN_OFFSETS:
                size, t = _pad_to(parts, size, text, t, (PIECE - off - a) % PIECE)
                assert (size + a + off) % PIECE == 0
                period = bytes((fresh + j) % 0x80 + 0x80 for j in range(plen)); fresh += plen
                L = pieces * PIECE
                parts.append(np.frombuffer((period * (L // plen + 1))[:L], np.uint8))
                starts.append((size, plen, L)); size += L
    parts.append(text[t:t + 3000])
    data = np.concatenate(parts)
    assert len(data) >= BIG
    m, _ = _matches(helpers.orc_compress(data)[1])
    by_start = {s: l for s, l, _ in m}
    for s, plen, L in starts:                                   # each run is one match: all of it but its first period
        assert by_start.get(s + plen, 0) >= L - plen, (s, plen, L)
    # a match the dense window cannot size (>= 60 bytes: the general path) begins in the last 64 positions of a piece, whose
    # window has moved the ring on and asked for the next piece
    late = [s for s, l, _ in m if l >= 60 and (s + a) % PIECE >= PIECE - 64]
    assert len(late) >= 2 * 3 * (len(RUN_OFFSETS) - 1), len(late)
    # and a match jumps the whole ring while that piece is on its way: the parse starts the ring again and drops it
    assert sum(1 for s, l, _ in m if l > 2 * PIECE and (s + a) % PIECE >= PIECE - 64) >= 2 * (len(RUN_OFFSETS) - 1)
    return data


def test_window_leaves_with_a_piece_on_its_way(gpu):
    ring._check_both(gpu, [_runs_at_piece_ends(0), _runs_at_piece_ends(5)], [0, 5])


@functools.lru_cache(maxsize=None)
def _noise_behind_piece_starts(a):
    """3 KiB of random bytes beginning 0..48 bytes behind a piece boundary, text after them"""
    rng = np.random.default_rng(41 + a)
    text = ring._text()
    parts, size, t, begins = [text[:8000]], 8000, 8000, []
    for off in range(49):
        size, t = _pad_to(parts, size, text, t, (off - a) % PIECE)
        assert (size + a) % PIECE == off
        parts.append(rng.integers(0, 256, 3 * PIECE, dtype=np.uint8)); begins.append(size); size += 3 * PIECE
    parts.append(text[t:t + 3000])
    data = np.concatenate(parts)
    assert len(data) >= BIG
    m, lits = _matches(helpers.orc_compress(data)[1])
    assert sum(1 for l in lits if l >= 2048) >= len(begins), sorted(lits)[-60:]
    for b in begins:                                            # no match inside the noise: the search goes sparse there
        assert not any(b + 64 <= s < b + 3 * PIECE - 64 for s, _, _ in m), b
    return data


def test_sparse_batch_behind_a_due_piece(gpu):
    ring._check_both(gpu, [_noise_behind_piece_starts(0), _noise_behind_piece_starts(5)], [0, 5])


# ------------------------------------------------------------------------------------------------ lanes that share a slot
PERIODS = tuple(range(1, 10)) + (63, 64, 65)


@functools.lru_cache(maxsize=None)
def _periodic(p):
    rng = np.random.default_rng(50 + p)
    while True:
        unit = rng.integers(0, 256, p, dtype=np.uint8)
        if p == 1 or len(set(unit.tolist())) > 1:
            break
    data = np.tile(unit, (BIG + 200) // p + 1)[:BIG + 100 + p]
    m, _ = _matches(helpers.orc_compress(data)[1])
    assert len(m) == 1 and m[0][2] == p and m[0][1] >= BIG, (p, m[:3])
    return data


def test_periodic_blocks(gpu):
    ring._check_both(gpu, [_periodic(p) for p in PERIODS], [3 * i % 16 for i in range(len(PERIODS))])


def _same_slot_strings(rng, d):
    """two 5-byte strings of bytes >= 0x80 with one table slot that can lie d positions apart: for d < 5 the second begins with
    the first one's tail"""
    w = np.uint64(1) << (np.uint64(8) * np.arange(5, dtype=np.uint64))
    with np.errstate(over="ignore"):
        while True:
            a = rng.integers(0x80, 256, 5, dtype=np.uint8)
            b = rng.integers(0x80, 256, (1024, 5), dtype=np.uint8)
            if d < 5:
                b[:, :5 - d] = a[d:]
            v = (b.astype(np.uint64) * w).sum(axis=1, dtype=np.uint64)
            slots = ((v << np.uint64(24)) * np.uint64(889523592379)) >> np.uint64(52)
            for k in np.flatnonzero(slots == np.uint64(_slot(np.concatenate([a, np.zeros(3, np.uint8)]), 0))):
                if not np.array_equal(a, b[k]):
                    return a, b[k].copy()


@functools.lru_cache(maxsize=None)
def _shared_slots():
    """text in which strings with one table slot lie 1..63 positions apart, two and three to a window, each group three times:
    behind the first, the table holds candidates that pass (the same string earlier) and that fail (its slot's other string)"""
    rng = np.random.default_rng(61)
    text = ring._text()
    assert text[:260000].max() < 0x80
    data = text[:260000].copy()
    groups, at = [], 4000
    for d in range(1, 64):
        a, b = _same_slot_strings(rng, d)
        places = [(0, a), (d, b)]
        if d + 5 <= 58 and d >= 5:                             # a third one, a copy of the first: same slot, and a match
            places.append((d + 5 + d % 3, a))
        for rep in range(3):
            for o, s in places:
                data[at + o:at + o + 5] = s
            if rep == 2:
                data[at + places[-1][0] + 5] ^= 0x40            # behind the strings: the last match ends at another place
            groups.append((at, [o for o, _ in places]))
            at += 700 + 13 * d
    assert at < len(data) - 1000 and len(data) >= BIG
    for at, offs in groups:                                     # from the encoder's hash: the planted positions share a slot
        assert len({_slot(data, at + o) for o in offs}) == 1, (at, offs)
        assert max(offs) < 64
    m, _ = _matches(helpers.orc_compress(data)[1])
    planted = sum(1 for s, _, off in m for at, _ in groups if at - 4 <= s < at + 70 and off >= 700)
    assert planted >= 63, planted                              # the repeats are found as matches of their first copies
    return data


def test_planted_strings_share_slots(gpu):
    data = _shared_slots()
    ring._check_both(gpu, [data, data[1:], data[2000:]], [0, 7, 12])


@functools.lru_cache(maxsize=None)
def _first_bytes_recur():
    """the block's first bytes come again later: candidates at positions 0..3, which the window compares in memory"""
    text = ring._text()
    data = text[:BIG + 3000].copy()
    for k in range(4):
        data[3000 + 2500 * k:3000 + 2500 * k + 14] = data[k:k + 14]
        data[40000 + 2500 * k:40000 + 2500 * k + 9] = data[k:k + 9]
    m, _ = _matches(helpers.orc_compress(data)[1])
    cands = {s - off for s, _, off in m}
    assert {0, 1, 2, 3} & cands and 0 in cands, sorted(cands)[:8]
    return data


def test_candidates_at_the_block_start(gpu):
    data = _first_bytes_recur()
    ring._check_both(gpu, [data, data], [0, 9])


# ------------------------------------------------------------------------------------------------ one launch of everything
def test_mixed_launch(gpu):
    rng = np.random.default_rng(71)
    text = ring._text()
    ends, _ = _block_ends()
    none = np.zeros(0, np.uint8)
    srcs = [text[:1000], _runs_at_piece_ends(5), none, text[:BIG - 1], _noise_behind_piece_starts(0), ends[40], none,
            rng.integers(0, 256, 5000, dtype=np.uint8), _shared_slots(), _periodic(3), text[7:19], _first_bytes_recur(),
            ends[655], _periodic(64), text[100:100 + BIG - 12], none]
    assert sum(1 for s in srcs if 0 < len(s) < BIG) >= 5 and sum(1 for s in srcs if len(s) >= BIG) >= 8
    align = [3, 5, 1, 14, 0, 7, 15, 4, 0, 11, 6, 9, 2, 13, 8, 10]    # (the two generators built for an alignment keep theirs)
    ring._check_both(gpu, srcs, align)
