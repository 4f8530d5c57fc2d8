"""The exact LZ4 fast encoder's input ring (lz4_encode.hip, blocks of 65 547 bytes and above): the dense windows read the stream
from an LDS ring that is filled 1 KiB at a time with aligned loads and shares its memory with the sparse batch's scoreboard.
Results and bytes against the oracle, in raw mode (guard bytes behind the result) and in container mode: block sizes and source
alignments around the ring's pieces, matches that jump past the ring, sparse <-> dense transitions, literal runs at their length
thresholds, a launch mixed with blocks of the 16-bit table, and capacities at which the output fills.  Every generator asserts,
from the oracle's own output, that its input is what it claims."""
import functools

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
GUARD = 0x5A
PIECE, RING = 1024, 2048            # the ring's refill and its size (kPiece, kRing of lz4_encode.hip)
BIG = 65547                         # the smallest block of the 32-bit table


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _layout(srcs, align):
    """source offsets: block i begins `align[i]` bytes behind a multiple of 16 (tensors are at least 16-byte aligned); block 0 of
    align 0 begins at byte 0 and the buffer ends with the last block's last byte"""
    offs, pos = [], 0
    for s, a in zip(srcs, align):
        pos += (a - pos) % 16
        offs.append(pos); pos += len(s)
    buf = np.zeros(pos, np.uint8)
    for s, o in zip(srcs, offs):
        buf[o:o + len(s)] = s
    return buf, offs


def _check_raw(gpu, srcs, caps, align=None):
    buf, offs = _layout(srcs, align or [0] * len(srcs))
    dsts, dpos = [], 5
    for c in caps:
        dsts.append(dpos); dpos += c + 40
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, [len(s) for s in srcs], caps))
    d_out = torch.full((dpos,), GUARD, dtype=torch.uint8, device="cuda")
    gpu.lz4_compress_fast(_dev(buf), d_out, batch)
    res = [int(r) for r in batch.download()["result"]]
    out = d_out.cpu().numpy()
    for i, (s, c, d) in enumerate(zip(srcs, caps, dsts)):
        want_r, want = helpers.orc_compress(s, c)
        assert res[i] == want_r, (i, len(s), c, res[i], want_r)
        if want_r > 0:
            assert np.array_equal(out[d:d + want_r], want), (i, len(s), c)
        assert (out[d + max(want_r, 0):d + c + 40] == GUARD).all(), (i, len(s), c, "bytes written past the result")
    return res


def _check_container(gpu, srcs, align=None):
    """container mode (capacity n-1, stored when it does not fit) against the oracle's block payloads"""
    buf, offs = _layout(srcs, align or [0] * len(srcs))
    lens = [len(s) for s in srcs]
    dsts, dpos = [], 0
    for n in lens:
        dsts.append(dpos); dpos += n + 64
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, lens, lens))
    d_out = torch.full((dpos,), GUARD, dtype=torch.uint8, device="cuda")
    gpu.encode_blocks(_dev(buf), d_out, batch)
    enc = batch.download()
    out = d_out.cpu().numpy()
    for i, s in enumerate(srcs):
        want_r, want = helpers.orc_compress(s, max(len(s) - 1, 0))
        if want_r <= 0:
            want_r, want = len(s), s
        r = int(enc["result"][i])
        assert r == want_r, (i, len(s), r, want_r)
        assert np.array_equal(out[dsts[i]:dsts[i] + r], want), i
        assert (out[dsts[i] + r:dsts[i] + lens[i] + 64] == GUARD).all(), (i, "bytes written past the result")
        assert int(enc["xxh32"][i]) == helpers.orc_xxh32(want), i


def _check_both(gpu, srcs, align=None):
    _check_raw(gpu, srcs, [helpers.oracle().orc_lz4_compress_bound(len(s)) for s in srcs], align)
    _check_container(gpu, srcs, align)


def _sequences(comp):
    """(literal length, match length) of every sequence of an LZ4 block; the last has match length None"""
    seqs, i, n = [], 0, len(comp)
    while i < n:
        tok = int(comp[i]); i += 1
        lit = tok >> 4
        if lit == 15:
            while True:
                b = int(comp[i]); i += 1; lit += b
                if b != 255:
                    break
        i += lit
        if i >= n:
            seqs.append((lit, None)); break
        i += 2
        ml = tok & 15
        if ml == 15:
            while True:
                b = int(comp[i]); i += 1; ml += b
                if b != 255:
                    break
        seqs.append((lit, ml + 4))
    return seqs


@functools.lru_cache(maxsize=None)
def _text():
    t = helpers.corpus(400000)          # the corpus begins with its text class
    t.setflags(write=False)
    return t


RUN_LENGTHS = (RING - 1, RING, RING + 1, 3 * RING + 7)


@functools.lru_cache(maxsize=None)
def _runs_block():
    """text, then runs of one byte and of a period of three (each run of bytes of its own, which the text does not contain),
    3000 bytes of text between them"""
    text = _text()
    assert text[:120000].max() < 0x80
    parts, t, fresh = [text[:30000]], 30000, 0x80
    for plen in (1, 3):
        for L in RUN_LENGTHS:
            period = bytes(range(fresh, fresh + plen)); fresh += plen
            parts.append(np.frombuffer((period * (L // plen + 1))[:L], np.uint8))
            parts.append(text[t:t + 3000]); t += 3000
    parts.append(text[t:t + 12000])
    data = np.concatenate(parts)
    assert len(data) >= BIG
    matches = [m for _, m in _sequences(helpers.orc_compress(data)[1]) if m is not None]
    assert max(matches) > RING
    for plen in (1, 3):
        for L in RUN_LENGTHS:                                   # the run is one match: all of it but its first period
            assert any(L - plen - 8 <= m <= L - plen for m in matches), (plen, L)
    return data


@functools.lru_cache(maxsize=None)
def _alternating_block():
    """3 KiB of random bytes and 3 KiB of text in turn: the parse leaves the dense windows for sparse batches and comes back"""
    rng = np.random.default_rng(31)
    text = _text()
    parts = [text[:6000]]
    for i in range(14):
        parts.append(rng.integers(0, 256, 3072, dtype=np.uint8))
        parts.append(text[6000 + 3072 * i:6000 + 3072 * (i + 1)])
    data = np.concatenate(parts)
    assert len(data) >= BIG
    seqs = _sequences(helpers.orc_compress(data)[1])
    long_lit = [i for i, (lit, m) in enumerate(seqs) if lit >= 2048]
    assert len(long_lit) >= 12, len(long_lit)
    for i in long_lit:                                          # a match ends each long literal run, and more follow in the text
        assert seqs[i][1] is not None and seqs[i + 1][1] is not None and seqs[i + 1][0] < 64, (i, seqs[i:i + 2])
    return data


LIT_LENGTHS = (14, 15, 269, 270, 600)


@functools.lru_cache(maxsize=None)
def _literal_runs_block():
    """text, then literal runs (fresh random bytes) of the threshold lengths, each ended by a short copy from a few KiB back, so
    that they begin and end at every place of a 64-position window"""
    rng = np.random.default_rng(32)
    out = bytearray(_text()[:60000].tobytes())
    for rep in range(8):
        for lit in LIT_LENGTHS:
            for d in (-1, 0, 1):
                out += rng.integers(0, 256, lit + d, dtype=np.uint8).tobytes()
                start = len(out) - int(rng.integers(64, 4096))
                out += out[start:start + int(rng.integers(8, 40))]
    out += _text()[60000:62000].tobytes()
    data = np.frombuffer(bytes(out), np.uint8).copy()
    assert len(data) >= BIG
    seen = {lit for lit, _ in _sequences(helpers.orc_compress(data)[1])}
    assert set(LIT_LENGTHS) <= seen, sorted(seen)
    return data


def test_sizes_around_pieces_and_ring(gpu):
    """blocks that begin on a 16-byte boundary and end 0..16 bytes either side of a refill boundary and of a ring boundary"""
    text = _text()
    sizes = [BIG, BIG + 1] + [k + d for k in (67 * PIECE, 34 * RING) for d in range(-16, 17)]
    assert (67 * PIECE) % RING == PIECE
    srcs = [text[i * 97:i * 97 + n] for i, n in enumerate(sizes)]
    _check_both(gpu, srcs)


def test_source_offsets(gpu):
    """every source alignment; the first block begins at byte 0 of its tensor, the last ends at the tensor's last byte"""
    text = _text()
    srcs = [text[1000 * a:1000 * a + BIG + 1500 + 37 * a] for a in range(16)]
    align = list(range(16))
    buf, offs = _layout(srcs, align)
    assert offs[0] == 0 and [o % 16 for o in offs] == align and offs[-1] + len(srcs[-1]) == len(buf)
    _check_both(gpu, srcs, align)
    order = list(reversed(range(16)))                           # and the other way round: the aligned block last
    _check_both(gpu, [srcs[a] for a in order], order)


def test_matches_that_jump_past_the_ring(gpu):
    data = _runs_block()
    _check_both(gpu, [data, data[:BIG]], [0, 5])


def test_sparse_and_dense_in_turn(gpu):
    data = _alternating_block()
    _check_both(gpu, [data, data[3000:]], [0, 9])


def test_literal_runs_across_windows(gpu):
    data = _literal_runs_block()
    _check_both(gpu, [data, data[1:], data[2:]], [0, 0, 3])


def test_mixed_with_small_blocks(gpu):
    rng = np.random.default_rng(33)
    text = _text()
    srcs = [text[:1000], _runs_block(), text[:BIG - 1], _alternating_block(), rng.integers(0, 256, 5000, dtype=np.uint8),
            _literal_runs_block(), text[5000:5000 + 300000], text[:12], rng.integers(0, 256, BIG + 3000, dtype=np.uint8)]
    _check_both(gpu, srcs, [0, 1, 2, 15, 4, 8, 7, 6, 11])


def test_output_fills_inside_the_ring(gpu):
    """raw mode with capacities below, at and above the compressed size: the parse gives up (result 0) at many places of a
    ring's span, and fits exactly"""
    data = _text()[:BIG + 5000]
    csz = helpers.orc_compress(data)[0]
    assert 0 < csz < len(data)
    caps = [csz * k // 7 + j for k in range(1, 7) for j in (0, 1, 7)] + [csz - 1, csz, csz + 1]
    res = _check_raw(gpu, [data] * len(caps), caps, [3 * i % 16 for i in range(len(caps))])
    assert res[-3:] == [0, csz, csz] and not any(res[:-3])
