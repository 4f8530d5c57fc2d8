"""The exact LZ4 fast encoder's byte emitter (lz4_emit.hip): the parse (K2) writes sequence records, a second kernel writes the
LZ4 bytes.  Edge cases of that hand-off against the oracle, byte for byte: block sizes around the minimum and the 16-bit /
32-bit table switch, literal runs and match lengths at their length-byte thresholds, stored blocks, exact capacities, a
block of last literals only, a launch cut into pieces, and the drain of a full record area inside the parse."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers
from helpers import B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 0x5A


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw_encode(gpu, srcs, caps, src_shift=3):
    """fourmc_gpu_lz4_compress_fast over one batch; returns results, outputs and whether every byte behind each result
    (up to cap + 40) is still the guard."""
    offs, pos = [], src_shift
    for s in srcs:
        offs.append(pos); pos += len(s)
    buf = np.zeros(pos + 64, np.uint8)
    for s, o in zip(srcs, offs):
        buf[o:o + len(s)] = s
    dsts, dpos = [], 5
    for c in caps:
        dsts.append(dpos); dpos += c + 40
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, [len(s) for s in srcs], caps))
    d_out = torch.full((dpos + 64,), GUARD, dtype=torch.uint8, device="cuda")
    gpu.lz4_compress_fast(_dev(buf), d_out, batch)
    res = [int(r) for r in batch.download()["result"]]
    out = d_out.cpu().numpy()
    outs = [out[d:d + max(r, 0)].copy() for d, r in zip(dsts, res)]
    clean = [bool((out[d + max(r, 0):d + c + 40] == GUARD).all()) for d, c, r in zip(dsts, caps, res)]
    return res, outs, clean


def _check_raw(gpu, srcs, caps):
    res, outs, clean = _raw_encode(gpu, srcs, caps)
    for i, (s, c) in enumerate(zip(srcs, caps)):
        want_r, want = helpers.orc_compress(s, c)
        assert res[i] == want_r, (i, len(s), c, res[i], want_r)
        if want_r > 0:
            assert np.array_equal(outs[i], want), (i, len(s), c)
        assert clean[i], (i, len(s), c, "bytes written past the result")
    return res


def _check_container(gpu, srcs):
    """container mode (capacity n-1, stored when it does not fit) against the oracle's block payloads"""
    offs, pos = [], 0
    for s in srcs:
        offs.append(pos); pos += len(s)
    buf = np.zeros(pos + 64, np.uint8)
    for s, o in zip(srcs, offs):
        buf[o:o + len(s)] = s
    lens = [len(s) for s in srcs]
    dsts = [i * (B + 64) for i in range(len(srcs))]
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, lens, lens))
    d_out = torch.full((len(srcs) * (B + 64) + 64,), GUARD, dtype=torch.uint8, device="cuda")
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
        assert (out[dsts[i] + r:dsts[i] + B + 64] == GUARD).all(), (i, "bytes written past the result")
        assert int(enc["xxh32"][i]) == helpers.orc_xxh32(want), i


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


def _runs_input(rng, lits, matches):
    """Random bytes in which the greedy parse meets literal runs and matches of about the given lengths: each literal run is
    fresh random bytes, each match copies (overlapping when longer than its distance) bytes a few KiB back."""
    out = bytearray(rng.integers(0, 256, 4096, dtype=np.uint8).tobytes())
    for lit, m in zip(lits, matches):
        out += rng.integers(0, 256, lit, dtype=np.uint8).tobytes()
        start = len(out) - int(rng.integers(64, 4096))
        for k in range(m):
            out.append(out[start + k])
    out += rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    return np.frombuffer(bytes(out), np.uint8).copy()


def test_block_sizes(gpu):
    rng = np.random.default_rng(11)
    text = helpers.corpus(B)
    srcs = []
    for n in (0, 1, 12, 13, 14, 65535, 65546, 65547, 65548, 100000):
        srcs.append(text[:n].copy())
        srcs.append(rng.integers(0, 4, n, dtype=np.uint8))
    bound = [helpers.oracle().orc_lz4_compress_bound(len(s)) for s in srcs]
    _check_raw(gpu, srcs, bound)
    _check_raw(gpu, srcs, [max(len(s) - 1, 0) for s in srcs])
    _check_container(gpu, srcs)


def test_length_thresholds(gpu):
    """literal runs and match lengths of 14, 15, 269, 270 and above 64 KiB: the token nibble, one length byte, two"""
    rng = np.random.default_rng(12)
    edges = [v + d for v in (14, 15, 18, 19, 269, 270, 273, 274) for d in (-1, 0, 1)] * 4
    lits = edges + [70000, 3, 0, 1]
    matches = list(reversed(edges)) + [20, 70000, 40, 5]
    data = _runs_input(rng, lits, matches)
    comp = helpers.orc_compress(data)[1]
    seen = _sequences(comp)
    lit_seen = {lit for lit, _ in seen}
    ml_seen = {m for _, m in seen if m is not None}
    assert {14, 15, 269, 270} <= lit_seen and max(lit_seen) >= 65536, sorted(lit_seen)[:40]
    assert {18, 19, 273, 274} <= ml_seen and max(ml_seen) >= 65536, sorted(ml_seen)[:40]   # match codes 14, 15, 269, 270
    zeros = np.zeros(300000, np.uint8)                                                          # one match of ~300 KB
    srcs = [data, zeros, data[: len(data) // 2]]
    _check_raw(gpu, srcs, [helpers.oracle().orc_lz4_compress_bound(len(s)) for s in srcs])
    _check_container(gpu, srcs)


def test_incompressible_and_exact_capacity(gpu):
    rng = np.random.default_rng(13)
    noise = rng.integers(0, 256, B, dtype=np.uint8)
    text = helpers.corpus(2 * B)
    blocks = [noise, text[:B].copy(), text[B:B + 777777].copy(), noise[:70000].copy()]
    _check_container(gpu, blocks)
    _check_raw(gpu, blocks, [len(s) - 1 for s in blocks])                       # noise: 0 (does not fit)
    sizes = [helpers.orc_compress(s)[0] for s in blocks]
    assert sizes[0] > B and sizes[1] < B
    res = _check_raw(gpu, blocks, sizes)                                        # exactly the compressed size
    assert res == sizes
    res = _check_raw(gpu, blocks, [c - 1 for c in sizes])                       # one less: 0
    assert res == [0, 0, 0, 0]


def test_last_literals_only(gpu):
    rng = np.random.default_rng(14)
    srcs = [rng.integers(0, 256, n, dtype=np.uint8) for n in (13, 64, 300, 5000, 65547, 200000)]
    for s in srcs:
        assert len(_sequences(helpers.orc_compress(s)[1])) == 1
    _check_raw(gpu, srcs, [helpers.oracle().orc_lz4_compress_bound(len(s)) for s in srcs])


def _child(env_extra, code):
    env = dict(os.environ)
    env.update(env_extra)
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout, r.stdout + r.stderr


_CHILD = """
import numpy as np, torch, helpers
from test_gpu_lz4_emit import _check_raw, _check_container
p = helpers.pkg(); p.gpu_init(0)
B = p.BLOCKSIZE
text = helpers.corpus(6 * B)
rng = np.random.default_rng(15)
blocks = [text[i * B:(i + 1) * B].copy() for i in range(5)] + [rng.integers(0, 256, B, dtype=np.uint8), text[5 * B:5 * B + 4321].copy()]
_check_container(p, blocks)
_check_raw(p, blocks, [helpers.oracle().orc_lz4_compress_bound(len(s)) for s in blocks])
_check_raw(p, blocks[:3] + [rng.integers(0, 3, 3 * B, dtype=np.uint8)], [B] * 3 + [3 * B])
print("ok")
"""


def test_pieces_halve_when_the_record_workspace_is_refused(gpu):
    """a 4 MiB block's record area is 16 MiB: refusing leases above three of them cuts the launch into pieces of two blocks"""
    _child({"FOURMC_WS_FAIL_ABOVE": str(3 * (16 << 20) + 64 * 1024)}, _CHILD)


def test_drain_of_a_full_record_area(gpu):
    """record areas of 300 records: every block drains its records into the output inside the parse, many times"""
    _child({"FOURMC_LZ4_RECORDS": "300"}, _CHILD)
