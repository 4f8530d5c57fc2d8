"""GPU: the exact LZ4 fast encoder (lz4_encode.hip, lz4_emit.hip) on the catalogue of tests/lz4_enc_shapes.py.  One raw-mode launch holds
every (input, capacity) pair, the ring cases once per source alignment 0 .. 15: result and bytes must equal the oracle port's (pinned to
the reference on the same pairs by tests/test_lz4_enc_shapes_cpu.py), the 40 bytes behind each capacity stay untouched and the payloads
decode back.  The same launch runs once more in a child process with record areas of 300 records, so that the drain inside the parse
runs at places no input chose.  Container mode over every non-empty case, and the host's one-block twin on fifteen named cases."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import helpers
import lz4_enc_shapes as ls

gpu_test = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, FILL = 40, 0x5A


def _place(blocks):
    """every input once at an odd byte offset (as test_gpu_hc_opt_shapes._place does), and the ring cases once more at every source alignment
    0 .. 15.  `blocks`: (label, data, alignment or None).  Returns the buffer and each block's offset."""
    pos, at = 1, {}
    for _, d, a in blocks:
        key = (id(d), a)
        if key in at: continue
        if a is None: pos += 1 - (pos & 1)
        else: pos += (a - pos) % 16
        at[key] = pos; pos += len(d) + 2
    buf = np.zeros(pos + 64, np.uint8)
    for _, d, a in blocks: buf[at[id(d), a]:at[id(d), a] + len(d)] = d
    offs = [at[id(d), a] for _, d, a in blocks]
    assert all(o & 1 if a is None else o % 16 == a for o, (_, _, a) in zip(offs, blocks))
    return buf, offs


def _raw_blocks():
    """(label, data, alignment, cap, result, bytes) of the raw launch"""
    out = []
    for label, d, cap, r, comp, ring in ls.expected():
        for a in (range(16) if ring and len(d) >= ls.BIG else (None,)):
            out.append((label if a is None else f"{label}|align={a}", d, a, cap, r, comp))
    return out


def _raw_launch(gpu, what):
    """the launch and its checks; returns the failures"""
    blocks = _raw_blocks()
    buf, offs = _place([(l, d, a) for l, d, a, _, _, _ in blocks])
    dsts, dpos = [], 3
    for _, _, _, cap, _, _ in blocks:
        dsts.append(dpos); dpos += cap + GUARD
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, [len(d) for _, d, _, _, _, _ in blocks], [cap for _, _, _, cap, _, _ in blocks]))
    d_out = torch.full((dpos + 64,), FILL, dtype=torch.uint8, device="cuda")
    d_src = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    t0 = time.time()
    gpu.lz4_compress_fast(d_src, d_out, batch)
    torch.cuda.synchronize()
    print(f"{what}: {len(blocks)} blocks, {len(buf) / 2 ** 20:.1f} MiB of input, in {time.time() - t0:.3f} s")
    res = [int(r) for r in batch.download()["result"]]
    out = d_out.cpu().numpy()
    bad = []
    for (label, d, a, cap, r, comp), got, o in zip(blocks, res, dsts):
        if got != r: bad.append((label, "result", got, r))
        elif not np.array_equal(out[o:o + max(got, 0)], comp): bad.append((label, "bytes", int(np.flatnonzero(out[o:o + got] != comp)[0])))
        elif not (out[o + cap:o + cap + GUARD] == FILL).all(): bad.append((label, "guard"))
        elif got > 0 and len(d):
            n, back = helpers.orc_decompress(out[o:o + got], len(d))
            if n != len(d) or not np.array_equal(back, d): bad.append((label, "decode", n))
    return bad


@gpu_test
def test_raw_mode_equals_port_on_every_pair(gpu):
    bad = _raw_launch(gpu, "raw mode")
    assert not bad, (len(bad), bad[:12])


_CHILD = """
import helpers
import test_gpu_lz4_enc_shapes as t
p = helpers.pkg(); p.gpu_init(0)
bad = t._raw_launch(p, "raw mode, record areas of %d records" % t.ls.RECORDS)
assert not bad, (len(bad), bad[:12])
print("ok")
"""


@gpu_test
def test_raw_mode_with_small_record_areas(gpu):
    """the same launch in a fresh child process with FOURMC_LZ4_RECORDS=300 (the mechanism of tests/test_gpu_lz4_mode_changes.py): every block of
    more than 172 sequences drains its area inside the parse, wherever that falls; results and bytes are the default run's, which are the port's"""
    env = dict(os.environ)
    env["FOURMC_LZ4_RECORDS"] = str(ls.RECORDS)
    r = subprocess.run([sys.executable, "-c", _CHILD], cwd=os.path.join(ROOT, "tests"), env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout, r.stdout + r.stderr


@gpu_test
def test_container_blocks_equal_port_and_decode_back(gpu):
    """encode_blocks over every non-empty case: the payload is the port's output at capacity n - 1, or the stored input where that is 0; its
    XXH32; and decode_blocks gives the input back"""
    cs = [c for c in ls.cases() if len(c.data)]
    buf, offs = _place([(c.name, c.data, 5 * i % 16 if c.ring else None) for i, c in enumerate(cs)])
    lens = [len(c.data) for c in cs]
    dsts, dpos = [], 0
    for n in lens:
        dsts.append(dpos); dpos += n + GUARD
    d_src = torch.from_numpy(buf).cuda()
    d_stage = torch.full((dpos + 64,), FILL, dtype=torch.uint8, device="cuda")
    enc = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, lens, lens))
    torch.cuda.synchronize()
    t0 = time.time()
    gpu.encode_blocks(d_src, d_stage, enc)
    torch.cuda.synchronize()
    print(f"container mode: {len(cs)} blocks in {time.time() - t0:.3f} s")
    e = enc.download()
    stage = d_stage.cpu().numpy()
    stored = 0
    for b, c in enumerate(cs):
        r, comp = ls.port(c.data, len(c.data) - 1)
        want = comp if r > 0 else c.data
        stored += r <= 0
        assert int(e["result"][b]) == len(want), c.name
        assert np.array_equal(stage[dsts[b]:dsts[b] + len(want)], want), c.name
        assert (stage[dsts[b] + len(want):dsts[b] + lens[b] + GUARD] == FILL).all(), (c.name, "bytes written past the result")
        assert int(e["xxh32"][b]) == helpers.orc_xxh32(want), c.name
    assert stored >= 5, stored                                     # (the random and the short cases do not fit n - 1)
    dec = gpu.DeviceBatch(gpu.make_blocks(dsts, offs, e["result"].astype(np.uint32), lens, e["xxh32"]))
    d_out = torch.zeros(len(buf) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.time()
    gpu.decode_blocks(d_stage, d_out, dec)
    torch.cuda.synchronize()
    print(f"container mode: {len(cs)} blocks decoded in {time.time() - t0:.3f} s")
    d = dec.download()
    out = d_out.cpu().numpy()
    for b, c in enumerate(cs):
        assert int(d["result"][b]) == len(c.data), c.name
        assert np.array_equal(out[offs[b]:offs[b] + len(c.data)], c.data), c.name


HOST_TWIN = ("n13", "n140", "small_text", "small_landing", "small_back65_byte", "small_cut63", "n131073", "features", "end131", "slots", "landing",
             "rt_misses", "dist65536", "back64_anchor", "wide2_last16", "fill_dense")


@gpu_test
def test_host_one_block_twin_equals_port(gpu):
    """fourmc_LZ4_compress_default, what the JNI compressBytesDirect calls: each named case at one of its capacities, the refusing ones too"""
    L = gpu.binding.lib()
    by = ls.by_name()
    t0 = time.time()
    refused = 0
    for i, k in enumerate(HOST_TWIN):
        s = by[k].data
        cs = ls.caps(s)
        cap = cs[i % len(cs)]
        dst = np.full(max(cap, 1) + GUARD, FILL, np.uint8)
        r = L.fourmc_LZ4_compress_default(s.ctypes.data, dst.ctypes.data, len(s), cap)
        want_r, want = ls.port(s, cap)
        refused += want_r == 0
        assert r == want_r and np.array_equal(dst[:max(r, 0)], want), (k, cap, r, want_r)
        assert (dst[max(cap, 1):max(cap, 1) + GUARD] == FILL).all(), (k, cap)
    assert refused >= 3, refused
    print(f"host twin: {len(HOST_TWIN)} calls in {time.time() - t0:.3f} s")
