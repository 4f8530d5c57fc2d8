"""GPU: LZ4 HC at every level 1..8 and 4mc Medium on the search-and-parse catalogue (tests/hc_shapes.py): one launch per level
holding every (input, capacity) pair; result and bytes must equal the oracle port's (pinned to the reference on the same pairs by
tests/test_hc_shapes_cpu.py), payloads decode back, and the bytes behind each capacity stay untouched."""
import time

import numpy as np
import pytest
import torch

import helpers
import hc_shapes as hs

pytestmark = pytest.mark.gpu
GUARD, FILL = 40, 0x5A


def _launch(gpu, level):
    pairs = hs.expected(level)
    offs, pos, src_of = [], 1, {}
    for _, d, _, _, _ in pairs:                                    # every input once, at an odd byte offset
        if id(d) not in src_of:
            src_of[id(d)] = pos; pos += len(d) + (len(d) & 1) + 2
        offs.append(src_of[id(d)])
    assert all(o & 1 for o in offs)
    buf = np.zeros(pos + 64, np.uint8)
    for _, d, _, _, _ in pairs:
        buf[src_of[id(d)]:src_of[id(d)] + len(d)] = d
    dsts, room, dpos = [], [], 0
    for _, d, cap, _, _ in pairs:
        room.append(hs.bound(len(d)) if cap < 0 else cap)          # (Medium without a limit writes at most the bound)
        dsts.append(dpos); dpos += room[-1] + GUARD
    caps = [0xFFFFFFFF if cap < 0 else cap for _, _, cap, _, _ in pairs]
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, [len(d) for _, d, _, _, _ in pairs], caps))
    d_out = torch.full((dpos + 64,), FILL, dtype=torch.uint8, device="cuda")
    d_src = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    t0 = time.time()
    if level == "mc": gpu.lz4_compress_mc(d_src, d_out, batch)
    else: gpu.lz4_compress_hc(d_src, d_out, batch, level)
    torch.cuda.synchronize()
    print(f"level {level}: {len(pairs)} blocks in {time.time() - t0:.3f} s")
    res = [int(r) for r in batch.download()["result"]]
    out = d_out.cpu().numpy()
    bad = []
    for (label, d, cap, r, comp), got, o, rm in zip(pairs, res, dsts, room):
        if got != r: bad.append((label, "result", got, r))
        elif not np.array_equal(out[o:o + max(got, 0)], comp): bad.append((label, "bytes", int(np.flatnonzero(out[o:o + got] != comp)[0])))
        elif not (out[o + rm:o + rm + GUARD] == FILL).all(): bad.append((label, "guard"))
        elif got > 0:                                              # (an empty input refused at capacity 0 leaves nothing to decode)
            n, back = helpers.orc_decompress(out[o:o + got], len(d))
            if n != len(d) or not np.array_equal(back, d): bad.append((label, "decode", n))
    assert not bad, (level, len(bad), bad[:12])


@pytest.mark.parametrize("level", hs.LEVELS)
def test_hc_level_equals_port_on_every_shape(gpu, level):
    _launch(gpu, level)


def test_medium_equals_port_on_every_shape(gpu):
    _launch(gpu, "mc")


HOST_TWIN = ("behind1", "behind2", "behind4", "behind8", "behind16", "tie_both", "fwd33_rest", "end_scalar", "back17", "back33_rest",
             "back_lookback", "fold10_twice", "n13", "n76", "flush")


@pytest.mark.parametrize("level", hs.LEVELS)
def test_host_one_block_twin_equals_port(gpu, level):
    """fourmc_LZ4_compress_HC, what the JNI compressBytesDirectHC(level) calls"""
    L = gpu.binding.lib()
    by = {c.name: c for c in hs.cases()}
    for k in HOST_TWIN:
        s = by[k].data
        cs = hs.caps(s, level)                                     # bound, n-1, r, r-1, r-6, n/2: the refusing ones too
        cap = cs[(len(k) + level) % len(cs)]
        dst = np.full(max(cap, 1) + GUARD, FILL, np.uint8)
        r = L.fourmc_LZ4_compress_HC(s.ctypes.data, dst.ctypes.data, len(s), cap, level)
        want_r, want = hs.port(s, level, cap)
        assert r == want_r and np.array_equal(dst[:max(r, 0)], want), (level, k, cap, r, want_r)
        assert (dst[cap:cap + GUARD] == FILL).all(), (level, k, cap)
