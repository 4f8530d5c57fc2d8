"""GPU: the zstd frame encoder at every level 1..12 on the search, parse and entropy catalogue (tests/zstd_enc_shapes.py): one launch
per level holding every (input, capacity) pair of that level; result and frame must equal the oracle port's (pinned to the
reference's ZSTD_compress on the same triples by tests/test_zstd_enc_shapes_cpu.py), every frame decodes back, and the bytes behind
each capacity stay untouched.  Levels 1 and 3 run once more with the batched search alone (FOURMC_ZSTD_SERIAL=1), so that both
shapes of the fast and dfast finders are held to the port and not only to each other."""
import time

import numpy as np
import pytest
import torch

import helpers
import zstd_enc_shapes as zs

pytestmark = pytest.mark.gpu
GUARD, FILL = 40, 0x5A


def _launch(gpu, level, tag=""):
    pairs = zs.expected(level)
    offs, pos, src_of = [], 1, {}
    for _, d, _, _, _ in pairs:                                    # every input once, at an odd byte offset
        if id(d) not in src_of:
            src_of[id(d)] = pos; pos += len(d) + (len(d) & 1) + 2
        offs.append(src_of[id(d)])
    assert all(o & 1 for o in offs)
    buf = np.zeros(pos + 64, np.uint8)
    for _, d, _, _, _ in pairs:
        buf[src_of[id(d)]:src_of[id(d)] + len(d)] = d
    dsts, dpos = [], 0
    for _, _, cap, _, _ in pairs:
        dsts.append(dpos); dpos += cap + GUARD
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, [len(d) for _, d, _, _, _ in pairs], [cap for _, _, cap, _, _ in pairs]))
    d_out = torch.full((dpos + 64,), FILL, dtype=torch.uint8, device="cuda")
    d_src = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    t0 = time.time()
    gpu.zstd_compress(d_src, d_out, batch, level)
    torch.cuda.synchronize()
    print(f"level {level}{tag}: {len(pairs)} frames in {time.time() - t0:.3f} s")
    res = [int(r) for r in batch.download()["result"]]
    out = d_out.cpu().numpy()
    bad = []
    for (label, d, cap, r, frame), got, o in zip(pairs, res, dsts):
        if got != r: bad.append((label, "result", got, r))
        elif not np.array_equal(out[o:o + max(got, 0)], frame): bad.append((label, "bytes", int(np.flatnonzero(out[o:o + got] != frame)[0])))
        elif not (out[o + cap:o + cap + GUARD] == FILL).all(): bad.append((label, "guard"))
        elif got > 0:
            n, back = helpers.orc_zstd_decompress(out[o:o + got], len(d))
            if n != len(d) or not np.array_equal(back, d): bad.append((label, "decode", n))
    assert not bad, (level, tag, len(bad), bad[:12])


@pytest.mark.parametrize("level", zs.LEVELS)
def test_zstd_level_equals_port_on_every_shape(gpu, level):
    _launch(gpu, level)


@pytest.mark.parametrize("level", [1, 3])
def test_zstd_batched_search_alone_equals_port_on_every_shape(gpu, level, monkeypatch):
    monkeypatch.setenv("FOURMC_ZSTD_SERIAL", "1")
    _launch(gpu, level, " (batched search alone)")


HOST_TWIN = ("text0", "text18", "text255", "text16385", "zeros1000", "zeros_2blocks", "lits1000", "lit_rle", "skew12_600", "skew_2blocks",
             "ll_sweep", "ml_sweep", "offsets", "behind7", "behind16")


@pytest.mark.parametrize("level", zs.LEVELS)
def test_host_twin_equals_port(gpu, level):
    """fourmc_ZSTD_compress, what the JNI compressBytesDirectHC(level) calls"""
    L = gpu.lib()
    by = {c.name: c for c in zs.cases()}
    for k in HOST_TWIN:
        s = by[k].data
        cs = zs.caps(s, level)                                     # bound, n - 1, r, r - 1, r - 7, n / 3: the refusing ones too
        cap = cs[(len(k) + level) % len(cs)]
        dst = np.full(max(cap, 1) + GUARD, FILL, np.uint8)
        r = L.fourmc_ZSTD_compress(dst.ctypes.data, cap, s.ctypes.data, len(s), level)
        want_r, want = zs.port(s, level, cap)
        assert r == (want_r if want_r >= 0 else (1 << 64) + want_r), (level, k, cap, r, want_r)
        if want_r > 0: assert np.array_equal(dst[:want_r], want), (level, k, cap)
        assert (dst[cap:cap + GUARD] == FILL).all(), (level, k, cap)
