"""GPU: LZ4 HC at levels 9..12 (lz4hc_opt_encode.hip) on the search, pattern, swap and price catalogue (tests/hc_opt_shapes.py): one
launch per level holding every (input, capacity) pair; result and bytes must equal the oracle port's (pinned to the reference on
the same pairs by tests/test_hc_opt_shapes_cpu.py), payloads decode back, and the bytes behind each capacity stay untouched."""
import time

import numpy as np
import pytest
import torch

import helpers
import hc_opt_shapes as ho

pytestmark = pytest.mark.gpu
GUARD, FILL = 40, 0x5A


def _place(datas):
    """every input once, at an odd byte offset"""
    pos, at = 1, {}
    for d in datas:
        if id(d) not in at:
            at[id(d)] = pos; pos += len(d) + (len(d) & 1) + 2
    buf = np.zeros(pos + 64, np.uint8)
    for d in datas:
        buf[at[id(d)]:at[id(d)] + len(d)] = d
    assert all(o & 1 for o in at.values())
    return buf, [at[id(d)] for d in datas]


@pytest.mark.parametrize("level", ho.LEVELS)
def test_hc_level_equals_port_on_every_shape(gpu, level):
    pairs = ho.expected(level)
    buf, offs = _place([d for _, d, _, _, _ in pairs])
    dsts, dpos = [], 0
    for _, _, cap, _, _ in pairs:
        dsts.append(dpos); dpos += cap + GUARD
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, dsts, [len(d) for _, d, _, _, _ in pairs], [cap for _, _, cap, _, _ in pairs]))
    d_out = torch.full((dpos + 64,), FILL, dtype=torch.uint8, device="cuda")
    d_src = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    t0 = time.time()
    gpu.lz4_compress_hc(d_src, d_out, batch, level)
    torch.cuda.synchronize()
    print(f"level {level}: {len(pairs)} blocks in {time.time() - t0:.3f} s")
    res = [int(r) for r in batch.download()["result"]]
    out = d_out.cpu().numpy()
    bad = []
    for (label, d, cap, r, comp), got, o in zip(pairs, res, dsts):
        if got != r: bad.append((label, "result", got, r))
        elif not np.array_equal(out[o:o + max(got, 0)], comp): bad.append((label, "bytes", int(np.flatnonzero(out[o:o + got] != comp)[0])))
        elif not (out[o + cap:o + cap + GUARD] == FILL).all(): bad.append((label, "guard"))
        elif got > 0:
            n, back = helpers.orc_decompress(out[o:o + got], len(d))
            if n != len(d) or not np.array_equal(back, d): bad.append((label, "decode", n))
    assert not bad, (level, len(bad), bad[:12])


@pytest.mark.parametrize("level", ho.LEVELS)
def test_container_blocks_equal_port_and_decode_back(gpu, level):
    """encode_blocks(HC, level) over every case once: the payload is the port's output at capacity n - 1, or the stored input where
    that is <= 0; its XXH32; and decode_blocks gives the input back"""
    cs = [c for c in ho.cases_of(level) if len(c.data)]           # (a container has no empty block)
    buf, offs = _place([c.data for c in cs])
    lens = [len(c.data) for c in cs]
    d_src = torch.from_numpy(buf).cuda()
    d_stage = torch.full((len(buf) + 64,), FILL, dtype=torch.uint8, device="cuda")
    enc = gpu.DeviceBatch(gpu.make_blocks(offs, offs, lens, lens))
    torch.cuda.synchronize()
    t0 = time.time()
    gpu.encode_blocks(d_src, d_stage, enc, codec=gpu.CODEC_LZ4_HC, level=level)
    torch.cuda.synchronize()
    print(f"level {level}: {len(cs)} container blocks in {time.time() - t0:.3f} s")
    e = enc.download()
    stage = d_stage.cpu().numpy()
    for b, c in enumerate(cs):
        r, comp = ho.port(c.data, level, len(c.data) - 1)
        want = comp if r > 0 else c.data
        assert int(e["result"][b]) == len(want), (level, c.name)
        assert np.array_equal(stage[offs[b]:offs[b] + len(want)], want), (level, c.name)
        assert int(e["xxh32"][b]) == helpers.orc_xxh32(want), (level, c.name)
    dec = gpu.DeviceBatch(gpu.make_blocks(offs, offs, e["result"].astype(np.uint32), lens, e["xxh32"]))
    d_out = torch.zeros(len(buf) + 64, dtype=torch.uint8, device="cuda")
    gpu.decode_blocks(d_stage, d_out, dec, codec=gpu.CODEC_LZ4_HC)
    d = dec.download()
    out = d_out.cpu().numpy()
    for b, c in enumerate(cs):
        assert int(d["result"][b]) == len(c.data), (level, c.name)
        assert np.array_equal(out[offs[b]:offs[b] + len(c.data)], c.data), (level, c.name)


HOST_TWIN = ("n13", "run", "period2_long", "runs_grow", "runs_nogap", "four_differ", "swap_late", "same97", "chunks64", "clusters", "wide_lane63_hi",
             "first200_4082", "lit15_ml19", "back64", "text1_1200")


@pytest.mark.parametrize("level", ho.LEVELS)
def test_host_one_block_twin_equals_port(gpu, level):
    """fourmc_LZ4_compress_HC, what the JNI compressBytesDirectHC(level) calls"""
    L = gpu.binding.lib()
    by = {c.name: c for c in ho.cases()}
    t0 = time.time()
    for k in HOST_TWIN:
        s = by[k].data
        cs = ho.caps(s, level)                                     # bound, n-1, r, r-1, r-6, n/2: the refusing ones too
        cap = cs[(len(k) + level) % len(cs)]
        dst = np.full(max(cap, 1) + GUARD, FILL, np.uint8)
        r = L.fourmc_LZ4_compress_HC(s.ctypes.data, dst.ctypes.data, len(s), cap, level)
        want_r, want = ho.port(s, level, cap)
        assert r == want_r and np.array_equal(dst[:max(r, 0)], want), (level, k, cap, r, want_r)
        assert (dst[cap:cap + GUARD] == FILL).all(), (level, k, cap)
    print(f"level {level}: {len(HOST_TWIN)} host calls in {time.time() - t0:.3f} s")
