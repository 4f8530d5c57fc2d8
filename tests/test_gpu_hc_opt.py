"""GPU: LZ4 HC levels 9..12 (lz4hc_opt_encode.hip) byte for byte against the reference's own LZ4_compress_HC
(oracle/_ref/libref4mc.so; native/lz4/lz4hc.c:958-973): level 9 is the hash chain with pattern analysis (:553-788),
10..12 the optimal parser (:1330-1626) with pattern analysis and chain swap (:239-447).  Return values included: 0 when
the output does not fit.  Levels <= 0 map to 9 and levels > 12 to 12 (:840-841), on every entry point."""
import numpy as np
import pytest
import torch

import helpers
from hc_opt_inputs import shapes as _shapes
from helpers import B

pytestmark = pytest.mark.gpu
U8 = np.uint8


@pytest.fixture(scope="module")
def ref():
    r = helpers.ref()
    if r is None:
        pytest.fail("oracle/_ref/libref4mc.so is missing: __graft_entry__.build() makes it where /root/reference exists, and it travels with the tree")
    return r


def _bound(n):
    return n + n // 255 + 16


def _ref_hc(ref, s, cap, level):
    s = np.ascontiguousarray(s, dtype=U8)
    d = np.zeros(max(cap, 1) + 64, U8)
    r = ref.LZ4_compress_HC(s.ctypes.data, d.ctypes.data, len(s), cap, level)
    return r, d[:max(r, 0)].copy()


def _dev_hc(gpu, items, caps, level):
    """one launch of fourmc_gpu_lz4_compress_hc over `items`; returns [(result, bytes)]"""
    offs, pos = [], 0
    for d in items:
        offs.append(pos); pos += (len(d) + 63) // 64 * 64 + 64
    src = np.zeros(pos + 64, U8)
    for d, o in zip(items, offs):
        src[o:o + len(d)] = d
    doffs, dpos = [], 0
    for c in caps:
        doffs.append(dpos); dpos += (max(c, 1) + 63) // 64 * 64 + 64
    d_dst = torch.full((dpos + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    batch = gpu.DeviceBatch(gpu.make_blocks(offs, doffs, [len(d) for d in items], caps))
    gpu.lz4_compress_hc(torch.from_numpy(src).cuda(), d_dst, batch, level)
    torch.cuda.synchronize()
    res = batch.download()["result"]
    out = d_dst.cpu().numpy()
    return [(int(res[i]), out[doffs[i]: doffs[i] + max(int(res[i]), 0)]) for i in range(len(items))]


def _check(gpu, ref, named, level, caps_of):
    """every (input, cap) pair in ONE launch, compared with the reference"""
    names, items, caps = [], [], []
    for k, s in named.items():
        for cap in caps_of(ref, s, level):
            names.append((k, cap)); items.append(np.ascontiguousarray(s, dtype=U8)); caps.append(cap)
    got = _dev_hc(gpu, items, caps, level)
    for (k, cap), s, (r, o) in zip(names, items, got):
        want_r, want = _ref_hc(ref, s, cap, level)
        assert r == want_r, (level, k, cap, r, want_r)
        assert np.array_equal(o, want), (level, k, cap)


def _four_caps(ref, s, level):
    """bound, n - 1, n / 2, and one byte less than the reference needs (for inputs that end in literals: the last literals)"""
    n = len(s)
    caps = [_bound(n), max(n - 1, 0), n // 2]
    r, _ = _ref_hc(ref, s, _bound(n), level)
    if r > 1:
        caps.append(r - 1)
    return caps


@pytest.mark.parametrize("level", [9, 10, 11, 12])
def test_shapes_sizes_and_caps_equal_the_reference(gpu, ref, level):
    shapes = _shapes()
    if level == 12:                                  # 16384 attempts per search: adversarial inputs stay at most 256 KiB
        shapes = {k: v[: 256 << 10] for k, v in shapes.items()}
    _check(gpu, ref, shapes, level, _four_caps)


@pytest.mark.parametrize("level,blocks", [(9, (0, 1, 3, 5, 8, 11)), (10, (0, 1, 3, 5, 8, 11)), (11, (0, 2, 3, 7)), (12, (2, 3, 8))])
def test_full_corpus_blocks_equal_the_reference(gpu, ref, level, blocks):
    named = {"blk%d" % k: helpers.corpus(B, first_block=k) for k in blocks}
    _check(gpu, ref, named, level, lambda r, s, lv: [_bound(len(s)), len(s) - 1])


def test_levels_outside_9_to_12_map_like_the_reference(gpu, ref):
    ed = helpers.edge_inputs()
    named = {k: ed[k] for k in ("hello10", "text_60k", "period37", "lit_then_run", "random_small", "thirteen")}
    for level, same_as in ((0, 9), (-7, 9), (13, 12), (1000, 12)):
        names = list(named)
        got = _dev_hc(gpu, [named[k] for k in names], [_bound(len(named[k])) for k in names], level)
        for k, (r, o) in zip(names, got):
            want_r, want = _ref_hc(ref, named[k], _bound(len(named[k])), same_as)
            assert (r, o.tobytes()) == (want_r, want.tobytes()), (level, k)
            assert _ref_hc(ref, named[k], _bound(len(named[k])), level)[0] == want_r, (level, k)


@pytest.mark.parametrize("level", [9, 10])
def test_one_launch_of_many_blocks_keeps_them_independent(gpu, ref, level):
    rng = np.random.default_rng(level)
    data = helpers.corpus(2 * B, first_block=6)
    items, caps = [], []
    for i in range(80):
        n = int(rng.choice([0, 1, 13, 100, 5000, 65536, 70000, int(rng.integers(0, 200000))]))
        o = int(rng.integers(0, 2 * B - n))
        items.append(np.ascontiguousarray(data[o:o + n])); caps.append(_bound(n) if i % 3 else max(n - 1, 0))
    got = _dev_hc(gpu, items, caps, level)
    for i, (s, cap, (r, o)) in enumerate(zip(items, caps, got)):
        want_r, want = _ref_hc(ref, s, cap, level)
        assert r == want_r and np.array_equal(o, want), (level, i, len(s), cap)


@pytest.mark.parametrize("level", [9, 10, 11, 12])
def test_container_blocks_store_or_compress_and_decode_back(gpu, ref, level):
    """fourmc_gpu_4mc_encode_blocks(HC, level): payload = LZ4_compress_HC(cap = n - 1), stored when that is <= 0, XXH32 of the
    payload, and the device decoder gives the input back"""
    ed = helpers.edge_inputs()
    srcs = [ed["text_60k"], ed["random_small"], ed["zeros_64k"], ed["period200"], helpers.corpus(B, first_block=3)[:300000],
            np.frombuffer(b"abcabcabcabcabcab", U8)]
    offs, pos = [], 0
    for s in srcs:
        offs.append(pos); pos += (len(s) + 63) // 64 * 64 + 64
    buf = np.zeros(pos + 64, U8)
    for s, o in zip(srcs, offs):
        buf[o:o + len(s)] = s
    lens = [len(s) for s in srcs]
    d_src = torch.from_numpy(buf).cuda()
    d_stage = torch.zeros(pos + 64, dtype=torch.uint8, device="cuda")
    enc = gpu.DeviceBatch(gpu.make_blocks(offs, offs, lens, lens))
    gpu.encode_blocks(d_src, d_stage, enc, codec=gpu.CODEC_LZ4_HC, level=level)
    e = enc.download()
    stage = d_stage.cpu().numpy()
    for b, s in enumerate(srcs):
        r, comp = _ref_hc(ref, s, len(s) - 1, level)
        want = comp if r > 0 else s
        assert int(e["result"][b]) == len(want), (level, b)
        assert np.array_equal(stage[offs[b]: offs[b] + len(want)], want), (level, b)
        assert int(e["xxh32"][b]) == helpers.orc_xxh32(want), (level, b)
    dec = gpu.DeviceBatch(gpu.make_blocks(offs, offs, e["result"].astype(np.uint32), lens, e["xxh32"]))
    d_out = torch.zeros(pos + 64, dtype=torch.uint8, device="cuda")
    gpu.decode_blocks(d_stage, d_out, dec, codec=gpu.CODEC_LZ4_HC)
    d = dec.download()
    out = d_out.cpu().numpy()
    for b, s in enumerate(srcs):
        assert int(d["result"][b]) == len(s), (level, b)
        assert np.array_equal(out[offs[b]: offs[b] + len(s)], s), (level, b)


@pytest.mark.parametrize("level", [9, 12])
def test_host_one_block_twin_equals_the_reference(gpu, ref, level):
    """fourmc_LZ4_compress_HC, what the JNI compressBytesDirectHC(level) calls (native/jniCompressor.c:157)"""
    L = gpu.binding.lib()
    ed = helpers.edge_inputs()
    for k in ("hello10", "text_60k", "lit_then_run", "period7", "random_small", "empty"):
        s = np.ascontiguousarray(ed[k])
        for cap in (_bound(len(s)), max(len(s) - 1, 0)):
            dst = np.zeros(max(cap, 1) + 16, U8)
            r = L.fourmc_LZ4_compress_HC(s.ctypes.data, dst.ctypes.data, len(s), cap, level)
            want_r, want = _ref_hc(ref, s, cap, level)
            assert r == want_r and np.array_equal(dst[:max(r, 0)], want), (level, k, cap)
