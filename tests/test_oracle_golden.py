"""CPU: pins the oracle (oracle/*.c) against the golden vectors generated from the reference
itself (tests/golden/make_golden.py) and, when oracle/_ref is built, against the reference's own
compiled sources on seeded + fuzzed inputs.  No GPU, no product code."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import helpers
from helpers import B

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_xxh32_known_answers():
    for k in json.load(open(os.path.join(G, "xxh32_kat.json"))):
        d = np.frombuffer(bytes.fromhex(k["hex"]), dtype=np.uint8)
        assert helpers.orc_xxh32(d, k["seed"]) == k["xxh32"]


def test_small_container_files_match_reference_cli():
    files = json.load(open(os.path.join(G, "small_files.json")))
    for name, f in files.items():
        data = np.frombuffer(bytes.fromhex(f["input_hex"]), dtype=np.uint8)
        img = helpers.orc_container(data)
        assert img.tobytes().hex() == f["4mc_fast_hex"], name
        n, out, used = helpers.orc_container_decode(img, len(data))
        assert n == len(data) and used == len(img) and np.array_equal(out, data), name
    # vectors quoted in SURVEY.md §8(c)
    assert files["empty"]["4mc_fast_hex"].endswith("849b8d65")
    assert "0000003b000000100f7fec0a6f68656c6c6f2006001d5068656c6c6f" in files["hello10"]["4mc_fast_hex"]


def test_corpus_manifest_lz4_fast():
    m = json.load(open(os.path.join(G, "corpus_manifest.json")))
    data = helpers.corpus(m["corpus"]["bytes"], m["corpus"]["first_block"], m["corpus"]["seed"])
    assert hashlib.sha256(data.tobytes()).hexdigest() == m["corpus"]["sha256"], "corpus generator drifted"
    lvl = m["levels"]["4mc-1"]
    img = helpers.orc_container(data)
    assert len(img) == lvl["file_bytes"] and hashlib.sha256(img.tobytes()).hexdigest() == lvl["sha256"]
    for b, (u, c, s) in enumerate(lvl["blocks"]):
        blk = data[b * B: b * B + u]
        r, comp = helpers.orc_compress(blk, u - 1)
        payload = comp if r > 0 else blk
        assert (len(payload), helpers.orc_xxh32(payload)) == (c, s), b
    assert img.tobytes().hex().endswith(lvl["footer_hex"])


def test_decoder_roundtrip_edges():
    for name, d in helpers.edge_inputs().items():
        r, comp = helpers.orc_compress(d)
        assert r > 0
        n, out = helpers.orc_decompress(comp, len(d))
        assert n == len(d) and np.array_equal(out, d), name


@pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not built (needs /root/reference)")
def test_port_equals_reference_sources():
    ref = helpers.ref()
    rng = np.random.default_rng(3)
    inputs = dict(helpers.edge_inputs())
    for ln in (1, 2, 11, 12, 13, 14, 64, 65, 4095, 65535, 65546, 65547, 65548):
        inputs[f"rnd{ln}"] = (rng.integers(0, 4, ln) * 17).astype(np.uint8)
    for name, d in inputs.items():
        bound = helpers.oracle().orc_lz4_compress_bound(len(d))
        for cap in (bound, max(len(d) - 1, 0), max(len(d) // 2, 0)):
            out = np.zeros(bound + 64, np.uint8)
            r_ref = ref.LZ4_compress_default(d.ctypes.data, out.ctypes.data, len(d), cap)
            r, comp = helpers.orc_compress(d, cap)
            assert r == r_ref, (name, cap)
            assert np.array_equal(comp, out[:max(r_ref, 0)]), (name, cap)
        assert helpers.orc_xxh32(d, 5) == ref.XXH32(d.ctypes.data, len(d), 5)
    # fuzzed streams: same accept/reject and the same negative codes
    n_checked = 0
    for name in ("text_60k", "period37", "lit_then_run", "hello10", "far_repeat"):
        d = inputs[name][:120000]
        _, comp = helpers.orc_compress(d)
        for t in range(300):
            m = comp.copy()
            k = t % 4
            if k == 0: m[rng.integers(0, len(m))] ^= 1 << rng.integers(0, 8)
            elif k == 1: m = m[: rng.integers(1, len(m))]
            elif k == 2:
                i = rng.integers(0, len(m)); m[i:i + 3] = rng.integers(0, 256, len(m[i:i + 3]), dtype=np.uint8)
            else: m = np.concatenate([m, rng.integers(0, 256, rng.integers(1, 9), dtype=np.uint8)])
            cap = len(d) + (0 if t % 2 else 100)
            r, out = helpers.orc_decompress(m, cap)
            if r == -(2 ** 31):
                continue                      # offset 0: undefined behaviour in the reference
            o2 = np.zeros(cap + 64, np.uint8)
            r_ref = ref.LZ4_decompress_safe(m.ctypes.data, o2.ctypes.data, len(m), cap)
            assert r == r_ref, (name, t, r, r_ref)
            if r >= 0:
                assert np.array_equal(out, o2[:r])
            n_checked += 1
    assert n_checked > 1000


# ------------------------------------------------------------------------------------------ zstd decode port
def test_zstd_port_golden_frames_and_4mz_files():
    z = json.load(open(os.path.join(G, "zstd_frames.json")))
    for name, e in z.items():
        for lvl, hx in e["frames"].items():
            for slack in (0, 123):
                r, out = helpers.orc_zstd_decompress(bytes.fromhex(hx), e["input_bytes"] + slack)
                assert r == e["input_bytes"], (name, lvl, r)
                assert hashlib.sha256(out.tobytes()).hexdigest() == e["input_sha256"], (name, lvl)
            # one byte short of the content size -> dstSize_tooSmall in the reference
            if e["input_bytes"] > 0:
                assert helpers.orc_zstd_decompress(bytes.fromhex(hx), e["input_bytes"] - 1)[0] < 0
    files = json.load(open(os.path.join(G, "small_files.json")))
    p = helpers.pkg()
    for name, f in files.items():
        img = np.frombuffer(bytes.fromhex(f["4mz_fast_hex"]), np.uint8)
        blocks, _ = p.split_container(img, p.MAGIC_4MZ)
        got = b""
        for b in blocks:
            pay = img[int(b["src_off"]): int(b["src_off"]) + int(b["src_len"])]
            assert helpers.orc_xxh32(pay) == int(b["xxh32"])
            if b["src_len"] == b["dst_cap"]:
                got += pay.tobytes()
            else:
                r, out = helpers.orc_zstd_decompress(pay.tobytes(), int(b["dst_cap"]))
                assert r == int(b["dst_cap"])
                got += out.tobytes()
        assert got == bytes.fromhex(f["input_hex"]), name


@pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not built (needs /root/reference)")
def test_zstd_port_equals_reference_sources():
    ref = helpers.ref()
    rng = np.random.default_rng(23)
    data = helpers.corpus(12 * B)
    for lvl, blocks in ((1, range(12)), (3, (0, 4, 7)), (6, (1, 4, 10)), (12, (3,))):
        for b in blocks:
            src = data[b * B:(b + 1) * B]
            out = np.zeros(B + 65536, np.uint8)
            r = ref.ZSTD_compress(out.ctypes.data, len(out), src.ctypes.data, B, lvl)
            assert not ref.ZSTD_isError(r)
            d, dec = helpers.orc_zstd_decompress(out[:r].tobytes(), B)
            assert d == B and np.array_equal(dec, src), (lvl, b)
    # mutated frames: same accept/reject as ZSTD_decompress, identical bytes when accepted
    z = json.load(open(os.path.join(G, "zstd_frames.json")))
    n = lenient = 0
    for name in ("text_30k", "lit_then_run_30k", "two_symbols_30k", "period37_20k"):
        for lvl in ("1", "3", "6", "12"):
            base = np.frombuffer(bytes.fromhex(z[name]["frames"][lvl]), np.uint8)
            cap = z[name]["input_bytes"]
            for t in range(120):
                m = base.copy()
                k = t % 4
                if k == 0: m[rng.integers(0, len(m))] ^= 1 << rng.integers(0, 8)
                elif k == 1: m = m[: rng.integers(1, len(m))]
                elif k == 2:
                    i = rng.integers(4, len(m)); m[i:i + 2] = rng.integers(0, 256, len(m[i:i + 2]), dtype=np.uint8)
                else: m = np.concatenate([m, rng.integers(0, 256, rng.integers(1, 6), dtype=np.uint8)])
                m = np.ascontiguousarray(m)
                dst = np.zeros(cap + 64, np.uint8)
                rr = ref.ZSTD_decompress(dst.ctypes.data, cap, m.ctypes.data, len(m))
                r, out = helpers.orc_zstd_decompress(m.tobytes(), cap)
                if ref.ZSTD_isError(rr):
                    assert r < 0, (name, lvl, t, r)              # never accept what the reference rejects
                elif r >= 0:
                    assert r == rr and np.array_equal(out, dst[:rr]), (name, lvl, t, r, rr)   # same bytes when both accept
                else:
                    lenient += 1    # (until round 3: damaged streams the reference's double-symbol Huffman decoder let through;
                                    #  its end rules are restated now and none may be left)
                n += 1
    assert n > 1500 and lenient == 0, (n, lenient)             # (round 3: both Huffman decoders' end rules and the bit reader's reads past a stream's start are restated)


# ------------------------------------------------------------------------------------------ LZ4 HC port
def test_lz4hc_port_golden_manifest():
    """`4mc -3` (LZ4 HC level 4) per-block sizes/checksums written by the reference CLI."""
    m = json.load(open(os.path.join(G, "corpus_manifest.json")))
    data = helpers.corpus(m["corpus"]["bytes"])
    for b, (u, c, x) in enumerate(m["levels"]["4mc-3"]["blocks"]):
        if b % 3 and b != 12:
            continue                                   # HC is slow on one host core: sample + the ragged tail
        blk = data[b * B: b * B + u]
        r, comp = helpers.orc_compress_hc(blk, 4, u - 1)
        payload = comp if r > 0 else blk
        assert (len(payload), helpers.orc_xxh32(payload)) == (c, x), b
    u, c, x = m["levels"]["4mc-4"]["blocks"][3]        # `4mc -4` = HC level 8
    r, comp = helpers.orc_compress_hc(data[3 * B: 3 * B + u], 8, u - 1)
    assert (len(comp), helpers.orc_xxh32(comp)) == (c, x)


@pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not built (needs /root/reference)")
def test_lz4hc_port_equals_reference_sources():
    ref = helpers.ref()
    for name, d in helpers.edge_inputs().items():
        d = np.ascontiguousarray(d)
        bound = helpers.oracle().orc_lz4_compress_bound(len(d))
        for lvl in range(1, 9):
            for cap in (bound, max(len(d) - 1, 0), len(d) // 3):
                out = np.zeros(bound + 64, np.uint8)
                rr = ref.LZ4_compress_HC(d.ctypes.data, out.ctypes.data, len(d), cap, lvl)
                r, comp = helpers.orc_compress_hc(d, lvl, cap)
                assert r == rr and np.array_equal(comp, out[:max(rr, 0)]), (name, lvl, cap, r, rr)


# ------------------------------------------------------------------------------------------ 4mc Medium port
def test_lz4mc_port_golden_manifest():
    m = json.load(open(os.path.join(G, "corpus_manifest.json")))
    data = helpers.corpus(m["corpus"]["bytes"])
    for b, (u, c, x) in enumerate(m["levels"]["4mc-2"]["blocks"]):
        blk = data[b * B: b * B + u]
        r, comp = helpers.orc_compress_mc(blk, u - 1)
        payload = comp if r > 0 else blk
        assert (len(payload), helpers.orc_xxh32(payload)) == (c, x), b


@pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not built (needs /root/reference)")
def test_lz4mc_port_equals_reference_sources():
    import ctypes as C
    ref = helpers.ref()
    ref.LZ4_compressMC.argtypes = [C.c_void_p, C.c_void_p, C.c_int]; ref.LZ4_compressMC.restype = C.c_int
    ref.LZ4_compressMC_limitedOutput.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]; ref.LZ4_compressMC_limitedOutput.restype = C.c_int
    for name, d in helpers.edge_inputs().items():
        d = np.ascontiguousarray(d)
        for cap in (-1, max(len(d) - 1, 0), len(d) // 2):
            out = np.zeros(len(d) + len(d) // 255 + 80, np.uint8)
            rr = (ref.LZ4_compressMC(d.ctypes.data, out.ctypes.data, len(d)) if cap < 0
                  else ref.LZ4_compressMC_limitedOutput(d.ctypes.data, out.ctypes.data, len(d), cap))
            r, comp = helpers.orc_compress_mc(d, cap)
            assert r == rr and np.array_equal(comp, out[:max(rr, 0)]), (name, cap, r, rr)


# ------------------------------------------------------------------------------------------ zstd encoder port (levels 1 .. 12; 4mz uses 1, 3, 6, 12)
def test_zstd_enc_port_golden_frames():
    """The committed frames the reference's ZSTD_compress wrote (tests/golden/zstd_frames.json) - every strategy 4mz reaches:
    fast, dfast, lazy / lazy2 (rows and chains), btlazy2 (level 12, 16 KiB + 1 .. 256 KiB), btopt (level 12, <= 16 KiB)."""
    import hashlib
    z = json.load(open(os.path.join(G, "zstd_frames.json")))
    inputs = helpers.golden_zstd_inputs()
    assert set(z) == set(inputs)
    for name, e in z.items():
        d = np.ascontiguousarray(inputs[name])
        assert hashlib.sha256(d.tobytes()).hexdigest() == e["input_sha256"], name
        for lvl, hx in e["frames"].items():
            r, comp = helpers.orc_zstd_compress(d, int(lvl), len(d) + 1024)
            assert r == len(hx) // 2 and comp.tobytes().hex() == hx, (name, lvl)


@pytest.mark.parametrize("level,key", [(1, "4mz-1"), (3, "4mz-2"), (6, "4mz-3"), (12, "4mz-4")])
def test_zstd_enc_port_golden_manifest(level, key):
    """`4mc -z -1` / `-z -2` (ZSTD_compress level 1 / 3, capacity n-1) per-block sizes/checksums written by the reference CLI."""
    m = json.load(open(os.path.join(G, "corpus_manifest.json")))
    data = helpers.corpus(m["corpus"]["bytes"])
    for b, (u, c, x) in enumerate(m["levels"][key]["blocks"]):
        if level == 12 and b % 3:
            continue                                   # level 12 runs at ~25 MB/s on one host core: sample
        blk = data[b * B: b * B + u]
        r, comp = helpers.orc_zstd_compress(blk, level, u - 1)
        payload = comp if r > 0 else blk
        assert (len(payload), helpers.orc_xxh32(payload)) == (c, x), b
        if r > 0 and b % 4 == 0:                       # and the frames decode back with the decoder port
            assert np.array_equal(helpers.orc_zstd_decompress(comp, u)[1], blk)


@pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not built (needs /root/reference)")
def test_zstd_enc_port_level12_size_classes():
    """Level 12: lazy2 above 256 KiB, btlazy2 (binary tree) down to 16 KiB + 1, btopt (optimal parser) at 16 KiB and
    below - all three pinned to the reference's own ZSTD_compress here."""
    import ctypes as C
    ref = helpers.ref()
    ref.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]; ref.ZSTD_compress.restype = C.c_size_t
    assert helpers.orc_zstd_compress(helpers.corpus(16384), 12)[0] > 0 and helpers.orc_zstd_compress(helpers.corpus(300000), 12)[0] > 0
    assert helpers.orc_zstd_compress(helpers.corpus(1000), 13)[0] == -1000         # a level beyond the port (btlazy2 on full blocks, btultra): refused, not guessed

    def check(d, cap, tag):
        d = np.array(d, dtype=np.uint8, copy=True)
        out = np.zeros(max(cap, 1) + 64, np.uint8)
        rr = ref.ZSTD_compress(out.ctypes.data, cap, d.ctypes.data, len(d), 12)
        rr = rr if rr < (1 << 62) else rr - (1 << 64)
        r, comp = helpers.orc_zstd_compress(d, 12, cap)
        assert r == rr and np.array_equal(comp, out[:max(rr, 0)]), (tag, len(d), cap, r, rr)
        return rr

    rng = np.random.default_rng(12)
    src = helpers.corpus(3 * B, first_block=2)
    for n in (16385, 16390, 32768, 65535, 65536, 65537, 100000, 131071, 131072, 131073, 200000, 262143, 262144):
        off = int(rng.integers(0, 2 * B))
        check(src[off:off + n], helpers.zstd_bound(n), "size")
        check(src[off:off + n], n - 1, "size n-1")
    # btopt: price model switches at 1024 bytes (predefined costs), window / table clamps below
    for n in (0, 1, 2, 3, 7, 8, 9, 12, 13, 17, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2048, 4095, 4096, 4097, 8192, 10000, 16383, 16384):
        for _ in range(2):
            off = int(rng.integers(0, 2 * B))
            check(src[off:off + n], helpers.zstd_bound(n), "btopt size")
            check(src[off:off + n], max(n - 1, 0), "btopt size n-1")
    for name, d in helpers.edge_inputs().items():
        for d in ([d[:262144]] if len(d) > 16384 else []) + [d[:16384], d[:5000], d[:700]]:
            for cap in {max(len(d) - 1, 0), helpers.zstd_bound(len(d)), len(d) // 3}:
                check(d, cap, name)
    import test_gpu_fuzz                                                # the structured fuzz inputs of the GPU suite, cut to btopt sizes
    for d in test_gpu_fuzz._inputs(77, 120):
        d = d[: int(rng.integers(0, 16385))] if len(d) > 16384 else d
        check(d, max(len(d) - 1, 0), "btopt fuzz")
    d = src[5000: 5000 + 70000]
    c = check(d, helpers.zstd_bound(len(d)), "bound")
    for cap in range(max(0, c - 16), c + 6):
        check(d, cap, "tight")


@pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("level", [2, 4, 5, 7, 8, 9, 10, 11])
def test_zstd_enc_port_other_levels_equal_reference_sources(level):
    """The levels 4mz does not use but the JNI entry point may pass (1..12 run on the device): the port against the reference's own
    ZSTD_compress over the size classes of the level table, edge inputs, and the capacities 4mz / the bound give."""
    import ctypes as C
    ref = helpers.ref()
    ref.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]; ref.ZSTD_compress.restype = C.c_size_t
    src = helpers.corpus(2 * B, first_block=5)
    cases = [(k, v) for k, v in helpers.edge_inputs().items()]
    for n in (700, 5000, 16384, 16385, 60000, 131072, 131073, 262144, 262145, 600000):
        cases.append(("n%d" % n, src[12345:12345 + n]))
    for name, d in cases:
        d = np.ascontiguousarray(d)
        for cap in (helpers.zstd_bound(len(d)), max(len(d) - 1, 0)):
            out = np.zeros(max(cap, 1) + 64, np.uint8)
            rr = ref.ZSTD_compress(out.ctypes.data, cap, d.ctypes.data, len(d), level)
            rr = rr if rr < (1 << 62) else rr - (1 << 64)
            r, comp = helpers.orc_zstd_compress(d, level, cap)
            assert r == rr and np.array_equal(comp, out[:max(rr, 0)]), (name, len(d), cap, r, rr)


@pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not built (needs /root/reference)")
@pytest.mark.parametrize("level", [1, 3, 6])
def test_zstd_enc_port_equals_reference_sources(level):
    import ctypes as C
    ref = helpers.ref()
    ref.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]; ref.ZSTD_compress.restype = C.c_size_t
    ref.ZSTD_compressBound.argtypes = [C.c_size_t]; ref.ZSTD_compressBound.restype = C.c_size_t

    def check(d, cap, tag):
        d = np.ascontiguousarray(d)
        out = np.zeros(max(cap, 1) + 64, np.uint8)
        rr = ref.ZSTD_compress(out.ctypes.data, cap, d.ctypes.data, len(d), level)
        rr = rr if rr < (1 << 62) else rr - (1 << 64)           # size_t error code -> -(error number)
        r, comp = helpers.orc_zstd_compress(d, level, cap)
        assert r == rr and np.array_equal(comp, out[:max(rr, 0)]), (tag, len(d), cap, r, rr)
        return rr

    for n in (0, 1, 6, 7, 18, 19, 63, 64, 300, 1024, 1025, 16384, 16385, 131072, 131073, 262144, 262145, 700001):
        assert helpers.zstd_bound(n) == ref.ZSTD_compressBound(n)
    rng = np.random.default_rng(11)
    for name, d in helpers.edge_inputs().items():
        for cap in {max(len(d) - 1, 0), helpers.zstd_bound(len(d)), len(d) // 3, 18}:
            check(d, cap, name)
    # size classes of the level table (16 KiB / 128 KiB / 256 KiB) and 128 KiB sub-block tails
    src = helpers.corpus(3 * B, first_block=5)
    for n in (16383, 16384, 16385, 131071, 131072, 131073, 131079, 262144, 262145, 262151, 524289, 1500001, 2 * 1024 * 1024 + 77, 3 * 1024 * 1024):
        off = int(rng.integers(0, B))
        check(src[off:off + n], n - 1, "size")
    # capacity sweep around the real frame size: every overflow rule of the bit/byte writers
    for n in (100, 1000, 20000, 140000):
        d = src[7 * n: 8 * n]
        c = check(d, helpers.zstd_bound(n), "bound")
        for cap in range(max(0, c - 24), c + 10):
            check(d, cap, "tight")
