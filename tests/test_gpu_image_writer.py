"""The streaming image writer (fourmc_gpu_image_writer_*, ImageWriter): for every way the input is cut into appends, the image is
the one compress_image writes for the concatenation - and so the CLI's file - with bounded staging, stream-order safety, other
engine calls and other writers in between, the capacity refusal, and poisoning after a failure."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

ROOT = helpers.ROOT
B = helpers.B
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "corpus_manifest.json")))
EINVAL, ENOMEM = -3, -4
CONFIGS = [(z, lv) for z in (False, True) for lv in (1, 2, 3, 4)]


def _sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def _magic(p, z):
    return p.MAGIC_4MZ if z else p.MAGIC_4MC


def _cuda(data):
    return torch.from_numpy(np.ascontiguousarray(data)).cuda() if len(data) else torch.zeros(0, dtype=torch.uint8, device="cuda")


def compress(p, d_src, z, level):
    d_img = torch.empty(p.image_bound(d_src.numel()), dtype=torch.uint8, device="cuda")
    n = p.compress_image(d_src, d_img, _magic(p, z), level)
    return d_img[:n].cpu().numpy().tobytes()


def write(p, d_src, cuts, z, level, batch_blocks=0, cap=None):
    """The image of d_src appended in pieces of the sizes `cuts` (the last one may be None: the rest)"""
    d_img = torch.empty(cap or p.image_bound(d_src.numel()), dtype=torch.uint8, device="cuda")
    with p.ImageWriter(d_img, _magic(p, z), level, batch_blocks) as w:
        at = 0
        for c in cuts:
            c = d_src.numel() - at if c is None else c
            w.append(d_src[at:at + c])
            at += c
        assert at == d_src.numel()
        n = w.finish()
    return d_img[:n].cpu().numpy().tobytes()


def random_cuts(total, seed, hi=3 * B // 2):
    rng = np.random.default_rng(seed)
    cuts = []
    while sum(cuts) < total:
        cuts.append(int(min(rng.integers(1, hi), total - sum(cuts))))
    return cuts


def cli_compress(exe, tmp_path, data, z, level, tag):
    src, out = tmp_path / f"in_{tag}", tmp_path / f"out_{tag}"
    src.write_bytes(bytes(data))
    r = subprocess.run([exe] + (["-z"] if z else []) + [f"-{level}", "-f", str(src), str(out)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return out.read_bytes()


@pytest.fixture(scope="module")
def p(gpu):
    return gpu


@pytest.fixture(scope="module")
def golden():
    c = MANIFEST["corpus"]
    data = helpers.corpus(c["bytes"], first_block=c["first_block"], seed=c["seed"])
    assert _sha(data) == c["sha256"]
    return data


# ---- 1: every CLI configuration, every way of cutting ------------------------------------------------------------------
@pytest.mark.parametrize("z,level", CONFIGS)
def test_every_cut_gives_the_image_of_the_concatenation(p, golden, tmp_path, z, level):
    data = golden[:2 * B + 4321]
    d_src = _cuda(data)
    want = compress(p, d_src, z, level)
    cuttings = {
        "one": [None],
        "edges": [0, 1, B - 1, 1, B + 5, None],
        "random": random_cuts(len(data), 7 + level + 10 * z),
        "multiples": [B, B, None],
    }
    for name, cuts in cuttings.items():
        assert write(p, d_src, cuts, z, level) == want, (z, level, name)
    if level == 1:
        assert cli_compress(p.cli_path(), tmp_path, data, z, level, "own") == want
        ref = helpers.ref_cli()
        if ref is not None:
            assert cli_compress(ref, tmp_path, data, z, level, "ref") == want, "reference CLI"


# ---- 2: edge inputs ----------------------------------------------------------------------------------------------------
def test_edge_inputs(p, golden):
    empty = _cuda(golden[:0])
    want = compress(p, empty, False, 1)
    assert len(want) == 44
    assert write(p, empty, [], False, 1) == want
    assert write(p, empty, [0, 0, 0], False, 1) == want
    assert write(p, empty, [], True, 1) == compress(p, empty, True, 1)
    for n, cuts in ((B, [None]), (B, [B // 2, None]), (B - 1, [1, None]), (B + 1, [1, None]), (B + 1, [B, 1])):
        d_src = _cuda(golden[:n])
        for z in (False, True):
            assert write(p, d_src, cuts, z, 1) == compress(p, d_src, z, 1), (n, cuts, z)


# ---- 3: the golden corpus against its manifest -------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["4mc-1", "4mc-2", "4mc-3", "4mc-4", "4mz-1", "4mz-2"])
def test_golden_corpus_in_random_chunks(p, golden, name):
    z, level = name.startswith("4mz"), int(name[-1])
    d_src = _cuda(golden)
    img = write(p, d_src, random_cuts(len(golden), 100 + level + 10 * z, hi=5 * B // 2), z, level)
    want = MANIFEST["levels"][name]
    assert len(img) == want["file_bytes"] and _sha(img) == want["sha256"], name
    d_img = _cuda(np.frombuffer(img, np.uint8))
    d_dst = torch.zeros(len(golden), dtype=torch.uint8, device="cuda")
    st = p.decompress_image(d_img, d_dst, _magic(p, z))
    assert st["exit_code"] == 0 and st["blocks"] == 13 and st["decoded_bytes"] == len(golden), st
    assert torch.equal(d_dst, d_src)
    info, ent = p.image_index(d_img)
    assert info["nblocks"] == 13 and info["framing"] == 0 and info["total_bytes"] == len(golden)
    usize = np.minimum(B, len(golden) - np.arange(13, dtype=np.int64) * B)
    assert ent["usize"].tolist() == usize.tolist()
    assert ent["data_off"].tolist() == (np.arange(13, dtype=np.int64) * B).tolist()
    off = 12 + np.concatenate([[0], np.cumsum(12 + ent["csize"].astype(np.int64))[:-1]])
    assert ent["image_off"].tolist() == off.tolist()


# ---- 4: bounded staging ------------------------------------------------------------------------------------------------
def test_small_batches(p, golden):
    data = np.concatenate([golden, golden[:B // 3]])[:9 * B + 777]
    d_src = _cuda(data)
    want = compress(p, d_src, False, 1)
    for batch in (1, 3):
        assert write(p, d_src, [None], False, 1, batch_blocks=batch) == want, batch
        assert write(p, d_src, [B + 3, 4 * B, None], False, 1, batch_blocks=batch) == want, batch


def test_512_blocks_in_random_chunks_at_batch_64(p):
    base = helpers.corpus(48 * B)
    d_src = torch.from_numpy(base).cuda().repeat(512 // 48 + 1)[:512 * B - 12345].contiguous()
    want = compress(p, d_src, False, 1)
    got = write(p, d_src, random_cuts(d_src.numel(), 512, hi=40 * B), False, 1, batch_blocks=64)
    assert _sha(got) == _sha(want) and len(got) == len(want)


# ---- 5: stream order: a chunk may be overwritten once the stream has passed its append ----------------------------------
def test_chunks_overwritten_after_their_append(p, golden):
    data = golden[:3 * B + 999]
    d_src = _cuda(data)
    for z, level in ((False, 1), (True, 1), (False, 3)):
        want = compress(p, d_src, z, level)
        d_img = torch.empty(p.image_bound(d_src.numel()), dtype=torch.uint8, device="cuda")
        with p.ImageWriter(d_img, _magic(p, z), level, batch_blocks=2) as w:
            at = 0
            for c in random_cuts(d_src.numel(), 5 + level, hi=2 * B):
                chunk = d_src[at:at + c].clone()
                w.append(chunk)
                chunk.fill_(0xA5)                    # on the writer's stream, behind the append's work
                del chunk                            # back to the caching allocator: record_stream holds it for the writer
                scratch = torch.full((c,), 0x5A, dtype=torch.uint8, device="cuda")
                del scratch
                at += c
            n = w.finish()
        assert d_img[:n].cpu().numpy().tobytes() == want, (z, level)


# ---- 6: other engine calls and other writers in between -----------------------------------------------------------------
def test_other_engine_calls_between_appends(p, golden):
    data = golden[:4 * B + 5]
    d_src = _cuda(data)
    want = compress(p, d_src, False, 3)
    other = _cuda(golden[5 * B:8 * B + 17])
    other_img = compress(p, other, False, 1)
    d_other_img = _cuda(np.frombuffer(other_img, np.uint8))
    d_img = torch.empty(p.image_bound(d_src.numel()), dtype=torch.uint8, device="cuda")
    w = p.ImageWriter(d_img, p.MAGIC_4MC, 3, batch_blocks=2)
    cuts = [B + 7, 2 * B, 100, None]
    at = 0
    for i, c in enumerate(cuts):
        c = d_src.numel() - at if c is None else c
        w.append(d_src[at:at + c])
        at += c
        # the same stream, other data: whole-image compress / decompress / read, and block encode
        assert compress(p, other, True, 1 + i % 2)[:4] == b"4MZ\0"
        assert compress(p, other, False, 1) == other_img
        d_dst = torch.zeros(other.numel(), dtype=torch.uint8, device="cuda")
        assert p.decompress_image(d_other_img, d_dst, p.MAGIC_4MC)["exit_code"] == 0 and torch.equal(d_dst, other)
        res = p.image_read(d_other_img, [(B - 10, 20 + i, 0)], d_dst)
        assert res.tolist() == [20 + i]
        blocks = p.make_blocks([0, B], [0, B], [B, B], [B, B])
        batch = p.DeviceBatch(blocks)
        stage = torch.empty(2 * B, dtype=torch.uint8, device="cuda")
        p.encode_blocks(other, stage, batch, p.CODEC_LZ4_HC, 4)
        assert (batch.download()["result"] > 0).all()
    n = w.finish()
    assert d_img[:n].cpu().numpy().tobytes() == want


def test_two_writers_at_once(p, golden):
    a, b = _cuda(golden[:3 * B + 11]), _cuda(golden[6 * B:8 * B + 4000])
    want_a, want_b = compress(p, a, False, 1), compress(p, b, True, 1)
    ca, cb = random_cuts(a.numel(), 1), random_cuts(b.numel(), 2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for sa, sb in ((s1, s2), (None, None)):             # two streams, then both on the current stream
        for s in (sa, sb):
            if s is not None:
                s.wait_stream(torch.cuda.current_stream())
        ia = torch.empty(p.image_bound(a.numel()), dtype=torch.uint8, device="cuda")
        ib = torch.empty(p.image_bound(b.numel()), dtype=torch.uint8, device="cuda")
        wa = p.ImageWriter(ia, p.MAGIC_4MC, 1, batch_blocks=1, stream=sa)
        wb = p.ImageWriter(ib, p.MAGIC_4MZ, 1, batch_blocks=2, stream=sb)
        pa = pb = 0
        for i in range(max(len(ca), len(cb))):
            if i < len(ca):
                wa.append(a[pa:pa + ca[i]]); pa += ca[i]
            if i < len(cb):
                wb.append(b[pb:pb + cb[i]]); pb += cb[i]
        na, nb = wa.finish(), wb.finish()
        torch.cuda.synchronize()
        assert ia[:na].cpu().numpy().tobytes() == want_a
        assert ib[:nb].cpu().numpy().tobytes() == want_b


# ---- 7: capacity -------------------------------------------------------------------------------------------------------
def test_capacity_refusal_leaves_the_writer_usable(p, golden):
    data = golden[:2 * B + 50]
    d_src = _cuda(data)
    want = compress(p, d_src, False, 1)
    d_img = torch.empty(p.image_bound(d_src.numel()), dtype=torch.uint8, device="cuda")
    big = _cuda(golden[:2 * B + 51])
    with p.ImageWriter(d_img, p.MAGIC_4MC, 1) as w:
        with pytest.raises(p.EngineError, match=r"\(-3\).*capacity"):
            w.append(big)
        w.append(d_src[:B + 1])
        with pytest.raises(p.EngineError, match=r"\(-3\)"):
            w.append(big[:B + 50])                        # one byte past the bound
        w.append(d_src[B + 1:])
        with pytest.raises(p.EngineError, match=r"\(-3\)"):
            w.append(big[:1])
        n = w.finish()
    assert d_img[:n].cpu().numpy().tobytes() == want
    with pytest.raises(p.EngineError, match=r"\(-3\)"):
        p.ImageWriter(d_img, 0x11223344, 1)
    with pytest.raises(p.EngineError, match=r"\(-3\)"):
        p.ImageWriter(d_img[:43], p.MAGIC_4MC, 1)


# ---- 8: poisoning ------------------------------------------------------------------------------------------------------
POISON = r"""
import ctypes as C, importlib, json, sys
sys.path.insert(0, sys.argv[1])
import torch
p = importlib.import_module("4mc_amd")
p.gpu_init(0)
L = p.lib()
B = p.BLOCKSIZE
src = torch.full((2 * B + 5,), 7, dtype=torch.uint8, device="cuda")
img = torch.empty(p.image_bound(src.numel()), dtype=torch.uint8, device="cuda")
h = C.c_void_p(0)
s = torch.cuda.current_stream().cuda_stream
out = {"begin": L.fourmc_gpu_image_writer_begin(C.byref(h), img.data_ptr(), img.numel(), p.MAGIC_4MC, 3, 0, s)}
out["append1"] = L.fourmc_gpu_image_writer_append(h, src.data_ptr(), 2 * B)
out["append2"] = L.fourmc_gpu_image_writer_append(h, src.data_ptr(), 5)
n = C.c_uint64(0)
out["finish"] = L.fourmc_gpu_image_writer_finish(h, C.byref(n))
torch.cuda.synchronize()
print(json.dumps(out))
"""


def test_a_failure_poisons_the_writer(p):
    env = dict(os.environ, FOURMC_WS_FAIL_ABOVE="1")
    r = subprocess.run([sys.executable, "-c", POISON, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out == {"begin": 0, "append1": ENOMEM, "append2": ENOMEM, "finish": ENOMEM}, out


# ---- 9: the Python object ----------------------------------------------------------------------------------------------
def test_python_writer_lifecycle(p, golden):
    d_src = _cuda(golden[:B + 3])
    d_img = torch.empty(p.image_bound(d_src.numel()), dtype=torch.uint8, device="cuda")
    w = p.ImageWriter(d_img)
    w.append(d_src)
    n = w.finish()
    assert d_img[:n].cpu().numpy().tobytes() == compress(p, d_src, False, 1)
    assert w.closed
    for call in (lambda: w.append(d_src), w.finish, w.abort):
        with pytest.raises(p.EngineError, match="finished or aborted"):
            call()
    with pytest.raises(ValueError):
        with p.ImageWriter(d_img, p.MAGIC_4MZ, 2) as w2:
            w2.append(d_src[:100])
            raise ValueError("boom")
    assert w2.closed
    with pytest.raises(p.EngineError, match="finished or aborted"):
        w2.append(d_src[:1])
    w3 = p.ImageWriter(d_img)
    w3.append(d_src[:10])
    w3.abort()
    with pytest.raises(p.EngineError, match="finished or aborted"):
        w3.finish()
