"""GPU: ZSTD frame decode on every frame shape the reference can write (tests/zstd_shapes.py), on both decode paths: the entropy
stage + execute kernel (split) and the one-wave kernel.  The committed fixture subset (tests/golden/zstd_shapes.json) always
runs; the generated set and the reference's verdicts on damaged frames need oracle/_ref."""
import ctypes as C
import hashlib
import subprocess

import numpy as np
import pytest
import torch

import helpers
import zstd_shapes as zs
from helpers import B
from test_gpu_zstd import _decode

pytestmark = pytest.mark.gpu
needs_ref = pytest.mark.skipif(helpers.ref() is None, reason="oracle/_ref not present")


def _cases():
    """[(name, frame, output length, output sha256)]: the fixture, and the generated set when the reference is built."""
    out = [("fx:" + n, f, ln, sha) for n, f, ln, sha in zs.fixture_frames()]
    if helpers.ref() is not None:
        out += [(n, f, len(e), hashlib.sha256(e).hexdigest()) for n, f, e in zs.frames()]
    return out


class _Paths:
    """Both decode paths in turn, with the research build's execute-kernel counters; restores the setting."""
    def __init__(self, gpu):
        self.gpu = gpu

    def __enter__(self):
        self.gpu.use_research(True); self.gpu.gpu_init()
        self.lib = self.gpu.lib()
        self.before = self.lib.fourmc_gpu_get_zstd_decode_split()
        return self

    def __exit__(self, *a):
        self.lib.fourmc_gpu_set_zstd_decode_split(self.before)
        self.gpu.use_research(False)

    def set(self, split):
        self.lib.fourmc_gpu_set_zstd_decode_split(split)

    def counts(self):
        done, back = C.c_ulonglong(0), C.c_ulonglong(0)
        assert self.lib.fourmc_gpu_debug_zstd_exec_counts(C.byref(done), C.byref(back)) == 0
        return done.value, back.value


def _guards_intact(raw, dsts, caps):
    return all(np.all(raw[d + c:d + c + 64] == 0xA5) for d, c in zip(dsts, caps))


def test_zstd_shapes_valid_frames_both_paths(gpu):
    """Every frame class at exact capacity, at capacity + 300 and at one capacity too small, on both paths: the reference's result
    and bytes, nothing written past the capacity.  At exact capacity each class is launched alone and the execute kernel's counters
    are read: a class the split path's decline rules (zstd_decode.hip, zstd_decode_frame_v2 steps 0 and 1a) do not name is
    completed by the execute kernel, a class they name is not and still decodes correctly."""
    cases = _cases()
    table = []
    with _Paths(gpu) as P:
        for split in (1, 0):
            P.set(split)
            for name, f, n, sha in cases:
                P.counts()                                              # (reset)
                res, outs, raw, dsts = _decode(gpu, [f], [n])
                done, back = P.counts()
                by_design = zs.rejected_by_design(f)
                if by_design: assert res[0] < 0, (name, split, res[0])
                else:
                    assert res[0] == n, (name, split, res[0])
                    assert hashlib.sha256(outs[0].tobytes()).hexdigest() == sha, (name, split)
                assert _guards_intact(raw, dsts, [n]), (name, split)
                named = zs.declines(f, n)
                if split: table.append((name, "handed to the one-wave path by rule" if named else "execute kernel", done, back))
                assert (done, back) == ((0, 0) if (named or not split) else (1, 0)), (name, split, named, done, back)
            # capacity + 300, and one capacity too small (one byte short for every other class, half for the rest), in one launch
            frames = [f for _, f, _, _ in cases] + [f for _, f, n, _ in cases if n > 0]
            small = [n - 1 if i % 2 else n // 2 for i, (_, _, n, _) in enumerate(cases) if n > 0]
            caps = [n + 300 for _, _, n, _ in cases] + small
            res, outs, raw, dsts = _decode(gpu, frames, caps)
            assert _guards_intact(raw, dsts, caps), split
            for (name, f, n, sha), r, o in zip(cases, res, outs):
                if zs.rejected_by_design(f): assert r < 0, (name, split, r)
                else: assert r == n and hashlib.sha256(o.tobytes()).hexdigest() == sha, (name, split, r)
            for (name, f, n, _), r, c in zip([c for c in cases if c[2] > 0], res[len(cases):], small):
                assert r < 0, (name, split, c, r)
                if helpers.ref() is not None: assert zs.ref_decode(f, c)[0] < 0, name
                assert helpers.orc_zstd_decompress(f, c)[0] < 0, name
    print("\nframe class | completed by | execute kernel done / handed back")
    for row in table: print("%-40s | %-36s | %d / %d" % row)
    assert any(t[1] == "execute kernel" for t in table) and any(t[1] != "execute kernel" for t in table)


def _launch_damaged(gpu, P, items, chunks=(200, 320)):
    """items [(label, bytes, cap)] through both paths in launches of 200 and 320 frames (with and without the helper wave):
    {split: (results, outputs)}"""
    got = {}
    for split in (1, 0):
        P.set(split)
        rs, os_, at, k = [], [], 0, 0
        while at < len(items):
            part = items[at:at + chunks[k % 2]]; at += len(part); k += 1
            caps = [c for _, _, c in part]
            res, outs, raw, dsts = _decode(gpu, [m for _, m, _ in part], caps)
            assert _guards_intact(raw, dsts, caps), (split, at)
            rs += [int(r) for r in res]; os_ += [o.tobytes() for o in outs]
        got[split] = (rs, os_)
    return got


@needs_ref
def test_zstd_shapes_damaged_frames_both_paths(gpu):
    """The damaged set of the CPU test (structure-aware damage of every frame class): on both paths the verdict is the
    reference's and the oracle's, and so are the bytes of every accepted frame.  Nothing is excluded."""
    items = zs.damaged_set()
    with _Paths(gpu) as P:
        got = _launch_damaged(gpu, P, items)
    lenient = accepted = 0
    for i, (label, m, cap) in enumerate(items):
        rr, want = zs.ref_decode(m, cap)
        wr, w = helpers.orc_zstd_decompress(m, cap)
        for split in (1, 0):
            r, o = got[split][0][i], got[split][1][i]
            assert (r < 0) == (wr < 0) and (r < 0 or (r == wr and o == w.tobytes())), (label, split, r, wr)
            if rr < 0: assert r < 0, (label, split, r)
            elif r >= 0: assert r == rr and o == want, (label, split, r, rr)
            else: lenient += 1
        accepted += rr >= 0
    print(f"damaged frames: {len(items)}, accepted by the reference and both paths: {accepted}")
    assert lenient == 0


def test_zstd_shapes_mixed_launch_neighbours_undisturbed(gpu):
    """One launch mixes ordinary level-1 frames with the unusual ones and with damaged ones: every frame gets the verdict and the
    bytes it gets alone (the oracle's, which the CPU test holds to the reference's), whatever its neighbours are."""
    data = helpers.corpus(B)
    fx = zs.fixture_frames()
    items = []                                                          # (label, frame, cap, expected result, expected bytes)
    for i, (name, f, n, sha) in enumerate(fx):
        src = data[i * 100000: i * 100000 + 150000 + 777 * i]
        r, comp = helpers.orc_zstd_compress(src, 1)
        assert r > 0
        items.append((f"ordinary{i}", bytes(comp[:r]), len(src)))
        items.append((name, f, n))
        items += [(lab, m, n) for lab, m in zs.damaged(name, f, 4, seed=0xB0)]
    want = [helpers.orc_zstd_decompress(f, c) for _, f, c in items]
    assert sum(r >= 0 for r, _ in want) > len(fx) and sum(r < 0 for r, _ in want) > len(fx) // 2
    with _Paths(gpu) as P:
        for split in (1, 0):
            P.set(split)
            caps = [c for _, _, c in items]
            res, outs, raw, dsts = _decode(gpu, [f for _, f, _ in items], caps)
            assert _guards_intact(raw, dsts, caps), split
            for (label, _, _), r, o, (wr, w) in zip(items, res, outs, want):
                assert (r < 0) == (wr < 0), (label, split, r, wr)
                if wr >= 0: assert r == wr and np.array_equal(o, w), (label, split)


@needs_ref
def test_zstd_shapes_container_of_reference_frames(gpu, tmp_path):
    """A .4mz image whose blocks are the reference's frames of level 19 and level -5 (and one block kept raw) goes through
    decode_blocks, decompress_image, ImageReader in small chunks and `4mc -d -z`: all give the input."""
    ref = helpers.ref()
    data = np.concatenate([helpers.corpus(B), helpers.corpus(B, logs=True), np.random.default_rng(3).integers(0, 256, B, dtype=np.uint8),
                           helpers.corpus(B, first_block=5)[: 1234567]])
    calls = []

    def codec(ctx, src, n, dst, cap):
        level = 19 if len(calls) % 2 == 0 else -5
        calls.append(level)
        r = ref.ZSTD_compress(dst, cap, src, n, level)
        return 0 if ref.ZSTD_isError(r) else int(r)                    # does not fit: the container keeps the block raw
    fn = helpers._BLOCK_FN(codec)
    L = helpers.oracle()
    cap = L.orc_container_bound(len(data))
    img = np.empty(cap, np.uint8)
    n = L.orc_container_compress(data.ctypes.data, len(data), img.ctypes.data, cap, gpu.MAGIC_4MZ, C.cast(fn, C.c_void_p), None)
    assert n > 0 and calls == [19, -5, 19, -5]
    img = img[:n].copy()
    want = data.tobytes()
    d_img = torch.from_numpy(np.concatenate([img, np.zeros(64, np.uint8)])).cuda()
    # decode_blocks
    blocks, used = gpu.split_container(img, gpu.MAGIC_4MZ)
    assert used == len(img) and len(blocks) == 4
    batch = gpu.DeviceBatch(blocks)
    d_out = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    gpu.decode_blocks(d_img, d_out, batch, codec=gpu.CODEC_ZSTD)
    assert int(batch.download()["result"].sum()) == len(data)
    assert d_out[: len(data)].cpu().numpy().tobytes() == want
    # decompress_image
    d_out = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda")
    st = gpu.decompress_image(d_img, d_out[: len(data)], gpu.MAGIC_4MZ, image_bytes=len(img))
    assert st["decoded_bytes"] == len(data) and d_out[: len(data)].cpu().numpy().tobytes() == want, st
    # ImageReader in small chunks
    d_out = torch.full((len(data) + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    with gpu.ImageReader(d_out[: len(data)], gpu.MAGIC_4MZ, 2) as r:
        for a in range(0, len(img), 300001):
            r.append(torch.from_numpy(img[a:a + 300001].copy()).cuda())
        st2 = r.finish()
    assert st2 == st, (st2, st)
    assert d_out[: len(data)].cpu().numpy().tobytes() == want and bool((d_out[len(data):] == 0x5A).all())
    # the CLI
    src = tmp_path / "ref.4mz"; src.write_bytes(img.tobytes())
    out = tmp_path / "ref.out"
    r = subprocess.run([gpu.cli_path(), "-d", "-z", "-f", str(src), str(out)], capture_output=True)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == want
