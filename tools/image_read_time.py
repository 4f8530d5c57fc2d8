"""Times random access into a device image on one GPU (hipEvents through torch.cuda.Event), 2048 S-mix blocks (48 distinct,
replicated), 4mc level 1:
  image_decode_blocks(0, n)               against  decompress_image on the same image
  image_read, one range over everything   against  decompress_image
  image_read, 256 x 64 KiB at seeded      against  decode_blocks on host-built descriptors of exactly the distinct blocks those
  random offsets                                   ranges touch
  the index alone (image_index, summary)  at 2048 blocks and at 16384 (stored blocks of 1..64 bytes: the cost is per block),
                                          against the fast parser's size query (decompress_image with no destination)
Prints one JSON line; [median, min, max] ms of --reps after one warm-up call of each.
    python tools/image_read_time.py [--blocks 2048] [--reps 5]"""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
from image_time import timed  # noqa: E402


def stored_image(p, nblocks, seed=3):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, 65, nblocks)
    raw = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8)
    L = p.lib()
    pays, sums, at = [], [], 0
    for s in sizes.tolist():
        pay = raw[at:at + s]
        at += s
        pays.append(pay.tobytes())
        sums.append(L.fourmc_XXH32(pay.ctypes.data, s, 0))
    return p.assemble_container(p.MAGIC_4MC, sizes, sizes, sums, pays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ranges", type=int, default=256)
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    p.gpu_init(0)
    B, nb = p.BLOCKSIZE, a.blocks
    base = helpers.corpus(48 * B)
    d_src = torch.from_numpy(base).cuda().repeat(nb // 48 + 1)[:nb * B].contiguous()
    d_img = torch.empty(p.image_bound(nb * B), dtype=torch.uint8, device="cuda")
    n = p.compress_image(d_src, d_img, p.MAGIC_4MC, 1)
    d_img = d_img[:n]
    res = {"blocks": nb, "bytes": nb * B, "reps": a.reps}
    d_dst = torch.empty(nb * B, dtype=torch.uint8, device="cuda")
    res["decompress_image_ms"] = timed(lambda: p.decompress_image(d_img, d_dst, p.MAGIC_4MC), a.reps)
    r = [0]

    def blocks():
        r[0] = p.image_decode_blocks(d_img, 0, nb, d_dst)
    d_dst.zero_()
    res["image_decode_blocks_ms"] = timed(blocks, a.reps)
    assert r[0] == nb * B and torch.equal(d_dst, d_src)
    whole = np.array([[0, nb * B, 0]], dtype=np.uint64)
    rr = [None]

    def read_all():
        rr[0] = p.image_read(d_img, whole, d_dst)
    d_dst.zero_()
    res["image_read_whole_ms"] = timed(read_all, a.reps)
    assert rr[0].tolist() == [nb * B] and torch.equal(d_dst, d_src)
    # 256 ranges of 64 KiB at seeded random offsets, packed back to back
    rng = np.random.default_rng(2026)
    K, L64 = a.ranges, 64 * 1024
    off = rng.integers(0, nb * B - L64, K).astype(np.uint64)
    q = np.stack([off, np.full(K, L64, np.uint64), np.arange(K, dtype=np.uint64) * L64], 1)
    d_out = torch.empty(K * L64, dtype=torch.uint8, device="cuda")

    def read_some():
        rr[0] = p.image_read(d_img, q, d_out)
    res["image_read_256x64k_ms"] = timed(read_some, a.reps)
    assert (rr[0] == L64).all()
    want = torch.cat([d_src[int(o):int(o) + L64] for o in off])
    assert torch.equal(d_out, want)
    # the blocks API on host-built descriptors of exactly the distinct blocks those ranges touch
    info, ent = p.image_index(d_img)
    touched = np.unique(np.concatenate([off // B, (off + L64 - 1) // B])).astype(np.int64)
    k = len(touched)
    dblocks = p.make_blocks(ent["image_off"][touched] + 12, np.arange(k, dtype=np.uint64) * B, ent["csize"][touched],
                            ent["usize"][touched], ent["xxh32"][touched])
    dbatch = p.DeviceBatch(dblocks)
    d_stage = torch.empty(k * B, dtype=torch.uint8, device="cuda")
    res["touched_blocks"] = int(k)
    res["decode_blocks_touched_ms"] = timed(lambda: p.decode_blocks(d_img, d_stage, dbatch), a.reps)
    del d_stage, d_out
    # the index alone: the summary, one read-back
    ii = p.ImageIndexInfo()

    def index(t, nbytes):
        assert p.lib().fourmc_gpu_image_index(t.data_ptr(), nbytes, None, 0, C.byref(ii), None) == 0
    res["image_index_ms"] = timed(lambda: index(d_img, n), a.reps)
    res["parse_fast_ms"] = timed(lambda: p.decompress_image(d_img, None, p.MAGIC_4MC), a.reps)
    small = stored_image(p, 16384)
    d_small = torch.from_numpy(np.frombuffer(small, np.uint8).copy()).cuda()
    assert p.image_index(d_small)[0]["nblocks"] == 16384
    res["image_index_16384_ms"] = timed(lambda: index(d_small, len(small)), a.reps)
    res["parse_fast_16384_ms"] = timed(lambda: p.decompress_image(d_small, None, p.MAGIC_4MC), a.reps)
    res = {k_: ([round(x, 4) for x in v] if isinstance(v, tuple) else v) for k_, v in res.items()}
    res["note"] = "[median, min, max] ms; every call includes its own stream synchronizations"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
