"""Times the whole-image device API on one GPU (hipEvents through torch.cuda.Event), 2048 S-mix blocks (48 distinct, replicated):
  compress_image                 against  encode_blocks + pack_image (offsets precomputed, already in HBM)
  decompress_image               against  decode_blocks on host-built descriptors of the same image
  the parser alone (size query)  fast path, and the walk (FOURMC_IMAGE_PARSE=walk)
Prints one JSON line; median of --reps after one warm-up call of each.
    python tools/image_time.py [--blocks 2048] [--reps 5]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402


def timed(fn, reps):
    out = []
    for i in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    p.gpu_init(0)
    B, nb = p.BLOCKSIZE, a.blocks
    base = helpers.corpus(48 * B)
    d_src = torch.from_numpy(base).cuda().repeat(nb // 48 + 1)[:nb * B].contiguous()
    d_img = torch.empty(p.image_bound(nb * B), dtype=torch.uint8, device="cuda")
    res = {"blocks": nb, "bytes": nb * B, "reps": a.reps}
    n = [0]

    def comp():
        n[0] = p.compress_image(d_src, d_img, p.MAGIC_4MC, 1)
    res["compress_image_ms"] = timed(comp, a.reps)
    # the blocks API: descriptors and offsets prepared beforehand, only the launches are timed
    offs = np.arange(nb, dtype=np.uint64) * B
    blocks = p.make_blocks(offs, offs, [B] * nb, [B] * nb)
    batch = p.DeviceBatch(blocks)
    d_stage = torch.empty(nb * B, dtype=torch.uint8, device="cuda")
    p.encode_blocks(d_src, d_stage, batch)
    enc = batch.download()
    d_off = torch.from_numpy(p.container.block_offsets(enc["result"]).astype(np.int64)).cuda()
    d_img2 = torch.empty_like(d_img)

    def blocks_api():
        p.encode_blocks(d_src, d_stage, batch)
        p.pack_image(d_stage, d_img2, batch, d_off)
    res["encode_blocks_plus_pack_ms"] = timed(blocks_api, a.reps)
    del d_stage, d_img2
    img_n = n[0]
    d_dst = torch.empty(nb * B, dtype=torch.uint8, device="cuda")
    res["decompress_image_ms"] = timed(lambda: p.decompress_image(d_img[:img_n], d_dst, p.MAGIC_4MC), a.reps)
    ioff = p.container.block_offsets(enc["result"])
    dblocks = p.make_blocks(ioff + 12, offs, enc["result"], [B] * nb, enc["xxh32"])
    dbatch = p.DeviceBatch(dblocks)
    res["decode_blocks_ms"] = timed(lambda: p.decode_blocks(d_img, d_dst, dbatch), a.reps)
    assert torch.equal(d_dst, d_src)
    res["parse_fast_ms"] = timed(lambda: p.decompress_image(d_img[:img_n], None, p.MAGIC_4MC), a.reps)
    os.environ["FOURMC_IMAGE_PARSE"] = "walk"
    try:
        res["parse_walk_ms"] = timed(lambda: p.decompress_image(d_img[:img_n], None, p.MAGIC_4MC), a.reps)
    finally:
        os.environ.pop("FOURMC_IMAGE_PARSE", None)
    res = {k: ([round(x, 4) for x in v] if isinstance(v, tuple) else v) for k, v in res.items()}
    res["note"] = "[median, min, max] ms; parse_* = the size query (parse + one read-back of the summary)"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
