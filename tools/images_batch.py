"""Times the decode of many images with one call against one call per image (hipEvents through torch.cuda.Event), on one GPU.
For every shape k x b: k .4mc images of b S-mix blocks each (48 distinct blocks, replicated), packed into one device buffer, and
  decompress_images              one call over the k images
  a loop of decompress_image     the same images one after another (two synchronizations and one under-filled launch each)
  one image of k * b blocks      decompress_image on the same data as a single image: what the batch can at best cost
  the size query of the batch    decompress_images with no destination
Every output is compared with the source.  Prints one JSON line; median of --reps after one warm-up call of each.
    python tools/images_batch.py [--shapes 8x4,64x4,128x16,512x4] [--reps 5]"""
import argparse
import importlib
import json
import os
import statistics
import sys

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
    return [round(x, 4) for x in (statistics.median(out), min(out), max(out))]


def one_shape(p, base, k, b, reps):
    B = p.BLOCKSIZE
    nb = k * b
    d_src = base.repeat(nb // 48 + 1)[:nb * B].contiguous()
    per = (p.image_bound(b * B) + 63) & ~63
    d_images = torch.zeros(k * per + 4096, dtype=torch.uint8, device="cuda")
    lens = [p.compress_image(d_src[j * b * B:(j + 1) * b * B], d_images[j * per:(j + 1) * per], p.MAGIC_4MC, 1) for j in range(k)]
    items = [(j * per, lens[j], j * b * B, b * B) for j in range(k)]
    d_dst = torch.empty(nb * B, dtype=torch.uint8, device="cuda")
    res = {"images": k, "blocks_per_image": b, "blocks": nb, "image_bytes": sum(lens)}

    def batch():
        st = p.decompress_images(d_images, items, d_dst, p.MAGIC_4MC)
        assert all(s["reason"] == 0 and s["decoded_bytes"] == b * B for s in st)
    res["batched_ms"] = timed(batch, reps)
    assert torch.equal(d_dst, d_src)
    d_dst.zero_()

    def loop():
        for j in range(k):
            st = p.decompress_image(d_images[j * per:j * per + lens[j]], d_dst[j * b * B:(j + 1) * b * B], p.MAGIC_4MC)
            assert st["reason"] == 0
    res["loop_of_single_calls_ms"] = timed(loop, reps)
    assert torch.equal(d_dst, d_src)
    res["size_query_ms"] = timed(lambda: p.decompress_images(d_images, items, None, p.MAGIC_4MC), reps)
    del d_images
    d_one = torch.empty(p.image_bound(nb * B) + 4096, dtype=torch.uint8, device="cuda")
    n = p.compress_image(d_src, d_one, p.MAGIC_4MC, 1)
    d_dst.zero_()
    res["one_image_ms"] = timed(lambda: p.decompress_image(d_one[:n], d_dst, p.MAGIC_4MC), reps)
    assert torch.equal(d_dst, d_src)
    res["loop_over_batched"] = round(res["loop_of_single_calls_ms"][0] / res["batched_ms"][0], 2)
    res["batched_minus_one_image_ms"] = round(res["batched_ms"][0] - res["one_image_ms"][0], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x16", help="comma-separated k x b: images x blocks per image")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    arch = p.gpu_init(0)
    base = torch.from_numpy(helpers.corpus(48 * p.BLOCKSIZE)).cuda()
    shapes = [tuple(int(v) for v in s.lower().split("x")) for s in a.shapes.split(",")]
    out = {"arch": arch, "reps": a.reps, "note": "[median, min, max] ms", "shapes": [one_shape(p, base, k, b, a.reps) for k, b in shapes]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
