"""Times the decode of many images with one call against one call per image (hipEvents through torch.cuda.Event), on one GPU.
For every shape k x b: k .4mc images of b S-mix blocks each (48 distinct blocks, replicated), packed into one device buffer, and
  decompress_images              one call over the k images
  a loop of decompress_image     the same images one after another (two synchronizations and one under-filled launch each)
  one image of k * b blocks      decompress_image on the same data as a single image: what the batch can at best cost
  the size query of the batch    decompress_images with no destination
Every output is compared with the source.  Prints one JSON line; median of --reps after one warm-up call of each.
    python tools/images_batch.py [--shapes 8x4,64x4,128x16,512x4] [--reps 5]
--encode times the other direction, .4mc level 1, for the same shapes, then for one image of 2048 blocks and for 4096 sources of
8 KiB (the case the batch's tight staging is for):
  compress_images                one call over the k sources
  a loop of compress_image       the same sources one after another (one synchronization and one under-filled launch each)
  one image of k * b blocks      compress_image on the same data as a single image
The two contenders alternate within every repeat, after one warm-up of each; [median, min, max] over the repeats.  Every image of
the batch is compared with the loop's.
    python tools/images_batch.py --encode [--shapes 8x4,64x4,128x16,512x4,1x2048,4096x8k] [--reps 5]"""
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


def _time_once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def alternated(fns, reps):
    """{name: [median, min, max] ms}: one warm-up of each, then `reps` rounds in which each runs once, in turn"""
    for fn in fns.values():
        fn()
    out = {name: [] for name in fns}
    for r in range(reps):
        for name, fn in fns.items():
            out[name].append(_time_once(fn))
        print("  repeat %d: %s" % (r + 1, {name: round(v[-1], 2) for name, v in out.items()}), file=sys.stderr, flush=True)
    return {name: [round(x, 4) for x in (statistics.median(v), min(v), max(v))] for name, v in out.items()}


def encode_shape(p, base, k, src_each, reps, one_image=True):
    """k sources of src_each bytes, back to back in one buffer"""
    B = p.BLOCKSIZE
    total = k * src_each
    d_src = base.repeat(total // base.numel() + 1)[:total].contiguous()
    per = (p.image_bound(src_each) + 63) & ~63
    d_batch = torch.zeros(k * per + 4096, dtype=torch.uint8, device="cuda")
    d_loop = torch.zeros(k * per + 4096, dtype=torch.uint8, device="cuda")
    items = [(j * src_each, src_each, j * per, per) for j in range(k)]
    got = {}

    def batch():
        got["batch"] = p.compress_images(d_src, items, d_batch, p.MAGIC_4MC, 1)

    def loop():
        got["loop"] = [p.compress_image(d_src[j * src_each:(j + 1) * src_each], d_loop[j * per:(j + 1) * per], p.MAGIC_4MC, 1) for j in range(k)]
    fns = {"batched_ms": batch, "loop_of_single_calls_ms": loop}
    if one_image and k > 1:
        d_one = torch.empty(p.image_bound(total), dtype=torch.uint8, device="cuda")
        fns["one_image_ms"] = lambda: p.compress_image(d_src, d_one, p.MAGIC_4MC, 1)
    res = {"images": k, "source_bytes_each": src_each, "blocks": k * ((src_each + B - 1) // B)}
    res.update(alternated(fns, reps))
    assert got["batch"] == got["loop"]
    for j in range(0, k, max(1, k // 64)):                # the images themselves: up to 64 of them, spread over the batch
        assert torch.equal(d_batch[j * per:j * per + got["batch"][j]], d_loop[j * per:j * per + got["loop"][j]]), j
    res["image_bytes"] = sum(got["batch"])
    res["loop_over_batched"] = round(res["loop_of_single_calls_ms"][0] / res["batched_ms"][0], 2)
    return res


def parse_shape(s, B):
    """k x b: b blocks of 4 MiB per source; a trailing k (8k) means KiB instead"""
    k, b = s.lower().split("x")
    return int(k), int(b[:-1]) * 1024 if b.endswith("k") else int(b) * B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x16", help="comma-separated k x b: images x blocks per image")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--encode", action="store_true", help="time compress_images against the loop of compress_image")
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    arch = p.gpu_init(0)
    base = torch.from_numpy(helpers.corpus(48 * p.BLOCKSIZE)).cuda()
    if a.encode:
        shapes = a.shapes if a.shapes != ap.get_default("shapes") else "8x4,64x4,128x16,512x4,1x2048,4096x8k"
        rows = [encode_shape(p, base, *parse_shape(s, p.BLOCKSIZE), a.reps) for s in shapes.split(",")]
        print(json.dumps({"arch": arch, "reps": a.reps, "direction": "encode, .4mc level 1", "note": "[median, min, max] ms, alternated", "shapes": rows}))
        return
    shapes = [tuple(int(v) for v in s.lower().split("x")) for s in a.shapes.split(",")]
    out = {"arch": arch, "reps": a.reps, "note": "[median, min, max] ms", "shapes": [one_shape(p, base, k, b, a.reps) for k, b in shapes]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
