"""Times the lines of every split of one image with one call against one call per split (hipEvents through torch.cuda.Event), on
one GPU.  The image: --blocks (256) blocks of log text, compressed on the device with compress_image.  For 1, 4 and 16 blocks per
split the image is cut into its splits, every split gets a region of its own in one destination and one pair of tables, and
  image_read_lines_batch          one call over all the splits
  a loop of image_read_lines      the same splits one after another, into the same regions
run in turn within every repeat, after one warm-up of each; [median, min, max] ms over the repeats.  The loop's results, starts
and text lengths are compared with the batch's.  Prints one JSON line.
    python tools/lines_batch.py [--blocks 256] [--per 1,4,16] [--reps 5] [--zstd]"""
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


def one_shape(p, d_img, size, heads, per, reps):
    """the splits of `per` blocks each: [heads[i], heads[i + per]), the first from 0 and the last to the image's end"""
    n = len(heads)
    edges = [heads[i] for i in range(0, n, per)] + [size]
    edges[0] = 0
    splits = list(zip(edges, edges[1:]))
    k = len(splits)
    # the sizes: a size query, then a count into regions of exactly those sizes
    need = [r["data_bytes"] for r in p.image_read_lines_batch(d_img, [(s, e, 0, 0, 0, 0) for s, e in splits], d_img[:1], image_bytes=size)]
    off = [0]
    for v in need:
        off.append((off[-1] + v + 63) & ~63)
    d_dst = torch.empty(off[-1] + 64, dtype=torch.uint8, device="cuda")
    lines = [r["result"] for r in p.image_read_lines_batch(d_img, [(s, e, off[i], need[i], 0, 0) for i, (s, e) in enumerate(splits)], d_dst,
                                                           image_bytes=size)]
    assert min(lines) >= 0, lines
    toff = [0]
    for v in lines:
        toff.append(toff[-1] + v + 1)
    d_st = [torch.zeros(toff[-1], dtype=torch.int64, device="cuda") for _ in range(2)]
    d_tl = [torch.zeros(toff[-1], dtype=torch.int32, device="cuda") for _ in range(2)]
    items = [(s, e, off[i], need[i], toff[i], lines[i] + 1) for i, (s, e) in enumerate(splits)]
    got = {}

    def batch():
        got["batch"] = [r["result"] for r in p.image_read_lines_batch(d_img, items, d_dst, d_st[0], d_tl[0], image_bytes=size)]

    def loop():
        got["loop"] = [p.image_read_lines(d_img, s, e, d_dst[o:o + c], d_st[1][t:t + lc], d_tl[1][t:t + lc], image_bytes=size).result
                       for s, e, o, c, t, lc in items]
    g0 = p.image_lines_batch_stats()
    res = {"blocks_per_split": per, "splits": k, "lines": sum(lines), "content_bytes": sum(need)}
    res.update(alternated({"batched_ms": batch, "loop_of_single_calls_ms": loop}, reps))
    g1 = p.image_lines_batch_stats()
    assert got["batch"] == got["loop"] == lines
    assert torch.equal(d_st[0], d_st[1]) and torch.equal(d_tl[0], d_tl[1])
    calls = reps + 1
    res["groups_per_call"], res["tail_rounds_per_call"], res["block_decodes_per_call"] = [(b - a) // calls for a, b in zip(g0, g1)]
    res["loop_over_batched"] = round(res["loop_of_single_calls_ms"][0] / res["batched_ms"][0], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--per", default="1,4,16", help="comma-separated blocks per split")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--zstd", action="store_true", help="a .4mz image instead of .4mc")
    a = ap.parse_args()
    assert a.reps >= 5, "the median of at least 5 repetitions"
    p = importlib.import_module("4mc_amd")
    arch = p.gpu_init(0)
    B = p.BLOCKSIZE
    magic = p.MAGIC_4MZ if a.zstd else p.MAGIC_4MC
    base = torch.from_numpy(helpers.corpus(min(a.blocks, 16) * B, logs=True)).cuda()
    d_src = base.repeat(a.blocks // 16 + 1)[:a.blocks * B].contiguous()
    d_img = torch.zeros(p.image_bound(a.blocks * B) + 4096, dtype=torch.uint8, device="cuda")
    size = p.compress_image(d_src, d_img, magic, 1)
    del d_src, base
    _, ent = p.image_index(d_img, image_bytes=size)
    heads = [int(v) for v in ent["image_off"]]
    assert len(heads) == a.blocks
    rows = [one_shape(p, d_img, size, heads, int(per), a.reps) for per in a.per.split(",")]
    print(json.dumps({"arch": arch, "format": "4mz" if a.zstd else "4mc", "blocks": a.blocks, "image_bytes": size, "reps": a.reps,
                      "note": "[median, min, max] ms, alternated", "shapes": rows}))


if __name__ == "__main__":
    main()
