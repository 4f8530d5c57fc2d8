"""Times the lines of every one-block split of every image of a dataset with ONE call (images_read_lines) against the loop of
image_read_lines_batch per image, on one GPU (hipEvents through torch.cuda.Event).  The dataset: --images (64,512,4096) images of
--per (1,4) blocks of log text each, in one device buffer, image i at an offset of residue 0 mod 64.  16 distinct images are
compressed on the device with compress_image and the dataset repeats them.  Every image is cut into its one-block splits, every
split gets a region of its own in one destination and one pair of tables, and
  images_read_lines                     one call over all the splits of all the images
  a loop of image_read_lines_batch      one call per image over that image's splits, into the same regions
run in turn within every repeat, after one warm-up of each; [median, min, max] ms over the repeats.  The loop's results, starts and
text lengths are compared with the one call's.  Prints one JSON line.
    python tools/lines_dataset.py [--images 64,512,4096] [--per 1,4] [--reps 5] [--zstd | --mixed]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import helpers  # noqa: E402
from lines_batch import alternated  # noqa: E402

DISTINCT = 16


def distinct_images(p, per, block_bytes, fmt):
    """DISTINCT images of `per` blocks each -> [(device bytes, [header offsets])]; fmt: "4mc", "4mz" or "mixed" (alternating)"""
    n = per * block_bytes
    out = []
    text = torch.from_numpy(helpers.corpus(DISTINCT * block_bytes + n, logs=True)).cuda()
    for k in range(DISTINCT):
        d_src = text[k * block_bytes:k * block_bytes + n].contiguous()
        d_img = torch.zeros(p.image_bound(n) + 64, dtype=torch.uint8, device="cuda")
        z = fmt == "4mz" or (fmt == "mixed" and k % 2 == 1)
        size = p.compress_image(d_src, d_img, p.MAGIC_4MZ if z else p.MAGIC_4MC, 1)
        _, ent = p.image_index(d_img, image_bytes=size)
        out.append((d_img[:size].clone(), [int(v) for v in ent["image_off"]]))
    return out


def one_shape(p, nimages, per, block_bytes, fmt, reps):
    kinds = distinct_images(p, per, block_bytes, fmt)
    refs, off = [], 0
    for i in range(nimages):
        size = kinds[i % DISTINCT][0].numel()
        refs.append((off, size))
        off = (off + size + 63) & ~63
    d_images = torch.zeros(off + 64, dtype=torch.uint8, device="cuda")
    for i, (o, size) in enumerate(refs):
        d_images[o:o + size] = kinds[i % DISTINCT][0]
    splits = []                                             # (image, split_start, split_end): every block alone
    for i, (o, size) in enumerate(refs):
        heads = kinds[i % DISTINCT][1]
        edges = [0] + heads[1:] + [size]
        splits += [(i, a, z) for a, z in zip(edges, edges[1:])]
    need = [r["data_bytes"] for r in p.images_read_lines(d_images, refs, [(i, a, z, 0, 0, 0, 0) for i, a, z in splits], d_images[:1])]
    offs = [0]
    for v in need:
        offs.append((offs[-1] + v + 63) & ~63)
    d_dst = torch.empty(offs[-1] + 64, dtype=torch.uint8, device="cuda")
    lines = [r["result"] for r in p.images_read_lines(d_images, refs, [(i, a, z, offs[j], need[j], 0, 0) for j, (i, a, z) in enumerate(splits)],
                                                      d_dst)]
    assert min(lines) >= 0, min(lines)
    toff = [0]
    for v in lines:
        toff.append(toff[-1] + v + 1)
    d_st = [torch.zeros(toff[-1], dtype=torch.int64, device="cuda") for _ in range(2)]
    d_tl = [torch.zeros(toff[-1], dtype=torch.int32, device="cuda") for _ in range(2)]
    items = [(i, a, z, offs[j], need[j], toff[j], lines[j] + 1) for j, (i, a, z) in enumerate(splits)]
    by_image = [[] for _ in refs]
    for it in items:
        by_image[it[0]].append(it[1:])
    views = [d_images[o:] for o, _ in refs]
    got = {}

    def one_call():
        got["one"] = [r["result"] for r in p.images_read_lines(d_images, refs, items, d_dst, d_st[0], d_tl[0])]

    def loop():
        out = []
        for k, (o, size) in enumerate(refs):
            out += [r["result"] for r in p.image_read_lines_batch(views[k], by_image[k], d_dst, d_st[1], d_tl[1], image_bytes=size)]
        got["loop"] = out
    s0 = p.images_lines_stats()
    res = {"images": nimages, "blocks_per_image": per, "splits": len(splits), "lines": sum(lines), "content_bytes": sum(need),
           "images_bytes": off}
    res.update(alternated({"one_call_ms": one_call, "loop_of_one_image_calls_ms": loop}, reps))
    s1 = p.images_lines_stats()
    assert got["one"] == got["loop"] == lines
    assert torch.equal(d_st[0], d_st[1]) and torch.equal(d_tl[0], d_tl[1])
    calls = reps + 1
    (res["groups_per_call"], res["tail_rounds_per_call"], res["block_decodes_per_call"],
     res["index_launches_per_call"]) = [(b - a) // calls for a, b in zip(s0, s1)]
    res["loop_over_one_call"] = round(res["loop_of_one_image_calls_ms"][0] / res["one_call_ms"][0], 2)
    del d_images, d_dst, d_st, d_tl, views
    p.release_workspaces()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", default="64,512,4096", help="comma-separated image counts")
    ap.add_argument("--per", default="1,4", help="comma-separated blocks per image")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--zstd", action="store_true", help=".4mz images instead of .4mc")
    ap.add_argument("--mixed", action="store_true", help=".4mc and .4mz images alternating")
    a = ap.parse_args()
    assert a.reps >= 5, "the median of at least 5 repetitions"
    p = importlib.import_module("4mc_amd")
    arch = p.gpu_init(0)
    fmt = "mixed" if a.mixed else "4mz" if a.zstd else "4mc"
    rows = []
    for n in a.images.split(","):
        for per in a.per.split(","):
            print("%s images of %s blocks" % (n, per), file=sys.stderr, flush=True)
            rows.append(one_shape(p, int(n), int(per), p.BLOCKSIZE, fmt, a.reps))
    print(json.dumps({"arch": arch, "format": fmt, "block_bytes": p.BLOCKSIZE, "reps": a.reps, "split_group": os.environ.get("FOURMC_SPLIT_GROUP", "256"),
                      "note": "[median, min, max] ms, alternated", "shapes": rows}))


if __name__ == "__main__":
    main()
