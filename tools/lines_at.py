"""Times lines by number (image_line_index + image_read_lines_at) against the only other way to the same rows: image_read_lines(0,
size) over the whole image plus a torch gather from the decoded copy and its two tables.  One GPU, hipEvents through
torch.cuda.Event around each call.  The image: --blocks (256, 1 GiB) blocks of log text, compressed on the device with
compress_image.  The index build is timed once (after one warm-up build).  Then for each request count of --counts, with random line
numbers (duplicates allowed) and rows of --row-bytes:
  lines_at        image_read_lines_at with the index
  read_all+gather image_read_lines(0, size) into a buffer of the decoded size, then rows = dst[starts[k] + j] where j < text_len[k]
run in turn within every repeat, after one warm-up of each; [median, min, max] ms over --reps (>= 10) repeats.  The rows and lengths of
the two are compared.  Memory: the device memory each way holds while it runs beyond the image itself (torch.cuda.mem_get_info
before and after, the engine's workspaces released in between), so the engine's staging counts.  Prints one JSON line.
    python tools/lines_at.py [--blocks 256] [--counts 16,256,4096,65536] [--row-bytes 256] [--reps 10] [--zstd]"""
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


def held(p, fn):
    """device bytes in use after fn() beyond what was in use before it, the engine's workspaces and torch's cache emptied first;
    whatever fn returns is dropped before the next measurement"""
    p.release_workspaces()
    torch.cuda.empty_cache()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    keep = fn()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    del keep
    return free0 - free1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=256)
    ap.add_argument("--counts", default="16,256,4096,65536", help="comma-separated request counts")
    ap.add_argument("--row-bytes", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--zstd", action="store_true", help="a .4mz image instead of .4mc")
    a = ap.parse_args()
    assert a.reps >= 10, "the median of at least 10 repetitions"
    p = importlib.import_module("4mc_amd")
    arch = p.gpu_init(0)
    B = p.BLOCKSIZE
    magic = p.MAGIC_4MZ if a.zstd else p.MAGIC_4MC
    base = torch.from_numpy(helpers.corpus(min(a.blocks, 16) * B, logs=True)).cuda()
    d_src = base.repeat(a.blocks // 16 + 1)[:a.blocks * B].contiguous()
    total = d_src.numel()
    d_img = torch.zeros(p.image_bound(total) + 4096, dtype=torch.uint8, device="cuda")
    size = p.compress_image(d_src, d_img, magic, 1)
    del d_src, base
    torch.cuda.empty_cache()

    index, info = p.image_line_index(d_img, image_bytes=size)                 # warm-up: code objects, workspaces
    assert info["result"] == 0 and info["nblocks"] == a.blocks, info
    lines = info["lines"]
    index_ms = _time_once(lambda: p.image_line_index(d_img, image_bytes=size))
    index_held = held(p, lambda: p.image_line_index(d_img, image_bytes=size))
    row_bytes = a.row_bytes
    col = torch.arange(row_bytes, device="cuda")[None, :]

    def read_all(ks):
        d_dst = torch.empty(total, dtype=torch.uint8, device="cuda")
        d_st = torch.empty(lines + 1, dtype=torch.int64, device="cuda")
        d_tl = torch.empty(lines, dtype=torch.int32, device="cuda")
        r = p.image_read_lines(d_img, 0, size, d_dst, d_st, d_tl, image_bytes=size)
        assert r.result == lines
        tl = d_tl[ks]
        at = torch.clamp(d_st[ks][:, None] + col, max=total - 1)
        rows = torch.where(col < tl[:, None], d_dst[at], torch.zeros((), dtype=torch.uint8, device="cuda"))
        return rows, tl, (d_dst, d_st, d_tl)

    shapes = []
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    for n in [int(v) for v in a.counts.split(",")]:
        ks = torch.randint(0, lines, (n,), generator=gen, device="cuda", dtype=torch.int64)
        got = {}

        def new():
            got["new"] = p.image_read_lines_at(d_img, index, ks, row_bytes, image_bytes=size)

        def old():
            got["old"] = read_all(ks)[:2]
        res = {"requests": n}
        res.update(alternated({"lines_at_ms": new, "read_all_gather_ms": old}, a.reps))
        assert got["new"]["out"]["result"] == n
        assert torch.equal(got["new"]["rows"], got["old"][0]) and torch.equal(got["new"]["text_len"], got["old"][1])
        res["blocks_staged"], res["rounds"] = got["new"]["out"]["blocks_staged"], got["new"]["out"]["rounds"]
        got.clear()
        res["lines_at_held_bytes"] = held(p, lambda: p.image_read_lines_at(d_img, index, ks, row_bytes, image_bytes=size))
        res["read_all_gather_held_bytes"] = held(p, lambda: read_all(ks))
        res["read_all_over_lines_at"] = round(res["read_all_gather_ms"][0] / res["lines_at_ms"][0], 2)
        shapes.append(res)
    print(json.dumps({"arch": arch, "format": "4mz" if a.zstd else "4mc", "blocks": a.blocks, "image_bytes": size, "content_bytes": total,
                      "lines": lines, "row_bytes": row_bytes, "reps": a.reps, "index_build_ms": round(index_ms, 3),
                      "index_build_held_bytes": index_held, "index_bytes": index.numel() * 8,
                      "note": "[median, min, max] ms, alternated; held: device bytes in use after the call beyond the image", "shapes": shapes}))


if __name__ == "__main__":
    main()
