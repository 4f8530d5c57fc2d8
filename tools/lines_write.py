"""Times write_lines_images (fourmc_gpu_images_write_lines: text lines as the .4mc / .4mz part files of a TextOutputFormat job) on one
GPU, hipEvents through torch.cuda.Event, for .4mc level 1 (or --zstd: .4mz level 1), on log text from the corpus generator cut into
lines at its LFs.  Two shapes: --items k (default 256) items that share --bytes (default 1 GiB) of text, and one item of all of it.
Three variants, alternating rep by rep so that drift and other people's work on the host fall on all of them:
  (a) write_lines_images on the lines (starts and text lengths, as image_read_lines leaves them);
  (b) compress_images_writes on the same text already packed, with the same write table: the floor; (a) - (b) is what the pack costs;
  (c) the pack composed from torch ops (cumsum, repeat_interleave, an index copy, a scatter of the newlines) followed by (b): what a
      caller writes without this call.
pack_lines alone is timed too.  The images of (a), (b) and (c) are compared byte for byte.  Device memory: what each of (a) and (c)
holds at its end beyond the inputs and outputs (torch.cuda.mem_get_info before and after, caches emptied before: the engine's
workspaces and torch's cached blocks stay allocated, so the difference is the variant's peak).
Prints one JSON line; [median, min, max] ms over --reps (at least 5) after one warm-up call of each.
    python tools/lines_write.py [--bytes N] [--items 256] [--reps 7] [--zstd]"""
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


def lines_of(text):
    """(text cut behind its last LF, starts, text_len) of the lines of a uint8 CUDA tensor"""
    ends = (text == 10).nonzero().reshape(-1)
    text = text[:int(ends[-1]) + 1].contiguous()
    starts = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), ends[:-1] + 1])
    return text, starts.contiguous(), (ends - starts).to(torch.int32).contiguous()


def torch_pack(text, starts, text_len):
    """the packed text and the write table of ALL lines from torch ops"""
    lens = text_len.to(torch.int64)
    piece = lens + 1
    end = torch.cumsum(piece, 0)
    off = end - piece
    line = torch.repeat_interleave(torch.arange(lens.numel(), device="cuda"), piece)
    idx = starts[line] + (torch.arange(int(end[-1]), device="cuda") - off[line])
    packed = text[idx.clamp_(max=text.numel() - 1)]
    packed[end - 1] = 10
    writes = torch.stack([text_len, torch.ones_like(text_len)], 1).reshape(-1).contiguous()
    return packed, writes


def used(fn):
    """bytes of device memory fn leaves allocated (engine workspaces, torch's cached blocks): its peak beyond what was there"""
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    fn()
    torch.cuda.synchronize()
    return free0 - torch.cuda.mem_get_info()[0]


def shape(p, text, starts, text_len, k, magic, reps):
    n, T = text_len.numel(), text.numel()
    cuts = [n * j // k for j in range(k + 1)]
    first = [int(v) for v in starts[torch.tensor(cuts[:-1], device="cuda")]] + [T]
    src = p.LinesSource(text, text_len, starts=starts)
    items = [(cuts[j], cuts[j + 1] - cuts[j], 0, 0) for j in range(k)]
    q = p.write_lines_images(src, items, None, magic, 1)
    assert [s["text_bytes"] for s in q] == [first[j + 1] - first[j] for j in range(k)]
    at, regions = 0, []
    for s in q:
        regions.append((at, s["image_bytes"]))
        at += (s["image_bytes"] + 63) & ~63
    d_a, d_b, d_c = (torch.zeros(at + 4096, dtype=torch.uint8, device="cuda") for _ in range(3))
    rows_a = [(cuts[j], cuts[j + 1] - cuts[j], regions[j][0], regions[j][1]) for j in range(k)]
    # the text already packed: the lines are the text's own, in order, so it is the text itself; pack_lines says so
    d_packed = torch.zeros(T + 64, dtype=torch.uint8, device="cuda")
    d_writes = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    rows_p = [(cuts[j], cuts[j + 1] - cuts[j], first[j], first[j + 1] - first[j], 2 * cuts[j]) for j in range(k)]
    rows_b = [(first[j], first[j + 1] - first[j], regions[j][0], regions[j][1], 2 * cuts[j], 2 * (cuts[j + 1] - cuts[j]), 0) for j in range(k)]
    got = {}

    def a():
        got["a"] = p.write_lines_images(src, rows_a, d_a, magic, 1)

    def pack():
        got["p"] = p.pack_lines(src, rows_p, d_packed, d_writes)

    def b():
        got["b"] = p.compress_images_writes(d_packed, rows_b, d_b, magic, 1, d_writes=d_writes)

    def c():
        packed, writes = torch_pack(text, starts, text_len)
        got["c"] = p.compress_images_writes(packed, rows_b, d_c, magic, 1, d_writes=writes)

    p.release_workspaces(); torch.cuda.empty_cache()
    mem_a = used(a)
    p.release_workspaces(); torch.cuda.empty_cache()
    pack()
    b()
    mem_c = used(c)
    torch.cuda.synchronize()
    assert all(s["reason"] == 0 for s in got["a"] + got["p"] + got["b"] + got["c"])
    assert torch.equal(d_packed[:T], text), "the packed text is not the text"
    same = all(got["a"][j]["image_bytes"] == got["b"][j]["image_bytes"] == got["c"][j]["image_bytes"] for j in range(k))
    same = same and torch.equal(d_a, d_b) and torch.equal(d_a, d_c)
    times = {"a": [], "pack": [], "b": [], "c": []}
    for r in range(reps):
        for name, fn in (("a", a), ("pack", pack), ("b", b), ("c", c)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    med = {name: [round(x, 4) for x in (statistics.median(t), min(t), max(t))] for name, t in times.items()}
    cost = med["a"][0] - med["b"][0]
    return {"items": k, "lines": n, "text_bytes": T, "image_bytes": sum(s["image_bytes"] for s in got["a"]), "blocks": sum(s["blocks"] for s in got["a"]),
            "same_bytes_a_b_c": bool(same),
            "a_write_lines_images_ms": med["a"], "b_compress_images_writes_prepacked_ms": med["b"], "c_torch_pack_then_b_ms": med["c"],
            "pack_lines_alone_ms": med["pack"], "a_minus_b_ms": round(cost, 4), "pack_share_of_b": round(cost / med["b"][0], 4),
            "pack_GBps_from_a_minus_b": round(T / cost / 1e6, 2) if cost > 0 else None, "pack_GBps_alone": round(T / med["pack"][0] / 1e6, 2),
            "per_rep_a_minus_b_ms": [round(x - y, 4) for x, y in zip(times["a"], times["b"])],
            "device_memory_a_bytes": mem_a, "device_memory_c_bytes": mem_c}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--items", type=int, default=256, help="0: skip the many-items shape")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--zstd", action="store_true")
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    arch = p.gpu_init(0)
    magic = p.MAGIC_4MZ if a.zstd else p.MAGIC_4MC
    base = torch.from_numpy(helpers.corpus(min(a.bytes, 48 * p.BLOCKSIZE), logs=True)).cuda()
    text, starts, text_len = lines_of(base.repeat(a.bytes // base.numel() + 1)[:a.bytes].contiguous())
    out = {"arch": arch, "reps": max(a.reps, 5), "format": ".4mz level 1" if a.zstd else ".4mc level 1", "note": "[median, min, max] ms"}
    if a.items:
        out["many_items"] = shape(p, text, starts, text_len, a.items, magic, max(a.reps, 5))
    out["one_item"] = shape(p, text, starts, text_len, 1, magic, max(a.reps, 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
