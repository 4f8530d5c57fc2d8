"""Times compress_images_writes (fourmc_gpu_images_compress_writes: .4mc / .4mz images cut as Hadoop's FourMcOutputStream cuts them)
on one GPU, hipEvents through torch.cuda.Event, for .4mc level 1 (or --zstd: .4mz level 1).
Case 1, --streams k (default 256) streams of ONE write() of 4 MiB each: one compress_images_writes call against one compress_images
call on the same sources, the two alternating.  Both run the same codec launches over the same blocks (the raw call into the bound here, the container
call into u - 1 bytes there), so the difference is the plan, its read-back and the seal; the bytes of both are compared.
Case 2, one stream of --big-bytes (default 1 GiB) with a device table of --write-bytes per write() (default 64: 16 Mi entries): the
plan alone (the size query: tile sums, their prefixes, the chase and its read-back) against the whole call, which runs the chase
once more for the group table; the image is decoded back and compared with the source.
Prints one JSON line; [median, min, max] ms over --reps (at least 5) after one warm-up call of each, and the spread (max - min) / median.
    python tools/images_writes.py [--streams 256] [--big-bytes N] [--write-bytes 64] [--reps 7] [--zstd]"""
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


def spread(t):
    return round((t[2] - t[1]) / t[0], 4)


def many(p, base, k, each, magic, reps):
    total = k * each
    d_src = base.repeat(total // base.numel() + 1)[:total].contiguous()
    per = (max(p.image_bound(each), p.image_writes_bound(each)) + 63) & ~63
    d_w, d_i = (torch.zeros(k * per + 4096, dtype=torch.uint8, device="cuda") for _ in range(2))
    res = {"streams": k, "stream_bytes": each}
    got, lens = [], []

    def writes():
        got[:] = p.compress_images_writes(d_src, [(j * each, each, j * per, per, 0, 0, 0) for j in range(k)], d_w, magic, 1)
        assert all(st["reason"] == 0 for st in got)

    def images():
        lens[:] = p.compress_images(d_src, [(j * each, each, j * per, per) for j in range(k)], d_i, magic, 1)
    # alternating, so that a drift of the clocks and other people's work on the host fall on both
    tw, ti = [], []
    for r in range(reps + 1):
        for fn, out in ((writes, tw), (images, ti)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r:
                out.append(a.elapsed_time(b))
    res["compress_images_writes_ms"] = [round(x, 4) for x in (statistics.median(tw), min(tw), max(tw))]
    res["compress_images_ms"] = [round(x, 4) for x in (statistics.median(ti), min(ti), max(ti))]
    res["per_rep_writes_minus_images_ms"] = [round(x - y, 4) for x, y in zip(tw, ti)]
    same = all(got[j]["image_bytes"] == lens[j] and torch.equal(d_w[j * per:j * per + lens[j]], d_i[j * per:j * per + lens[j]]) for j in range(k))
    res["same_bytes_as_compress_images"] = same
    res["compressed_bytes"] = sum(st["image_bytes"] for st in got)
    res["stored_blocks"] = sum(st["stored_blocks"] for st in got)
    res["size_query_ms"] = timed(lambda: p.compress_images_writes(d_src, [(j * each, each, 0, 0, 0, 0, 0) for j in range(k)], None, magic, 1), reps)
    res["writes_minus_images_ms"] = round(res["compress_images_writes_ms"][0] - res["compress_images_ms"][0], 4)
    res["spread"] = {"writes": spread(res["compress_images_writes_ms"]), "images": spread(res["compress_images_ms"])}
    d_dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    back = p.decompress_images(d_w, [(j * per, got[j]["image_bytes"], j * each, each) for j in range(k)], d_dst, magic)
    assert all(b["exit_code"] == 0 for b in back) and torch.equal(d_dst, d_src)
    return res


def one_big(p, base, n, w, magic, reps):
    d_src = base.repeat(n // base.numel() + 1)[:n].contiguous()
    nw = -(-n // w)
    d_writes = torch.full((nw,), w, dtype=torch.int32, device="cuda")
    if n % w:
        d_writes[-1] = n % w
    cap = p.image_writes_bound(n)
    d_image = torch.zeros(cap + 4096, dtype=torch.uint8, device="cuda")
    item = [(0, n, 0, cap, 0, nw, 0)]
    q = p.compress_images_writes(d_src, item, None, magic, 1, d_writes=d_writes)[0]
    res = {"stream_bytes": n, "write_bytes": w, "writes": nw, "blocks": q["blocks"]}
    res["plan_alone_ms"] = timed(lambda: p.compress_images_writes(d_src, item, None, magic, 1, d_writes=d_writes), reps)
    got = []

    def encode():
        got[:] = p.compress_images_writes(d_src, item, d_image, magic, 1, d_writes=d_writes, images_bytes=cap)
        assert got[0]["reason"] == 0
    res["encode_ms"] = timed(encode, reps)
    res["compressed_bytes"] = got[0]["image_bytes"]
    d_dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    st = p.decompress_image(d_image, d_dst, magic, image_bytes=got[0]["image_bytes"])
    assert st["exit_code"] == 0 and st["blocks"] == q["blocks"] and torch.equal(d_dst, d_src)
    res["plan_share_of_encode"] = round(res["plan_alone_ms"][0] / res["encode_ms"][0], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--big-bytes", type=int, default=1 << 30, help="0: skip the one big stream")
    ap.add_argument("--write-bytes", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--zstd", action="store_true")
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    arch = p.gpu_init(0)
    magic = p.MAGIC_4MZ if a.zstd else p.MAGIC_4MC
    base = torch.from_numpy(helpers.corpus(48 * p.BLOCKSIZE)).cuda()
    out = {"arch": arch, "reps": max(a.reps, 5), "format": ".4mz level 1" if a.zstd else ".4mc level 1", "note": "[median, min, max] ms"}
    if a.streams:
        out["many_streams"] = many(p, base, a.streams, p.BLOCKSIZE, magic, max(a.reps, 5))
    if a.big_bytes:
        out["one_stream"] = one_big(p, base, a.big_bytes, a.write_bytes, magic, max(a.reps, 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
