"""Times the streaming image writer on one GPU (hipEvents through torch.cuda.Event), 2048 S-mix blocks (48 distinct, replicated;
8 GiB), 4mc level 1:
  one append of everything + finish, batch_blocks = n        against  compress_image on the same input
  8 appends of exactly n/8 blocks, batch_blocks = n/8          against  one append of everything at batch_blocks = n/8
  8 appends of n/8 blocks + 4097 bytes (the last one shorter:  against  the row above
  every append leaves a carry), batch_blocks = n/8
  device memory taken by begin at batch_blocks = n/8           against  compress_image's staging for the same input
Each timed run is one hipEvent pair around the appends and finish on the current stream; begin (which allocates) is outside it.
Prints one JSON line; [median, min, max] ms of --reps after one warm-up run of each.
    python tools/image_writer_time.py [--blocks 2048] [--reps 5] [--only eight]
--only eight runs just the 8-append case (one warm-up, one run): the shape for a kernel / API trace."""
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
from image_time import timed  # noqa: E402


def timed_writer(p, d_img, batch, cuts_fn, reps):
    """begin outside the events; the appends and finish inside"""
    out, n = [], 0
    for i in range(reps + 1):
        w = p.ImageWriter(d_img, p.MAGIC_4MC, 1, batch)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for chunk in cuts_fn():
            w.append(chunk)
        n = w.finish()
        b.record()
        torch.cuda.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    return (statistics.median(out), min(out), max(out)), n


def pieces(d_src, sizes):
    at = 0
    for s in sizes:
        yield d_src[at:at + s]
        at += s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=["eight"], default=None)
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    p.gpu_init(0)
    B, nb = p.BLOCKSIZE, a.blocks
    base = helpers.corpus(48 * B)
    d_src = torch.from_numpy(base).cuda().repeat(nb // 48 + 1)[:nb * B].contiguous()
    total = nb * B
    d_img = torch.empty(p.image_bound(total), dtype=torch.uint8, device="cuda")
    eighth = nb // 8
    exact = [eighth * B] * 8
    if a.only == "eight":
        t, n = timed_writer(p, d_img, eighth, lambda: pieces(d_src, exact), 1)
        print(json.dumps({"case": "eight_appends", "ms": round(t[0], 4), "image_bytes": n}))
        return
    res = {"blocks": nb, "bytes": total, "reps": a.reps}
    # memory: compress_image's staging (kept per stream) and begin's one allocation, both as the device's free memory drops
    p.release_workspaces()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    want = p.compress_image(d_src, d_img, p.MAGIC_4MC, 1)
    torch.cuda.synchronize()
    res["compress_image_staging_bytes"] = free0 - torch.cuda.mem_get_info()[0]
    ref = d_img[:want].clone()
    n = [0]

    def comp():
        n[0] = p.compress_image(d_src, d_img, p.MAGIC_4MC, 1)
    res["compress_image_ms"] = timed(comp, a.reps)
    p.release_workspaces()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    w = p.ImageWriter(d_img, p.MAGIC_4MC, 1, eighth)
    torch.cuda.synchronize()
    res["writer_begin_bytes_batch_%d" % eighth] = free0 - torch.cuda.mem_get_info()[0]
    w.abort()

    def check(nbytes, what):
        assert nbytes == want and torch.equal(d_img[:want], ref), what
    res["writer_one_append_batch_%d_ms" % nb], m = timed_writer(p, d_img, nb, lambda: [d_src], a.reps)
    check(m, "one append, batch n")
    res["writer_one_append_batch_%d_ms" % eighth], m = timed_writer(p, d_img, eighth, lambda: [d_src], a.reps)
    check(m, "one append, batch n/8")
    res["writer_8_appends_exact_ms"], m = timed_writer(p, d_img, eighth, lambda: pieces(d_src, exact), a.reps)
    check(m, "8 exact appends")
    carry = [eighth * B + 4097] * 7
    carry.append(total - sum(carry))
    res["writer_8_appends_carry_ms"], m = timed_writer(p, d_img, eighth, lambda: pieces(d_src, carry), a.reps)
    check(m, "8 appends with a carry")
    res = {k: ([round(x, 4) for x in v] if isinstance(v, tuple) else v) for k, v in res.items()}
    res["note"] = "[median, min, max] ms; begin outside the timed span; finish's one synchronization inside"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
