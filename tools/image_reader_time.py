"""Times the streaming image reader on one GPU (hipEvents through torch.cuda.Event): the .4mc (level 1) and .4mz (level 1) images
of 2048 S-mix blocks (48 distinct, replicated; 8 GiB of content), each fed in chunks of 4 MiB + 1 byte, 64 MiB and 1 GiB, at
batch_blocks 64 and 512, against one decompress_image of the same image.  Each timed run is one hipEvent pair around the appends
and finish on the current stream; begin (which allocates) is outside it.  Every run's status must equal decompress_image's and
its output the input.  Prints one JSON line; [median, min, max] ms of --reps after one warm-up run of each.
    python tools/image_reader_time.py [--blocks 2048] [--reps 3] [--only 4mc:64MiB:512]
--only runs one case (one warm-up, one run) and the whole-image decode of that image: the shape for a kernel trace, from which
the walk's share is the image_rd_walk_kernel time over the run's total (rocprofv3 --kernel-trace --stats)."""
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

CHUNKS = {"4MiB+1": 4 * 1024 * 1024 + 1, "64MiB": 64 << 20, "1GiB": 1 << 30}


def timed_reader(p, d_img, m, d_dst, magic, chunk, batch, reps):
    """begin outside the events; the appends and finish inside"""
    out, st = [], None
    for i in range(reps + 1):
        r = p.ImageReader(d_dst, magic, batch)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for at in range(0, m, chunk):
            r.append(d_img[at:min(m, at + chunk)])
        st = r.finish()
        b.record()
        torch.cuda.synchronize()
        if i:
            out.append(a.elapsed_time(b))
    return (statistics.median(out), min(out), max(out)), st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None, help="fmt:chunk:batch, e.g. 4mc:64MiB:512")
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    p.gpu_init(0)
    B, nb = p.BLOCKSIZE, a.blocks
    base = helpers.corpus(48 * B)
    d_src = torch.from_numpy(base).cuda().repeat(nb // 48 + 1)[:nb * B].contiguous()
    total = nb * B
    d_dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    only = a.only.split(":") if a.only else None
    res = {"blocks": nb, "bytes": total, "reps": a.reps}
    for fmt, magic in (("4mc", p.MAGIC_4MC), ("4mz", p.MAGIC_4MZ)):
        if only and only[0] != fmt:
            continue
        d_img = torch.empty(p.image_bound(total), dtype=torch.uint8, device="cuda")
        m = p.compress_image(d_src, d_img, magic, 1)
        p.release_workspaces()
        want = [None]

        def whole():
            want[0] = p.decompress_image(d_img, d_dst, magic, image_bytes=m)
        reps = 1 if only else a.reps
        res[f"{fmt}_image_bytes"] = m
        res[f"{fmt}_decompress_image_ms"] = timed(whole, reps)
        assert want[0]["reason"] == 0 and torch.equal(d_dst, d_src), fmt
        for cname, chunk in CHUNKS.items():
            for batch in (64, 512):
                if only and (only[1] != cname or int(only[2]) != batch):
                    continue
                d_dst.zero_()
                t, st = timed_reader(p, d_img, m, d_dst, magic, chunk, batch, reps)
                assert st == want[0] and torch.equal(d_dst, d_src), (fmt, cname, batch, st)
                res[f"{fmt}_reader_{cname}_batch_{batch}_ms"] = t
        del d_img
        p.release_workspaces()
    res = {k: ([round(x, 3) for x in v] if isinstance(v, tuple) else v) for k, v in res.items()}
    res["note"] = "[median, min, max] ms; begin outside the timed span; the append read-backs and finish's synchronization inside"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
