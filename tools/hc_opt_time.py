#!/usr/bin/env python3
"""LZ4 HC levels 9..12 (lz4hc_opt_encode.hip): device time of one container-mode encode launch over N blocks of the S-mix
(HIP events; replicas of 48 distinct 4 MiB blocks), its bytes checked against the reference on the distinct blocks it covers
(at most `--check`), and, with --cpu, the reference's own LZ4_compress_HC rate on this host's cores for the same blocks.
   python tools/hc_opt_time.py LEVEL BLOCKS [--check K] [--cpu] [--out results.jsonl]"""
import argparse
import importlib
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("level", type=int)
ap.add_argument("blocks", type=int)
ap.add_argument("--check", type=int, default=4)
ap.add_argument("--cpu", action="store_true")
ap.add_argument("--out")
a = ap.parse_args()
B = helpers.B
ndist = min(48, a.blocks)
base = helpers.corpus(ndist * B)
ref = helpers.ref()
rec = {"level": a.level, "blocks": a.blocks}

if a.cpu:
    # the reference on every host core: ctypes drops the GIL for the call, one thread per core
    def one(b):
        s = np.ascontiguousarray(base[b * B:(b + 1) * B]); d = np.empty(B + B // 255 + 16, np.uint8)
        return ref.LZ4_compress_HC(s.ctypes.data, d.ctypes.data, B, B - 1, a.level)
    cores = os.cpu_count()
    t0 = time.time()
    with ThreadPoolExecutor(cores) as ex:
        list(ex.map(one, range(ndist)))
    dt = time.time() - t0
    rec.update({"cpu_cores": cores, "cpu_blocks": ndist, "cpu_s": round(dt, 3), "cpu_MBps": round(ndist * B / dt / 1e6, 2)})
else:
    import torch
    p = importlib.import_module("4mc_amd"); p.gpu_init(0)
    nb = a.blocks
    d_src = torch.from_numpy(base).cuda().repeat(-(-nb // ndist))[: nb * B].contiguous()
    offs = np.arange(nb, dtype=np.uint64) * B; lens = np.full(nb, B, dtype=np.uint32)
    st = torch.empty(nb * B, dtype=torch.uint8, device="cuda")
    warm = p.DeviceBatch(p.make_blocks([0], [0], [4096], [4096]))              # engine and workspace set-up outside the timing
    p.encode_blocks(d_src, st, warm, codec=p.CODEC_LZ4_HC, level=a.level); torch.cuda.synchronize()
    enc = p.DeviceBatch(p.make_blocks(offs, offs, lens, lens))
    s = torch.cuda.Event(enable_timing=True); t = torch.cuda.Event(enable_timing=True)
    s.record(); p.encode_blocks(d_src, st, enc, codec=p.CODEC_LZ4_HC, level=a.level); t.record(); torch.cuda.synchronize()
    ms = s.elapsed_time(t)
    res = enc.download()["result"].astype(np.int64)
    ok = True
    for b in range(min(a.check, ndist)):
        src = np.ascontiguousarray(base[b * B:(b + 1) * B]); d = np.empty(B + 64, np.uint8)
        r = ref.LZ4_compress_HC(src.ctypes.data, d.ctypes.data, B, B - 1, a.level)
        want = d[:r] if r > 0 else src
        got = st[b * B: b * B + int(res[b])].cpu().numpy()
        ok &= int(res[b]) == len(want) and np.array_equal(got, want)
    rec.update({"device_ms": round(ms, 1), "GBps": round(nb * B / ms / 1e6, 4),
                "ratio": round(nb * B / float(res.sum()), 4), "checked": min(a.check, ndist), "bytes_equal_reference": bool(ok)})
print(json.dumps(rec), flush=True)
if a.out:
    with open(a.out, "a") as f:
        f.write(json.dumps(rec) + "\n")
