"""Times the decode of .zst streams (fourmc_gpu_zsts_decompress) on one GPU, hipEvents through torch.cuda.Event.
The streams are what ZstCodec writes - ZSTD_compressStream over log text, then ZSTD_endStream, level 1 - and are written here
with the reference's library (oracle/_ref/libref4mc.so), so the tool needs it.  Per shape k:bytes (default 256 streams of 4 MiB,
8 of 128 MiB, 1 of 1 GiB):
  zsts_decompress        one call over the k streams
  the size query         the same call with no destination: the walk, the entropy stage and two read-backs
  zstd_decompress        the baseline: fourmc_gpu_zstd_decompress with one descriptor per stream and the exact capacity - the only
                         device decode of such a file before this call existed (a frame of more than 64 blocks: one wavefront)
Every output is compared with the source.  Prints one JSON line; [median, min, max] ms over --reps after one warm-up call of each.
--cache DIR keeps the written streams; --write-only writes them and stops.  Under a profiler whose process has a zstd library of
its own loaded, write the streams first, in a run without it: the reference's library must not resolve its calls there.
    python tools/zst_batch.py [--shapes 256:4194304,8:134217728,1:1073741824] [--reps 3] [--level 1] [--no-baseline] [--cache DIR]
--encode times the write side instead (fourmc_gpu_zsts_compress): per shape, level (--levels, default 1,3) and text (log text, the
S-mix text of the corpus generator) one call over the k streams, [median, min, max] ms over --reps after --warmup calls; every
image is decoded back on the device and compared with its source, and - where oracle/_ref is built - stream 0 is compared with the
reference's bytes and the time zst_model.zstcodec takes for that one stream on one host core is printed next to the device's.
    python tools/zst_batch.py --encode [--shapes ...] [--levels 1,3] [--reps 3] [--warmup 1] [--texts logs,mix]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
import zst_model as zm  # noqa: E402

TEXT = 128 << 20                # distinct log text; longer sources repeat it (beyond every window of level 1)


def timed(fn, reps, warmup=1):
    out = []
    for i in range(reps + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append(a.elapsed_time(b))
    return [round(x, 3) for x in (statistics.median(out), min(out), max(out))]


def shape(p, text, k, each, level, reps, baseline, cache):
    distinct = max(1, min(k, TEXT // each))
    srcs = [np.resize(text[(j * each) % TEXT:], each) if each > TEXT else text[j * each:(j + 1) * each] for j in range(distinct)]
    imgs = []
    for j, s in enumerate(srcs):
        path = os.path.join(cache, f"zst_l{level}_{each}_{j}.zst") if cache else None
        if path and os.path.exists(path):
            imgs.append(open(path, "rb").read())
            continue
        imgs.append(zm.streamed(s, {zm.P_LEVEL: level}))
        if path:
            os.makedirs(cache, exist_ok=True)
            open(path, "wb").write(imgs[-1])
    if p is None:
        return None
    per = [(len(i) + 64 + 63) & ~63 for i in imgs]
    offs, at = [], 0
    for j in range(k):
        offs.append(at)
        at += per[j % distinct]
    h_images = np.zeros(at + 64, np.uint8)
    for j in range(k):
        h_images[offs[j]:offs[j] + len(imgs[j % distinct])] = np.frombuffer(imgs[j % distinct], np.uint8)
    d_images = torch.from_numpy(h_images).cuda()
    d_src = torch.from_numpy(np.concatenate([srcs[j % distinct] for j in range(k)])).cuda()
    items = [(offs[j], len(imgs[j % distinct]), j * each, each) for j in range(k)]
    d_dst = torch.zeros(k * each + 64, dtype=torch.uint8, device="cuda")
    res = {"streams": k, "stream_bytes": each, "compressed_bytes": sum(len(imgs[j % distinct]) for j in range(k))}
    got = []

    def batch():
        got[:] = p.decompress_zsts(d_images, items, d_dst)
        assert all(s["reason"] == 0 and s["decoded_bytes"] == each for s in got), got[0]
    p.zst_stats()
    res["zsts_decompress_ms"] = timed(batch, reps)
    res["blocks"] = sum(s["blocks"] for s in got)
    res["stats_per_call"] = {n: v // (reps + 1) for n, v in p.zst_stats().items()}
    assert torch.equal(d_dst[:k * each], d_src)
    res["size_query_ms"] = timed(lambda: p.decompress_zsts(d_images, items, None), reps)
    res["GBps_out"] = round(k * each / res["zsts_decompress_ms"][0] / 1e6, 3)
    if baseline:
        d_dst.zero_()
        blocks = p.make_blocks([o for o, _, _, _ in items], [d for _, _, d, _ in items], [n for _, n, _, _ in items], [each] * k)
        b = p.DeviceBatch(blocks)

        def serial():
            p.zstd_decompress(d_images, d_dst, b)
        res["zstd_decompress_ms"] = timed(serial, reps)
        assert list(b.download()["result"]) == [each] * k
        assert torch.equal(d_dst[:k * each], d_src)
        res["baseline_over_new"] = round(res["zstd_decompress_ms"][0] / res["zsts_decompress_ms"][0], 2)
    return res


def encode_shape(p, text, k, each, level, reps, warmup):
    """One compress_zsts call over k streams of `each` bytes of `text`."""
    import time
    distinct = max(1, min(k, TEXT // each))
    srcs = [np.resize(text[(j * each) % TEXT:], each) if each > TEXT else text[j * each:(j + 1) * each] for j in range(distinct)]
    d_src = torch.from_numpy(np.concatenate([srcs[j % distinct] for j in range(k)] + [np.zeros(64, np.uint8)])).cuda()
    bound = p.zst_bound(each)
    per = (bound + 64 + 63) & ~63
    items = [(j * each, each, j * per, bound, level) for j in range(k)]
    d_img = torch.zeros(k * per + 64, dtype=torch.uint8, device="cuda")
    got = []

    def batch():
        got[:] = p.compress_zsts(d_src, items, d_img)
        assert all(s["reason"] == 0 for s in got), got[0]
    res = {"streams": k, "stream_bytes": each, "level": level, "zsts_compress_ms": timed(batch, reps, warmup)}
    res["image_bytes"] = sum(s["image_bytes"] for s in got)
    res["GBps_in"] = round(k * each / res["zsts_compress_ms"][0] / 1e6, 3)
    d_back = torch.zeros(k * each + 64, dtype=torch.uint8, device="cuda")
    back = p.decompress_zsts(d_img, [(j * per, got[j]["image_bytes"], j * each, each) for j in range(k)], d_back)
    assert all(b["reason"] == 0 and b["decoded_bytes"] == each for b in back), back[0]
    assert torch.equal(d_back[:k * each], d_src[:k * each])
    if helpers.ref() is not None:
        t = time.perf_counter()
        want = zm.zstcodec(srcs[0], level)
        res["host_one_stream_ms"] = round((time.perf_counter() - t) * 1e3, 3)
        res["stream0_equals_reference"] = d_img[:got[0]["image_bytes"]].cpu().numpy().tobytes() == want
    return res


def main_encode(a):
    p = importlib.import_module("4mc_amd")
    out = {"arch": p.gpu_init(0), "reps": a.reps, "warmup": a.warmup, "note": "[median, min, max] ms", "shapes": []}
    for name in a.texts.split(","):
        text = helpers.corpus(TEXT, logs=name == "logs")
        for s in a.shapes.split(","):
            k, each = (int(v) for v in s.split(":"))
            for level in (int(v) for v in a.levels.split(",")):
                r = encode_shape(p, text, k, each, level, a.reps, a.warmup)
                r["text"] = name
                out["shapes"].append(r)
                print(json.dumps(r), flush=True)
                torch.cuda.empty_cache()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encode", action="store_true", help="time fourmc_gpu_zsts_compress instead of the decode")
    ap.add_argument("--levels", default="1,3")
    ap.add_argument("--texts", default="logs,mix")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="256:4194304,8:134217728,1:1073741824")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--cache", metavar="DIR", help="keep the written streams in DIR and read them from there when they exist")
    ap.add_argument("--write-only", action="store_true", help="with --cache: write the streams and stop (no device is touched)")
    a = ap.parse_args()
    if a.encode:
        return main_encode(a)
    assert helpers.ref() is not None, "the streams are written with oracle/_ref/libref4mc.so"
    if a.write_only:
        text = helpers.corpus(TEXT, logs=True)
        for s in a.shapes.split(","):
            k, each = (int(v) for v in s.split(":"))
            shape(None, text, k, each, a.level, 0, False, a.cache)
        return
    p = importlib.import_module("4mc_amd")
    out = {"arch": p.gpu_init(0), "reps": a.reps, "level": a.level, "round_blocks": p.lib().fourmc_gpu_get_zst_round_blocks(),
           "note": "[median, min, max] ms", "shapes": []}
    text = helpers.corpus(TEXT, logs=True)
    for s in a.shapes.split(","):
        k, each = (int(v) for v in s.split(":"))
        out["shapes"].append(shape(p, text, k, each, a.level, a.reps, not a.no_baseline, a.cache))
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
