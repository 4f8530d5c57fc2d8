"""Times the decode of Hadoop block streams (fourmc_gpu_bstream_*) on one GPU, hipEvents through torch.cuda.Event.
Case 1, --streams k (default 256) streams of ONE group of --stream-bytes each (default M, the most one chunk holds), written by
compress_bstream with the LZ4 fast codec (or --zstd: level 1) into one device buffer:
  decompress_bstreams            one call over the k streams
  a loop of decompress_bstream   the same streams one after another (two synchronizations and a one-chunk launch each)
  decompress_images              the same payloads as k .4mc (.4mz) images of one block each: what the footer index costs against the walk
  the size query                 decompress_bstreams with no destination: the walk and its read-back alone
Case 2, one stream of --big-bytes (default 1 GiB) in groups of M: the walk alone (the size query of decompress_bstream: one lane
chases two dependent reads per group) against the whole decode.
--encode times the writers instead:
Case 1, the same k sources as streams of one write() each: one compress_bstreams call against a loop of k compress_bstream calls
(one synchronization and a one-chunk launch each); the bytes of both are compared.
Case 2, one stream of --big-bytes with a device table of --write-bytes per write() (default 64: 16 Mi entries for 1 GiB): the plan
alone (the size query: tile sums, their prefixes, the chase and its read-back) against the whole call, which runs the chase once
more for the group table; the stream is decoded back and compared with the source.
Every output is compared with the source.  Prints one JSON line; [median, min, max] ms over --reps after one warm-up call of each.
    python tools/bstream_batch.py [--encode] [--streams 256] [--stream-bytes N] [--big-bytes N] [--write-bytes 64] [--reps 5] [--zstd]"""
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


def many(p, base, k, each, codec, level, reps):
    total = k * each
    d_src = base.repeat(total // base.numel() + 1)[:total].contiguous()
    per = (p.bstream_bound(each, codec, 0) + 63) & ~63
    d_streams = torch.zeros(k * per + 4096, dtype=torch.uint8, device="cuda")
    lens = [p.compress_bstream(d_src[j * each:(j + 1) * each], d_streams[j * per:(j + 1) * per], codec, level) for j in range(k)]
    items = [(j * per, lens[j], j * each, each) for j in range(k)]
    d_dst = torch.empty(total, dtype=torch.uint8, device="cuda")
    res = {"streams": k, "stream_bytes": each, "compressed_bytes": sum(lens)}

    def batch():
        st = p.decompress_bstreams(d_streams, items, d_dst, codec)
        assert all(s["reason"] == 0 and s["decoded_bytes"] == each for s in st)
    res["batched_ms"] = timed(batch, reps)
    assert torch.equal(d_dst, d_src)
    d_dst.zero_()

    def loop():
        for j in range(k):
            st = p.decompress_bstream(d_streams[j * per:j * per + lens[j]], d_dst[j * each:(j + 1) * each], codec)
            assert st["reason"] == 0
    res["loop_of_single_calls_ms"] = timed(loop, reps)
    assert torch.equal(d_dst, d_src)
    res["size_query_ms"] = timed(lambda: p.decompress_bstreams(d_streams, items, None, codec), reps)
    del d_streams
    # the same payloads behind a footer index
    magic = p.MAGIC_4MZ if codec == p.CODEC_ZSTD else p.MAGIC_4MC
    iper = (p.image_bound(each) + 63) & ~63
    d_images = torch.zeros(k * iper + 4096, dtype=torch.uint8, device="cuda")
    ilens = p.compress_images(d_src, [(j * each, each, j * iper, iper) for j in range(k)], d_images, magic, 1)
    iitems = [(j * iper, ilens[j], j * each, each) for j in range(k)]
    d_dst.zero_()

    def images():
        st = p.decompress_images(d_images, iitems, d_dst, magic)
        assert all(s["reason"] == 0 for s in st)
    res["decompress_images_ms"] = timed(images, reps)
    assert torch.equal(d_dst, d_src)
    res["loop_over_batched"] = round(res["loop_of_single_calls_ms"][0] / res["batched_ms"][0], 2)
    res["batched_minus_images_ms"] = round(res["batched_ms"][0] - res["decompress_images_ms"][0], 4)
    return res


def one_big(p, base, n, codec, level, reps):
    d_src = base.repeat(n // base.numel() + 1)[:n].contiguous()
    d_stream = torch.zeros(p.bstream_bound(n, codec, 0) + 4096, dtype=torch.uint8, device="cuda")
    ln = p.compress_bstream(d_src, d_stream, codec, level)
    d_dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    res = {"stream_bytes": n, "compressed_bytes": ln}
    q = p.decompress_bstream(d_stream, None, codec, image_bytes=ln)
    res["groups"] = q["groups"]
    res["walk_alone_ms"] = timed(lambda: p.decompress_bstream(d_stream, None, codec, image_bytes=ln), reps)

    def decode():
        st = p.decompress_bstream(d_stream, d_dst, codec, image_bytes=ln)
        assert st["reason"] == 0 and st["decoded_bytes"] == n
    res["decode_ms"] = timed(decode, reps)
    assert torch.equal(d_dst, d_src)
    res["walk_share_of_decode"] = round(2 * res["walk_alone_ms"][0] / res["decode_ms"][0], 4)      # the decode walks twice
    return res


def many_encode(p, base, k, each, codec, level, reps):
    total = k * each
    d_src = base.repeat(total // base.numel() + 1)[:total].contiguous()
    per = (p.bstream_bound(each, codec, 0) + 63) & ~63
    d_one, d_loop = (torch.zeros(k * per + 4096, dtype=torch.uint8, device="cuda") for _ in range(2))
    items = [(j * each, each, j * per, per, 0, 0, 0) for j in range(k)]
    res = {"streams": k, "stream_bytes": each}
    got = []

    def batch():
        got[:] = p.compress_bstreams(d_src, items, d_one, codec, level)
        assert all(st["reason"] == 0 for st in got)
    res["one_call_ms"] = timed(batch, reps)
    lens = [0] * k

    def loop():
        for j in range(k):
            lens[j] = p.compress_bstream(d_src[j * each:(j + 1) * each], d_loop[j * per:(j + 1) * per], codec, level)
    res["loop_of_single_calls_ms"] = timed(loop, reps)
    assert lens == [st["image_bytes"] for st in got]
    for j in range(k):
        assert torch.equal(d_one[j * per:j * per + lens[j]], d_loop[j * per:j * per + lens[j]]), j
    res["compressed_bytes"] = sum(lens)
    res["size_query_ms"] = timed(lambda: p.compress_bstreams(d_src, items, None, codec, level), reps)
    res["loop_over_one_call"] = round(res["loop_of_single_calls_ms"][0] / res["one_call_ms"][0], 2)
    return res


def one_big_encode(p, base, n, w, codec, level, reps):
    d_src = base.repeat(n // base.numel() + 1)[:n].contiguous()
    nw = -(-n // w)
    d_writes = torch.full((nw,), w, dtype=torch.int32, device="cuda")
    if n % w:
        d_writes[-1] = n % w
    cap = p.bstream_writes_bound(n, codec)
    d_stream = torch.zeros(cap + 4096, dtype=torch.uint8, device="cuda")
    item = [(0, n, 0, cap, 0, nw, 0)]
    q = p.compress_bstreams(d_src, item, None, codec, level, d_writes=d_writes)[0]
    res = {"stream_bytes": n, "write_bytes": w, "writes": nw, "groups": q["groups"], "chunks": q["chunks"]}
    res["plan_alone_ms"] = timed(lambda: p.compress_bstreams(d_src, item, None, codec, level, d_writes=d_writes), reps)
    got = []

    def encode():
        got[:] = p.compress_bstreams(d_src, item, d_stream, codec, level, d_writes=d_writes, images_bytes=cap)
        assert got[0]["reason"] == 0
    res["encode_ms"] = timed(encode, reps)
    res["compressed_bytes"] = got[0]["image_bytes"]
    d_dst = torch.empty(n, dtype=torch.uint8, device="cuda")
    st = p.decompress_bstream(d_stream, d_dst, codec, image_bytes=got[0]["image_bytes"])
    assert st["reason"] == 0 and st["groups"] == q["groups"] and torch.equal(d_dst, d_src)
    res["plan_share_of_encode"] = round(res["plan_alone_ms"][0] / res["encode_ms"][0], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--stream-bytes", type=int, default=0, help="0: M, the most one chunk holds")
    ap.add_argument("--big-bytes", type=int, default=1 << 30, help="0: skip the one big stream")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--zstd", action="store_true")
    ap.add_argument("--encode", action="store_true", help="time the writers (compress_bstreams) instead of the readers")
    ap.add_argument("--write-bytes", type=int, default=64, help="--encode: the write() size of the one big stream's table")
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    arch = p.gpu_init(0)
    codec, level = (p.CODEC_ZSTD, 1) if a.zstd else (p.CODEC_LZ4_FAST, 0)
    base = torch.from_numpy(helpers.corpus(48 * p.BLOCKSIZE)).cuda()
    out = {"arch": arch, "reps": a.reps, "codec": "zstd 1" if a.zstd else "lz4 fast", "note": "[median, min, max] ms"}
    if a.encode:
        if a.streams:
            out["many_streams_encode"] = many_encode(p, base, a.streams, a.stream_bytes or p.bstream_max_input(codec), codec, level, a.reps)
        if a.big_bytes:
            out["one_stream_encode"] = one_big_encode(p, base, a.big_bytes, a.write_bytes, codec, level, a.reps)
        print(json.dumps(out))
        return
    if a.streams:
        out["many_streams"] = many(p, base, a.streams, a.stream_bytes or p.bstream_max_input(codec), codec, level, a.reps)
    if a.big_bytes:
        out["one_stream"] = one_big(p, base, a.big_bytes, codec, level, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
