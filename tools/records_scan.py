"""Times the line-record read of a device image on one GPU (hipEvents through torch.cuda.Event; image_time.timed), S-mix text
(48 distinct blocks, replicated), delimiter 10:
  (a) the delimiter scan and compaction alone (count - finish - write over bytes already decoded, through the research build's
      fourmc_gpu_debug_records_scan), and its count-only form, against a device-to-device copy of the same bytes.  The copy moves
      2 N bytes (N read, N written); the scan reads the data twice and writes 8 bytes per record, so the ratio its traffic predicts
      is (2 N + 8 R) / 2 N, printed as "expected_ratio" next to the measured one;
  (b) image_read_records over a whole-image split against image_decode_blocks of the same blocks (4mc level 1): the difference is
      what the records cost on top of the decode.
  (c) next to (a), on the same buffer and in the same alternation: the line-end scan of image_read_lines (Hadoop's default rule:
      LF, lone CR, CR LF; fourmc_gpu_debug_lines_scan), full and count-only.  It reads the data twice as well and writes 8 + 4 = 12
      bytes per line; the length pass then reads those 12 (a start counted once: its second reader is the neighbouring thread)
      and writes 4, 16 bytes per line.  28 in all: "lines_expected_ratio" is (2 N + 28 R) / 2 N.  --text chooses the buffer:
      lf (the corpus as it is), crlf (the byte before every LF becomes CR) or none (no CR and no LF at all); --scan-only
      skips (b).
The two sides of each pair alternate, --reps times each after a warm-up.  Prints one JSON line; [median, min, max] ms.
    python tools/records_scan.py [--blocks 2048] [--reps 5] [--text lf|crlf|none] [--scan-only]"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
from image_time import timed  # noqa: E402


def alternate(fns, reps):
    """{name: [median, min, max] ms}; one timed call of each in turn, reps times"""
    got = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            got[k].append(timed(fn, 1)[0])
    return {k: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--text", choices=("lf", "crlf", "none"), default="lf")
    ap.add_argument("--scan-only", action="store_true")
    a = ap.parse_args()
    p = importlib.import_module("4mc_amd")
    L = p.use_research()
    p.gpu_init(0)
    B, nb = p.BLOCKSIZE, a.blocks
    N = nb * B
    base = helpers.corpus(48 * B)
    base[base == 13] = 32
    if a.text == "crlf":
        at = (base == 10).nonzero()[0]
        base[at[at > 0] - 1] = 13
    elif a.text == "none":
        base[base == 10] = 32
    d = torch.from_numpy(base).cuda().repeat(nb // 48 + 1)[:N].contiguous()
    res = {"blocks": nb, "bytes": N, "reps": a.reps, "text": a.text}
    # (a) the scan alone
    n = C.c_int64(0)

    def scan(starts):
        ptr, cap = (starts.data_ptr(), starts.numel()) if starts is not None else (None, 0)
        assert L.fourmc_gpu_debug_records_scan(d.data_ptr(), N, 10, ptr, cap, C.byref(n), None) == 0
    nl = C.c_int64(0)

    def lines(starts, text_len):
        ptrs = (starts.data_ptr(), text_len.data_ptr(), starts.numel()) if starts is not None else (None, None, 0)
        assert L.fourmc_gpu_debug_lines_scan(d.data_ptr(), N, 0x7FFFFFFF, *ptrs, C.byref(nl), None) == 0
    scan(None)
    lines(None, None)
    R, RL = int(n.value), int(nl.value)
    d_starts = torch.empty(R + 1, dtype=torch.int64, device="cuda")
    d_lstarts = torch.empty(RL + 1, dtype=torch.int64, device="cuda")
    d_len = torch.empty(RL + 1, dtype=torch.int32, device="cuda")
    d_copy = torch.empty_like(d)
    res["records"], res["lines"] = R, RL
    res["mean_record_bytes"] = round(N / max(R, 1), 2)
    res.update(alternate({"scan_ms": lambda: scan(d_starts), "count_only_ms": lambda: scan(None),
                          "lines_scan_ms": lambda: lines(d_lstarts, d_len), "lines_count_only_ms": lambda: lines(None, None),
                          "d2d_copy_ms": lambda: d_copy.copy_(d)}, a.reps))
    assert n.value == R and nl.value == RL
    head = d[:min(64 * B, N - 1) + 1]
    want = torch.nonzero(head[:-1] == 10).flatten() + 1                   # the first 64 blocks' starts against torch
    assert d_starts[0] == 0 and torch.equal(d_starts[1:1 + len(want)], want)
    ends = (head[:-1] == 10) | ((head[:-1] == 13) & (head[1:] != 10))     # ... and the lines' starts and lengths
    lwant = torch.nonzero(ends).flatten() + 1
    assert d_lstarts[0] == 0 and torch.equal(d_lstarts[1:1 + len(lwant)], lwant)
    if len(lwant):
        first = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), lwant[:-1]])
        term = 1 + ((head[lwant - 1] == 10) & (lwant - first >= 2) & (head[torch.clamp(lwant - 2, min=0)] == 13)).to(torch.int64)
        assert torch.equal(d_len[:len(lwant)].to(torch.int64), lwant - first - term)
    res["lines_expected_ratio"] = round((2 * N + 28 * RL) / (2 * N), 4)
    res["lines_scan_over_copy"] = round(res["lines_scan_ms"][0] / res["d2d_copy_ms"][0], 4)
    res["lines_scan_GBps_of_input"] = round(N / res["lines_scan_ms"][0] / 1e6, 1)
    res["lines_count_only_GBps_of_input"] = round(N / res["lines_count_only_ms"][0] / 1e6, 1)
    res["count_only_GBps_of_input"] = round(N / res["count_only_ms"][0] / 1e6, 1)
    del d_lstarts, d_len
    res["expected_ratio"] = round((2 * N + 8 * R) / (2 * N), 4)
    res["scan_over_copy"] = round(res["scan_ms"][0] / res["d2d_copy_ms"][0], 4)
    res["scan_GBps_of_input"] = round(N / res["scan_ms"][0] / 1e6, 1)
    res["copy_GBps_moved"] = round(2 * N / res["d2d_copy_ms"][0] / 1e6, 1)
    del d_copy
    if a.scan_only:
        res["note"] = "[median, min, max] ms; every call includes its own stream synchronization"
        print(json.dumps(res))
        return
    # (b) on top of the decode
    d_img = torch.empty(p.image_bound(N), dtype=torch.uint8, device="cuda")
    k = p.compress_image(d, d_img, p.MAGIC_4MC, 1)
    d_img = d_img[:k]
    d_dst = torch.empty(N, dtype=torch.uint8, device="cuda")
    out = [None, None]

    def records():
        out[0] = p.image_read_records(d_img, 0, k, d_dst, d_starts)

    def blocks():
        out[1] = p.image_decode_blocks(d_img, 0, nb, d_dst)
    res.update(alternate({"image_read_records_ms": records, "image_decode_blocks_ms": blocks}, a.reps))
    assert out[0].result == R and out[0].data_bytes == N and out[1] == N and torch.equal(d_dst, d)
    res["records_minus_decode_ms"] = round(res["image_read_records_ms"][0] - res["image_decode_blocks_ms"][0], 4)
    res["note"] = "[median, min, max] ms; every call includes its own stream synchronizations"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
