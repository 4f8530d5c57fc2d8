"""Inputs for the LZ4 HC level 9..12 tests (tests/test_gpu_hc_opt.py on the device, tests/test_lz4hc_opt_model_cpu.py on the
CPU model): shapes that reach each branch the level 1..8 encoder never takes."""
import numpy as np

import helpers
from helpers import B

U8 = np.uint8


def shapes():
    """inputs that reach each branch the levels 1..8 kernel never takes"""
    rng = np.random.default_rng(2024)
    text = helpers.corpus(B, first_block=3)
    rnd = lambda k: rng.integers(0, 256, k, dtype=U8)
    out = {}
    for n in (0, 1, 12, 13, 14, 64, 4095, 65535, 65536, 65547, 300000):
        out["size%d" % n] = text[:n].copy()
    # pattern analysis (:339-409): one-byte runs, at the first position (the lowestMatchIndex clamp of the backward count) and
    # between literals; two-byte periods (refused by :345-346, they take the plain chain)
    out["run_at_start"] = np.concatenate([np.full(9000, 0x61, U8), rnd(3000), np.full(700, 0x61, U8), rnd(500)])
    parts = []
    for ln in (5, 9, 17, 40, 300, 2000, 70000, 6):
        parts += [rnd(int(rng.integers(3, 60))), np.full(ln, int(rng.integers(0, 4)), U8)]
    out["runs_mixed"] = np.concatenate(parts + [rnd(40)])
    out["period2"] = np.tile(np.array([7, 9], U8), 30000)
    out["period2_in_text"] = np.concatenate([text[:20000], np.tile(np.array([0x20, 0x2D], U8), 5000), text[40000:60000],
                                             np.tile(np.array([0x20, 0x2D], U8), 777), rnd(100)])
    # chain swap (:317-338): repetitive text, many equal-length candidates
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=U8)) for _ in range(24)]
    out["repetitive_text"] = np.frombuffer(b" ".join(words[i] for i in rng.integers(0, 24, 30000)), U8)[:150000].copy()
    # sufficient_len (64 / 128 / 4095) and the opt table's edge: matches longer than 64, 128, 4095
    for ln in (70, 130, 5000):
        a = rnd(ln)
        out["long%d" % ln] = np.concatenate([rnd(300), a, rnd(200), a, rnd(50), a[: ln // 2], rnd(30)])
    # len + cur >= LZ4_OPT_NUM (:1456): a first match of 200, then at cur = 18 (where the price steps) one of 4082
    s = rnd(200); y = rnd(3900)
    out["opt_num_edge"] = np.concatenate([s, rnd(300), s[18:], y, rnd(300), s, y, rnd(100)])
    # a repeat at distance exactly 65535 (reachable) and 65536 (not)
    for dist in (65535, 65536):
        a = rnd(100)
        out["dist%d" % dist] = np.concatenate([rnd(50), a, rnd(dist - 100), a, rnd(400)])
    for k, v in helpers.edge_inputs().items():
        out["edge_" + k] = v
    return out
