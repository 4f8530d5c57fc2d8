#!/usr/bin/env python3
"""Pins the schedule of the lane-level model (tools/model/lz4_fast_model.c) to the kernel's (4mc_amd/csrc/lz4_encode.hip).  Equal bytes do
not prove that the model's windows are the kernel's; the K2_PROF side build counts window events for blocks of exactly 4 MiB:
    make -C 4mc_amd/csrc prof      # -> 4mc_amd/lib/libhadoop-4mc-prof.so
    FOURMC_LIB=4mc_amd/lib/libhadoop-4mc-prof.so python tools/k2_sched_check.py [table.md]
Blocks: the inputs of tests/lz4_enc_shapes.py packed into 4 MiB blocks and padded with corpus text so that the result stays below
B - 256 (the counters lie behind the payload), at source alignments 0 and 5, and the twelve S-mix classes of tools/k2_phases.py.  Each
block runs once; its counters are compared with the model's for the same block and alignment.  Cycle counters are ignored.  The
catalogue inputs cannot be checked one by one - the counters exist for 4 MiB blocks alone - and an assembled block parses differently
from its parts (the table carries over, and the 32-bit table is used throughout).  Not a pytest: run once, its table goes to DESIGN_NOTES.md."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
import lz4_enc_shapes as ls  # noqa: E402

B = 4 << 20
NAMES = ["text", "binary", "pcm6", "sdf", "binary", "db", "text", "code", "pcm11", "dict", "xml", "random"]     # tools/k2_phases.py
# K2_PROF's counters (lz4_encode.hip:741) and the model's (ls.COUNTERS): name -> (array, index); d = dst + n - 128, f = dst + n - 192, g = dst + n - 256
WHERE = {"nwin": ("d", 4), "nseq": ("d", 5), "nslow": ("d", 6), "none": ("f", 0), "cross": ("f", 1), "dcut": ("f", 2), "scut": ("f", 3), "nit": ("f", 6),
         "nrel": ("g", 0), "nrot": ("g", 1), "nrst": ("g", 2)}


def assembled():
    """(name, block): catalogue inputs of at most 1 MiB + 1 in their order, some 2.5 MiB per block, then corpus text up to 4 MiB"""
    text = helpers.corpus(B, first_block=6)
    out, parts, size, names = [], [], 0, []

    def close():
        nonlocal parts, size, names
        if parts:
            out.append((f"catalogue[{names[0]} .. {names[-1]}]", np.concatenate(parts + [text[:B - size]])))
        parts, size, names = [], 0, []
    for c in ls.cases():
        if not len(c.data) or len(c.data) > (1 << 20) + 1: continue
        if size + len(c.data) > 5 * B // 8: close()
        parts.append(c.data); size += len(c.data); names.append(c.name)
    close()
    out.append(("catalogue[n4m]", ls.by_name()["n4m"].data))
    return out


def kernel_counters(p, block, align):
    buf = np.zeros(B + 32, np.uint8)
    buf[align:align + B] = block
    src = torch.from_numpy(buf).cuda()
    assert src.data_ptr() % 16 == 0
    enc = p.DeviceBatch(p.make_blocks([align], [0], [B], [B]))
    stage = torch.zeros(B, dtype=torch.uint8, device="cuda")
    p.encode_blocks(src, stage, enc)
    torch.cuda.synchronize()
    r = int(enc.download()["result"][0])
    if r >= B - 256: return r, None
    arr = {"d": stage[B - 128:B - 72].cpu().numpy().view(np.uint64), "f": stage[B - 192:B - 136].cpu().numpy().view(np.uint64),
           "g": stage[B - 256:B - 224].cpu().numpy().view(np.uint64)}
    return r, {k: int(arr[a][i]) for k, (a, i) in WHERE.items()}


def main():
    p = importlib.import_module("4mc_amd"); p.gpu_init(0)
    assert "prof" in os.path.basename(p.lib_path()), "load the K2_PROF side build with FOURMC_LIB"
    data = helpers.corpus(12 * B)
    blocks = [(name, blk, a) for name, blk in assembled() for a in (0, 5)]
    blocks += [(f"S-mix {b}: {NAMES[b]}", data[b * B:(b + 1) * B], 0) for b in range(12)]
    lines = ["| block | align | result | " + " | ".join(ls.COUNTERS) + " | equal |", "|---|---|---|" + "---|" * (len(ls.COUNTERS) + 1)]
    differ = 0
    for name, blk, a in blocks:
        assert len(blk) == B
        r, k = kernel_counters(p, blk, a)
        mt = ls.model_trace(blk, cap=B - 1, align=a)
        want_r = mt.result if mt.result > 0 else B
        if k is None:
            lines.append(f"| {name} | {a} | {r} (model {want_r}) | " + " | ".join("-" for _ in ls.COUNTERS) + " | no counters: the result reaches B - 256 |")
            continue
        cells = [f"{k[c]}" if k[c] == mt.counters[c] else f"**{k[c]} / {mt.counters[c]}**" for c in ls.COUNTERS]
        same = all(k[c] == mt.counters[c] for c in ls.COUNTERS) and r == want_r
        differ += not same
        lines.append(f"| {name} | {a} | {r}" + ("" if r == want_r else f" / **{want_r}**") + " | " + " | ".join(cells) + f" | {'yes' if same else 'NO'} |")
    lines.append("")
    lines.append(f"{len(blocks)} blocks, {differ} with a counter that differs (kernel / model where they do)")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
