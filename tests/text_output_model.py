"""The writer rule of the line writers (include/fourmc_gpu.h, "text lines written as the part files of a TextOutputFormat job"),
restated: Hadoop's TextOutputFormat.LineRecordWriter with a null key issues, for every record, out.write(text) and then
out.write(NEWLINE) on the codec's stream.  Written from knowledge of Hadoop's classes; no JVM wrote a fixture.

  schedule(texts)             lines -> (data, write sizes)
  verdict(...)                what the pack says of an item, from plain Python lists
  image / bstream             the expected part file: the schedule through tests/fourmc_stream_model.py's closed form, or through
                              tests/bstream_writes_model.py's plan and the block streams' framing
and the catalogue of cases the CPU and the GPU tests share."""
import numpy as np

import bstream_model as bm
import bstream_writes_model as wm
import fourmc_stream_model as fm
import helpers

OK, SUM, WRITE, CAP, LINE = range(5)
NEWLINE = b"\n"
M = fm.M4


def schedule(texts):
    """(data, write sizes) of a job that writes these lines: text, newline, text, newline, ..."""
    return b"".join(bytes(t) + NEWLINE for t in texts), [w for t in texts for w in (len(t), 1)]


def verdict(text_bytes, text_len, starts, row_bytes, picks, cap=None):
    """(reason, T) of an item whose output lines are the table lines `picks`: _WRITE for a length above 0x7FFFFFFF, else _LINE for a
    line that cannot be read, else _CAP when `cap` (None: the query) is below T"""
    lines = [(text_len[k], starts[k] if starts is not None else k * row_bytes) if k < len(text_len) else None for k in picks]
    if any(q is not None and q[0] > 0x7FFFFFFF for q in lines):
        return WRITE, 0
    if any(q is None or (starts is None and q[0] > row_bytes) or q[1] + q[0] > text_bytes for q in lines):
        return LINE, 0
    T = sum(q[0] + 1 for q in lines)
    return (CAP if cap is not None and cap < T else OK), T


def image(texts, compress, magic):
    """(bytes, block offsets, block lengths, stored flags) of the .4mc / .4mz part file; compress: fourmc_stream_model.compressor(...)"""
    data, sizes = schedule(texts)
    return fm.image(data, sizes, compress, magic)


def bstream(texts, compress, zstd):
    """(bytes, groups, chunks) of the block stream: BE32(rawlen) then BE32(clen) payload per chunk for every written group of the
    plan, BE32(0) where the plan says so; compress: bstream_model.oracle_compressor(...)"""
    data, sizes = schedule(texts)
    groups, trailer = wm.plan(sizes, bm.max_input(zstd))
    out, at = bytearray(), 0
    for rawlen, chunks in groups:
        out += bm.be32(rawlen)
        for c in chunks:
            payload = bytes(compress(data[at:at + c]))
            out += bm.be32(len(payload)) + payload
            at += c
    assert at == len(data)
    return bytes(out + (bm.be32(0) if trailer else b"")), len(groups), sum(len(c) for _, c in groups)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
_TEXT = {}


def text(n, at=0):
    """n compressible bytes without CR or LF, from byte `at` of the corpus"""
    if "t" not in _TEXT:
        t = helpers.corpus(M + (1 << 20)).copy()
        t[(t == 10) | (t == 13)] = 32
        _TEXT["t"] = t.tobytes()
    assert at + n <= len(_TEXT["t"])
    return _TEXT["t"][at:at + n]


def cut_lengths():
    """name -> text lengths: the smallest inputs at which two writes per line differ from any simpler rule"""
    rng = np.random.default_rng(20241021)
    return {
        "[M-1]": [M - 1],                                # the newline fills the block exactly
        "[M]": [M],                                      # the block ends between text and LF; the next block is "\n"
        "[M+1]": [M + 1],                                # a chopped write whose 1-byte rest is not joined with the newline
        "[M-2, 5]": [M - 2, 5],                          # the second text closes the block first
        "[0, 0, 3, 0]": [0, 0, 3, 0],
        "no line": [],
        "70000 lines": [int(v) for v in rng.integers(0, 201, 70000)],
    }


def lines_of(lengths, at=0):
    """texts of these lengths, cut from the corpus one behind the other (each case from its own place)"""
    out = []
    for k in lengths:
        if at + k > M + (1 << 20):
            at = 0
        out.append(text(k, at))
        at += k
    return out
