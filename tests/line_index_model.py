"""The executable statement of "lines by number" (fourmc_gpu_image_line_index / _image_read_lines_at) that its tests share (a plain
module, not a conftest), built on lines_model.line_ends, whose rule it is.

With D[0, T) the content, P its line ends in order and E their number: lines = E + (T > 0 and T - 1 is no line end); line 0 starts
at 0, line k > 0 one past end k - 1; line k ends at end k, or at T for the final unterminated line.  The index is stated twice:
`index` is the closed form over P, `index_loop` what the device does - every block counted by itself, then the seam rule.  The
test_line_index_cpu.py holds one against the other, and `lines_at` against slicing by lines_model.Model.file_lines / term_len."""
import numpy as np

import lines_model as lm

LF, CR = lm.LF, lm.CR
ENTRY = np.dtype([("ends_before", "<u8"), ("ends", "<u4"), ("flags", "<u4")])


def _doff(usizes):
    return np.concatenate([[0], np.cumsum(np.asarray(usizes, dtype=np.int64))]).astype(np.int64)


def count_lines(data):
    d = np.asarray(data, dtype=np.uint8)
    P = lm.line_ends(d)
    return len(P) + (1 if len(d) and (not len(P) or P[-1] != len(d) - 1) else 0)


def index(data, usizes):
    """-> (entries, lines): nblocks + 1 entries, the last one the sentinel {E, 0, 0}.  The closed form."""
    d = np.asarray(data, dtype=np.uint8)
    T, doff = len(d), _doff(usizes)
    assert doff[-1] == T
    P = lm.line_ends(d)
    ent = np.zeros(len(usizes) + 1, dtype=ENTRY)
    for b in range(len(usizes)):
        a, z = int(doff[b]), int(doff[b + 1])
        i, j = int(np.searchsorted(P, a)), int(np.searchsorted(P, z))
        flags = 0
        if z > a:
            if d[z - 1] == CR and z < T and d[z] == LF:
                flags |= 1
            if d[a] == LF and a > 0 and d[a - 1] == CR:
                flags |= 2
            if j > i:
                flags |= (int(P[j - 1]) + 1 - a) << 8
        ent[b] = (i, j - i, flags)
    ent[len(usizes)] = (len(P), 0, 0)
    return ent, count_lines(d)


def index_loop(data, usizes):
    """the same, block by block: each block's ends taken by itself (a CR in its last byte ends a line, nothing lies in front of its
    first byte), its first and last byte, then the seams: a CR that the next content byte's LF takes back, looking past blocks
    without bytes"""
    d = np.asarray(data, dtype=np.uint8)
    doff = _doff(usizes)
    n = len(usizes)
    own = []
    for b in range(n):
        blk = d[doff[b]:doff[b + 1]]
        own.append((lm.line_ends(blk), len(blk), len(blk) and blk[-1] == CR, len(blk) and blk[0] == LF, len(blk) and blk[-1] in (LF, CR)))
    ent = np.zeros(n + 1, dtype=ENTRY)
    run = 0
    last_closed = True
    for b in range(n):
        ends, size, last_cr, first_lf, closed = own[b]
        flags = 0
        if size:
            nxt = next((j for j in range(b + 1, n) if own[j][1]), None)
            prv = next((j for j in range(b - 1, -1, -1) if own[j][1]), None)
            if last_cr and nxt is not None and own[nxt][3]:
                flags |= 1
                ends = ends[:-1]                            # the CR in the last byte ends nothing
            if first_lf and prv is not None and own[prv][2]:
                flags |= 2
            if len(ends):
                flags |= (int(ends[-1]) + 1) << 8
            last_closed = bool(closed)
        ent[b] = (run, len(ends), flags)
        run += len(ends)
    ent[n] = (run, 0, 0)
    total = int(doff[-1])
    return ent, run + (1 if total and not last_closed else 0)


def lines_at(data, ks, row_bytes, max_line_len=lm.DEFAULT_MAX, pad=0, P=None):
    """-> (rows [n, row_bytes] uint8, text_len int64, status int64) of the requests ks against the content, the image undamaged.
    P: line_ends(data), for a caller that asks many times about one content"""
    d = np.asarray(data, dtype=np.uint8)
    T = len(d)
    P = lm.line_ends(d) if P is None else P
    E = len(P)
    lines = E + (1 if T and (not E or P[-1] != T - 1) else 0)
    rows = np.full((len(ks), row_bytes), pad, dtype=np.uint8)
    tl = np.zeros(len(ks), np.int64)
    st = np.zeros(len(ks), np.int64)
    for i, k in enumerate(ks):
        k = int(k)
        if k >= lines:
            st[i] = -3
            continue
        s = 0 if k == 0 else int(P[k - 1]) + 1
        if k < E:
            p = int(P[k])
            t = 2 if d[p] == LF and p > 0 and d[p - 1] == CR else 1
            e = p + 1 - t
        else:
            e = T
        tl[i] = min(e - s, max_line_len)
        c = min(int(tl[i]), row_bytes)
        rows[i, :c] = d[s:s + c]
        st[i] = 1
    return rows, tl, st


def needed_blocks(data, usizes, ks, row_bytes, max_line_len=lm.DEFAULT_MAX):
    """the blocks a call stages for the requests ks: bp and be of every line there is, and between them the blocks its first
    L = min(row_bytes, max_line_len) bytes reach into"""
    d = np.asarray(data, dtype=np.uint8)
    doff = _doff(usizes)
    P = lm.line_ends(d)
    E, lines, T = len(P), count_lines(d), len(d)
    L = min(row_bytes, max_line_len)
    full = [b for b in range(len(usizes)) if usizes[b]]
    block_of = lambda pos: int(np.searchsorted(doff, pos, side="right")) - 1  # noqa: E731  (positions inside blocks with bytes)
    need = set()
    for k in ks:
        k = int(k)
        if k >= lines:
            continue
        bp = 0 if k == 0 else block_of(int(P[k - 1]))
        be = block_of(int(P[k])) if k < E else full[-1]
        s = 0 if k == 0 else int(P[k - 1]) + 1
        need.update((bp, be))
        need.update(j for j in range(bp + 1, be) if usizes[j] and doff[j] < s + L)
    return sorted(need)
