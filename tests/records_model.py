"""The executable statement of "the line records of a split" that the tests of fourmc_gpu_image_align_slices and
fourmc_gpu_image_read_records share (a plain module, not a conftest).

The specification is the reference's Java: FourMcBlockIndex.alignSlice{Start,End}ToIndex (FourMcBlockIndex.java:142-173), called by
FourMcInputFormat.getSplits, and FourMcLineRecordReader, which skips the first line of a split unless the split starts at 0 and then
reads lines while pos <= end.  There is no JVM here, so the rule is restated twice over (decoded bytes, block header offsets,
usizes): `Model.records` is the closed form the header documents, `Model.brute` the reader's loop; the CPU tests hold one against
the other."""
import bisect

import numpy as np

NOT_FOUND = (1 << 64) - 1


def layout(usizes, csizes):
    """header offsets of blocks with these compressed sizes, the end mark's offset, the file's size (native/4mc.c:293,:330-361)"""
    off, at = [], 12
    for c in csizes:
        off.append(at)
        at += 12 + int(c)
    return off, at, at + 12 + 20 + 4 * len(off)


def find_next(offsets, pos):
    """findNextPosition: the first block offset >= pos, or NOT_FOUND"""
    i = bisect.bisect_left(offsets, pos)
    return offsets[i] if i < len(offsets) else NOT_FOUND


def align_slice(offsets, start, end, file_size):
    """getSplits' inner step on one raw slice [start, end): the dict fourmc_image_slice holds afterwards"""
    r = {"start": start, "end": end, "split_start": start, "split_end": end, "first_block": 0, "block_count": 0, "result": 1}
    if not offsets:                                          # "leave the default split for empty block index"
        return r
    s = start
    if start != 0:
        s = find_next(offsets, start)
        if s == NOT_FOUND or s >= end:
            s = NOT_FOUND
    e = find_next(offsets, end)
    if e == NOT_FOUND:
        e = file_size
    r["split_start"], r["split_end"] = s, e
    if s == NOT_FOUND:
        r["result"] = 0
        return r
    r["first_block"] = bisect.bisect_left(offsets, s)
    r["block_count"] = bisect.bisect_left(offsets, e) - r["first_block"]
    return r


class Model:
    def __init__(self, data, offsets, usizes, end_mark, delim=10):
        self.data = np.asarray(data, dtype=np.uint8)
        self.offsets = [int(o) for o in offsets]
        self.doff = [0]
        for u in usizes:
            self.doff.append(self.doff[-1] + int(u))
        self.T = self.doff[-1]
        assert self.T == len(self.data)
        self.end_mark, self.delim = int(end_mark), delim
        self.P = np.flatnonzero(self.data == delim).astype(np.int64)

    def resolve(self, split_start, split_end):
        """(ds, de), or None for offsets the call refuses with -3"""
        n = len(self.offsets)
        ds = 0
        if split_start != 0:
            i = bisect.bisect_left(self.offsets, split_start)
            if i == n or self.offsets[i] != split_start:
                return None
            ds = self.doff[i]
        if split_end >= self.end_mark:
            return ds, self.T
        j = bisect.bisect_left(self.offsets, split_end)
        if j == n or self.offsets[j] != split_end or split_end < split_start:
            return None
        return ds, self.doff[j]

    def file_records(self):
        """the starts of every record of the content, and T behind them"""
        s = np.concatenate([[0], self.P + 1]) if self.T else np.zeros(1, np.int64)
        if s[-1] != self.T:
            s = np.append(s, self.T)
        return s

    def brute(self, split_start, split_end):
        """FourMcLineRecordReader in decoded offsets: the absolute starts of the records the split reads"""
        ds, de = self.resolve(split_start, split_end)
        after = lambda pos: next((i + 1 for i in range(pos, self.T) if self.data[i] == self.delim), self.T)  # noqa: E731
        pos = after(ds) if split_start != 0 else ds          # "skip the first line unless the split starts at 0"
        out = []
        while pos <= de and pos < self.T:                    # "read lines while pos <= end"
            out.append(pos)
            pos = after(pos)
        return out

    def records(self, split_start, split_end, dst_cap=None, starts_cap=None):
        """the closed form: what fourmc_image_records holds afterwards, "starts" (offsets in d_dst, records + 1 of them) and
        "need" = hi - ds, the dst_cap the call asks for even when the split turns out to own nothing"""
        r = {"result": 0, "base": 0, "data_off": 0, "data_bytes": 0, "reserved": 0, "starts": None, "need": 0}
        se = self.resolve(split_start, split_end)
        if se is None:
            r["result"] = -3
            return r
        ds, de = se
        P, T = self.P, self.T
        r["base"] = ds
        j = int(np.searchsorted(P, de))
        hi = int(P[j]) + 1 if j < len(P) else T
        r["need"] = hi - ds
        if dst_cap is not None and hi - ds > dst_cap:
            r["result"], r["data_bytes"] = -5, hi - ds
            return r
        lo = 0
        if split_start != 0:
            i = int(np.searchsorted(P, ds))
            lo = int(P[i]) + 1 if i < len(P) and P[i] < de else None
        s = np.zeros(1, np.int64)
        if lo is not None and lo < hi:
            s = np.concatenate([[lo], P[(P >= lo) & (P < hi)] + 1])
            if s[-1] != hi:
                s = np.append(s, hi)
            s = s - ds
        records = len(s) - 1
        if starts_cap is not None and records + 1 > starts_cap:
            r.update(result=-5, data_off=int(s[0]) if records else 0, data_bytes=hi - ds, reserved=records)
            return r
        if records:
            r.update(result=records, data_off=int(s[0]), data_bytes=hi - ds)
        r["starts"] = s
        return r


def families(B, text, noise):
    """The inputs both test files cover, for blocks of B bytes: name -> (content, delimiter).  text(n): n bytes of lines ending
    with byte 10; noise(n): n incompressible bytes."""
    def clean(a, lo, hi):
        v = a[lo:hi]
        v[v == 10] = 32
    out = {}
    a = text(3 * B + B // 3)
    clean(a, B - 9, B + 9); clean(a, 2 * B - 9, 2 * B + 9)
    a[B - 1] = 10                                           # a record ends exactly at a block end, the next starts block 1
    a[2 * B - 1] = 10; a[2 * B] = 10                        # ... and an empty record opens block 2
    out["block_edges"] = (a, 10)
    a = text(3 * B + B // 2)
    clean(a, B // 2, 2 * B + B // 2)                        # one record over blocks 0, 1 and 2
    out["three_blocks"] = (a, 10)
    a = text(3 * B + B // 2)
    clean(a, B // 2, len(a))                                # ... and one that runs to the end of the file, unterminated
    out["long_tail"] = (a, 10)
    a = text(2 * B + 100)
    a[B - 3:B + 3] = 10; a[0] = 10; a[-2:] = 10             # empty records at the start, across a block boundary, at the end
    out["empty_records"] = (a, 10)
    a = text(2 * B + 77)
    a[-1] = 120
    out["no_trailing_delimiter"] = (a, 10)
    a = text(2 * B + 5)
    clean(a, 0, len(a))
    out["no_delimiter"] = (a, 10)
    out["all_delimiters"] = (np.full(B + 1000, 10, np.uint8), 10)
    out["stored_block"] = (np.concatenate([text(B), noise(B), text(B // 2)]), 10)
    out["zero_blocks"] = (np.zeros(0, np.uint8), 10)
    out["one_block"] = (text(B // 4), 10)
    a = text(2 * B + 9)
    a[a == 0] = 1; a[a == 10] = 0
    out["delimiter_0"] = (a, 0)
    return out
