"""The executable statement of "the lines of a split by Hadoop's default rule" that the tests of fourmc_gpu_image_read_lines share
(a plain module, not a conftest), next to records_model.py, whose offsets, alignment and layout it reuses by import.

The specification is the reference's reader: FourMcLineRecordReader builds `new LineReader(codec.createInputStream(fileIn), job)`
and calls `in.readLine(value, maxLineLen)` (FourMcLineRecordReader.java:122,135,154), so every line is cut by LineReader's default
rule: LF, a lone CR and CR LF end a line, the terminator is not part of the value, the value is cut at max.line.length and the whole
line is consumed all the same.  There is no JVM here, so the rule is restated twice over the decoded bytes: `Model.lines` is the
closed form the header documents, `Model.brute` the reader's loop with LineReader.readDefaultLine's buffer refills and its
prevCharCR; the CPU tests hold one against the other.

One case is decided by the closed form and not by the loop: a CR as the last decoded byte before split_end with a non-LF byte behind
it.  The Java reader looks behind that CR by filling its buffer, which pulls the next compressed block and moves the file position
past the split's end, so neither it nor the next split's reader (which skips its first line) reads the line that starts at de.  Here
that line belongs to the earlier split: `brute` keeps its position in decoded offsets, where looking at a byte moves nothing."""
import numpy as np

import records_model as rm
from records_model import NOT_FOUND, align_slice, find_next, layout  # noqa: F401  (the tests take them from here)

LF, CR = 10, 13
BUFFER = 64 * 1024                                          # io.file.buffer.size, LineReader's default
DEFAULT_MAX = 0x7FFFFFFF


def line_ends(data):
    """positions p that end a line: D[p] == LF, or D[p] == CR and (p + 1 == T or D[p+1] != LF)"""
    d = np.asarray(data, dtype=np.uint8)
    if not len(d):
        return np.zeros(0, np.int64)
    nxt_lf = np.append(d[1:] == LF, False)
    return np.flatnonzero((d == LF) | ((d == CR) & ~nxt_lf)).astype(np.int64)


class Model(rm.Model):
    def __init__(self, data, offsets, usizes, end_mark, max_line_len=DEFAULT_MAX, buffer=BUFFER):
        super().__init__(data, offsets, usizes, end_mark, LF)
        self.max_line_len, self.buffer = int(max_line_len), int(buffer)
        self.P = line_ends(self.data)                       # over these positions rm.Model.records IS the ownership's closed form

    def file_lines(self):
        """the starts of every line of the content, and T behind them"""
        return self.file_records()

    def term_len(self, s, e):
        """terminator length of the line [s, e)"""
        if e - s >= 2 and self.data[e - 2] == CR and self.data[e - 1] == LF:
            return 2
        return 1 if e > s and self.data[e - 1] in (LF, CR) else 0

    def read_line(self, pos, state):
        """LineReader.readDefaultLine from decoded offset pos: (bytes consumed, text length).  `state` is the reader's buffer,
        [buffer start, buffer end, position in it]; it refills in reads of self.buffer bytes and carries prevCharCR across refills."""
        data, T = self.data, self.T
        txt = 0
        newline = 0
        prev_cr = False
        consumed = 0
        while True:
            start = state[2]
            if state[2] >= state[1]:                        # fill the buffer
                start = state[2] = state[0] = state[1]
                if prev_cr:
                    consumed += 1                           # "account for CR from previous read"
                state[1] = min(T, state[0] + self.buffer)
                if state[1] <= state[0]:
                    break                                   # EOF
            p = state[2]
            while p < state[1]:
                c = data[p]
                if c == LF:
                    newline = 2 if prev_cr else 1
                    p += 1
                    break
                if prev_cr:                                 # CR + not LF: the line ended at the CR, p stays on this byte
                    newline = 1
                    break
                prev_cr = c == CR
                p += 1
            state[2] = p
            read = p - start
            if prev_cr and newline == 0:
                read -= 1                                   # CR at the end of the buffer
            consumed += read
            append = read - newline
            if append > self.max_line_len - txt:
                append = self.max_line_len - txt
            if append > 0:
                txt += append
            if newline:
                break
        return consumed, txt

    def brute(self, split_start, split_end):
        """FourMcLineRecordReader in decoded offsets: [(absolute start, text length)] of the lines the split reads"""
        ds, de = self.resolve(split_start, split_end)
        state = [ds, ds, ds]
        pos = ds
        if split_start != 0:                                # "read and ignore the first line"
            pos += self.read_line(pos, state)[0]
        out = []
        while pos <= de:                                    # "if (pos <= end)"
            n, txt = self.read_line(pos, state)
            if n == 0:
                break
            out.append((pos, txt))
            pos += n
        return out

    def lines(self, split_start, split_end, dst_cap=None, lines_cap=None):
        """the closed form: what fourmc_image_lines holds afterwards, "starts" (offsets in d_dst, lines + 1 of them), "text_len"
        (one per line) and "need" = hi - ds"""
        r = self.records(split_start, split_end, dst_cap=dst_cap, starts_cap=lines_cap)
        r["text_len"] = None
        if r["starts"] is not None:
            s = r["starts"] + r["base"]
            a, e = s[:-1], s[1:]                            # term_len for every line at once
            last = self.data[e - 1] if len(a) else np.zeros(0, np.uint8)
            crlf = (last == LF) & (e - a >= 2) & (self.data[np.maximum(e - 2, 0)] == CR) if len(a) else np.zeros(0, bool)
            t = np.where(crlf, 2, np.where((last == LF) | (last == CR), 1, 0))
            r["text_len"] = np.minimum(e - a - t, self.max_line_len).astype(np.int64)
        return r


def families(B, text, noise):
    """The inputs both test files cover, for blocks of B bytes (B >= 16): name -> content.  text(n): n bytes of lines ending with
    LF and holding no CR; noise(n): n incompressible bytes."""
    def clean(a, lo=0, hi=None):
        v = a[lo:hi]
        v[(v == LF) | (v == CR)] = 32
        return a

    def crlf(a):
        """every LF of a at position >= 1 becomes the LF of a CR LF"""
        p = np.flatnonzero(a == LF)
        p = p[p > 0]
        a[p - 1] = CR
        return a
    out = {}
    out["crlf_text"] = crlf(text(2 * B + B // 3))
    a = text(2 * B + B // 5)
    a[a == LF] = CR
    out["cr_only"] = a
    out["lf_only"] = text(2 * B + B // 7)
    a = text(2 * B + 301)
    rng = np.random.default_rng(B)
    for tok in (b"\r\r", b"\n\r", b"\r\n\r\n", b"\n\n", b"\r\n", b"\r", b"\r\r\n"):
        for at in rng.integers(0, len(a) - 8, 6 + len(a) // 4096):
            a[at:at + len(tok)] = np.frombuffer(tok, np.uint8)
    out["mixed"] = a
    out["all_cr"] = np.full(B + 500, CR, np.uint8)
    out["all_lf"] = np.full(B + 500, LF, np.uint8)
    out["alternating_crlf"] = np.tile(np.frombuffer(b"\r\n", np.uint8), B + 51)[:2 * B + 101].copy()
    out["alternating_lfcr"] = np.tile(np.frombuffer(b"\n\r", np.uint8), B + 51)[:2 * B + 101].copy()
    out["no_terminator"] = clean(text(2 * B + 5))
    out["zero_blocks"] = np.zeros(0, np.uint8)
    out["one_block"] = crlf(text(B // 4))
    out["stored_block"] = np.concatenate([crlf(text(B)), noise(B), text(B // 2)])
    # a CR in the last byte of a block, followed in the next block by LF, by another byte, and by nothing (the last block)
    a = clean(text(3 * B), B - 9, B + 9)
    clean(a, 2 * B - 9, 2 * B + 9)
    a[B - 1] = CR; a[B] = LF
    a[2 * B - 1] = CR; a[2 * B] = 120
    a[3 * B - 1] = CR
    out["cr_at_block_end"] = a
    a = text(2 * B + 40)
    a[-2] = CR; a[-1] = LF
    out["ends_with_crlf"] = a
    a = text(2 * B + 40)
    a[-1] = CR
    out["ends_with_cr"] = a
    a = text(3 * B + 100)
    clean(a, B, 2 * B + 50)
    a[2 * B - 1] = CR                                       # the tail block of a split that ends at block 1 shows only this end
    out["tail_only_cr_last"] = a
    a = a.copy()
    a[2 * B] = LF                                           # ... and the block behind it opens with the LF of that CR
    out["tail_only_cr_last_lf"] = a
    a = text(3 * B + B // 2)
    clean(a, B // 2, 2 * B + B // 2)                        # one line over blocks 0, 1 and 2
    a[2 * B + B // 2] = CR; a[2 * B + B // 2 + 1] = LF
    out["three_blocks"] = a
    return out
