"""The Hadoop block-stream framing of the reference's eight raw codecs (Lz4Codec ... ZstdUltraCodec), restated in Python.

Writer: org.apache.hadoop.io.compress.BlockCompressorStream.write / finish / close over the buffer logic of the reference's
Lz4Compressor (Lz4Compressor.java:147-253; ZstdCompressor is the same code).  BlockCompressorStream is Hadoop's class: its source
is not in the reference tree and no JVM was at hand, so no file written by a JVM exists to compare with and tests/golden holds none
for this format.  The class is restated from knowledge of it; include/fourmc_gpu.h states the resulting format as the contract.
Input: the data, a list of write sizes and a block-compress callback (bytes -> bytes).  By itself the model produces the
accumulate path, the long-write path, the trailing BE32(0) and the four-byte empty stream.

Reader: the reader rule of include/fourmc_gpu.h (not BlockDecompressorStream: the header lists what differs), with the oracle's
decoders on the chunks."""
import numpy as np

import helpers

BUF = 4 << 20                            # LZ4_BUFFER_SIZE / the compressors' direct buffer
MAX_CLEN = 4 << 20
OK, BAD_RAWLEN, CLEN_UNREADABLE, BAD_CLEN, DATA_UNREADABLE, CORRUPT, SHAPE, DST_SMALL = range(8)


def lz4_bound(n):
    """LZ4_compressBound (lz4.h:212)"""
    return n + n // 255 + 16


def block_bound(n, zstd):
    return helpers.zstd_bound(n) if zstd else lz4_bound(n)


def max_input(zstd):
    """BlockCompressorStream's MAX_INPUT_SIZE as Lz4Codec.java:102-103 constructs it: bufferSize - compressionOverhead"""
    return BUF - (block_bound(BUF, zstd) - BUF)


def be32(v):
    return int(v).to_bytes(4, "big")


class _Compressor:
    """Lz4Compressor.java:147-253: a direct buffer of BUF bytes, a saved user buffer for what does not fit, one block per compress()"""

    def __init__(self, block_compress):
        self.cb = block_compress
        self.reset()

    def reset(self):
        self.finish_, self.finished_ = False, False
        self.direct = bytearray()        # uncompressedDirectBuf[0, position)
        self.user = b""                  # userBuf[userBufOff, +userBufLen)
        self.out = b""                   # compressedDirectBuf's remaining bytes
        self.bytes_read = 0

    def set_input(self, b):
        self.finished_ = False
        if len(b) > BUF - len(self.direct):
            self.user = bytes(b)
        else:
            self.direct += b
        self.bytes_read += len(b)

    def needs_input(self):
        return not (len(self.out) > 0 or len(self.direct) == BUF or len(self.user) > 0)

    def finish(self):
        self.finish_ = True

    def finished(self):
        return self.finish_ and self.finished_ and len(self.out) == 0

    def compress(self, cap):
        if self.out:
            n = min(len(self.out), cap)
            got, self.out = self.out[:n], self.out[n:]
            return got
        if not self.direct:
            take = min(len(self.user), BUF)                      # setInputFromSavedData
            if take:
                self.finished_ = False
                self.direct += self.user[:take]
                self.user = self.user[take:]
            if not self.direct:
                self.finished_ = True
                return b""
        comp = bytes(self.cb(bytes(self.direct)))
        self.direct = bytearray()
        if not self.user:
            self.finished_ = True
        n = min(len(comp), cap)
        self.out = comp[n:]
        return comp[:n]


class BlockCompressorStream:
    def __init__(self, block_compress, zstd):
        self.c = _Compressor(block_compress)
        self.max_input = max_input(zstd)
        self.buffer = BUF                                        # CompressorStream's byte[bufferSize]
        self.sink = bytearray()

    def _compress(self):
        got = self.c.compress(self.buffer)
        if got:
            self.sink += be32(len(got)) + got

    def write(self, b):
        b = bytes(b)
        n = len(b)
        limlen = self.c.bytes_read
        if n + limlen > self.max_input and limlen > 0:           # adding this write would exceed the maximum: flush what is there
            self.finish()
            self.c.reset()
        if n > self.max_input:                                   # the long write: one group, chunks of max_input
            self.sink += be32(n)
            off = 0
            while True:
                k = min(n - off, self.max_input)
                self.c.set_input(b[off:off + k])
                self.c.finish()
                while not self.c.finished():
                    self._compress()
                self.c.reset()
                off += k
                if off >= n:
                    break
            return
        self.c.set_input(b)
        if not self.c.needs_input():
            self.sink += be32(self.c.bytes_read)
            while True:
                self._compress()
                if self.c.needs_input():
                    break

    def finish(self):
        if not self.c.finished():
            self.sink += be32(self.c.bytes_read)
            self.c.finish()
            while not self.c.finished():
                self._compress()

    def close(self):
        self.finish()
        return bytes(self.sink)


def write_stream(data, write_sizes, block_compress, zstd=False):
    """the stream's bytes after write() calls of the given sizes over `data` (their sum must be len(data)) and close()"""
    data = bytes(data)
    assert sum(write_sizes) == len(data)
    s = BlockCompressorStream(block_compress, zstd)
    at = 0
    for w in write_sizes:
        s.write(data[at:at + w])
        at += w
    return s.close()


def write_groups(data, group_bytes, block_compress, zstd=False):
    """What fourmc_gpu_bstream_compress documents: `data` cut at every group_bytes, each piece the ONE group a stream writes for a
    piece that is alone in it - write(piece), close() - and 00 00 00 00 for no data.  For pieces above M / 2, and for group_bytes =
    floor(M / w) * w with writes of w bytes, write_stream gives the same bytes from the write() calls themselves."""
    data = bytes(data)
    assert 0 < group_bytes <= max_input(zstd)
    if not data:
        return write_stream(b"", [], block_compress, zstd)
    out = b""
    for at in range(0, len(data), group_bytes):
        piece = data[at:at + group_bytes]
        one = write_stream(piece, [len(piece)], block_compress, zstd)
        assert one[:4] == be32(len(piece)) and len(one) == 8 + int.from_bytes(one[4:8], "big")
        out += one
    return out


def oracle_compressor(codec, level):
    """bytes -> bytes by the oracle, as the eight compressor classes call it: unlimited output (capacity = the bound)"""
    def fast(b):
        r, out = helpers.orc_compress(np.frombuffer(b, np.uint8))
        assert r > 0
        return out.tobytes()

    def mc(b):
        r, out = helpers.orc_compress_mc(np.frombuffer(b, np.uint8))
        assert r > 0
        return out.tobytes()

    def hc(b):
        r, out = helpers.orc_compress_hc(np.frombuffer(b, np.uint8), level)
        assert r > 0
        return out.tobytes()

    def zstd(b):
        r, out = helpers.orc_zstd_compress(np.frombuffer(b, np.uint8), level)
        assert r > 0
        return out.tobytes()
    return (fast, mc, hc, zstd)[codec]


def walk(img, zstd):
    """The reader rule as pure header chasing: (chunks, groups, total, reason, fail_offset) with chunks = [(header offset, payload
    offset, clen, expected size, output offset, group number)] of the well-formed groups."""
    img = bytes(img)
    N, M = len(img), max_input(zstd)
    p, total, groups, chunks = 0, 0, 0, []
    reason, fail = OK, N
    while True:
        if N - p < 4:
            break                                                # 0 bytes left: the end; 1 - 3: the EOF Hadoop's reader swallows
        R = int.from_bytes(img[p:p + 4], "big")
        if R == 0:
            break
        if R > 0x7FFFFFFF:
            reason, fail = BAD_RAWLEN, p
            break
        q, done, mine = p + 4, 0, []
        while done < R:
            if N - q < 4:
                reason, fail = CLEN_UNREADABLE, q
                break
            clen = int.from_bytes(img[q:q + 4], "big")
            if clen == 0 or clen > MAX_CLEN:
                reason, fail = BAD_CLEN, q
                break
            if N - q - 4 < clen:
                reason, fail = DATA_UNREADABLE, q
                break
            expect = min(M, R - done)
            mine.append((q, q + 4, clen, expect, total + done, groups))
            done += expect
            q += 4 + clen
        if reason != OK:
            break                                                # a group cut short counts for nothing
        p, total, groups = q, total + R, groups + 1
        chunks += mine
    return chunks, groups, total, reason, fail


def read_stream(img, zstd=False, dst_cap=None):
    """(status dict, decoded bytes): decoded_bytes, total_bytes, fail_offset, groups, chunks, reason as fourmc_bstream_status has
    them.  dst_cap None: unlimited; "query": the size query (parse only)."""
    img = bytes(img)
    chunks, groups, total, reason, fail = walk(img, zstd)
    st = {"decoded_bytes": 0, "total_bytes": total, "fail_offset": fail, "groups": groups, "chunks": len(chunks), "reason": reason}
    if dst_cap == "query":
        return st, b""
    if dst_cap is not None and total > dst_cap:
        st.update(reason=DST_SMALL, fail_offset=len(img), groups=0, chunks=0)
        return st, b""
    out = bytearray()
    for k, (at, pay, clen, expect, _, g) in enumerate(chunks):
        comp = np.frombuffer(img[pay:pay + clen], np.uint8)
        r, got = helpers.orc_zstd_decompress(comp, expect) if zstd else helpers.orc_decompress(comp, expect)
        if r != expect:
            st.update(reason=CORRUPT if r < 0 else SHAPE, fail_offset=at, groups=g, chunks=k)
            break
        out += got.tobytes()
    st["decoded_bytes"] = len(out)
    return st, bytes(out)


def shape(img, zstd=False):
    """(groups, end): groups = [(rawlen, [expected size of each chunk])] by the walk, end = the offset behind the last whole group
    (test aid: the writer's shape invariant says each chunk decodes to exactly its expected size, which read_stream checks)"""
    chunks, groups, total, reason, fail = walk(img, zstd)
    assert reason == OK
    out = [[0, []] for _ in range(groups)]
    end = 0
    for at, pay, clen, expect, _, g in chunks:
        out[g][0] += expect
        out[g][1].append(expect)
        end = pay + clen
    return [(r, c) for r, c in out], end
