"""Hadoop's FourMcOutputStream / FourMzOutputStream, restated in Python: the writer behind FourMcCodec, FourMzCodec and their six
siblings, whose part files fourmc_gpu_images_compress_writes writes on the device.

What is restated, buffer by buffer and with its line numbers: FourMcOutputStream.java:69-223 (the header, write, finish, compress with
its stored branch, close; FourMzOutputStream is the same code) over Lz4Compressor.java:147-298 (the direct buffer, the saved user
buffer, bytesRead / bytesWritten, reset, finish, finished, needsInput, compress, uncompressedBytes; ZstdCompressor is the same code).
No JVM was at hand and nobody ran one: no file written by a JVM exists to compare with and tests/golden holds none for this writer.
The classes are restated from their source; include/fourmc_gpu.h states the resulting format as the contract.

M, the 4 MiB that is FOURMC_MAX_BLOCK_SIZE, the compressors' direct buffer and the stream's byte buffer at once (FourMcCodec.java:86,
:100; Lz4Compressor.java:86), is a parameter here, so that small values can be enumerated.

The module also holds the rule in closed form (cuts, image): what the header states and the device plans by."""
import numpy as np

import bstream_model as bm
import helpers

M4 = 4 << 20
MAGIC_4MC, MAGIC_4MZ = 0x344D4300, 0x344D5A00
be32 = bm.be32


def xxh32(b):
    return helpers.orc_xxh32(np.frombuffer(bytes(b), np.uint8)) if len(b) else helpers.orc_xxh32(np.zeros(0, np.uint8))


class Compressor(bm._Compressor):
    """Lz4Compressor.java:147-298 with a direct buffer of `buf` bytes.  The uncompressed direct buffer keeps its bytes when it is
    cleared (clear() moves the position only), which uncompressedBytes() relies on."""

    def __init__(self, block_compress, buf):
        self.buf = buf
        self.mem = bytearray(buf)            # uncompressedDirectBuf's memory; self.direct is [0, position)
        super().__init__(block_compress)

    def reset(self):                         # :255-264
        super().reset()
        self.bytes_written = 0

    def set_input(self, b):                  # :147-166
        self.finished_ = False
        if len(b) > self.buf - len(self.direct):
            self.user = bytes(b)             # save data; now !needsInput
        else:
            self.mem[len(self.direct):len(self.direct) + len(b)] = b
            self.direct += b
        self.bytes_read += len(b)

    def needs_input(self):                   # :195-199
        return not (len(self.out) > 0 or len(self.direct) == self.buf or len(self.user) > 0)

    def compress(self, cap):                 # :213-253
        if self.out:
            n = min(len(self.out), cap)
            got, self.out = self.out[:n], self.out[n:]
            self.bytes_written += n
            return got
        if not self.direct:
            take = min(len(self.user), self.buf)                 # setInputFromSavedData, :173-186
            if take:
                self.finished_ = False
                self.mem[:take] = self.user[:take]
                self.direct += self.user[:take]
                self.user = self.user[take:]
            if not self.direct:
                self.finished_ = True
                return b""
        comp = bytes(self.cb(bytes(self.direct)))                # compressBytesDirect: the JNI call, unlimited output
        self.direct = bytearray()                                # uncompressedDirectBuf.clear()
        if not self.user:
            self.finished_ = True
        n = min(len(comp), cap)
        self.bytes_written += n
        self.out = comp[n:]
        return comp[:n]

    def uncompressed_bytes(self):            # :294-298: bytesRead bytes from the cleared buffer's start
        return bytes(self.mem[:self.bytes_read])


class FourMcOutputStream:
    def __init__(self, block_compress, magic=MAGIC_4MC, M=M4):
        self.M = M                                               # FOURMC_MAX_BLOCK_SIZE
        self.c = Compressor(block_compress, M)
        self.buffer = M                                          # CompressorStream's byte[bufferSize], FourMcCodec.java:100
        self.magic = magic
        self.sink = bytearray()                                  # cout; len(sink) is cout.bytesWritten
        self.block_offsets = []
        self.closed = False
        head = be32(magic) + be32(1)                             # write4mcHeader, :69-80
        self.sink += head + be32(xxh32(head))

    def write(self, b):                                          # :140-182
        b = bytes(b)
        n = len(b)
        assert not self.c.finished(), "write beyond end of stream"
        if n == 0:                                               # :153
            return
        limlen = self.c.bytes_read
        if n + limlen > self.M and limlen > 0:                   # :158-161
            self.finish()
            self.c.reset()
        if n > self.M:                                           # :163-173
            off = 0
            while True:
                k = min(n - off, self.M)
                self.c.set_input(b[off:off + k])
                self.finish()
                self.c.reset()
                off += k
                if off >= n:
                    break
            return
        self.c.set_input(b)                                      # :176-181
        if not self.c.needs_input():
            while True:
                self._compress()
                if self.c.needs_input():
                    break

    def finish(self):                                            # :185-192
        if not self.c.finished():
            self.c.finish()
            while not self.c.finished():
                self._compress()

    def _compress(self):                                         # :195-223
        got = self.c.compress(self.buffer)
        if len(got) > 0:
            self.block_offsets.append(len(self.sink))            # :200
            self.sink += be32(self.c.bytes_read)
            if self.c.bytes_read <= self.c.bytes_written:        # :204: the block is written uncompressed
                raw = self.c.uncompressed_bytes()
                self.sink += be32(len(raw)) + be32(xxh32(raw)) + raw
                self.c.reset()                                   # :213-214
                self.c.finish()
            else:
                self.sink += be32(len(got)) + be32(xxh32(got)) + got

    def close(self):                                             # :102-137
        if self.closed:
            return bytes(self.sink)
        self.finish()
        self.sink += be32(0) * 3
        size = 20 + 4 * len(self.block_offsets)
        foot = be32(size) + be32(1)
        for i, o in enumerate(self.block_offsets):
            foot += be32(o if i == 0 else o - self.block_offsets[i - 1])
        foot += be32(size) + be32(self.magic)
        self.sink += foot + be32(xxh32(foot))
        self.closed = True
        return bytes(self.sink)


def write_image(data, write_sizes, block_compress, magic=MAGIC_4MC, M=M4):
    """the file after write() calls of the given sizes over `data` (their sum must be len(data)) and close()"""
    data = bytes(data)
    assert sum(write_sizes) == len(data)
    s = FourMcOutputStream(block_compress, magic, M)
    at = 0
    for w in write_sizes:
        s.write(data[at:at + w])
        at += w
    return s.close()


# ---- the rule in closed form ------------------------------------------------------------------------------------------------------
def cuts(write_sizes, M=M4):
    """the lengths of the blocks write() calls of these sizes give"""
    blocks, acc = [], 0
    for w in write_sizes:
        if w == 0:
            continue
        if acc > 0 and acc + w > M:
            blocks.append(acc)
            acc = 0
        if w > M:
            blocks += [M] * (w // M) + ([w % M] if w % M else [])
            continue
        acc += w
        if acc == M:
            blocks.append(acc)
            acc = 0
    if acc:
        blocks.append(acc)
    return blocks


def frame(blocks, magic):
    """header, [(u, payload)] as blocks (stored when len(payload) == u ... the caller decides), end mark, footer"""
    head = be32(magic) + be32(1)
    out = bytearray(head + be32(xxh32(head)))
    offs = []
    for u, payload in blocks:
        offs.append(len(out))
        out += be32(u) + be32(len(payload)) + be32(xxh32(payload)) + payload
    out += be32(0) * 3
    size = 20 + 4 * len(offs)
    foot = be32(size) + be32(1)
    for i, o in enumerate(offs):
        foot += be32(o if i == 0 else o - offs[i - 1])
    foot += be32(size) + be32(magic)
    return bytes(out + foot + be32(xxh32(foot)))


def image(data, write_sizes, block_compress, magic=MAGIC_4MC, M=M4):
    """the closed-form image, and what the device reports beside it: (bytes, block offsets, block lengths, stored flags)"""
    data = bytes(data)
    blocks, at, stored = [], 0, []
    for u in cuts(write_sizes, M):
        raw = data[at:at + u]
        comp = bytes(block_compress(raw))
        stored.append(u <= len(comp))
        blocks.append((u, raw if stored[-1] else comp))
        at += u
    assert at == len(data)
    offs, o = [], 12
    for u, p in blocks:
        offs.append(o)
        o += 12 + len(p)
    return frame(blocks, magic), offs, [u for u, _ in blocks], stored


def worst_case(write_sizes, M=M4):
    """the exact worst case of the image's length: every block stored"""
    c = cuts(write_sizes, M)
    return 12 + sum(12 + u for u in c) + 12 + 20 + 4 * len(c)


def max_blocks(S, M=M4):
    """the most blocks any schedule over S bytes has: a 1-byte write in front of a write of M + 1 bytes is 3 blocks in M + 2 bytes"""
    return 3 * (S // (M + 2)) + min(S % (M + 2), 2)


def writes_bound(S, M=M4):
    """fourmc_gpu_image_writes_bound"""
    return 12 + 16 * max_blocks(S, M) + S + 32


def parse(img):
    """[(header offset, u, c, checksum)] of the blocks, by walking the headers up to the end mark"""
    img = bytes(img)
    p, out = 12, []
    while True:
        u, c, x = (int.from_bytes(img[p + k:p + k + 4], "big") for k in (0, 4, 8))
        if u == 0 and c == 0 and x == 0:
            return out
        out.append((p, u, c, x))
        p += 12 + c


def compressor(magic, level):
    """bytes -> bytes by the oracle, as the eight compressor classes call the JNI (unlimited output), for the CLI level of
    fourmc_gpu_images_compress: .4mc 1 fast, 2 MC, 3 HC(4), 4 HC(8); .4mz zstd 1, 3, 6, 12"""
    if magic == MAGIC_4MC:
        return bm.oracle_compressor(0 if level <= 1 else 1 if level == 2 else 2, 4 if level == 3 else 8)
    return bm.oracle_compressor(3, 1 if level <= 1 else 3 if level == 2 else 6 if level == 3 else 12)
