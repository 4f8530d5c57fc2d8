""".zst files (what ZstCodec and the zstd tool write): a Python restatement of the frame and block walk of the device path
(4mc_amd/csrc/zst.hip), and the inputs of its tests, built with the reference's library (oracle/_ref/libref4mc.so).

  walk(image)        frames, skippable frames and blocks in front of the first frame whose headers fail, and that frame's offset
  block_table(image) per block of a VALID image: frame, type, and - for a compressed block - literals type and the symbol modes
  reach(image)       how many blocks refer to a table that a block of an EARLIER group of 64 table entries defines
  inputs()           the valid inputs A-F: name -> (image, source)
  damaged()          the damaged inputs G: [(class, label, image, the valid input it was made from)]
  expect(image)      what the device must report, from the walk and the reference's decoder run frame by frame
"""
import ctypes as C
import functools
import struct

import numpy as np

import helpers
import zstd_shapes as zs
from zstd_shapes import P_LEVEL, P_WLOG, P_CHECKSUM, P_TARGETCBLOCK, compress2, skippable, stream

MAGIC = 0xFD2FB528
BLOCK_MAX = 128 << 10


# ---------------------------------------------------------------------------------------------- the walk
def walk(image):
    """-> dict(frames, skippable, blocks, fail_offset, ok, spans): zstd frames, skippable frames and blocks in front of the first
    frame whose headers fail (all, if none), the offset of that frame's magic number (len(image) if none), and the (start, end,
    first block, blocks, skippable frames in front) of every complete frame.  The rules are ZSTD_decompress's (zstd_decompress.c:
    901-987, 989-1078; ZSTD_getcBlockSize zstd_decompress_block.c:57-80) plus the device's deviation: a dictionary ID fails."""
    p = bytes(image)
    n, ip = len(p), 0
    frames = skips = blocks = 0
    spans = []

    def result(fail):
        return {"frames": frames, "skippable": skips, "blocks": blocks, "fail_offset": n if fail is None else fail, "ok": fail is None,
                "spans": spans}
    while n - ip >= 5:
        at = ip
        magic = struct.unpack_from("<I", p, ip)[0]
        if magic & 0xFFFFFFF0 == 0x184D2A50:
            if n - ip < 8: return result(at)
            sz = struct.unpack_from("<I", p, ip + 4)[0]
            if sz > n - ip - 8: return result(at)
            ip += 8 + sz; skips += 1
            continue
        if magic != MAGIC or n - ip < 9: return result(at)
        fhd = p[ip + 4]
        fcs_id, single, has_sum, did = fhd >> 6, (fhd >> 5) & 1, (fhd >> 2) & 1, fhd & 3
        did_sz, fcs_sz = (0, 1, 2, 4)[did], (single if fcs_id == 0 else 1 << fcs_id)
        hsize = 5 + (0 if single else 1) + did_sz + fcs_sz
        if fhd & 8 or n - ip < hsize + 3: return result(at)
        hp = ip + 5
        if not single:
            if (p[hp] >> 3) + 10 > 31: return result(at)
            hp += 1
        if int.from_bytes(p[hp:hp + did_sz], "little"): return result(at)
        ip += hsize
        nb = 0
        while True:
            if n - ip < 3: return result(at)
            bh = p[ip] | p[ip + 1] << 8 | p[ip + 2] << 16
            ip += 3
            last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
            content = 1 if btype == 1 else bsize
            if btype == 3 or content > n - ip: return result(at)
            if btype == 2 and (bsize >= BLOCK_MAX or bsize < 2): return result(at)
            nb += 1; ip += content
            if last: break
        if has_sum:
            if n - ip < 4: return result(at)
            ip += 4
        spans.append((at, ip, blocks, nb, skips))
        frames += 1; blocks += nb
    return result(None if ip == n else ip)


def block_table(image):
    """Per block of a VALID image, in file order: dict(frame, type, off, size, ltype, nseq, modes, lit_end)."""
    p = bytes(image)
    out = []
    for f, (start, end, _, _, _) in enumerate(walk(p)["spans"]):
        fhd = p[start + 4]
        single, did, fcs_id = (fhd >> 5) & 1, fhd & 3, fhd >> 6
        ip = start + 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + (single if fcs_id == 0 else 1 << fcs_id)
        while True:
            bh = p[ip] | p[ip + 1] << 8 | p[ip + 2] << 16
            ip += 3
            last, btype, bsize = bh & 1, (bh >> 1) & 3, bh >> 3
            e = {"frame": f, "type": btype, "off": ip, "size": bsize, "ltype": None, "nseq": 0, "modes": 0}
            if btype == 2:
                b0 = p[ip]
                lt, sf = b0 & 3, (b0 >> 2) & 3
                if lt < 2:
                    lh = (1, 2, 1, 3)[sf]
                    lsize = (b0 >> 3) if lh == 1 else (b0 >> 4) + (p[ip + 1] << 4) + ((p[ip + 2] << 12) if lh == 3 else 0)
                    lcsize = 1 if lt == 1 else lsize
                else:
                    lh = (3, 3, 4, 5)[sf]
                    lcsize = (int.from_bytes(p[ip:ip + lh], "little") >> 4) >> (10, 10, 14, 18)[sf]
                s = ip + lh + lcsize
                c0 = p[s]
                if c0 == 0: nseq, w = 0, 1
                elif c0 < 128: nseq, w = c0, 1
                elif c0 < 255: nseq, w = ((c0 - 128) << 8) + p[s + 1], 2
                else: nseq, w = p[s + 1] + (p[s + 2] << 8) + 0x7F00, 3
                e.update(ltype=lt, nseq=nseq, modes=p[s + w] if nseq else 0, lit_end=s)
            out.append(e)
            ip += 1 if btype == 1 else bsize
            if last: break
    return out


def reach(image, group=64):
    """-> dict(treeless, ll, of, ml): blocks whose Huffman table (treeless literals) or LL / OF / ML table (Repeat mode) is defined by
    a block of an earlier group of `group` table entries, and "treeless_all": every treeless block."""
    tab = block_table(image)
    out = {"treeless": 0, "ll": 0, "of": 0, "ml": 0, "treeless_all": 0}
    last = {}
    for i, e in enumerate(tab):
        if i == 0 or tab[i - 1]["frame"] != e["frame"]: last = {}
        if e["type"] != 2: continue
        if e["ltype"] == 2: last["treeless"] = i
        elif e["ltype"] == 3:
            out["treeless_all"] += 1
            if last["treeless"] // group != i // group: out["treeless"] += 1
        if e["nseq"]:
            for name, sh in (("ll", 6), ("of", 4), ("ml", 2)):
                if (e["modes"] >> sh) & 3 != 3: last[name] = i
                elif last[name] // group != i // group: out[name] += 1
    return out


# ---------------------------------------------------------------------------------------------- the reference
def _ref_fn(name, restype, argtypes):
    f = getattr(helpers.ref(), name)
    f.restype, f.argtypes = restype, argtypes
    return f


def find_frame_size(image, at):
    """ZSTD_findFrameCompressedSize of image[at:] or -1."""
    f = _ref_fn("ZSTD_findFrameCompressedSize", C.c_size_t, [C.c_void_p, C.c_size_t])
    buf = np.frombuffer(bytes(image[at:]), np.uint8)
    r = f(buf.ctypes.data if len(buf) else None, len(buf))
    return -1 if helpers.ref().ZSTD_isError(r) else int(r)


def ref_decode(image, cap):
    """ZSTD_decompress of the whole file -> (size or -1, bytes)."""
    return zs.ref_decode(image, cap)


def expect(image, cap):
    """What the device reports for `image` with a destination of cap >= every frame's size: dict(ok, fail_offset, decoded, frames,
    skippable, blocks, data).  The frames the walk passes go through the reference one at a time; the first that fails - in the
    walk or in the reference - is the failing frame."""
    p = bytes(image)
    w = walk(p)
    done, data = 0, []
    for k, (start, end, b0, nb, sk) in enumerate(w["spans"]):
        r, out = ref_decode(p[start:end], cap)
        if r < 0:
            return {"ok": False, "fail_offset": start, "decoded": done, "frames": k, "skippable": sk, "blocks": b0, "data": b"".join(data)}
        done += r; data.append(out)
    return {"ok": w["ok"], "fail_offset": w["fail_offset"], "decoded": done, "frames": w["frames"], "skippable": w["skippable"],
            "blocks": w["blocks"], "data": b"".join(data)}


# ---------------------------------------------------------------------------------------------- inputs
def text(n, logs=False):
    return helpers.corpus(n, logs=logs).tobytes()


def streamed(src, params):
    """ZSTD_compressStream over the whole input, then ZSTD_endStream: no flush, no pledged size."""
    src = zs._u8(src)
    out = np.zeros(2 * len(src) + 4096, np.uint8)
    ob = helpers.ZstdOutBuffer(out.ctypes.data, len(out), 0)
    with zs._Cctx(params) as cx:
        ib = helpers.ZstdInBuffer(src.ctypes.data, len(src), 0)
        for directive in (0, 2):                                     # ZSTD_e_continue, ZSTD_e_end
            for _ in range(1 << 16):
                r = cx.L.ZSTD_compressStream2(cx.c, C.byref(ob), C.byref(ib), directive)
                assert not cx.L.ZSTD_isError(r)
                if ib.pos == len(src) and (directive == 0 or r == 0): break
            else: raise AssertionError("stream did not drain")
    return out[:ob.pos].tobytes()


def zstcodec(src, level):
    """What ZstCodec writes: ZSTD_initCStream(level), ZSTD_compressStream, ZSTD_endStream (jniZStreamCompressor.c:86-137)."""
    return streamed(src, {P_LEVEL: level})


A_SIZES = (0, 1, BLOCK_MAX, BLOCK_MAX + 1, 9175040)


@functools.lru_cache(None)
def inputs():
    """name -> (image, source) of the valid inputs A-F."""
    out = {}
    logs, big = text(A_SIZES[-1], logs=True), text(A_SIZES[-1])      # (log text: its long frame has treeless blocks across a group of 64)
    for level in (1, 3):
        for n in A_SIZES:
            out[f"A:l{level}:{n}"] = (zstcodec(logs[:n], level), logs[:n])
    b = big[:260000]
    out["B:flush1300"] = (stream(b, list(range(1300, len(b), 1300)), {P_LEVEL: 1}), b)
    c = big[:1 << 20]
    out["C:pledged"] = (compress2(c, {P_LEVEL: 3, P_TARGETCBLOCK: 1340}), c)
    out["C:streamed"] = (streamed(c, {P_LEVEL: 3, P_TARGETCBLOCK: 1340}), c)
    rng = np.random.default_rng(0x25D)
    head, mid = rng.integers(0, 256, 256 << 10, dtype=np.uint8).tobytes(), rng.integers(0, 256, 9 << 19, dtype=np.uint8).tobytes()
    d = head + mid + head
    out["D:far"] = (compress2(d, {P_LEVEL: 3, P_WLOG: 23}), d)
    out["D:far:checksum"] = (compress2(d, {P_LEVEL: 3, P_WLOG: 23, P_CHECKSUM: 1}), d)
    one, chk = big[5000:5000 + 300000], big[70000:70000 + 200000]
    parts = [out[f"A:l1:{A_SIZES[-1]}"][0], skippable(3, b"not for the decoder"), zs.compress(one, 3),
             compress2(chk, {P_LEVEL: 1, P_CHECKSUM: 1}), out["A:l1:0"][0]]
    out["E:concat"] = (b"".join(parts), logs + one + chk)
    f = b"\x5a" * 3000000
    out["F:rle"] = (zstcodec(f, 1), f)
    return out


def e_parts():
    """The offsets at which E's frames start, and its end."""
    img = inputs()["E:concat"][0]
    offs, at = [], 0
    while at < len(img):
        offs.append(at)
        at += find_frame_size(img, at)
    return offs + [len(img)]


def _block_offsets(image):
    """Offset of every block header of a one-frame image."""
    return [e["off"] - 3 for e in block_table(image)]


@functools.lru_cache(None)
def damaged():
    """[(class, label, image, base)]: the inputs G; `base` names the valid input the damage was done to."""
    I = inputs()
    E, B_, A = I["E:concat"][0], I["B:flush1300"][0], I[f"A:l1:{A_SIZES[-1]}"][0]
    out = []
    for k, o in enumerate(e_parts()[1:-1]):                          # at the boundary: a shorter valid file; 2 and 5 bytes behind it: not one
        for d in (0, 2, 5): out.append(("trunc_frame", f"E cut at frame {k + 1} + {d}", E[:o + d], "E:concat"))
    bo = _block_offsets(B_)
    for k in (63, 64, 65): out.append(("trunc_block", f"B cut at block {k}", B_[:bo[k]], "B:flush1300"))
    o = e_parts()[2]
    out.append(("magic", "E third frame's magic", E[:o] + bytes([E[o] ^ 0x40]) + E[o + 1:], "E:concat"))
    ao = _block_offsets(A)
    m = bytearray(A); m[ao[70]] |= 6
    out.append(("block_type", "A block 70 reserved type", bytes(m), f"A:l1:{A_SIZES[-1]}"))
    tab = block_table(A)
    # a flipped byte in an entropy stream need not fail: Huffman streams decode whatever bits they get and only their end is checked
    k = next(i for i, e in enumerate(tab) if i > 64 and e["type"] == 2 and e["ltype"] in (2, 3))
    for d in (200, 1000, tab[k]["lit_end"] - tab[k]["off"] - 1):     # inside the literals section; the last: the fourth stream's end mark
        m = bytearray(A); m[tab[k]["off"] + d] ^= 0x5A
        out.append(("huffman", f"A block {k} Huffman stream + {d}", bytes(m), f"A:l1:{A_SIZES[-1]}"))
    k = next(i for i, e in enumerate(tab) if i > 64 and e["type"] == 2 and e["nseq"] > 100)
    for d in (1, 40, 400):                                           # in front of the sequence bitstream's end mark
        m = bytearray(A); m[tab[k]["off"] + tab[k]["size"] - d] ^= 0x5A
        out.append(("sequences", f"A block {k} sequence bitstream - {d}", bytes(m), f"A:l1:{A_SIZES[-1]}"))
    out.append(("cut_block0", "B without block 0", B_[:bo[0]] + B_[bo[1]:], "B:flush1300"))
    D = I["D:far:checksum"][0]
    out.append(("checksum", "D wrong checksum", D[:-1] + bytes([D[-1] ^ 1]), "D:far:checksum"))
    small = I["A:l1:1"][0]
    for t in (1, 2, 3, 4): out.append(("trailing", f"{t} trailing bytes", small + b"\x00" * t, "A:l1:1"))
    out.append(("trailing", "a full bad magic", small + struct.pack("<I", 0xFD2FB529) + b"\x00" * 8, "A:l1:1"))
    return out


# ---------------------------------------------------------------------------------------------- fixture
# Two committed files (tests/golden/zst_*.zst), so that the device path's core runs without oracle/_ref: input B, a skippable frame,
# a checksum frame and the empty frame in one file, and input C streamed.  Their sources come from the corpus generator.
FIXTURES = ("zst_small.zst", "zst_blocks.zst")


def _fixture_sources():
    big = text(1 << 20)
    return {"zst_small.zst": big[:260000] + big[70000:70000 + 200000], "zst_blocks.zst": big}


def fixture_build():
    I = inputs()
    chk = text(1 << 20)[70000:70000 + 200000]
    small = b"".join([I["B:flush1300"][0], skippable(3, b"not for the decoder"), compress2(chk, {P_LEVEL: 1, P_CHECKSUM: 1}), I["A:l1:0"][0]])
    return {"zst_small.zst": small, "zst_blocks.zst": I["C:streamed"][0]}


def fixture():
    """name -> (image, source) from the committed files."""
    import os
    src = _fixture_sources()
    return {n: (open(os.path.join(zs.HERE, "golden", n), "rb").read(), src[n]) for n in FIXTURES}
