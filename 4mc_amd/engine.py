"""Device-resident calls: torch tensors are the HBM buffers, the C ABI does the work.

Mirrors the reference's per-block codec calls (LZ4_decompress_safe / LZ4_compress_default /
XXH32, native/4mc.c:301,311,637,661) in their batched form (include/fourmc_gpu.h).
"""
import ctypes as C

import numpy as np
import torch

from .binding import (ZST_REASONS, ZSTW_REASONS, ZstItem, ZstStatus, ZstwItem, ZstwStatus, BLOCK_DTYPE, BSTREAM_REASONS, BSTREAM_WRITE_REASONS, CODEC_LZ4_FAST, BstreamEncItem, BstreamItem, BstreamStatus, IMAGE_ENTRY_DTYPE, MAGIC_4MC, EngineError, ImageEncItem, ImageWrItem, LinesSrc, LinesPackItem, LinesWrItem, ImageIndexInfo, ImageItem, ImageLines, ImageLineInfo, ImageLinesAt, ImageRef, ImageSplitItem,
                      ImagesSlice, ImagesSplitItem,
                      ImageRange, ImageRecords, ImageSlice, ImageStatus, check, lib)


def _stream_ptr(stream):
    if stream is None:
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream)


def _ptr(t):
    assert t.is_cuda and t.is_contiguous()
    return int(t.data_ptr())


class DeviceBatch:
    """A descriptor array resident in HBM (n x struct fourmc_block)."""

    def __init__(self, blocks_np, device="cuda"):
        assert blocks_np.dtype == BLOCK_DTYPE
        self.n = len(blocks_np)
        raw = torch.from_numpy(np.ascontiguousarray(blocks_np).view(np.uint8).reshape(-1).copy())
        self.d = raw.to(device) if self.n else torch.empty(0, dtype=torch.uint8, device=device)

    def download(self):
        return self.d.cpu().numpy().view(BLOCK_DTYPE).copy()

    @property
    def ptr(self):
        return _ptr(self.d) if self.n else 0


def lz4_decompress(d_src, d_dst, batch, stream=None):
    """result[b] = LZ4_decompress_safe(src+src_off, dst+dst_off, src_len, dst_cap)."""
    check(lib().fourmc_gpu_lz4_decompress(_ptr(d_src), _ptr(d_dst), batch.ptr, batch.n, _stream_ptr(stream)),
          "fourmc_gpu_lz4_decompress")


def lz4_compress_hc(d_src, d_dst, batch, level, stream=None):
    """result[b] = LZ4_compress_HC(src+src_off, dst+dst_off, src_len, dst_cap, level)."""
    check(lib().fourmc_gpu_lz4_compress_hc(_ptr(d_src), _ptr(d_dst), batch.ptr, batch.n, level, _stream_ptr(stream)),
          "fourmc_gpu_lz4_compress_hc")


def lz4_compress_mc(d_src, d_dst, batch, stream=None):
    """result[b] = LZ4_compressMC_limitedOutput(...) (dst_cap 0xFFFFFFFF: LZ4_compressMC, unlimited)."""
    check(lib().fourmc_gpu_lz4_compress_mc(_ptr(d_src), _ptr(d_dst), batch.ptr, batch.n, _stream_ptr(stream)),
          "fourmc_gpu_lz4_compress_mc")


def zstd_decompress(d_src, d_dst, batch, stream=None):
    """result[b] = ZSTD_decompress(dst+dst_off, dst_cap, src+src_off, src_len) (negative on error)."""
    check(lib().fourmc_gpu_zstd_decompress(_ptr(d_src), _ptr(d_dst), batch.ptr, batch.n, _stream_ptr(stream)),
          "fourmc_gpu_zstd_decompress")


def zstd_compress(d_src, d_dst, batch, level=1, stream=None):
    """result[b] = ZSTD_compress(dst+dst_off, dst_cap, src+src_off, src_len, level) (-(error number) on error)."""
    check(lib().fourmc_gpu_zstd_compress(_ptr(d_src), _ptr(d_dst), batch.ptr, batch.n, level, _stream_ptr(stream)),
          "fourmc_gpu_zstd_compress")


def lz4_compress_fast(d_src, d_dst, batch, stream=None):
    """result[b] = LZ4_compress_default(src+src_off, dst+dst_off, src_len, dst_cap)."""
    check(lib().fourmc_gpu_lz4_compress_fast(_ptr(d_src), _ptr(d_dst), batch.ptr, batch.n, _stream_ptr(stream)),
          "fourmc_gpu_lz4_compress_fast")


def xxh32(d_src, batch, seed=0, stream=None):
    """xxh32[b] = XXH32(src+src_off, src_len, seed)."""
    check(lib().fourmc_gpu_xxh32(_ptr(d_src), batch.ptr, batch.n, seed, _stream_ptr(stream)), "fourmc_gpu_xxh32")


def encode_blocks(d_src, d_dst, batch, codec=CODEC_LZ4_FAST, level=0, stream=None):
    """One iteration of the reference's compress loop per block (native/4mc.c:301-329)."""
    check(lib().fourmc_gpu_4mc_encode_blocks(_ptr(d_src), _ptr(d_dst), batch.ptr, batch.n, codec, level,
                                             _stream_ptr(stream)), "fourmc_gpu_4mc_encode_blocks")


def decode_blocks(d_src, d_dst, batch, codec=CODEC_LZ4_FAST, stream=None):
    """One iteration of the reference's decode loop per block (native/4mc.c:603-668)."""
    check(lib().fourmc_gpu_4mc_decode_blocks(_ptr(d_src), _ptr(d_dst), batch.ptr, batch.n, codec,
                                             _stream_ptr(stream)), "fourmc_gpu_4mc_decode_blocks")


def pack_image(d_staging, d_image, batch, d_image_off, stream=None):
    """Block headers + payloads -> contiguous file image (native/4mc.c:309-315); d_image_off: int64/uint64 tensor."""
    check(lib().fourmc_gpu_4mc_pack_image(_ptr(d_staging), _ptr(d_image), batch.ptr, _ptr(d_image_off), batch.n,
                                          _stream_ptr(stream)), "fourmc_gpu_4mc_pack_image")


def release_workspaces():
    """Frees the device workspaces the engine keeps per stream (fourmc_gpu_release_workspaces); the next call allocates again."""
    check(lib().fourmc_gpu_release_workspaces(), "fourmc_gpu_release_workspaces")


def _dev_ptr(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype == torch.uint8):
        raise EngineError(f"{what}: a contiguous uint8 CUDA tensor is required")
    return int(t.data_ptr()) if t.numel() else 0


def image_bound(src_bytes):
    """Worst-case image size for src_bytes of input (fourmc_gpu_image_bound)."""
    return int(lib().fourmc_gpu_image_bound(int(src_bytes)))


def compress_image(d_src, d_image, magic=MAGIC_4MC, level=1, stream=None):
    """The whole .4mc / .4mz file of d_src into d_image (>= image_bound(d_src.numel()) bytes), as the CLI writes it at `level`.
    Returns the image length."""
    out = C.c_uint64(0)
    check(lib().fourmc_gpu_image_compress(_dev_ptr(d_src, "compress_image d_src"), d_src.numel(), _dev_ptr(d_image, "compress_image d_image"),
                                          d_image.numel(), C.byref(out), magic, level, _stream_ptr(stream)), "fourmc_gpu_image_compress")
    return int(out.value)


def compress_images(d_src, items, d_images, magic=MAGIC_4MC, level=1, src_bytes=None, images_bytes=None, stream=None):
    """Encode many sources of one buffer into many file images of one buffer with one call (fourmc_gpu_images_compress).  `items` is
    a sequence of (src_off, src_bytes, image_off, image_cap): input i is d_src[src_off:src_off + src_bytes] and its image goes to
    d_images[image_off:image_off + image_cap], image_cap >= image_bound(src_bytes).  src_bytes / images_bytes: how much of the two
    tensors the items may name (default: all of each).  Returns the list of image lengths, each what compress_image returns for
    that source alone, with the same bytes."""
    src = _dev_ptr(d_src, "compress_images d_src")
    dst = _dev_ptr(d_images, "compress_images d_images")
    total = d_src.numel() if src_bytes is None else int(src_bytes)
    cap = d_images.numel() if images_bytes is None else int(images_bytes)
    if total > d_src.numel() or cap > d_images.numel():
        raise EngineError("compress_images: %s beyond the tensor" % ("src_bytes" if total > d_src.numel() else "images_bytes"))
    q = [tuple(int(v) for v in it) for it in items]
    arr = (ImageEncItem * len(q))()
    for i, (so, sb, io, ic) in enumerate(q):
        arr[i].src_off, arr[i].src_bytes, arr[i].image_off, arr[i].image_cap = so, sb, io, ic
    check(lib().fourmc_gpu_images_compress(src, total, dst, cap, magic, level, C.cast(arr, C.c_void_p), len(q), _stream_ptr(stream)),
          "fourmc_gpu_images_compress")
    return [int(arr[i].image_bytes) for i in range(len(q))]


def image_parse_stats():
    """(fast, walk): images decompress_image has parsed so far with the footer-driven fast path and with the file-order walk."""
    f, w = C.c_ulonglong(0), C.c_ulonglong(0)
    lib().fourmc_gpu_image_parse_stats(C.byref(f), C.byref(w))
    return int(f.value), int(w.value)


def decompress_image(d_image, d_dst, magic=MAGIC_4MC, image_bytes=None, stream=None):
    """Decode the file image d_image[:image_bytes] (default: the whole tensor) into d_dst; d_dst None: parse only (size query).
    Returns the status as a dict; "message" is the CLI's text for the verdict."""
    n = d_image.numel() if image_bytes is None else int(image_bytes)
    if n > d_image.numel():
        raise EngineError("decompress_image: image_bytes beyond the tensor")
    st = ImageStatus()
    dst, cap = (0, 0) if d_dst is None else (_dev_ptr(d_dst, "decompress_image d_dst"), d_dst.numel())
    check(lib().fourmc_gpu_image_decompress(_dev_ptr(d_image, "decompress_image d_image"), n, dst, cap, magic, C.byref(st),
                                            _stream_ptr(stream)), "fourmc_gpu_image_decompress")
    res = {name: int(getattr(st, name)) for name, _ in ImageStatus._fields_}
    res["message"] = lib().fourmc_gpu_image_reason_text(st.reason).decode()
    return res


def decompress_images(d_images, items, d_dst, magic=MAGIC_4MC, images_bytes=None, stream=None):
    """Decode many file images of one buffer with one call (fourmc_gpu_images_decompress).  `items` is a sequence of
    (image_off, image_bytes, dst_off, dst_cap): image i is d_images[image_off:image_off + image_bytes] and its output region
    d_dst[dst_off:dst_off + dst_cap].  d_dst None: the size query (dst_off and dst_cap are ignored).  Returns one status dict per
    item, each what decompress_image returns for that image alone."""
    ptr = _dev_ptr(d_images, "decompress_images d_images")
    n = _image_len(d_images, images_bytes, "decompress_images")
    dst, cap = (0, 0) if d_dst is None else (_dev_ptr(d_dst, "decompress_images d_dst"), d_dst.numel())
    q = [tuple(int(v) for v in it) for it in items]
    arr = (ImageItem * len(q))()
    for i, (io, ib, do, dc) in enumerate(q):
        arr[i].image_off, arr[i].image_bytes, arr[i].dst_off, arr[i].dst_cap = io, ib, do, dc
    if d_dst is not None and dst == 0:          # an empty tensor has no address, and to the library NULL is the size query
        raise EngineError("decompress_images: d_dst is empty (None asks for the sizes)")
    check(lib().fourmc_gpu_images_decompress(ptr, n, dst, cap, magic, C.cast(arr, C.c_void_p), len(q), _stream_ptr(stream)),
          "fourmc_gpu_images_decompress")
    out = []
    for i in range(len(q)):
        st = arr[i].status
        res = {name: int(getattr(st, name)) for name, _ in ImageStatus._fields_}
        res["message"] = lib().fourmc_gpu_image_reason_text(st.reason).decode()
        out.append(res)
    return out


def bstream_max_input(codec=CODEC_LZ4_FAST):
    """M, the most input bytes one chunk of a Hadoop block stream holds (fourmc_gpu_bstream_max_input); 0 for an unknown codec."""
    return int(lib().fourmc_gpu_bstream_max_input(int(codec)))


def bstream_bound(src_bytes, codec=CODEC_LZ4_FAST, group_bytes=0):
    """Worst-case length of the block stream compress_bstream writes for src_bytes of input (fourmc_gpu_bstream_bound)."""
    return int(lib().fourmc_gpu_bstream_bound(int(src_bytes), int(codec), int(group_bytes)))


def compress_bstream(d_src, d_image, codec=CODEC_LZ4_FAST, level=0, group_bytes=0, stream=None):
    """d_src as the block stream one of the reference's eight raw codecs writes (fourmc_gpu_bstream_compress): groups of group_bytes
    of input (0: bstream_max_input(codec)), one chunk each.  (codec, level) as bstream_codec(ext) gives them.  d_image holds at
    least bstream_bound(d_src.numel(), codec, group_bytes) bytes.  Returns the stream's length."""
    out = C.c_uint64(0)
    check(lib().fourmc_gpu_bstream_compress(_dev_ptr(d_src, "compress_bstream d_src"), d_src.numel(), _dev_ptr(d_image, "compress_bstream d_image"),
                                            d_image.numel(), C.byref(out), int(codec), int(level), int(group_bytes), _stream_ptr(stream)),
          "fourmc_gpu_bstream_compress")
    return int(out.value)


def _writes_ptr(t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype in (torch.int32, torch.uint32)):
        raise EngineError("compress_bstreams d_writes: a contiguous int32 / uint32 CUDA tensor is required (the bits are read as uint32)")
    return int(t.data_ptr())


def bstream_writes_bound(src_bytes, codec=CODEC_LZ4_FAST):
    """A capacity that holds for the stream of EVERY schedule of write() calls over src_bytes (fourmc_gpu_bstream_writes_bound)."""
    return int(lib().fourmc_gpu_bstream_writes_bound(int(src_bytes), int(codec)))


def _compress_writes(who, item_cls, fn, mid, row, d_src, items, d_images, d_writes, src_total, images_bytes, stream):
    """What compress_bstreams and compress_images_writes share: the pointer and total checks, the write table, the images pointer,
    the item fill and the call of lib().<fn> with `mid` between the images and the items; row(item) is one entry of the result."""
    q = [tuple(int(v) for v in it) for it in items]
    src = 0 if d_src is None or d_src.numel() == 0 else _dev_ptr(d_src, f"{who} d_src")
    total = (0 if d_src is None else d_src.numel()) if src_total is None else int(src_total)
    if d_src is not None and total > d_src.numel():
        raise EngineError(f"{who}: src_total {total} lies beyond the tensor's {d_src.numel()} bytes")
    tab, ntab = 0, 0
    if d_writes is not None and d_writes.numel():
        tab, ntab = _writes_ptr(d_writes), d_writes.numel()
    img, cap = 0, 0
    if d_images is not None:
        img = _dev_ptr(d_images, f"{who} d_images")
        cap = _image_len(d_images, images_bytes, who)
        if img == 0:
            raise EngineError(f"{who}: d_images is empty (None asks for the sizes)")
    arr = (item_cls * max(len(q), 1))()
    for i, (so, sb, io, ic, wo, nw, wb) in enumerate(q):
        a = arr[i]
        a.src_off, a.src_bytes, a.image_off, a.image_cap, a.writes_off, a.n_writes, a.write_bytes = so, sb, io, ic, wo, nw, wb
    check(getattr(lib(), fn)(src, total, tab, ntab, img, cap, *mid, C.cast(arr, C.c_void_p), len(q), _stream_ptr(stream)), fn)
    return [dict(row(arr[i]), reason=int(arr[i].reason),
                 name=BSTREAM_WRITE_REASONS[arr[i].reason] if 0 <= arr[i].reason < len(BSTREAM_WRITE_REASONS) else "?")
            for i in range(len(q))]


def compress_bstreams(d_src, items, d_images, codec=CODEC_LZ4_FAST, level=0, d_writes=None, src_total=None, images_bytes=None, stream=None):
    """Write many block streams with one call, each shaped by its job's write() sizes (fourmc_gpu_bstreams_compress).  `items` is a
    sequence of (src_off, src_bytes, image_off, image_cap, writes_off, n_writes, write_bytes): n_writes entries of d_writes (a uint32
    or int32 CUDA tensor) from writes_off on are the stream's write sizes; n_writes 0 is the uniform schedule of write_bytes per
    write (0: one write of the whole source).  d_images None: the size query (image_bytes = the exact worst case of each schedule).
    Returns one dict per item: image_bytes, groups, chunks, reason (a FOURMC_BSW_* number) and "name" (its entry of
    BSTREAM_WRITE_REASONS)."""
    return _compress_writes("compress_bstreams", BstreamEncItem, "fourmc_gpu_bstreams_compress", (int(codec), int(level)),
                            lambda a: {"image_bytes": int(a.image_bytes), "groups": int(a.groups), "chunks": int(a.chunks)},
                            d_src, items, d_images, d_writes, src_total, images_bytes, stream)


def image_writes_bound(src_bytes):
    """A capacity that holds for the image of EVERY schedule of write() calls over src_bytes (fourmc_gpu_image_writes_bound)."""
    return int(lib().fourmc_gpu_image_writes_bound(int(src_bytes)))


def compress_images_writes(d_src, items, d_images, magic=MAGIC_4MC, level=1, d_writes=None, src_total=None, images_bytes=None, stream=None):
    """Write many .4mc / .4mz images with one call, each cut into blocks as Hadoop's FourMcOutputStream cuts it for its job's write()
    sizes (fourmc_gpu_images_compress_writes).  `items` is a sequence of (src_off, src_bytes, image_off, image_cap, writes_off,
    n_writes, write_bytes), as compress_bstreams takes them; `level` is compress_images' level.  d_images None: the size query
    (image_bytes = the exact worst case of each schedule).  Returns one dict per item: image_bytes, blocks, stored_blocks, reason (a
    FOURMC_BSW_* number) and "name" (its entry of BSTREAM_WRITE_REASONS)."""
    return _compress_writes("compress_images_writes", ImageWrItem, "fourmc_gpu_images_compress_writes", (int(magic), int(level)),
                            lambda a: {"image_bytes": int(a.image_bytes), "blocks": int(a.blocks), "stored_blocks": int(a.stored_blocks)},
                            d_src, items, d_images, d_writes, src_total, images_bytes, stream)


class LinesSource:
    """Lines in device memory, as the line readers hand them out (struct fourmc_lines_src).  `text`: a uint8 CUDA tensor of any
    shape; `text_len`: int32 / uint32, one entry per table line; `starts`: int64 offsets into text (image_read_lines' table), or
    None for rows of `row_bytes` (image_read_lines_at's; default: the row length of a two-dimensional text); `pick`: int64 table
    line numbers, or None for the table's own order.  table_lines defaults to text_len.numel(), text_bytes to text.numel()."""

    def __init__(self, text, text_len, starts=None, row_bytes=0, pick=None, text_bytes=None, table_lines=None):
        words = (torch.int32, getattr(torch, "uint32", torch.int32))

        def table(t, kinds, what):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype in kinds):
                raise EngineError(f"LinesSource {what}: a contiguous CUDA tensor of {' / '.join(str(k) for k in kinds)} is required")
            return t
        self.text = None if text is None else table(text, (torch.uint8,), "text")
        self.text_len = None if text_len is None else table(text_len, words, "text_len")
        self.starts = None if starts is None else table(starts, (torch.int64,), "starts")
        self.pick = None if pick is None else table(pick, (torch.int64,), "pick")
        if starts is None and not row_bytes and self.text is not None and self.text.dim() == 2:
            row_bytes = self.text.shape[1]
        self.row_bytes = int(row_bytes)
        self.text_bytes = (0 if self.text is None else self.text.numel()) if text_bytes is None else int(text_bytes)
        self.table_lines = (0 if self.text_len is None else self.text_len.numel()) if table_lines is None else int(table_lines)
        if self.text is not None and self.text_bytes > self.text.numel():
            raise EngineError("LinesSource: text_bytes lies beyond the text tensor")
        if any(t is not None and self.table_lines > t.numel() for t in (self.text_len, self.starts)):
            raise EngineError("LinesSource: table_lines lies beyond the tables")

    def struct(self):
        def at(t):
            return int(t.data_ptr()) if t is not None and t.numel() else None
        return LinesSrc(at(self.text), self.text_bytes, at(self.starts), self.row_bytes, at(self.text_len), self.table_lines,
                        at(self.pick), 0 if self.pick is None else self.pick.numel())


def _lines_src(src):
    return src if isinstance(src, LinesSource) else LinesSource(**src)


def _bsw_name(reason):
    return BSTREAM_WRITE_REASONS[reason] if 0 <= reason < len(BSTREAM_WRITE_REASONS) else "?"


def pack_lines(src, items, d_packed, d_writes=None, packed_total=None, stream=None):
    """Lines into the data and the write() sizes of a TextOutputFormat job (fourmc_gpu_lines_pack): for every item text_0 LF text_1
    LF ... at d_packed[packed_off:] and the sizes len_0, 1, len_1, 1, ... at d_writes[writes_off:], ready for compress_images_writes,
    compress_bstreams or compress_zsts.  `src`: a LinesSource, or a dict of its arguments; `items`: a sequence of (line_off, n_lines,
    packed_off, packed_cap, writes_off); d_writes: an int32 / uint32 CUDA tensor.  d_packed None: the size query.  Returns one dict
    per item: packed_bytes, reason (a FOURMC_BSW_* number) and "name" (its entry of BSTREAM_WRITE_REASONS)."""
    s = _lines_src(src).struct()
    q = [tuple(int(v) for v in it) for it in items]
    dst, cap, tab, ntab = 0, 0, 0, 0
    if d_packed is not None:
        dst = _dev_ptr(d_packed, "pack_lines d_packed")
        cap = _image_len(d_packed, packed_total, "pack_lines")
        if dst == 0:
            raise EngineError("pack_lines: d_packed is empty (None asks for the sizes)")
    if d_writes is not None and d_writes.numel():
        tab, ntab = _writes_ptr(d_writes), d_writes.numel()
    arr = (LinesPackItem * max(len(q), 1))()
    for i, (lo, nl, po, pc, wo) in enumerate(q):
        a = arr[i]
        a.line_off, a.n_lines, a.packed_off, a.packed_cap, a.writes_off = lo, nl, po, pc, wo
    check(lib().fourmc_gpu_lines_pack(C.byref(s), dst, cap, tab, ntab, C.cast(arr, C.c_void_p), len(q), _stream_ptr(stream)), "fourmc_gpu_lines_pack")
    return [{"packed_bytes": int(arr[i].packed_bytes), "reason": int(arr[i].reason), "name": _bsw_name(arr[i].reason)} for i in range(len(q))]


def _write_lines(who, fn, mid, src, items, d_images, images_bytes, stream):
    s = _lines_src(src).struct()
    q = [tuple(int(v) for v in it) for it in items]
    img, cap = 0, 0
    if d_images is not None:
        img = _dev_ptr(d_images, f"{who} d_images")
        cap = _image_len(d_images, images_bytes, who)
        if img == 0:
            raise EngineError(f"{who}: d_images is empty (None asks for the sizes)")
    arr = (LinesWrItem * max(len(q), 1))()
    for i, (lo, nl, io, ic) in enumerate(q):
        a = arr[i]
        a.line_off, a.n_lines, a.image_off, a.image_cap = lo, nl, io, ic
    check(getattr(lib(), fn)(C.byref(s), img, cap, *mid, C.cast(arr, C.c_void_p), len(q), _stream_ptr(stream)), fn)
    return [{"text_bytes": int(arr[i].text_bytes), "image_bytes": int(arr[i].image_bytes), "blocks": int(arr[i].blocks),
             "stored_blocks": int(arr[i].stored_blocks), "reason": int(arr[i].reason), "name": _bsw_name(arr[i].reason)} for i in range(len(q))]


def write_lines_images(src, items, d_images, magic=MAGIC_4MC, level=1, images_bytes=None, stream=None):
    """Lines as the .4mc / .4mz part files of a TextOutputFormat job, many per call (fourmc_gpu_images_write_lines): each item's image
    is what compress_images_writes writes for the lines' text with a newline behind each and two write() calls per line.  `src`: a
    LinesSource or a dict of its arguments; `items`: a sequence of (line_off, n_lines, image_off, image_cap); `level`:
    compress_images' level.  d_images None: the size query.  Returns one dict per item: text_bytes, image_bytes, blocks,
    stored_blocks, reason (a FOURMC_BSW_* number) and "name" (its entry of BSTREAM_WRITE_REASONS)."""
    return _write_lines("write_lines_images", "fourmc_gpu_images_write_lines", (int(magic), int(level)), src, items, d_images, images_bytes, stream)


def write_lines_bstreams(src, items, d_images, codec=CODEC_LZ4_FAST, level=0, images_bytes=None, stream=None):
    """Lines as the Lz4Codec / ZstdCodec part files of a TextOutputFormat job, many per call (fourmc_gpu_bstreams_write_lines): as
    write_lines_images, over compress_bstreams; (codec, level) as bstream_codec(ext) gives them.  `blocks` counts the chunks."""
    return _write_lines("write_lines_bstreams", "fourmc_gpu_bstreams_write_lines", (int(codec), int(level)), src, items, d_images, images_bytes, stream)


def _bstream_dict(st):
    res = {name: int(getattr(st, name)) for name, _ in BstreamStatus._fields_ if name != "pad"}
    res["name"] = BSTREAM_REASONS[st.reason] if 0 <= st.reason < len(BSTREAM_REASONS) else "?"
    res["message"] = lib().fourmc_gpu_bstream_reason_text(st.reason).decode()
    return res


def decompress_bstream(d_image, d_dst, codec=CODEC_LZ4_FAST, image_bytes=None, stream=None):
    """Decode the block stream d_image[:image_bytes] (default: the whole tensor) into d_dst; d_dst None: the size query.  `codec`
    selects the family (any LZ4 selector, or CODEC_ZSTD).  Returns the status as a dict: decoded_bytes, total_bytes, fail_offset,
    groups, chunks, reason (a FOURMC_BS_* number), "name" (its entry of BSTREAM_REASONS) and "message"."""
    n = _image_len(d_image, image_bytes, "decompress_bstream")
    st = BstreamStatus()
    dst, cap = (0, 0) if d_dst is None else (_dev_ptr(d_dst, "decompress_bstream d_dst"), d_dst.numel())
    if d_dst is not None and dst == 0:          # an empty tensor has no address, and to the library NULL is the size query
        raise EngineError("decompress_bstream: d_dst is empty (None asks for the size)")
    check(lib().fourmc_gpu_bstream_decompress(_dev_ptr(d_image, "decompress_bstream d_image"), n, dst, cap, int(codec), C.byref(st),
                                              _stream_ptr(stream)), "fourmc_gpu_bstream_decompress")
    return _bstream_dict(st)


def decompress_bstreams(d_images, items, d_dst, codec=CODEC_LZ4_FAST, images_bytes=None, stream=None):
    """Decode many block streams of one buffer with one call (fourmc_gpu_bstreams_decompress).  `items` is a sequence of
    (image_off, image_bytes, dst_off, dst_cap); d_dst None: the size query.  Returns one status dict per item, each what
    decompress_bstream returns for that stream alone."""
    ptr = _dev_ptr(d_images, "decompress_bstreams d_images")
    n = _image_len(d_images, images_bytes, "decompress_bstreams")
    dst, cap = (0, 0) if d_dst is None else (_dev_ptr(d_dst, "decompress_bstreams d_dst"), d_dst.numel())
    if d_dst is not None and dst == 0:
        raise EngineError("decompress_bstreams: d_dst is empty (None asks for the sizes)")
    q = [tuple(int(v) for v in it) for it in items]
    arr = (BstreamItem * max(len(q), 1))()
    for i, (io, ib, do, dc) in enumerate(q):
        arr[i].image_off, arr[i].image_bytes, arr[i].dst_off, arr[i].dst_cap = io, ib, do, dc
    check(lib().fourmc_gpu_bstreams_decompress(ptr, n, dst, cap, int(codec), C.cast(arr, C.c_void_p), len(q), _stream_ptr(stream)),
          "fourmc_gpu_bstreams_decompress")
    return [_bstream_dict(arr[i].status) for i in range(len(q))]


def _zst_dict(st):
    res = {name: int(getattr(st, name)) for name, _ in ZstStatus._fields_ if name != "pad"}
    res["name"] = ZST_REASONS[st.reason] if 0 <= st.reason < len(ZST_REASONS) else "?"
    res["message"] = lib().fourmc_gpu_zst_reason_text(st.reason).decode()
    return res


def decompress_zst(d_image, d_dst=None, image_bytes=None, stream=None):
    """Decode the .zst file d_image[:image_bytes] (default: the whole tensor) into d_dst (fourmc_gpu_zst_decompress); d_dst None:
    the size query.  Returns the status as a dict: decoded_bytes, total_bytes, fail_offset, frames, skippable, blocks, reason (a
    FOURMC_ZST_* number), codec_result, "name" (its entry of ZST_REASONS) and "message"."""
    n = _image_len(d_image, image_bytes, "decompress_zst")
    st = ZstStatus()
    dst, cap = (0, 0) if d_dst is None else (_dev_ptr(d_dst, "decompress_zst d_dst"), d_dst.numel())
    if d_dst is not None and dst == 0:          # an empty tensor has no address, and to the library NULL is the size query
        raise EngineError("decompress_zst: d_dst is empty (None asks for the size)")
    check(lib().fourmc_gpu_zst_decompress(_dev_ptr(d_image, "decompress_zst d_image"), n, dst, cap, C.byref(st), _stream_ptr(stream)),
          "fourmc_gpu_zst_decompress")
    return _zst_dict(st)


def decompress_zsts(d_images, items, d_dst, images_bytes=None, stream=None):
    """Decode many .zst files of one buffer with one call (fourmc_gpu_zsts_decompress).  `items` is a sequence of
    (image_off, image_bytes, dst_off, dst_cap); d_dst None: the size query.  Returns one status dict per item, each what
    decompress_zst returns for that file alone."""
    ptr = _dev_ptr(d_images, "decompress_zsts d_images")
    n = _image_len(d_images, images_bytes, "decompress_zsts")
    dst, cap = (0, 0) if d_dst is None else (_dev_ptr(d_dst, "decompress_zsts d_dst"), d_dst.numel())
    if d_dst is not None and dst == 0:
        raise EngineError("decompress_zsts: d_dst is empty (None asks for the sizes)")
    q = [tuple(int(v) for v in it) for it in items]
    arr = (ZstItem * max(len(q), 1))()
    for i, (io, ib, do, dc) in enumerate(q):
        arr[i].image_off, arr[i].image_bytes, arr[i].dst_off, arr[i].dst_cap = io, ib, do, dc
    check(lib().fourmc_gpu_zsts_decompress(ptr, n, dst, cap, C.cast(arr, C.c_void_p), len(q), _stream_ptr(stream)), "fourmc_gpu_zsts_decompress")
    return [_zst_dict(arr[i].status) for i in range(len(q))]


def zst_stats():
    """{"fast_frames", "serial_frames", "fast_blocks"} of the .zst decodes since the last call on this device (fourmc_gpu_zst_stats)."""
    c = (C.c_ulonglong * 3)()
    lib().fourmc_gpu_zst_stats(C.byref(c, 0), C.byref(c, 8), C.byref(c, 16))
    return {"fast_frames": int(c[0]), "serial_frames": int(c[1]), "fast_blocks": int(c[2])}


def zst_bound(n):
    """Capacity that holds the .zst image of every source of n bytes (fourmc_gpu_zst_bound)."""
    return int(lib().fourmc_gpu_zst_bound(int(n)))


def zst_codec_level(v):
    """The level ZstCodec hands to zstd for a configured io.compress.zst.compression.level of v (fourmc_zst_codec_level)."""
    return int(lib().fourmc_zst_codec_level(int(v)))


def _zstw_dict(st):
    res = {name: int(getattr(st, name)) for name, _ in ZstwStatus._fields_ if name != "pad"}
    res["name"] = ZSTW_REASONS[st.reason] if 0 <= st.reason < len(ZSTW_REASONS) else "?"
    res["message"] = lib().fourmc_gpu_zstw_reason_text(st.reason).decode()
    return res


def compress_zst(d_src, d_image, level=1, src_bytes=None, stream=None):
    """Write the .zst file of d_src[:src_bytes] (default: the whole tensor) into d_image, whose length is the capacity
    (fourmc_gpu_zst_compress): the bytes of ZSTD_initCStream(level), ZSTD_compressStream, ZSTD_endStream.  Returns the status as a
    dict: image_bytes, blocks, reason (a FOURMC_ZSTW_* number), codec_result, "name" (its entry of ZSTW_REASONS) and "message"."""
    n = _image_len(d_src, src_bytes, "compress_zst")
    st = ZstwStatus()
    src = _dev_ptr(d_src, "compress_zst d_src") if d_src.numel() else 0
    check(lib().fourmc_gpu_zst_compress(src, n, _dev_ptr(d_image, "compress_zst d_image"), d_image.numel(), int(level), C.byref(st),
                                        _stream_ptr(stream)), "fourmc_gpu_zst_compress")
    return _zstw_dict(st)


def compress_zsts(d_src, items, d_images, src_total=None, stream=None):
    """Write many .zst files with one call (fourmc_gpu_zsts_compress).  `items` is a sequence of (src_off, src_bytes, image_off,
    image_cap, level); levels may differ.  Returns one status dict per item, each what compress_zst returns for that stream alone."""
    n = _image_len(d_src, src_total, "compress_zsts")
    src = _dev_ptr(d_src, "compress_zsts d_src") if d_src.numel() else 0
    q = [tuple(int(v) for v in it) for it in items]
    arr = (ZstwItem * max(len(q), 1))()
    for i, (so, sb, io, ic, lv) in enumerate(q):
        arr[i].src_off, arr[i].src_bytes, arr[i].image_off, arr[i].image_cap, arr[i].level = so, sb, io, ic, lv
    check(lib().fourmc_gpu_zsts_compress(src, n, _dev_ptr(d_images, "compress_zsts d_images"), d_images.numel(), C.cast(arr, C.c_void_p),
                                         len(q), _stream_ptr(stream)), "fourmc_gpu_zsts_compress")
    return [_zstw_dict(arr[i].status) for i in range(len(q))]


def _image_len(d_image, image_bytes, what):
    n = d_image.numel() if image_bytes is None else int(image_bytes)
    if n > d_image.numel():
        raise EngineError(f"{what}: image_bytes beyond the tensor")
    return n


def image_index(d_image, image_bytes=None, stream=None):
    """The footer index of the single-stream image d_image[:image_bytes] (default: the whole tensor), built on the device.
    Returns (info, entries): info as a dict (nblocks, framing, total_bytes, is_zstd: the file API's answers for the same bytes)
    and the entries (image_off, data_off, usize, csize, xxh32) as a numpy structured array of nblocks rows."""
    ptr = _dev_ptr(d_image, "image_index d_image")
    n = _image_len(d_image, image_bytes, "image_index")
    info = ImageIndexInfo()
    check(lib().fourmc_gpu_image_index(ptr, n, 0, 0, C.byref(info), _stream_ptr(stream)), "fourmc_gpu_image_index")
    k = max(int(info.nblocks), 0)
    ent = np.zeros(k, dtype=IMAGE_ENTRY_DTYPE)
    if k:
        d_ent = torch.empty(k * IMAGE_ENTRY_DTYPE.itemsize, dtype=torch.uint8, device=d_image.device)
        check(lib().fourmc_gpu_image_index(ptr, n, _ptr(d_ent), k, C.byref(info), _stream_ptr(stream)), "fourmc_gpu_image_index")
        ent = d_ent.cpu().numpy().view(IMAGE_ENTRY_DTYPE).copy()
    res = {name: int(getattr(info, name)) for name, _ in ImageIndexInfo._fields_ if name != "pad"}
    return res, ent


def image_decode_blocks(d_image, first, count, d_dst, image_bytes=None, stream=None):
    """Blocks [first, first+count) of the image into d_dst (fourmc_file_decode_blocks on the device).  Returns what the file
    function returns for the same bytes: the decoded bytes, or -1 / -2 / -3 / -4 / -5."""
    ptr = _dev_ptr(d_image, "image_decode_blocks d_image")
    dst = _dev_ptr(d_dst, "image_decode_blocks d_dst")
    n = _image_len(d_image, image_bytes, "image_decode_blocks")
    out = C.c_int64(0)
    check(lib().fourmc_gpu_image_decode_blocks(ptr, n, int(first), int(count), dst, d_dst.numel(), C.byref(out), _stream_ptr(stream)),
          "fourmc_gpu_image_decode_blocks")
    return int(out.value)


def image_read(d_image, ranges, d_dst, image_bytes=None, stream=None):
    """Decoded byte ranges of the image: `ranges` is a sequence of (offset, length, dst_off); range i writes the content's bytes
    [offset, offset+length) to d_dst[dst_off:].  Returns an int64 numpy array of the per-range results (length, 0, the index
    code, -3, -5 or -4; include/fourmc_gpu.h)."""
    ptr = _dev_ptr(d_image, "image_read d_image")
    dst = _dev_ptr(d_dst, "image_read d_dst")
    n = _image_len(d_image, image_bytes, "image_read")
    q = np.asarray(ranges, dtype=np.uint64).reshape(-1, 3)
    arr = (ImageRange * len(q))()
    for i, (o, ln, d) in enumerate(q.tolist()):
        arr[i].offset, arr[i].length, arr[i].dst_off, arr[i].result = o, ln, d, 0
    check(lib().fourmc_gpu_image_read(ptr, n, C.cast(arr, C.c_void_p), len(q), dst, d_dst.numel(), _stream_ptr(stream)), "fourmc_gpu_image_read")
    return np.array([arr[i].result for i in range(len(q))], dtype=np.int64)


def image_align_slices(d_image, slices, image_bytes=None, stream=None):
    """Raw byte slices [(start, end), ...] of the image file, as FileInputFormat cuts them, aligned to block headers on the device
    (FourMcInputFormat.getSplits' inner step).  Returns one dict per slice: start, end, split_start, split_end, first_block,
    block_count and result (1 kept, 0 dropped, or the index code of an image that cannot be indexed)."""
    ptr = _dev_ptr(d_image, "image_align_slices d_image")
    n = _image_len(d_image, image_bytes, "image_align_slices")
    q = np.asarray(slices, dtype=np.uint64).reshape(-1, 2)
    arr = (ImageSlice * len(q))()
    for i, (a, z) in enumerate(q.tolist()):
        arr[i].start, arr[i].end = a, z
    check(lib().fourmc_gpu_image_align_slices(ptr, n, C.cast(arr, C.c_void_p), len(q), _stream_ptr(stream)), "fourmc_gpu_image_align_slices")
    return [{name: int(getattr(arr[i], name)) for name, _ in ImageSlice._fields_} for i in range(len(q))]


def image_read_records(d_image, split_start, split_end, d_dst, starts=None, delim=10, image_bytes=None, stream=None):
    """The records (lines ending with the byte `delim`) that the split [split_start, split_end) of the image owns by the line
    reader's rule: d_dst[:data_bytes] receives the decoded content from the split's first block on, `starts` (an int64 CUDA tensor,
    or None to count only) the offset in d_dst of each record and, behind the last, data_bytes.  Returns the ImageRecords struct
    (result: the records owned, or a negative code; include/fourmc_gpu.h)."""
    ptr = _dev_ptr(d_image, "image_read_records d_image")
    dst = _dev_ptr(d_dst, "image_read_records d_dst")
    n = _image_len(d_image, image_bytes, "image_read_records")
    sp, cap = 0, 0
    if starts is not None:
        if not (isinstance(starts, torch.Tensor) and starts.is_cuda and starts.is_contiguous() and starts.dtype == torch.int64):
            raise EngineError("image_read_records starts: a contiguous int64 CUDA tensor is required")
        sp, cap = int(starts.data_ptr()), starts.numel()
    out = ImageRecords()
    check(lib().fourmc_gpu_image_read_records(ptr, n, int(split_start), int(split_end), int(delim) & 0xFF, dst, d_dst.numel(), sp, cap,
                                              C.byref(out), _stream_ptr(stream)), "fourmc_gpu_image_read_records")
    return out


def image_read_lines(d_image, split_start, split_end, d_dst, starts=None, text_len=None, max_line_len=0x7FFFFFFF, image_bytes=None,
                     stream=None):
    """The lines that the split [split_start, split_end) of the image owns, cut as Hadoop's default LineReader cuts them: LF, a
    lone CR and CR LF end a line.  d_dst[:data_bytes] receives the decoded content from the split's first block on, `starts` (an
    int64 CUDA tensor) the offset in d_dst of each line and, behind the last, data_bytes, `text_len` (an int32 or uint32 CUDA
    tensor) each line's length without its terminator, cut at max_line_len.  Both tables or neither (count only); `starts` needs
    one entry more than there are lines, `text_len` one per line.  Returns the ImageLines struct (result: the lines owned, or a
    negative code; include/fourmc_gpu.h)."""
    ptr = _dev_ptr(d_image, "image_read_lines d_image")
    dst = _dev_ptr(d_dst, "image_read_lines d_dst")
    n = _image_len(d_image, image_bytes, "image_read_lines")
    if (starts is None) != (text_len is None):
        raise EngineError("image_read_lines: starts and text_len go together (both None: count only)")
    if not 0 <= int(max_line_len) <= 0x7FFFFFFF:
        raise EngineError("image_read_lines max_line_len: 0 .. 0x7FFFFFFF")
    sp, tp, cap = 0, 0, 0
    if starts is not None:
        if not (isinstance(starts, torch.Tensor) and starts.is_cuda and starts.is_contiguous() and starts.dtype == torch.int64):
            raise EngineError("image_read_lines starts: a contiguous int64 CUDA tensor is required")
        words = (torch.int32, getattr(torch, "uint32", torch.int32))
        if not (isinstance(text_len, torch.Tensor) and text_len.is_cuda and text_len.is_contiguous() and text_len.dtype in words):
            raise EngineError("image_read_lines text_len: a contiguous int32 or uint32 CUDA tensor is required")
        # the call writes text_len[0, lines) only, so a table of one entry per line serves lines_cap = its size + 1
        sp, tp, cap = int(starts.data_ptr()), int(text_len.data_ptr()), min(starts.numel(), text_len.numel() + 1)
    out = ImageLines()
    check(lib().fourmc_gpu_image_read_lines(ptr, n, int(split_start), int(split_end), int(max_line_len), dst, d_dst.numel(), sp, tp, cap,
                                            C.byref(out), _stream_ptr(stream)), "fourmc_gpu_image_read_lines")
    return out


_SPLIT_KEYS = ("split_start", "split_end", "dst_off", "dst_cap", "table_off", "lines_cap")


def image_read_lines_batch(d_image, splits, d_dst, starts=None, text_len=None, max_line_len=0x7FFFFFFF, image_bytes=None, stream=None):
    """image_read_lines for many splits of one image with one call (fourmc_gpu_image_read_lines_batch).  `splits` is a sequence of
    (split_start, split_end, dst_off, dst_cap, table_off, lines_cap) tuples, or of dicts with those keys (table_off and lines_cap
    default to 0): split i's content goes to d_dst[dst_off:dst_off + dst_cap] and its tables are starts[table_off:table_off +
    lines_cap] and text_len[table_off:table_off + lines_cap], the starts being offsets in the split's own region.  Both tables or
    neither (count only).  Returns one dict per split with the fields of ImageLines (result, base, data_off, data_bytes, reserved),
    each what image_read_lines returns for that split with those regions."""
    ptr = _dev_ptr(d_image, "image_read_lines_batch d_image")
    dst = _dev_ptr(d_dst, "image_read_lines_batch d_dst")
    n = _image_len(d_image, image_bytes, "image_read_lines_batch")
    if (starts is None) != (text_len is None):
        raise EngineError("image_read_lines_batch: starts and text_len go together (both None: count only)")
    if not 0 <= int(max_line_len) <= 0x7FFFFFFF:
        raise EngineError("image_read_lines_batch max_line_len: 0 .. 0x7FFFFFFF")
    sp, tp, entries = 0, 0, 0
    if starts is not None:
        if not (isinstance(starts, torch.Tensor) and starts.is_cuda and starts.is_contiguous() and starts.dtype == torch.int64):
            raise EngineError("image_read_lines_batch starts: a contiguous int64 CUDA tensor is required")
        words = (torch.int32, getattr(torch, "uint32", torch.int32))
        if not (isinstance(text_len, torch.Tensor) and text_len.is_cuda and text_len.is_contiguous() and text_len.dtype in words):
            raise EngineError("image_read_lines_batch text_len: a contiguous int32 or uint32 CUDA tensor is required")
        # a split's region of text_len is read and written one entry short of its lines_cap, as in image_read_lines
        sp, tp, entries = int(starts.data_ptr()), int(text_len.data_ptr()), min(starts.numel(), text_len.numel() + 1)
    rows = [tuple(int(q.get(k, 0)) for k in _SPLIT_KEYS) if isinstance(q, dict) else tuple(int(v) for v in q) for q in splits]
    arr = (ImageSplitItem * len(rows))()
    for i, row in enumerate(rows):
        if len(row) != 6:
            raise EngineError("image_read_lines_batch splits: (split_start, split_end, dst_off, dst_cap, table_off, lines_cap) each")
        (arr[i].split_start, arr[i].split_end, arr[i].dst_off, arr[i].dst_cap, arr[i].table_off, arr[i].lines_cap) = row
    check(lib().fourmc_gpu_image_read_lines_batch(ptr, n, int(max_line_len), dst, d_dst.numel(), sp, tp, entries, C.cast(arr, C.c_void_p),
                                                  len(rows), _stream_ptr(stream)), "fourmc_gpu_image_read_lines_batch")
    return [{name: int(getattr(arr[i].out, name)) for name, _ in ImageLines._fields_} for i in range(len(rows))]


def image_lines_batch_stats():
    """(groups, tail_rounds, block_decodes) image_read_lines_batch has processed, run and made so far in this process."""
    g, r, d = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
    lib().fourmc_gpu_image_lines_batch_stats(C.byref(g), C.byref(r), C.byref(d))
    return int(g.value), int(r.value), int(d.value)


def image_line_index(d_image, image_bytes=None, stream=None):
    """The line index of the single-stream image d_image[:image_bytes] (fourmc_gpu_image_line_index): the whole image is decoded
    once, in groups, and nothing of it is kept.  Returns (index, info): the index as an int64 CUDA tensor of shape [nblocks + 1, 2]
    (16 bytes an entry: ends_before, then ends and flags; view its bytes through IMAGE_LINE_ENTRY_DTYPE on the host), None when
    the image cannot be indexed or a block is damaged; info as a dict (result, lines, ends, total_bytes, nblocks)."""
    ptr = _dev_ptr(d_image, "image_line_index d_image")
    n = _image_len(d_image, image_bytes, "image_line_index")
    head = ImageIndexInfo()
    check(lib().fourmc_gpu_image_index(ptr, n, 0, 0, C.byref(head), _stream_ptr(stream)), "fourmc_gpu_image_index")
    entries = max(int(head.nblocks), 0) + 1
    index = torch.zeros((entries, 2), dtype=torch.int64, device=d_image.device)
    info = ImageLineInfo()
    check(lib().fourmc_gpu_image_line_index(ptr, n, _ptr(index), entries, C.byref(info), _stream_ptr(stream)), "fourmc_gpu_image_line_index")
    res = {name: int(getattr(info, name)) for name, _ in ImageLineInfo._fields_ if name != "pad"}
    return (index if res["result"] == 0 else None), res


def image_read_lines_at(d_image, index, d_lines, row_bytes, max_line_len=0x7FFFFFFF, pad=0, image_bytes=None, stream=None):
    """Lines by their numbers (fourmc_gpu_image_read_lines_at): `index` is image_line_index's tensor, `d_lines` an int64 CUDA tensor
    of line numbers (it never visits the host; duplicates are fine).  Only the blocks those lines touch are decoded.  Returns a dict:
    rows, a uint8 tensor [n, row_bytes] (row i: the first min(text_len[i], row_bytes) bytes of line d_lines[i]'s text, then `pad`);
    text_len (int32: the text's length cut at max_line_len, so text_len > row_bytes says the row is a prefix); status (int32: 1
    written, -3 no such line, -4 a block the line needs is damaged); out, the call's struct as a dict (result, served,
    blocks_staged, rounds)."""
    ptr = _dev_ptr(d_image, "image_read_lines_at d_image")
    nbytes = _image_len(d_image, image_bytes, "image_read_lines_at")
    if not (isinstance(index, torch.Tensor) and index.is_cuda and index.is_contiguous() and index.dtype == torch.int64 and index.dim() == 2
            and index.shape[1] == 2):
        raise EngineError("image_read_lines_at index: image_line_index's int64 CUDA tensor of shape [nblocks + 1, 2] is required")
    if not (isinstance(d_lines, torch.Tensor) and d_lines.is_cuda and d_lines.is_contiguous() and d_lines.dtype == torch.int64 and d_lines.dim() == 1):
        raise EngineError("image_read_lines_at d_lines: a contiguous one-dimensional int64 CUDA tensor is required")
    if not 1 <= int(row_bytes) <= 0xFFFFFFFF:
        raise EngineError("image_read_lines_at row_bytes: 1 .. 0xFFFFFFFF")
    if not 0 <= int(max_line_len) <= 0x7FFFFFFF:
        raise EngineError("image_read_lines_at max_line_len: 0 .. 0x7FFFFFFF")
    n = d_lines.numel()
    if n > 0xFFFFFFFF:
        raise EngineError("image_read_lines_at d_lines: at most 0xFFFFFFFF requests")
    rows = torch.empty((n, int(row_bytes)), dtype=torch.uint8, device=d_image.device)
    text_len = torch.empty(n, dtype=torch.int32, device=d_image.device)
    status = torch.empty(n, dtype=torch.int32, device=d_image.device)
    out = ImageLinesAt()
    check(lib().fourmc_gpu_image_read_lines_at(ptr, nbytes, _ptr(index), index.shape[0], _ptr(d_lines) if n else 0, n, int(max_line_len),
                                               _ptr(rows) if n else 0, int(row_bytes), int(pad) & 0xFF, _ptr(text_len) if n else 0,
                                               _ptr(status) if n else 0, C.byref(out), _stream_ptr(stream)), "fourmc_gpu_image_read_lines_at")
    return {"rows": rows, "text_len": text_len, "status": status,
            "out": {name: int(getattr(out, name)) for name, _ in ImageLinesAt._fields_}}


def image_lines_at_stats():
    """(rounds, block_decodes, blocks_staged) image_read_lines_at has run, made and staged so far in this process."""
    r, d, b = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
    lib().fourmc_gpu_image_lines_at_stats(C.byref(r), C.byref(d), C.byref(b))
    return int(r.value), int(d.value), int(b.value)


def _image_refs(images, who):
    refs = [tuple(int(v) for v in im) for im in images]
    arr = (ImageRef * max(len(refs), 1))()
    for k, im in enumerate(refs):
        if len(im) != 2:
            raise EngineError("%s images: (image_off, image_bytes) each" % who)
        arr[k].image_off, arr[k].image_bytes = im
    return arr, len(refs)


def images_read_lines(d_images, images, splits, d_dst, starts=None, text_len=None, max_line_len=0x7FFFFFFF, images_bytes=None, stream=None):
    """image_read_lines_batch for the splits of many images that lie in one device buffer (fourmc_gpu_images_read_lines).  `images`
    is a sequence of (image_off, image_bytes), `splits` a sequence of (image, split_start, split_end, dst_off, dst_cap, table_off,
    lines_cap) with `image` an index into `images` and the split offsets counted in that image.  The regions, the tables and the
    returned dicts (one per split) are image_read_lines_batch's; .4mc and .4mz images may be mixed, and an image that cannot be
    indexed gives only its own splits the index code."""
    ptr = _dev_ptr(d_images, "images_read_lines d_images")
    dst = _dev_ptr(d_dst, "images_read_lines d_dst")
    n = _image_len(d_images, images_bytes, "images_read_lines")
    if (starts is None) != (text_len is None):
        raise EngineError("images_read_lines: starts and text_len go together (both None: count only)")
    if not 0 <= int(max_line_len) <= 0x7FFFFFFF:
        raise EngineError("images_read_lines max_line_len: 0 .. 0x7FFFFFFF")
    sp, tp, entries = 0, 0, 0
    if starts is not None:
        if not (isinstance(starts, torch.Tensor) and starts.is_cuda and starts.is_contiguous() and starts.dtype == torch.int64):
            raise EngineError("images_read_lines starts: a contiguous int64 CUDA tensor is required")
        words = (torch.int32, getattr(torch, "uint32", torch.int32))
        if not (isinstance(text_len, torch.Tensor) and text_len.is_cuda and text_len.is_contiguous() and text_len.dtype in words):
            raise EngineError("images_read_lines text_len: a contiguous int32 or uint32 CUDA tensor is required")
        sp, tp, entries = int(starts.data_ptr()), int(text_len.data_ptr()), min(starts.numel(), text_len.numel() + 1)
    refs, nimages = _image_refs(images, "images_read_lines")
    rows = [tuple(int(v) for v in q) for q in splits]
    arr = (ImagesSplitItem * max(len(rows), 1))()
    for i, row in enumerate(rows):
        if len(row) != 7:
            raise EngineError("images_read_lines splits: (image, split_start, split_end, dst_off, dst_cap, table_off, lines_cap) each")
        (arr[i].image, arr[i].split_start, arr[i].split_end, arr[i].dst_off, arr[i].dst_cap, arr[i].table_off, arr[i].lines_cap) = row
    check(lib().fourmc_gpu_images_read_lines(ptr, n, C.cast(refs, C.c_void_p), nimages, int(max_line_len), dst, d_dst.numel(), sp, tp, entries,
                                             C.cast(arr, C.c_void_p), len(rows), _stream_ptr(stream)), "fourmc_gpu_images_read_lines")
    return [{name: int(getattr(arr[i].out, name)) for name, _ in ImageLines._fields_} for i in range(len(rows))]


def images_lines_stats():
    """(groups, tail_rounds, block_decodes, index_launches) of images_read_lines so far in this process."""
    g, r, d, x = C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0), C.c_ulonglong(0)
    lib().fourmc_gpu_images_lines_stats(C.byref(g), C.byref(r), C.byref(d), C.byref(x))
    return int(g.value), int(r.value), int(d.value), int(x.value)


def images_align_slices(d_images, images, slices, images_bytes=None, stream=None):
    """image_align_slices for the raw slices [(image, start, end), ...] of many images in one device buffer
    (fourmc_gpu_images_align_slices).  Returns one dict per slice: image and the fields image_align_slices returns."""
    ptr = _dev_ptr(d_images, "images_align_slices d_images")
    n = _image_len(d_images, images_bytes, "images_align_slices")
    refs, nimages = _image_refs(images, "images_align_slices")
    q = [tuple(int(v) for v in sl) for sl in slices]
    arr = (ImagesSlice * max(len(q), 1))()
    for i, sl in enumerate(q):
        if len(sl) != 3:
            raise EngineError("images_align_slices slices: (image, start, end) each")
        arr[i].image, arr[i].s.start, arr[i].s.end = sl
    check(lib().fourmc_gpu_images_align_slices(ptr, n, C.cast(refs, C.c_void_p), nimages, C.cast(arr, C.c_void_p), len(q), _stream_ptr(stream)),
          "fourmc_gpu_images_align_slices")
    return [dict({"image": int(arr[i].image)}, **{name: int(getattr(arr[i].s, name)) for name, _ in ImageSlice._fields_}) for i in range(len(q))]


class ImageWriter:
    """Streaming writes of one .4mc / .4mz image into d_image (fourmc_gpu_image_writer_*): append() chunks of any size as they
    arrive, finish() for the image length.  The image is the one compress_image writes for the concatenation of the chunks.
    Appends queue work on `stream` (default: the current stream) and return; only finish() synchronizes.  As a context manager
    the writer is aborted when the block raises, or when it ends without finish()."""

    def __init__(self, d_image, magic=MAGIC_4MC, level=1, batch_blocks=0, stream=None):
        ptr = _dev_ptr(d_image, "ImageWriter d_image")
        self._stream = torch.cuda.current_stream() if stream is None else stream
        h = C.c_void_p(0)
        check(lib().fourmc_gpu_image_writer_begin(C.byref(h), ptr, d_image.numel(), magic, level, batch_blocks,
                                                  _stream_ptr(self._stream)), "fourmc_gpu_image_writer_begin")
        self._h = h.value
        self._image = d_image                     # the queued packs write into it until finish

    def _handle(self, what):
        if not self._h:
            raise EngineError(f"ImageWriter.{what}: the writer is finished or aborted")
        return self._h

    def append(self, chunk):
        """Queues the chunk (a contiguous uint8 CUDA tensor); the caching allocator keeps its memory until the stream has read it."""
        h = self._handle("append")
        ptr = _dev_ptr(chunk, "ImageWriter.append chunk")
        if chunk.numel():
            chunk.record_stream(self._stream)
        check(lib().fourmc_gpu_image_writer_append(h, ptr, chunk.numel()), "fourmc_gpu_image_writer_append")

    def finish(self):
        """Writes the last block, the header and the footer; returns the image length.  The writer is closed whatever happens."""
        h = self._handle("finish")
        self._h = None
        out = C.c_uint64(0)
        check(lib().fourmc_gpu_image_writer_finish(h, C.byref(out)), "fourmc_gpu_image_writer_finish")
        return int(out.value)

    def abort(self):
        """Frees the writer without an image."""
        h = self._handle("abort")
        self._h = None
        lib().fourmc_gpu_image_writer_abort(h)

    @property
    def closed(self):
        return not self._h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._h:
            self.abort()
        return False

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                self.abort()
            except Exception:
                pass


def _status_dict(st):
    res = {name: int(getattr(st, name)) for name, _ in ImageStatus._fields_}
    res["message"] = lib().fourmc_gpu_image_reason_text(st.reason).decode()
    return res


class ImageReader:
    """Streaming reads of one .4mc / .4mz image into d_dst (fourmc_gpu_image_reader_*): append() chunks of the image in file order
    as they arrive, finish() for the status.  The status and the bytes are the ones decompress_image gives for the concatenation of
    the chunks.  Appends queue work on `stream` (default: the current stream); they synchronize it once per walk over the chunk.
    As a context manager the reader is aborted when the block raises, or when it ends without finish()."""

    def __init__(self, d_dst, magic=MAGIC_4MC, batch_blocks=0, stream=None):
        ptr = _dev_ptr(d_dst, "ImageReader d_dst")
        self._stream = torch.cuda.current_stream() if stream is None else stream
        h = C.c_void_p(0)
        check(lib().fourmc_gpu_image_reader_begin(C.byref(h), ptr, d_dst.numel(), magic, batch_blocks, _stream_ptr(self._stream)),
              "fourmc_gpu_image_reader_begin")
        self._h = h.value
        self._dst = d_dst                         # the queued decodes write into it until finish

    def _handle(self, what):
        if not self._h:
            raise EngineError(f"ImageReader.{what}: the reader is finished or aborted")
        return self._h

    def append(self, chunk):
        """Queues the chunk (a contiguous uint8 CUDA tensor); the caching allocator keeps its memory until the stream has read it."""
        h = self._handle("append")
        ptr = _dev_ptr(chunk, "ImageReader.append chunk")
        if chunk.numel():
            chunk.record_stream(self._stream)
        check(lib().fourmc_gpu_image_reader_append(h, ptr, chunk.numel()), "fourmc_gpu_image_reader_append")

    def finish(self):
        """Decodes the last batch and returns the status as decompress_image does (a dict with "message").  The reader is closed
        whatever happens."""
        h = self._handle("finish")
        self._h = None
        st = ImageStatus()
        check(lib().fourmc_gpu_image_reader_finish(h, C.byref(st)), "fourmc_gpu_image_reader_finish")
        return _status_dict(st)

    def abort(self):
        """Frees the reader without a status."""
        h = self._handle("abort")
        self._h = None
        lib().fourmc_gpu_image_reader_abort(h)

    @property
    def closed(self):
        return not self._h

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        if self._h:
            self.abort()
        return False

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                self.abort()
            except Exception:
                pass
