"""4mc_amd — MI355X (gfx950) block engine for the 4mc / 4mz splittable container.

The product is the C-ABI shared library ``4mc_amd/lib/libhadoop-4mc.so`` (HIP kernels + C host
code, see ``include/fourmc_gpu.h`` / ``include/fourmc.h``) and the ``4mc_amd/bin/4mc`` CLI.  This
package is only the thin Python plumbing used by tests, ``bench.py`` and multi-GPU launches:
ctypes bindings over the C ABI, PyTorch tensors as device memory / streams, ``torch.distributed``
(RCCL) for the one collective of the path (the per-rank block-index gather).

There is no CPU fallback anywhere in this package: every codec call goes through the C ABI into
the HIP kernels, and a missing library or missing GPU raises.

The directory name starts with a digit (the reference is called 4mc), so import it with
``importlib.import_module("4mc_amd")``.
"""
from .binding import (  # noqa: F401
    BLOCK_DTYPE, BLOCKSIZE, MAGIC_4MC, MAGIC_4MZ, CODEC_LZ4_FAST, CODEC_LZ4_MC, CODEC_LZ4_HC,
    CODEC_ZSTD, BLK_BADSUM, BLK_CORRUPT, EngineError, lib, lib_path, research_lib_path, use_research, cli_path, exported_symbols,
    make_blocks, gpu_init, ImageStatus, ImageItem, ImageEncItem, ImageEntry, ImageIndexInfo, ImageRange, IMAGE_ENTRY_DTYPE, ImageSlice, ImageRecords, ImageLines, ImageSplitItem,
    ImageRef, ImagesSplitItem, ImagesSlice, ImageLineEntry, ImageLineInfo, ImageLinesAt, IMAGE_LINE_ENTRY_DTYPE, BstreamStatus, BstreamItem, BstreamEncItem, ImageWrItem, LinesSrc, LinesPackItem, LinesWrItem, BSTREAM_REASONS, BSTREAM_WRITE_REASONS, bstream_codec,
    ZstStatus, ZstItem, ZST_REASONS, ZstwStatus, ZstwItem, ZSTW_REASONS,
)
from .engine import (  # noqa: F401
    lz4_decompress, zstd_decompress, zstd_compress, lz4_compress_fast, lz4_compress_hc, lz4_compress_mc, xxh32, encode_blocks, decode_blocks, pack_image, DeviceBatch, release_workspaces,
    compress_image, compress_images, decompress_image, decompress_images, image_bound, image_parse_stats, image_index, image_decode_blocks, image_read, image_align_slices, image_read_records, image_read_lines, image_read_lines_batch, image_lines_batch_stats, ImageWriter,
    images_read_lines, images_lines_stats, images_align_slices,
    image_line_index, image_read_lines_at, image_lines_at_stats,
    ImageReader,
    bstream_max_input, bstream_bound, compress_bstream, decompress_bstream, decompress_bstreams, compress_bstreams, bstream_writes_bound,
    compress_images_writes, image_writes_bound,
    LinesSource, pack_lines, write_lines_images, write_lines_bstreams,
    decompress_zst, decompress_zsts, zst_stats,
    compress_zst, compress_zsts, zst_bound, zst_codec_level,
)
from .container import (  # noqa: F401
    frame_header, frame_footer, parse_footer, assemble_container, split_container, shard_range,
    gather_block_index,
)
