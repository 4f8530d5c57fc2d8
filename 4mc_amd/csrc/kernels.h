// 4mc_amd/csrc/kernels.h — launchers of the gfx950 kernels (internal to the engine).
#ifndef FOURMC_KERNELS_H
#define FOURMC_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif
// The launchers are the engine's own: C linkage for the objects of this library, but not part of its dynamic symbol table
// (the boundary is include/fourmc_gpu.h, include/fourmc.h and the JNI names).
#pragma GCC visibility push(hidden)

// what a hash launch covers for each block descriptor
enum {
    FOURMC_HASH_SRC        = 0,   // XXH32(src + src_off, src_len)          -> blocks[b].xxh32
    FOURMC_HASH_DST_RESULT = 1,   // XXH32(dst + dst_off, max(result,0))    -> blocks[b].xxh32
    FOURMC_VERIFY_SRC      = 2    // compare XXH32(src..) with blocks[b].xxh32; mismatch -> result = BADSUM,
                                  // match -> result = 0
};

/* what an LZ4 decode launch of n blocks runs: resolved once per call by fourmc_lz4_decode_plan, handed to the launcher */
typedef struct fourmc_lz4_plan {
    int      path;          /* decode path after "auto" has been resolved (lz4_decode.hip) */
    uint32_t batch;         /* blocks per piece of the launch (paths with a workspace) */
    size_t   work_bytes;    /* device workspace to lease: 0 for the paths that need none */
    int      ok;            /* 0: the pieces cannot get smaller (the workspace cannot be had) */
} fourmc_lz4_plan;
fourmc_lz4_plan fourmc_lz4_decode_plan(uint32_t n, uint32_t shrink);
size_t     fourmc_lz4_parse_work_bytes(uint32_t n);
size_t     fourmc_lz4_decode_tok_offset(void);
hipError_t fourmc_launch_lz4_decode(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                                    uint32_t n, int container_mode, const fourmc_lz4_plan* plan, void* d_work, hipStream_t stream);
hipError_t fourmc_launch_lz4_rows(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                                  uint32_t n, int container_mode, hipStream_t stream);
hipError_t fourmc_launch_lz4_lanes(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                                  uint32_t n, int container_mode, hipStream_t stream);
hipError_t fourmc_launch_lz4_wx(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                                  uint32_t n, int container_mode, hipStream_t stream, const uint32_t* pick, uint32_t want);
size_t     fourmc_lz4_seg_work_bytes(uint32_t n);
uint32_t   fourmc_lz4_seg_batch(void);              /* blocks per launch of the segment-parallel path (bounds its workspace) */
size_t     fourmc_lz4_tile_work_bytes(uint32_t n);
uint32_t   fourmc_lz4_tile_batch(void);             /* blocks per launch of the tile path */
hipError_t fourmc_launch_lz4_tile(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                  int container_mode, void* d_work, hipStream_t stream);
hipError_t fourmc_launch_lz4_seg(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                 int container_mode, void* d_work, hipStream_t stream);
hipError_t fourmc_launch_lz4_seg_walk(const void* d_src, fourmc_block* d_blocks, uint32_t n, int container_mode,
                                      void* d_work, hipStream_t stream);
hipError_t fourmc_launch_lz4_ring(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                  int container_mode, void* d_work, hipStream_t stream);
hipError_t fourmc_launch_lz4_parse(const void* d_src, const void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                   int container_mode, void* d_work, hipStream_t stream);
hipError_t fourmc_launch_lz4_exec(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                  const void* d_work, hipStream_t stream);
/* LZ4 fast encode, the reference's parse (lz4_encode.hip): the parse writes sequence records to d_work, then the emit kernel
 * (lz4_emit.hip) writes the payloads on the same stream.  d_work holds fourmc_lz4_fast_work_bytes(n) bytes */
uint32_t   fourmc_lz4_fast_reccap(void);
size_t     fourmc_lz4_fast_work_bytes(uint32_t n);
hipError_t fourmc_launch_lz4_encode_fast(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                                         uint32_t n, int container_mode, void* d_work, hipStream_t stream);
hipError_t fourmc_launch_lz4_emit(const void* d_src, void* d_dst, const fourmc_block* d_blocks, uint32_t n,
                                  const void* d_work, uint32_t reccap, hipStream_t stream);
size_t     fourmc_lz4_par_work_bytes(uint32_t n);
hipError_t fourmc_launch_lz4_encode_par(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                        int container_mode, void* d_work, hipStream_t stream);
hipError_t fourmc_launch_pack_image(const void* d_staging, void* d_image, const fourmc_block* d_blocks,
                                    const uint64_t* d_image_off, uint32_t n, hipStream_t stream);
size_t     fourmc_lz4hc_work_bytes(uint32_t n);
hipError_t fourmc_launch_lz4hc_encode(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                      void* d_work, int level, int container_mode, hipStream_t stream);
/* LZ4 HC levels 9..12 (lz4hc_opt_encode.hip): one wavefront per block, the chain ring in LDS */
size_t     fourmc_lz4hc_opt_work_bytes(uint32_t n);
hipError_t fourmc_launch_lz4hc_opt_encode(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                          void* d_work, int level, int container_mode, hipStream_t stream);
hipError_t fourmc_launch_lz4mc_encode(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                      void* d_work, int container_mode, hipStream_t stream);
/* whole file images (image.hip): what the parse leaves for the engine's one read-back, and what the encode's scan leaves */
typedef struct fourmc_image_parse {
    uint64_t nblocks;       /* well-formed blocks, in file order, before the parser stopped */
    uint64_t total;         /* sum of their usize */
    uint64_t fail_offset;   /* image offset of the framing error (image_bytes when there is none) */
    uint32_t streams;       /* streams whose header passed */
    int32_t  reason;        /* FOURMC_IMG_*: the framing verdict */
    uint32_t fast;          /* 1: the fast path accepted the image (the walk has nothing to do) */
    uint32_t pad;
} fourmc_image_parse;
typedef struct fourmc_image_enc_summary {
    uint64_t image_bytes;
    uint32_t bad_blocks;    /* encoder results outside [1, src_len] (never, for the container encode) */
    uint32_t pad;
} fourmc_image_enc_summary;
hipError_t fourmc_launch_image_enc_desc(fourmc_block* d_blocks, uint64_t src_bytes, uint32_t n, hipStream_t s);
hipError_t fourmc_launch_image_enc_frame(void* d_image, fourmc_block* d_blocks, uint64_t* d_off, uint32_t n, uint32_t magic,
                                         const void* d_staging, fourmc_image_enc_summary* d_sum, hipStream_t s);
/* the streaming writer's batches (fourmc_gpu_image_writer_*): descriptors of n blocks of src_bytes at src0 of their source and dst0
 * of the staging; the scan of one batch from the running offset d_off[0] (the writer's index at the batch's first block number) into
 * d_off[0..n], its bad results added to d_sum->bad_blocks, then the pack; the header, end mark and footer of n blocks from d_off */
hipError_t fourmc_launch_image_wr_desc(fourmc_block* d_blocks, uint64_t src0, uint64_t dst0, uint64_t src_bytes, uint32_t n, hipStream_t s);
hipError_t fourmc_launch_image_wr_batch(void* d_image, fourmc_block* d_blocks, uint64_t* d_off, uint32_t n, const void* d_staging,
                                        fourmc_image_enc_summary* d_sum, hipStream_t s);
hipError_t fourmc_launch_image_wr_tail(void* d_image, const uint64_t* d_off, uint32_t n, uint32_t magic, hipStream_t s);
/* fast: the footer-driven parser; walk: the file-order walk (count mode skips itself when the fast path accepted the image).
 * d_blocks NULL: count into *d_ps; else fill the descriptors of the parse *d_ps holds. */
hipError_t fourmc_launch_image_parse(const void* d_image, uint64_t image_bytes, uint32_t magic, int fast, int walk,
                                     fourmc_image_parse* d_ps, fourmc_block* d_blocks, hipStream_t s);
hipError_t fourmc_launch_image_reduce(const fourmc_block* d_blocks, uint32_t n, const fourmc_image_parse* d_ps,
                                      fourmc_image_status* d_status, hipStream_t s);
/* many images in one call (fourmc_gpu_images_decompress): what the plan leaves for the engine's first read-back */
typedef struct fourmc_images_summary {
    uint64_t nblocks;       /* descriptors of all images together (size query: every well-formed block) */
    uint32_t fast, walk;    /* images the fast path / the walk accepted */
} fourmc_images_summary;
/* d_desc NULL: count every image into d_ps[i] (fast: try the footer-driven parser first); else fill the descriptors of the parse
 * d_ps[i] holds at d_desc + d_first[i], offsets relative to d_images and to the items' common destination */
hipError_t fourmc_launch_images_parse(const void* d_images, const fourmc_image_item* d_items, uint32_t n, uint32_t magic, int fast,
                                      fourmc_image_parse* d_ps, const uint64_t* d_first, fourmc_block* d_desc, hipStream_t s);
/* d_first[i] = descriptors before image i (none for an image that ends FOURMC_IMG_DST_SMALL), *d_sum; query: the parse-only statuses */
hipError_t fourmc_launch_images_plan(const fourmc_image_item* d_items, uint32_t n, const fourmc_image_parse* d_ps, int query,
                                     uint64_t* d_first, fourmc_images_summary* d_sum, fourmc_image_status* d_status, hipStream_t s);
hipError_t fourmc_launch_images_reduce(const fourmc_image_item* d_items, uint32_t n, const fourmc_image_parse* d_ps,
                                       const uint64_t* d_first, const fourmc_block* d_desc, fourmc_image_status* d_status, hipStream_t s);
/* many images in one call, the encode (fourmc_gpu_images_compress).  The sizes are known on the host, so its argument loop computes
 * each image's slice of the tables and sends it up with the item: block b of image i is descriptor first + b, its source
 * src_off + b * 4 MiB of d_src and its staging slot stage_off + b * 4 MiB (only an image's last block is short: slots abut). */
typedef struct fourmc_image_enc_plan {  /* 40 bytes */
    uint64_t src_off, src_bytes;        /* the item's source */
    uint64_t image_off;                 /* where its image starts in d_images */
    uint64_t stage_off;                 /* the staging slot of its first block */
    uint32_t first, nblocks;            /* its descriptors, and its entries of the dense offset table */
} fourmc_image_enc_plan;
typedef struct fourmc_image_enc_result {
    uint64_t image_bytes;
    uint64_t bad_blocks;                /* encoder results outside [1, src_len] in this image: the engine folds them */
} fourmc_image_enc_result;
/* the descriptors of all nblocks blocks (offsets relative to d_src and to the staging); no launch without blocks */
hipError_t fourmc_launch_images_enc_desc(const fourmc_image_enc_plan* d_plans, uint32_t n, fourmc_block* d_blocks, uint32_t nblocks,
                                         hipStream_t s);
/* after the container encode: per image the scan from image_off + 12 into d_off (dense, nblocks entries, absolute in d_images),
 * its end mark's offset into d_end[i] and its length and bad results into d_res[i]; ONE pack over all blocks; per image the
 * header, end mark and footer */
hipError_t fourmc_launch_images_enc_frame(void* d_images, const fourmc_image_enc_plan* d_plans, uint32_t n, fourmc_block* d_blocks,
                                          uint32_t nblocks, uint64_t* d_off, uint64_t* d_end, uint32_t magic, const void* d_staging,
                                          fourmc_image_enc_result* d_res, hipStream_t s);
/* random access (image.hip, second half): the index summary plus where the last block must end (read_index's data_end) */
typedef struct fourmc_image_index_dev {
    fourmc_image_index_info info;
    uint64_t data_end;
} fourmc_image_index_dev;
/* what the read plan leaves for the engine's second read-back */
typedef struct fourmc_image_plan {
    uint64_t ndirect;       /* descriptors decoded straight into a range's destination */
    uint32_t nstaged;       /* distinct partly covered blocks = staging slots */
    uint32_t max_piece;     /* longest (range, staged block) piece in bytes */
} fourmc_image_plan;
/* per range: the blocks it covers, its direct descriptors, where they start */
typedef struct fourmc_image_rplan {
    uint32_t b0, b1;        /* first and last covering block */
    uint32_t nd, pad;       /* direct descriptors */
    uint64_t dbase;         /* index of its first direct descriptor */
    uint64_t pad2;
} fourmc_image_rplan;
/* decode_blocks: the framing verdict of [first, first+count) and the bytes it holds */
typedef struct fourmc_image_span {
    int64_t  framing;
    uint64_t out;
} fourmc_image_span;
/* d_ent NULL: the summary only; else min(n, cap) entries */
hipError_t fourmc_launch_image_index(const void* d_image, uint64_t image_bytes, fourmc_image_index_dev* d_idx,
                                     fourmc_image_entry* d_ent, uint64_t cap, hipStream_t s);
/* Many images with one index launch (fourmc_gpu_images_read_lines / _images_align_slices): where image i lies in the buffer and
 * where its entries go in the one entry table.  nblocks is 0 until the summaries have come back, and stays 0 for an image that
 * cannot be indexed, so nothing ever looks an entry of such an image up. */
typedef struct fourmc_images_tab {
    uint64_t image_off, image_bytes;
    uint64_t ent0;          /* index of its first entry in the table */
    uint32_t nblocks;       /* its blocks, for the kernels that search its entries */
    uint32_t cap;           /* entries the index kernel writes: nblocks, or 0 for an image no item names */
} fourmc_images_tab;
/* one wave per image: d_idx[i] = image i's summary; d_ent NULL: nothing else, else its first cap entries at d_ent + ent0 */
hipError_t fourmc_launch_images_index(const void* d_images, const fourmc_images_tab* d_tab, uint32_t nimages,
                                      fourmc_image_index_dev* d_idx, fourmc_image_entry* d_ent, hipStream_t s);
/* decode_blocks: the range's framing checks into *d_span, then its `count` descriptors (all-zero ones if a check failed) */
hipError_t fourmc_launch_image_span(const fourmc_image_entry* d_ent, const fourmc_image_index_dev* d_idx, uint64_t image_bytes,
                                    uint32_t first, uint32_t count, uint64_t dst_cap, fourmc_image_span* d_span,
                                    fourmc_block* d_desc, hipStream_t s);
hipError_t fourmc_launch_image_span_reduce(const fourmc_block* d_desc, uint32_t count, const fourmc_image_span* d_span,
                                           int64_t* d_result, hipStream_t s);
/* image_read, before the second read-back: covering blocks, early results, direct counts, staging flags -> slots, totals.
 * d_flags (n words) must be zero. */
hipError_t fourmc_launch_image_plan(const fourmc_image_entry* d_ent, uint32_t n, const fourmc_image_index_dev* d_idx,
                                    fourmc_image_range* d_ranges, uint32_t nranges, uint64_t dst_cap, fourmc_image_rplan* d_rp,
                                    uint32_t* d_flags, fourmc_image_plan* d_plan, hipStream_t s);
/* after it: the descriptors (direct ones at d_dst_delta + dst_off, staged ones at d_stage_delta + slot * 4 MiB, both relative to
 * the decode's base), the decode, the copies out of staging, the per-range results */
hipError_t fourmc_launch_image_read_desc(const fourmc_image_entry* d_ent, uint32_t n, const fourmc_image_range* d_ranges,
                                         uint32_t nranges, const fourmc_image_rplan* d_rp, const uint32_t* d_slot, uint32_t nstaged,
                                         uint64_t ndirect, uint64_t dst_delta, uint64_t stage_delta, fourmc_block* d_desc, hipStream_t s);
hipError_t fourmc_launch_image_read_copy(const fourmc_image_entry* d_ent, const fourmc_image_range* d_ranges, uint32_t nranges,
                                         const fourmc_image_rplan* d_rp, const uint32_t* d_slot, const void* d_stage, void* d_dst,
                                         uint32_t max_piece, hipStream_t s);
hipError_t fourmc_launch_image_read_reduce(const fourmc_image_entry* d_ent, fourmc_image_range* d_ranges, uint32_t nranges,
                                           const fourmc_image_rplan* d_rp, const uint32_t* d_slot, const fourmc_block* d_desc,
                                           uint64_t ndirect, hipStream_t s);
/* the streaming reader (fourmc_gpu_image_reader_*): the resumable walk's device state.  The first block is what the engine reads
 * back after each walk launch. */
typedef struct fourmc_image_rd_state {
    /* read back after every walk */
    uint64_t cpos;          /* where the walk stopped in the chunk */
    uint32_t batch_n;       /* complete blocks in the current batch (staging slots 0 .. batch_n-1) */
    uint32_t npieces;       /* copy pieces the walk emitted */
    uint32_t max_piece;     /* the longest of them */
    uint32_t final_;        /* the framing verdict is final: later bytes are not read */
    /* the walk */
    uint64_t pos;           /* image offset of the next byte to consume */
    uint64_t at;            /* image offset of the unit in progress (file header, block header, footer): the fail offset */
    uint64_t total;         /* sum of the usizes of the well-formed blocks */
    uint64_t stream_total0; /* total when the current stream's header passed */
    uint64_t nblocks;       /* well-formed blocks */
    uint64_t got;           /* bytes of the current payload / footer received */
    uint32_t phase, streams;
    int32_t  reason;        /* the verdict once final_ */
    uint32_t have;          /* header / size-field bytes in part */
    uint32_t usize, csize, sum, slot;   /* the current block; slot ~0u: not decoded (it ends beyond dst_cap) */
    uint32_t fsz, xbn;      /* the footer's size field; bytes in xbuf */
    uint64_t part[2];       /* a header in progress, byte k at bits 8 (k % 8) of word k / 8; a footer keeps its size and version
                             * at bytes 0..7 and its checksum at 8..11 */
    uint32_t xv[4];         /* streaming XXH32 of a footer or of an oversized block's payload: lanes, length, partial stripe */
    uint64_t xlen;
    uint64_t xbuf[2];
    /* the fold over the decoded batches */
    uint64_t done;          /* decoded bytes before the first failing block */
    uint64_t decoded;       /* blocks decoded so far (the global index of the next batch's first block) */
    uint64_t first_at;      /* image offset of the first failing block's header */
    uint32_t first;         /* its global index */
    int32_t  first_reason;  /* 0: none yet, else FOURMC_IMG_BLOCK_CHECKSUM / FOURMC_IMG_CORRUPT */
} fourmc_image_rd_state;
/* one copy of payload bytes from a chunk into a staging slot */
typedef struct fourmc_image_piece {
    uint64_t src, dst;      /* device addresses */
    uint64_t len;
    uint64_t pad;
} fourmc_image_piece;
/* the walk over chunk[start, bytes): descriptors (src_off relative to the staging, dst_off to d_dst) and header offsets of the
 * blocks it completes into slots batch_n.., copy pieces, until the chunk ends, the batch is full or the verdict is final */
hipError_t fourmc_launch_image_rd_walk(const void* d_chunk, uint64_t bytes, uint64_t start, fourmc_image_rd_state* d_st,
                                       uint32_t magic, uint64_t dst_cap, uint32_t batch, void* d_stage, fourmc_block* d_desc,
                                       uint64_t* d_at, fourmc_image_piece* d_pc, hipStream_t s);
hipError_t fourmc_launch_image_rd_gather(const fourmc_image_piece* d_pc, uint32_t npieces, uint64_t max_piece, hipStream_t s);
/* after a batch of n blocks has decoded: image_reduce's rule carried across batches; the batch is emptied */
hipError_t fourmc_launch_image_rd_fold(const fourmc_block* d_desc, const uint64_t* d_at, uint32_t n, fourmc_image_rd_state* d_st,
                                       hipStream_t s);
/* the deferred checks with N = image_bytes, the DST_SMALL rule and the fold into *d_status */
hipError_t fourmc_launch_image_rd_finish(const fourmc_image_rd_state* d_st, uint64_t image_bytes, uint64_t dst_cap,
                                         fourmc_image_status* d_status, hipStream_t s);
/* the line records of a split (records.hip): what the split's offsets resolve to, read back before anything is decoded */
typedef struct fourmc_records_plan {
    int64_t  code;          /* 0, or -3: a split offset that is neither 0 / a block header nor at or past the end mark */
    uint64_t ds, de;        /* decoded offsets of the blocks at split_start and split_end (0 / total_bytes when there is none) */
    uint64_t total;         /* total decoded size */
    uint32_t b0, b1;        /* the split's blocks are [b0, b1); b1 == nblocks when split_end is no block header */
} fourmc_records_plan;
/* one staged tail block, read back after its scan */
typedef struct fourmc_records_tail {
    int64_t  code;          /* 0, or -4: the block failed its XXH32 or its decode, or decoded to another size than its usize */
    uint64_t data_off;      /* decoded offset of the block's first byte */
    uint64_t hi;            /* found: decoded offset just behind the block's first delimiter */
    uint32_t found, pad;
} fourmc_records_tail;
/* the call's result on the device, and what the finish kernel tells the write kernel */
typedef struct fourmc_records_state {
    fourmc_image_records r;
    uint32_t write;         /* 1: the starts are to be written */
    uint32_t shift;         /* index of the start behind the first delimiter: 1 when the split starts the file, else 0 */
} fourmc_records_state;
#define FOURMC_RECORDS_TILE (16u * 1024u)       /* bytes one wave scans: one count per tile */
hipError_t fourmc_launch_image_align(const fourmc_image_entry* d_ent, uint32_t n, uint64_t image_bytes,
                                     fourmc_image_slice* d_slices, uint32_t nslices, hipStream_t s);
/* the same over the slices of many images, each against its own image's entries; a slice of an image without entries (nblocks 0
 * in the table) is left as it came */
hipError_t fourmc_launch_images_align(const fourmc_image_entry* d_ent, const fourmc_images_tab* d_tab, fourmc_images_slice* d_slices,
                                      uint32_t nslices, hipStream_t s);
hipError_t fourmc_launch_records_plan(const fourmc_image_entry* d_ent, uint32_t n, const fourmc_image_index_dev* d_idx,
                                      uint64_t split_start, uint64_t split_end, fourmc_records_plan* d_plan, hipStream_t s);
/* descriptors of blocks [first, first + count) with block i at data_off[i] - ds of the decode's destination (to_stage: at 0) */
hipError_t fourmc_launch_records_desc(const fourmc_image_entry* d_ent, uint32_t first, uint32_t count, uint64_t ds, int to_stage,
                                      fourmc_block* d_desc, hipStream_t s);
/* after block b has been decoded to d_stage through *d_desc: its verdict and its first delimiter */
hipError_t fourmc_launch_records_tail_find(const void* d_stage, const fourmc_block* d_desc, const fourmc_image_entry* d_ent,
                                           uint32_t b, uint8_t delim, fourmc_records_tail* d_tail, hipStream_t s);
/* tiles of d[0, len): FOURMC_RECORDS_TILE bytes each, counted from d rounded down to 16 bytes */
uint64_t   fourmc_records_tiles(const void* d, uint64_t len);
hipError_t fourmc_launch_records_count(const void* d, uint64_t len, uint8_t delim, uint64_t* d_cnt, uint64_t ntiles, hipStream_t s);
/* the counts into their exclusive prefix (in place), the body blocks' verdict, the ownership rule: *d_st */
hipError_t fourmc_launch_records_finish(const void* d, uint64_t len, uint8_t delim, uint64_t* d_cnt, uint64_t ntiles,
                                        const fourmc_block* d_desc, uint32_t ndesc, int first_split, uint64_t ds, uint64_t body,
                                        uint64_t* d_starts, uint64_t starts_cap, fourmc_records_state* d_st, hipStream_t s);
hipError_t fourmc_launch_records_write(const void* d, uint64_t len, uint8_t delim, const uint64_t* d_cnt, uint64_t ntiles,
                                       const fourmc_records_state* d_st, uint64_t* d_starts, hipStream_t s);
/* The same by Hadoop's default line rule (LF, lone CR, CR LF; fourmc_gpu_image_read_lines).  tail_find: found = 2 says that the
 * block ends with a CR whose fate the next block's first byte decides; the block behind it is then asked with `pending`. */
hipError_t fourmc_launch_lines_tail_find(const void* d_stage, const fourmc_block* d_desc, const fourmc_image_entry* d_ent,
                                         uint32_t b, int last_block, int pending, fourmc_records_tail* d_tail, hipStream_t s);
hipError_t fourmc_launch_lines_count(const void* d, uint64_t len, uint64_t* d_cnt, uint64_t ntiles, hipStream_t s);
hipError_t fourmc_launch_lines_finish(const void* d, uint64_t len, uint64_t* d_cnt, uint64_t ntiles, const fourmc_block* d_desc,
                                      uint32_t ndesc, int first_split, uint64_t ds, uint64_t body, uint64_t* d_starts,
                                      uint64_t starts_cap, uint32_t* d_tlen, fourmc_records_state* d_st, hipStream_t s);
/* the starts and each line's terminator length, then the pass that turns d_tlen into text lengths cut at max_line_len */
hipError_t fourmc_launch_lines_write(const void* d, uint64_t len, uint32_t max_line_len, const uint64_t* d_cnt, uint64_t ntiles,
                                     const fourmc_records_state* d_st, uint64_t* d_starts, uint32_t* d_tlen, hipStream_t s);
/* Many splits with one call (fourmc_gpu_image_read_lines_batch): the kernels above over a group of splits. */
/* The same kernels serve fourmc_gpu_images_read_lines: every request, job and span names its image, the entries of all images
 * lie in one table (image i's from fourmc_images_tab.ent0 on, image-relative), and a descriptor's src_off is the entry's offset
 * plus the image's.  The one-image call passes a table of one image at offset 0. */
typedef struct fourmc_split_req { uint64_t split_start, split_end; uint32_t image, pad; } fourmc_split_req;
/* one split still looking for its hi, for one round: entry e (its image's ent0 + the block) goes to staging slot `slot` and is
 * searched there; src_base: the image's offset in the buffer */
typedef struct fourmc_tail_job { uint32_t e, slot; int32_t last_block, pending; uint64_t src_base; } fourmc_tail_job;
/* one split whose content fits its region: what the body decode, the prefix copy and the scan need of it */
typedef struct fourmc_lines_span {
    uint8_t*  dst;          /* d_dst + dst_off */
    uint64_t  len;          /* hi - ds */
    uint64_t  tile0, ntiles;/* its tiles in the group's count table: fourmc_records_tiles(dst, len) of them from tile0 on */
    uint32_t  desc0, ndesc; /* its body blocks' descriptors in the group's table */
    uint32_t  e0;           /* the first body block's entry: its image's ent0 + b0 */
    int32_t   first_split;  /* split_start == 0 */
    uint64_t  ds, body;     /* decoded offset of dst[0]; de - ds */
    uint64_t* starts;       /* d_starts + table_off, NULL: count only */
    uint32_t* tlen;
    uint64_t  lines_cap;
    const uint8_t* stage;   /* the split's staging slot */
    uint64_t  copy_off, copy_len;   /* dst[copy_off, +copy_len) = stage[0, copy_len): the last tail block's prefix (0: none) */
    uint64_t  src_base;     /* the image's offset in the buffer the body decode reads from */
} fourmc_lines_span;
/* d_tab / d_idx: one entry per image; request i is planned against the entries and the summary of image d_req[i].image, and its
 * b0 / b1 count that image's blocks */
hipError_t fourmc_launch_lines_batch_plan(const fourmc_image_entry* d_ent, const fourmc_images_tab* d_tab, const fourmc_image_index_dev* d_idx,
                                          const fourmc_split_req* d_req, uint32_t m, fourmc_records_plan* d_plan, hipStream_t s);
/* per round: job j's block to slot * stride of the staging; after the decode, job j's verdict to d_tail[j] */
hipError_t fourmc_launch_lines_batch_tail_desc(const fourmc_image_entry* d_ent, const fourmc_tail_job* d_job, uint32_t nj,
                                               uint64_t stride, fourmc_block* d_desc, hipStream_t s);
hipError_t fourmc_launch_lines_batch_tail_find(const void* d_stage, uint64_t stride, const fourmc_block* d_desc,
                                               const fourmc_image_entry* d_ent, const fourmc_tail_job* d_job, uint32_t nj,
                                               fourmc_records_tail* d_tail, hipStream_t s);
/* d_first_desc[k] = spans[k].desc0 and d_first_tile[k] = spans[k].tile0: the tables a lane or a wave finds its span in.  The body
 * descriptors' offsets are relative to d_dst. */
hipError_t fourmc_launch_lines_batch_body_desc(const fourmc_image_entry* d_ent, const fourmc_lines_span* d_spans,
                                               const uint32_t* d_first_desc, uint32_t ns, uint32_t ndesc, const void* d_dst,
                                               fourmc_block* d_desc, hipStream_t s);
hipError_t fourmc_launch_lines_batch_copy(const fourmc_lines_span* d_spans, uint32_t ns, uint64_t longest, hipStream_t s);
hipError_t fourmc_launch_lines_batch_count(const fourmc_lines_span* d_spans, const uint64_t* d_first_tile, uint32_t ns,
                                           uint64_t* d_cnt, uint64_t ntiles, hipStream_t s);
hipError_t fourmc_launch_lines_batch_finish(const fourmc_lines_span* d_spans, uint32_t ns, uint64_t* d_cnt, const fourmc_block* d_desc,
                                            fourmc_records_state* d_st, hipStream_t s);
/* the write pass and the length pass; `longest`: the longest span's len */
hipError_t fourmc_launch_lines_batch_write(const fourmc_lines_span* d_spans, const uint64_t* d_first_tile, uint32_t ns,
                                           const uint64_t* d_cnt, uint64_t ntiles, uint64_t longest, uint32_t max_line_len,
                                           const fourmc_records_state* d_st, hipStream_t s);
/* Lines by number (lineat.hip, fourmc_gpu_image_line_index / _image_read_lines_at).  Blocks are staged one per slot of `stride`
 * bytes (a multiple of 16, the staging 16-byte aligned), block d_list[j] - or first + j where there is no list - in slot j. */
/* what the index's count launch leaves per block: its line ends with a CR in its last byte counted as one, and
 * info bit 0: the last byte is CR, bit 1: the first byte is LF, bit 2: the block is damaged, bit 3: the last byte is LF,
 * bits 8..31: the offset just behind its last end other than a CR in its last byte (0: none) */
typedef struct fourmc_lineat_blk { uint32_t cnt, info; } fourmc_lineat_blk;
typedef struct fourmc_lineat_sum { int64_t result; uint64_t lines, ends, total; } fourmc_lineat_sum;
/* one request between the rounds: its line's start (~0: not known before bp has been staged), the blocks holding end k - 1 and
 * end k, and the ranks of those ends inside them (je ~0u: the final unterminated line, which ends with the content) */
typedef struct fourmc_lineat_req { uint64_t start; uint32_t bp, be, js, je; } fourmc_lineat_req;    /* 24 bytes */
typedef struct fourmc_lineat_counts { uint32_t needed, served; } fourmc_lineat_counts;
hipError_t fourmc_launch_lineat_desc(const fourmc_image_entry* d_ent, const uint32_t* d_list, uint32_t first, uint32_t m, uint64_t stride,
                                     fourmc_block* d_desc, hipStream_t s);
/* a workgroup per staged block first + j: d_blk[first + j] */
hipError_t fourmc_launch_lineat_block_count(const void* d_stage, uint64_t stride, const fourmc_image_entry* d_ent, uint32_t first,
                                            const fourmc_block* d_desc, uint32_t m, fourmc_lineat_blk* d_blk, hipStream_t s);
/* one workgroup over all blocks: the seams, the flags, the 64-bit prefix; the entries (when d_index and nb + 1 <= cap) and *d_sum */
hipError_t fourmc_launch_lineat_index_finish(const fourmc_image_entry* d_ent, const fourmc_lineat_blk* d_blk, uint32_t nb, uint64_t total,
                                             fourmc_image_line_entry* d_index, uint64_t cap, fourmc_lineat_sum* d_sum, hipStream_t s);
/* every status = code, every text_len = 0 */
hipError_t fourmc_launch_lineat_fill(int32_t* d_status, uint32_t* d_text_len, uint32_t n, int32_t code, hipStream_t s);
/* one lane per request: d_req[i], status 0 (-3: no such line) and text_len 0, and d_flags[b] = 1 for the blocks it needs; then a
 * wave per refused request pads its row.  L = min(row_bytes, max_line_len).  d_flags (nb words) must be zero. */
hipError_t fourmc_launch_lineat_locate(const fourmc_image_entry* d_ent, uint32_t nb, uint64_t total, const fourmc_image_line_entry* d_index,
                                       const uint64_t* d_lines, uint32_t n, uint32_t L, fourmc_lineat_req* d_req, uint32_t* d_flags,
                                       uint8_t* d_rows, uint32_t row_bytes, uint8_t pad, uint32_t* d_text_len, int32_t* d_status, hipStream_t s);
/* the marked blocks in ascending order into d_list, their number into d_counts->needed */
hipError_t fourmc_launch_lineat_compact(const uint32_t* d_flags, uint32_t nb, uint32_t* d_list, fourmc_lineat_counts* d_counts, hipStream_t s);
/* per round of m staged blocks: the line ends of every 16 KiB tile, FOURMC_BLOCKSIZE / FOURMC_RECORDS_TILE words per slot */
hipError_t fourmc_launch_lineat_tiles(const void* d_stage, uint64_t stride, const fourmc_image_entry* d_ent, const uint32_t* d_list, uint32_t m,
                                      uint32_t* d_tcnt, hipStream_t s);
/* a wave per request: resolve what this round's blocks can, copy what lies in them, finish the request in the round of be */
hipError_t fourmc_launch_lineat_resolve(const void* d_stage, uint64_t stride, const fourmc_image_entry* d_ent, const fourmc_image_line_entry* d_index,
                                        const uint32_t* d_list, const fourmc_block* d_desc, uint32_t m, const uint32_t* d_tcnt,
                                        fourmc_lineat_req* d_req, uint32_t n, uint32_t max_line_len, uint8_t* d_rows, uint32_t row_bytes,
                                        uint8_t pad, uint32_t* d_text_len, int32_t* d_status, hipStream_t s);
/* d_counts->served += the requests with status 1 */
hipError_t fourmc_launch_lineat_served(const int32_t* d_status, uint32_t n, fourmc_lineat_counts* d_counts, hipStream_t s);
/* Hadoop block streams (bstream.hip, fourmc_gpu_bstream_*): what run 1 of the walk leaves per stream for the engine's read-back */
typedef struct fourmc_bstream_walk {    /* 40 bytes */
    uint64_t chunks;        /* chunks of the well-formed groups, in file order, before the walk stopped */
    uint64_t groups;        /* well-formed groups */
    uint64_t total;         /* sum of their rawlens */
    uint64_t fail_offset;   /* stream offset of the field that ended the walk (image_bytes when it ended cleanly) */
    int32_t  reason;        /* FOURMC_BS_*: the framing verdict */
    uint32_t pad;
} fourmc_bstream_walk;
/* the side table of run 2, one entry per descriptor: where the chunk's header lies in its stream, and the group it belongs to */
typedef struct fourmc_bstream_side { uint64_t at, group; } fourmc_bstream_side;
/* the encode's running state on the device: the stream offset behind the last group packed, and the bad codec results so far */
typedef struct fourmc_bstream_enc_summary { uint64_t image_bytes, bad; } fourmc_bstream_enc_summary;
/* d_desc NULL: run 1, d_ws[i] = stream i's summary; else run 2: the descriptors (offsets relative to d_images and to the items'
 * common destination) and side entries of the summaries d_ws holds, stream i's at d_first[i]; none for an item whose total exceeds
 * its dst_cap.  max_input: M of the codec family */
hipError_t fourmc_launch_bstream_walk(const void* d_images, const fourmc_bstream_item* d_items, uint32_t n, uint32_t max_input,
                                      fourmc_bstream_walk* d_ws, const uint64_t* d_first, fourmc_block* d_desc,
                                      fourmc_bstream_side* d_side, hipStream_t s);
hipError_t fourmc_launch_bstream_fold(const fourmc_bstream_item* d_items, uint32_t n, const fourmc_bstream_walk* d_ws,
                                      const uint64_t* d_first, const fourmc_block* d_desc, const fourmc_bstream_side* d_side,
                                      fourmc_bstream_status* d_status, hipStream_t s);
/* one staging piece of n groups: group b reads src0 + b * group_bytes of the source (src_bytes: the piece's bytes) and writes slot
 * b * stride of the staging; nolimit: dst_cap = 0xFFFFFFFF (LZ4_compressMC) instead of the bound */
hipError_t fourmc_launch_bstream_enc_desc(fourmc_block* d_blocks, uint64_t src0, uint64_t src_bytes, uint32_t group_bytes,
                                          uint32_t stride, uint32_t n, int zstd, int nolimit, hipStream_t s);
/* after the codec: the scan of 8 + csize from d_sum->image_bytes into d_off[0, n) and back into *d_sum, then the pack */
hipError_t fourmc_launch_bstream_enc_pack(void* d_image, fourmc_block* d_blocks, uint64_t* d_off, uint32_t n, int zstd,
                                          const void* d_staging, fourmc_bstream_enc_summary* d_sum, hipStream_t s);
/* fourmc_gpu_bstreams_compress: what the plan leaves per stream for the engine's read-back (the engine sends it back with
 * FOURMC_BSW_CAP set where the region is too small) */
typedef struct fourmc_bsw_plan {        /* 40 bytes */
    uint64_t groups, chunks;   /* the written groups and their chunks                                       */
    uint64_t worst;            /* the exact worst case of the stream's length                               */
    uint64_t stage;            /* the staging bytes of its chunks: each codec bound rounded up to 256 bytes */
    int32_t  reason;           /* FOURMC_BSW_*                                                              */
    uint32_t trailer;          /* 1: the stream ends with BE32(0)                                           */
} fourmc_bsw_plan;
/* the engine's prefix sums over the streams that are encoded (n + 1 entries): the first chunk, counted over all streams in file
 * order, the first entry of the group table and the first staging byte of each */
typedef struct fourmc_bsw_slice { uint64_t chunk0, group0, stage0; } fourmc_bsw_slice;
/* a written group of a stream with a table: its first source byte and first staging byte, both counted from the stream's own, its
 * rawlen (above M: a long group) and its first chunk's number in the stream */
typedef struct fourmc_bsw_group { uint64_t src, stage; uint32_t rawlen, chunk0; } fourmc_bsw_group;
/* beside the descriptor of a chunk of a round: its stream, its group's rawlen when it is the group's first chunk (else 0), and
 * whether the stream's trailer follows it */
typedef struct fourmc_bsw_side { uint32_t stream, rawlen, trailer, pad; } fourmc_bsw_side;
/* the tile sums of every table (d_tile0: n + 1 ascending tile numbers, 64 entries a tile) and, per stream with a table, their
 * inclusive prefixes in place and the verdict in d_plans[i].reason (the other fields 0) */
hipError_t fourmc_launch_bsw_sums(const uint32_t* d_writes, const fourmc_bstream_enc_item* d_items, const uint64_t* d_tile0, uint32_t n,
                                  uint64_t ntiles, uint64_t* d_sums, fourmc_bsw_plan* d_plans, hipStream_t s);
/* d_groups NULL: d_plans[i] = the plan of stream i (a stream with a table keeps a verdict the sums gave it); else the group tables
 * of the streams with a table whose reason is FOURMC_BSW_OK, at d_slices[i].group0 */
hipError_t fourmc_launch_bsw_chase(const uint32_t* d_writes, const fourmc_bstream_enc_item* d_items, const uint64_t* d_tile0,
                                   const uint64_t* d_prefix, uint32_t n, uint32_t max_input, int zstd, fourmc_bsw_plan* d_plans,
                                   const fourmc_bsw_slice* d_slices, fourmc_bsw_group* d_groups, hipStream_t s);
/* the descriptors and side entries of chunks c0 .. c0 + m - 1; the staging offsets count from chunk c0's slot */
hipError_t fourmc_launch_bsw_desc(const fourmc_bstream_enc_item* d_items, const fourmc_bsw_plan* d_plans, const fourmc_bsw_slice* d_slices,
                                  const fourmc_bsw_group* d_groups, uint32_t n, uint32_t max_input, int zstd, int nolimit, uint64_t c0,
                                  uint32_t m, fourmc_block* d_blocks, fourmc_bsw_side* d_side, hipStream_t s);
/* after the codec: the segmented scan of the round's chunks from and back into d_carry[stream], then the pack */
hipError_t fourmc_launch_bsw_pack(void* d_images, const fourmc_bstream_enc_item* d_items, fourmc_block* d_blocks,
                                  const fourmc_bsw_side* d_side, uint64_t* d_off, uint32_t m, int zstd, const void* d_staging,
                                  uint64_t* d_carry, fourmc_bstream_enc_summary* d_sum, hipStream_t s);
/* d_bytes[i] = the length of stream i (0 for one with a verdict); writes the four bytes of a stream without a chunk */
hipError_t fourmc_launch_bsw_result(const fourmc_bstream_enc_item* d_items, const fourmc_bsw_plan* d_plans, const uint64_t* d_carry,
                                    uint32_t n, void* d_images, uint64_t* d_bytes, hipStream_t s);
/* fourmc_gpu_images_compress_writes (image.hip): .4mc / .4mz images whose blocks are the chunks of the plan above at M = 4 MiB.
 * Per stream on the device: the bytes of its blocks placed so far (the 64-bit carry of the scan) and its stored blocks; what the
 * tail leaves per stream for the read-back. */
typedef struct fourmc_imgw_run { uint64_t bytes, stored; } fourmc_imgw_run;
typedef struct fourmc_imgw_result { uint64_t image_bytes, stored; } fourmc_imgw_result;
/* after the raw codec launch over the round's m blocks (d_blocks, d_side from fourmc_launch_bsw_desc): d_seal[b] describes the bytes
 * block b writes behind its header, counted from one base address - src_delta + src_off for a stored block (src_len <= result),
 * stage_delta + dst_off for a compressed one - in dst_off, their number in result and the block's length in src_len; d_idx[b] = the
 * absolute offset of block b's header in d_images, by a segmented scan from and back into d_run[stream]; bad codec results (outside
 * [1, bound]) are counted in *d_bad and stored */
hipError_t fourmc_launch_imgw_seal(const fourmc_block* d_blocks, const fourmc_bsw_side* d_side, uint32_t m, int zstd,
                                   const fourmc_bstream_enc_item* d_items, uint64_t src_delta, uint64_t stage_delta,
                                   fourmc_block* d_seal, uint64_t* d_idx, fourmc_imgw_run* d_run, uint64_t* d_bad, hipStream_t s);
/* one workgroup per stream that is FOURMC_BSW_OK: header, end mark and footer from its slice of d_idx; d_res[i] for every stream */
hipError_t fourmc_launch_imgw_tail(void* d_images, const fourmc_bstream_enc_item* d_items, const fourmc_bsw_plan* d_plans,
                                   const fourmc_bsw_slice* d_slices, const uint64_t* d_idx, const fourmc_imgw_run* d_run, uint32_t n,
                                   uint32_t magic, fourmc_imgw_result* d_res, hipStream_t s);
/* fourmc_gpu_lines_pack and the two line writers (lines_pack.hip).  An item on the device (the engine uploads n + 1 of them, the last
 * one with the totals in tile0 and off0): its lines, its place, its first tile of 64 lines counted over all items and the first of
 * its n_lines + 1 per-line offsets.  Its tile prefixes are the tiles + 1 entries of d_prefix from tile0 + (the item's number) on. */
typedef struct fourmc_lp_item {         /* 64 bytes */
    uint64_t line_off, n_lines, packed_off, packed_cap, writes_off;
    uint64_t tile0, off0, pad;
} fourmc_lp_item;
/* what the measure leaves per item for the read-back (n + 1 entries; entry n: bytes = packed_off = the bytes of all items that are
 * OK, chunk0 = the chunks of the gather) */
typedef struct fourmc_lp_sum {          /* 32 bytes */
    uint64_t bytes;            /* T: the packed text's length (0 for _WRITE and _LINE)                      */
    uint64_t packed_off;       /* where it goes: the item's own packed_off, or (mode 2) behind the items before it */
    uint64_t chunk0;           /* its first chunk of the gather, counted over all items                     */
    int32_t  reason;           /* FOURMC_BSW_OK / _WRITE / _LINE / _CAP                                     */
    uint32_t pad;
} fourmc_lp_sum;
/* the lengths, offsets in the tile (d_off), tile prefixes (d_prefix: ntiles + n entries), T and verdicts; mode 0: the query, 1: the
 * items' own places with _CAP, 2: the items placed one behind the other from byte 0; base16: the packed buffer's address mod 16 */
hipError_t fourmc_launch_lp_measure(const fourmc_lines_src* src, const fourmc_lp_item* d_items, uint32_t n, uint64_t ntiles, int mode,
                                    uint32_t base16, uint64_t* d_prefix, uint64_t* d_off, fourmc_lp_sum* d_sums, hipStream_t s);
/* for the items that are OK: the 64-bit offset of every line, the write table (d_writes NULL: none) and the gather into d_packed
 * (NULL: none), nchunks workgroups */
hipError_t fourmc_launch_lp_copy(const fourmc_lines_src* src, const fourmc_lp_item* d_items, const fourmc_lp_sum* d_sums, uint32_t n,
                                 uint64_t ntiles, uint64_t nchunks, const uint64_t* d_prefix, uint64_t* d_off, void* d_packed,
                                 uint32_t* d_writes, hipStream_t s);
#ifdef FOURMC_RESEARCH      /* the research side build exports these two: tools/zstd_timing.py and tools/k7x_prof.py size their read-backs with them */
#pragma GCC visibility push(default)
#endif
size_t     fourmc_zstd_scratch_bytes(uint32_t n);
size_t     fourmc_zstd_dec_counter_offset(void);
#ifdef FOURMC_RESEARCH
#pragma GCC visibility pop
#endif
hipError_t fourmc_launch_zstd_decode(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                     void* d_scratch, int container_mode, hipStream_t stream);
size_t     fourmc_zstd_enc_work_bytes(uint32_t n, int level);
int        fourmc_zstd_enc_level_ok(int level);                 /* 1: the device has every strategy the level's rows name (levels 1..12) */
hipError_t fourmc_launch_zstd_encode(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                     void* d_work, int container_mode, int level, int serial, hipStream_t stream);
/* streamed .zst frames (zstd_encode.hip): one wave per job.  d_jobs holds the n_fast jobs of the "fast" levels, then the n_dfast jobs
 * of the "dfast" levels; a job names its item, its level and its slice of d_work (fourmc_zstd_enc_work_bytes(1, level) bytes).  The
 * kernels write each job's item status on the device. */
typedef struct fourmc_zstw_job { uint32_t item; int32_t level; uint64_t work_off; } fourmc_zstw_job;
int        fourmc_zst_stream_strategy(int level);              /* 1 fast, 2 dfast, 0: not a level of the streamed kernels */
hipError_t fourmc_launch_zst_stream(const void* d_src, void* d_images, fourmc_zstw_item* d_items, const fourmc_zstw_job* d_jobs,
                                    uint32_t n_fast, uint32_t n_dfast, void* d_work, hipStream_t stream);
hipError_t fourmc_launch_xxh32(const void* d_base, fourmc_block* d_blocks, uint32_t n,
                               uint32_t seed, int mode, hipStream_t stream);
/* .zst streams (zst.hip).  The whole decode of n streams lives there; the engine hands it its workspace registries through `ws`
 * (which: 0 tables, 1 one round's areas, 2 the serial decoder's literal buffers; a buffer that grows loses its contents) and gets a
 * FOURMC_* code back, with the text in err */
typedef int (*fourmc_zst_ws_fn)(void* ctx, int which, size_t need, void** out);
int        fourmc_zst_run(const void* d_images, void* d_dst, fourmc_zst_item* items, uint32_t n, uint32_t round_blocks,
                          fourmc_zst_ws_fn ws, void* ws_ctx, char* err, size_t err_cap, hipStream_t s);
size_t     fourmc_zst_per_block_bytes(void);               /* workspace of one table entry of a round */
int        fourmc_zst_counts(unsigned long long* c3);      /* fast frames, serial frames, fast blocks since the last call; -1: device error */

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif

// the CLI's exit code for each verdict of an image decode (fourmc_file.c: the DIE() of each message)
static inline __host__ __device__ int32_t fourmc_image_exit_code(int32_t reason)
{
    switch (reason) {
        case FOURMC_IMG_OK: return 0;
        case FOURMC_IMG_BLOCK_SIZE_UNREADABLE: case FOURMC_IMG_DATA_UNREADABLE: case FOURMC_IMG_FOOTER_SHORT: return 2;
        case FOURMC_IMG_FOOTER_UNREADABLE: case FOURMC_IMG_DST_SMALL: return 1;
        default: return 4;
    }
}

// The codec's bound for n <= 4 MiB bytes of input, on the device: LZ4_compressBound (lz4.h:212) or ZSTD_compressBound (zstd.h:206).
// The engine's own arithmetic (M, fourmc_gpu_bstream_bound) goes through fourmc_LZ4_compressBound / fourmc_ZSTD_compressBound.
static inline __host__ __device__ uint32_t fourmc_bstream_block_bound(int zstd, uint32_t n)
{
    if (zstd) return n + (n >> 8) + (n < (128u << 10) ? ((128u << 10) - n) >> 11 : 0u);
    return n + n / 255u + 16u;
}

#ifdef __HIPCC__
// A block descriptor arrives through a vector load.  Everything a wave-per-block kernel derives from it (lengths, limits, loop
// counters, pointers) is wave-uniform: pin the fields to scalar registers, or those values live in vector registers and the
// kernel's scalar control flow is computed on the vector unit.
__device__ __forceinline__ fourmc_block uniform_block(const fourmc_block& v)
{
    auto u32 = [](uint32_t x) { return uint32_t(__builtin_amdgcn_readfirstlane(int(x))); };
    auto u64 = [&](uint64_t x) { return (uint64_t(u32(uint32_t(x >> 32))) << 32) | u32(uint32_t(x)); };
    fourmc_block r;
    r.src_off = u64(v.src_off); r.dst_off = u64(v.dst_off); r.src_len = u32(v.src_len); r.dst_cap = u32(v.dst_cap);
    r.result = int32_t(u32(uint32_t(v.result))); r.xxh32 = u32(v.xxh32);
    return r;
}
#endif
#endif
