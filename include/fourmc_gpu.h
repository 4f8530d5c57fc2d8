/*
 * include/fourmc_gpu.h — C ABI of the MI355X block engine behind 4mc's codec call sites.
 *
 * This is the drop-in boundary for the hot path of fingltd/4mc (SURVEY.md §8(a),(b)): every place
 * where the reference calls ONE codec function on ONE <=4 MiB block
 *     native/4mc.c:301,311,323  (compress loop),  :637,645,661 (decode loop), 4mz twins :467,:810
 *     native/jniCompressor.c:91,124,157   native/jniDecompressor.c:88
 *     native/jniZstdCompressor.c:93,126,159   native/jniZstdDecompressor.c:90
 * is served here, with independent blocks batched into single HIP launches on gfx950.
 *
 * Plain pointers and sizes only; no C++ or torch types.  `stream` is a hipStream_t passed as
 * void* (NULL = the null stream).  All `d_` pointers are device (HBM) pointers.
 * Every function returns FOURMC_OK or a negative FOURMC_E* code; nothing here ever falls back to
 * a CPU codec: without a usable gfx950 device the calls fail with FOURMC_ENODEV.
 */
#ifndef FOURMC_GPU_H
#define FOURMC_GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FOURMC_BLOCKSIZE   (4u * 1024u * 1024u)   /* native/4mc.c:116                          */
#define FOURMC_MAGIC_4MC   0x344D4300u            /* native/4mc.c:111                          */
#define FOURMC_MAGIC_4MZ   0x344D5A00u            /* native/4mc.c:112                          */

enum {
    FOURMC_OK       =  0,
    FOURMC_ENODEV   = -1,   /* no HIP device / wrong architecture                              */
    FOURMC_EHIP     = -2,   /* a HIP runtime call failed (fourmc_gpu_last_error() has the text) */
    FOURMC_EINVAL   = -3,
    FOURMC_ENOMEM   = -4,
    FOURMC_EUNSUP   = -5    /* codec/level not implemented on the device (zstd outside 1..12)  */
};

/* Codec selectors: the (function, level) pairs 4mc can reach (native/4mc.c:243-253,:411-419). */
enum {
    FOURMC_CODEC_LZ4_FAST = 0,   /* LZ4_compress_default            4mc -1  (Lz4Compressor)    */
    FOURMC_CODEC_LZ4_MC   = 1,   /* LZ4_compressMC                  4mc -2                     */
    FOURMC_CODEC_LZ4_HC   = 2,   /* LZ4_compress_HC(any level)      4mc -3 / -4 = 4 / 8        */
    FOURMC_CODEC_ZSTD     = 3    /* ZSTD_compress(level 1..12)      4mz -1..-4 = 1/3/6/12      */
};

/* One independent block.  Offsets are relative to the base pointers given to the batch call, so
 * one descriptor array describes a whole file image resident in HBM.  32 bytes, no padding. */
typedef struct fourmc_block {
    uint64_t src_off;   /* in : byte offset of the block's input                                */
    uint64_t dst_off;   /* in : byte offset of the block's output                               */
    uint32_t src_len;   /* in : input bytes                                                     */
    uint32_t dst_cap;   /* in : output capacity in bytes                                        */
    int32_t  result;    /* out: codec return value (reference convention, see each call)        */
    uint32_t xxh32;     /* out (encode/hash) or in (4mc decode: expected checksum)              */
} fourmc_block;

/* ---- device management ------------------------------------------------------------------- */
int         fourmc_gpu_device_count(void);           /* >=0, or FOURMC_ENODEV                    */
int         fourmc_gpu_init(int device);             /* select device, check gfx950              */
const char* fourmc_gpu_last_error(void);
const char* fourmc_gpu_arch(void);                   /* "gfx950:..." of the selected device      */

/* ---- raw block codecs, device resident (one launch for `n` blocks) ------------------------ */
/* result = LZ4_decompress_safe(src, dst, src_len, dst_cap)        native/lz4/lz4.c:2345        */
int fourmc_gpu_lz4_decompress(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                              uint32_t n, void* stream);
/* result = LZ4_compress_default(src, dst, src_len, dst_cap)       native/lz4/lz4.c:1435
 * (0 = does not fit dst_cap).  Payload bytes identical to the reference 64-bit LE build.      */
int fourmc_gpu_lz4_compress_fast(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                                 uint32_t n, void* stream);
/* result = LZ4_compress_HC(src, dst, src_len, dst_cap, level) for any int level, byte-identical payloads
 * (native/lz4/lz4hc.c:958-973): level <= 0 is the default 9 and level > 12 is 12 (:840-841); 1..8 hash chain
 * (4mc High = 4, Ultra = 8), 9 hash chain with pattern analysis, 10..12 the optimal parser.              */
int fourmc_gpu_lz4_compress_hc(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                               uint32_t n, int level, void* stream);
/* result = LZ4_compressMC_limitedOutput(src, dst, src_len, dst_cap), or LZ4_compressMC (no limit)
 * when dst_cap == 0xFFFFFFFF; byte-identical payloads           native/lz4/lz4mc.c:582-606         */
int fourmc_gpu_lz4_compress_mc(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                               uint32_t n, void* stream);
/* LZ4 fast encoder of fourmc_gpu_lz4_compress_fast and of the LZ4-fast container encode: 0 (default) the reference parse, payload
 * bytes identical to the reference build; 1 the ratio-tolerance encoder (lz4_par_encode.hip): every payload is one valid LZ4 block
 * that LZ4_decompress_safe decodes to the input, but NOT the reference's bytes - sizes within 3 % of the reference parse on the
 * S-mix (north_star: "otherwise compression ratio is reported within a stated tolerance").  Blocks up to 4 MiB are compressed as
 * 64 KiB segments in parallel; what lies beyond 4 MiB of a block goes out as literals.  env FOURMC_LZ4_ENCODE = exact | parallel. */
void fourmc_gpu_set_lz4_encode_mode(int mode);
int  fourmc_gpu_get_lz4_encode_mode(void);
/* Tuning knob (not part of the reference boundary): which LZ4 decode path serves the launches - 6 auto (default: the tile path
 * up to 1536 blocks per launch, the segment-parallel path above), 2 the exact walker alone (what an automatic choice ends at when
 * no workspace can be had), 11 the segment-parallel path, 13 the tile path; results are identical (env FOURMC_DECODE = auto | exact |
 * seg | tile).  Any other value selects auto: the designs measured and not kept are sources under tools/research/. */
void fourmc_gpu_set_lz4_decode_path(int path);
int  fourmc_gpu_get_lz4_decode_path(void);
/* Tuning knob: 4mz decode as entropy kernel + execute kernel (1, default; FOURMC_ZDECODE=split) or all in the one-wave kernel
 * (0; FOURMC_ZDECODE=single); results are identical. */
void fourmc_gpu_set_zstd_decode_split(int on);
int  fourmc_gpu_get_zstd_decode_split(void);
/* Statistics (read-only, not part of the reference boundary): one-block host calls made so far (the LZ4_* / ZSTD_* twins and the
 * JNI entry points: one call = one block) and the launches that served them - calls that arrive while a launch is in flight
 * share the next one (engine_host.hip: host_one), so launches < calls under concurrency. */
void fourmc_gpu_one_block_stats(unsigned long long* calls, unsigned long long* launches);
/* The engine keeps one device workspace per stream and reuses it (the segment-parallel LZ4 decode of 8192 blocks needs 92 GB, the zstd
 * level-12 encoder 48 MiB per block).  This frees them all, synchronizing each stream first; the next call allocates again. */
int fourmc_gpu_release_workspaces(void);
/* result = ZSTD_compress(dst + dst_off, dst_cap, src + src_off, src_len, level) as int: frame bytes, or
 * -(ZSTD error number), e.g. -70 = dstSize_tooSmall        native/zstd/compress/zstd_compress.c:4806
 * Levels 1 .. 12 are on the device, byte-identical for every input size: every strategy their rows of the level table name (clevels.h:25-130:
 * fast, dfast, greedy, lazy, lazy2 with the row-hash or hash-chain finder, and - for inputs of 256 KiB and less - btlazy2 / btopt).  4mz -1 .. -4
 * use 1, 3, 6, 12.  Levels 13 and above (btlazy2 on full blocks, btultra) and levels below 1 return FOURMC_EUNSUP - never different bytes. */
int fourmc_gpu_zstd_compress(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                             uint32_t n, int level, void* stream);

/* result = ZSTD_decompress(dst, dst_cap, src, src_len) as int: decoded bytes, or < 0 where the
 * reference returns an error code (ZSTD_isError)            native/zstd/decompress/zstd_decompress.c:1112 */
int fourmc_gpu_zstd_decompress(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                               uint32_t n, void* stream);
/* xxh32 = XXH32(src + src_off, src_len, seed)                     native/lz4/xxhash.c:392      */
int fourmc_gpu_xxh32(const void* d_src, fourmc_block* d_blocks, uint32_t n, uint32_t seed,
                     void* stream);

/* ---- container-level block ops (what one iteration of the 4mc.c loops does) --------------- */
/* Encode: codec with capacity src_len-1 (native/4mc.c:301); result<=0 => the block is stored
 * raw (:318-329): payload = input, result = src_len.  xxh32 = XXH32(stored payload) (:311,:323).
 * dst_cap must be >= src_len.  `codec`/`level` as FOURMC_CODEC_*.                               */
int fourmc_gpu_4mc_encode_blocks(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                                 uint32_t n, int codec, int level, void* stream);
/* Decode: verify XXH32(payload)==xxh32 (native/4mc.c:637,645); src_len==dst_cap => stored copy
 * (:635-642) else codec decode (:661).  result = decoded bytes, or
 * FOURMC_BLK_BADSUM / FOURMC_BLK_CORRUPT (the two exit-4 conditions of the reference CLI).      */
#define FOURMC_BLK_BADSUM   (-1000000001)
#define FOURMC_BLK_CORRUPT  (-1000000002)
int fourmc_gpu_4mc_decode_blocks(const void* d_src, void* d_dst, fourmc_block* d_blocks,
                                 uint32_t n, int codec, void* stream);

/* Pack: after fourmc_gpu_4mc_encode_blocks, copy each block's 12-byte big-endian header
 * (usize = src_len, csize = result, xxh32; native/4mc.c:309-312) and its payload from the staging
 * slot (d_staging + dst_off) to d_image + d_image_off[b].  d_image_off[b] is the absolute file
 * offset of block b's header = 12 + sum_{j<b}(12 + csize_j) (native/4mc.c:293), i.e. exactly the
 * footer-index entries; the caller (host or RCCL-gathered prefix sum) supplies them.            */
int fourmc_gpu_4mc_pack_image(const void* d_staging, void* d_image, const fourmc_block* d_blocks,
                              const uint64_t* d_image_off, uint32_t n, void* stream);

/* ---- whole file images in device memory ------------------------------------------------------------------------------------
 * "device image in -> device bytes out", with the result the CLI gives for the same bytes as a file.  The calls synchronize
 * `stream`: the encode once (the image size; the encode of many images once as well), the decode twice (the block count its workspace is sized by, then the status),
 * the decode of many images twice as well.  No per-block data crosses to the host. */
/* worst-case image size for src_bytes of input: header + 12 per block + src_bytes + end mark + footer */
uint64_t fourmc_gpu_image_bound(uint64_t src_bytes);
/* d_src[0, src_bytes) -> a complete .4mc (magic FOURMC_MAGIC_4MC) or .4mz (FOURMC_MAGIC_4MZ) file image at d_image, byte-identical
 * to what fourMCcompressFilename / fourMZcompressFilename(level) write for the same input (level as the file API and the CLI:
 * 4mc 1 fast, 2 medium, 3 high, >= 4 ultra; 4mz zstd 1 / 3 / 6 / 12).  image_cap must be >= fourmc_gpu_image_bound(src_bytes);
 * *image_bytes (host) = the image's length. */
int fourmc_gpu_image_compress(const void* d_src, uint64_t src_bytes, void* d_image, uint64_t image_cap,
                              uint64_t* image_bytes, uint32_t magic, int level, void* stream);
/* Many images with one call: the encode's side of fourmc_gpu_images_decompress below.  A job that writes a directory of part files
 * of a few blocks each pays, per fourmc_gpu_image_compress, one synchronization and a codec launch that holds a handful of blocks,
 * and every encoder launch lasts as long as its slowest block.  All sources lie in ONE device buffer and all images go to ONE
 * device buffer, so a single descriptor table describes every block of every image and one container encode serves them all.
 * The one rule.  After the call, items[i].image_bytes and d_images[image_off, image_off + image_bytes) equal what the single-image
 *   compress call above writes for d_src + src_off, src_bytes at the same magic and level: for every level of both formats (the
 *   level -> codec mapping is the shared one), an empty source (the 44-byte image), sources that are no multiple of 4 MiB, under
 *   FOURMC_LZ4_ENCODE=parallel / fourmc_gpu_set_lz4_encode_mode(1) (the bytes the single call gives in that mode), and when the
 *   engine cuts the encode into several launches, wherever a cut falls inside an image.
 * Writes.  Nothing outside the images: every byte of d_images outside each [image_off, image_off + image_bytes) keeps its value.
 * Sources.  Two items may name the same or overlapping source bytes.  d_src and d_images must not overlap each other (not checked).
 * Arguments.  Checked on the host before any device is looked for, the magic first; each of these returns FOURMC_EINVAL with
 *   `items` untouched: a magic that is neither 4mc nor 4mz; items NULL with n > 0; d_src NULL with a nonzero src_bytes; d_images
 *   NULL; a source that does not lie inside [0, src_total) or an image region that does not lie inside [0, images_bytes);
 *   image_cap < fourmc_gpu_image_bound(src_bytes); an item of more than 0x3FFFFFFF blocks; two image regions that overlap (every
 *   region is at least 44 bytes, so the same region twice is an overlap; regions that touch are fine).  n == 0 returns FOURMC_OK
 *   and does nothing.  More than 0x7FFFFFFF blocks in all: FOURMC_EUNSUP.  No device: FOURMC_ENODEV.  A block whose encoder result
 *   falls outside [1, src_len]: FOURMC_EINVAL, the guard image_compress has.  On every failure `items` is left as it came.
 * Staging.  The engine's image workspace holds the encoded blocks before the pack: block b of an image has a slot of its src_len
 *   rounded up to 256 bytes, every slot starts 256-byte aligned and the slots abut, so the staging is
 *   sum over the items of ((src_bytes + 255) & ~255) bytes, plus 4096 bytes of slack behind the last slot - not 4 MiB per block:
 *   ten thousand part files of a few KiB take their own size, not 40 GB.
 * Synchronizations of `stream`: one, however many images there are (the lengths and the count of bad encoder results come back
 *   together).  `items` crosses to the device once.
 * Not reproduced: .4mc and .4mz in one call, sources or images at unrelated device pointers, a batched streaming writer. */
typedef struct fourmc_image_enc_item {   /* 40 bytes */
    uint64_t src_off, src_bytes;         /* in : the input is d_src[src_off, src_off + src_bytes)                 */
    uint64_t image_off, image_cap;       /* in : its image goes to d_images[image_off, image_off + image_cap)     */
    uint64_t image_bytes;                /* out: the image's length                                               */
} fourmc_image_enc_item;
int fourmc_gpu_images_compress(const void* d_src, uint64_t src_total, void* d_images, uint64_t images_bytes,
                               uint32_t magic, int level, fourmc_image_enc_item* items /*host*/, uint32_t n, void* stream);

/* ---- streaming writes of one image: append chunks of any size as they arrive --------------------------------------------------
 * Output.  After finish, d_image[0, *image_bytes) is byte-identical to what fourmc_gpu_image_compress writes for the concatenation
 *   of every appended chunk at the same magic and level, and so to the file `4mc -<level>` / `4mc -z -<level>` writes for that
 *   input.  This holds for every way the input is cut into appends (empty ones, 1-byte ones, appends ending inside a block, exact
 *   multiples of 4 MiB, single appends larger than batch_blocks blocks): blocks are cut at every 4 MiB of the CONCATENATED input,
 *   as the CLI cuts them, and the last block is short.  The level -> codec mapping is the one image_compress shares with the file API, and every setting it
 *   obeys (FOURMC_LZ4_ENCODE among them) applies to the writer in the same way.
 * Begin.  Checks the magic and the pointers, then allocates everything the writer owns in one piece: a 4 MiB carry slot for the
 *   incomplete block, batch_blocks x 4 MiB of staging, the descriptors of one batch, the device index (one 8-byte offset per block
 *   image_cap can hold, plus one) and the device state.  batch_blocks 0 means 512, the file API's batch; it is lowered to the most
 *   blocks image_cap can hold.  The capacity check of append guarantees that the block count never exceeds the index, which never
 *   grows.  FOURMC_EINVAL for a bad magic, a NULL pointer or image_cap < fourmc_gpu_image_bound(0); FOURMC_ENODEV without a device;
 *   FOURMC_ENOMEM when the allocation fails.  On any error *w is left NULL.
 * Append.  Queues work on the writer's stream and returns: no host synchronization, no device-to-host copy, no hipMalloc / hipFree
 *   of its own (the engine's codec workspaces may still grow the first time a batch size is seen, as in every codec call; after
 *   that, appends of the same shape allocate nothing).  The chunk may be reused or freed once the stream has passed the append
 *   (the usual stream-order rule): the bytes of a block still incomplete are copied into the carry slot on the stream, and nothing
 *   reads d_src after the work this append queued.  Capacity is checked on the host before anything is queued: if
 *   fourmc_gpu_image_bound(total + bytes) > image_cap, where total is every byte appended so far, the append returns FOURMC_EINVAL
 *   and the writer is unchanged and still usable.  Chunks larger than batch_blocks blocks are encoded in pieces of at most
 *   batch_blocks blocks, so the writer's own memory stays bounded whatever the input's size.  A completed carry block is encoded
 *   in the same codec launch as the chunk's blocks (from the lower of the two addresses, with 64-bit offsets).
 * Finish.  Encodes the carried tail as the last short block, if there is one, then writes the file header, the end mark and the
 *   footer with its XXH32.  It synchronizes the stream once, to read back the image length and the count of bad encoder results;
 *   if any block's result fell outside [1, src_len] it fails with FOURMC_EINVAL, the guard image_compress has.  *image_bytes is
 *   the image's length.  finish frees the writer whatever it returns.
 * Failures.  After any failure other than the capacity refusal (FOURMC_ENOMEM from a codec workspace, FOURMC_EHIP, ...) the
 *   writer is poisoned: later appends return that first error, and finish returns it and frees.
 * Independence.  The writer owns its buffers and holds no per-stream workspace of the engine between calls, so other engine calls
 *   on the same stream may run between appends (image compress, decompress and read, block encode and decode), and several
 *   writers may be open at once, on one stream or several.  fourmc_gpu_release_workspaces does not touch a writer's buffers: only
 *   finish and abort free them.  A writer is used by one thread at a time.  abort frees the writer without an image (it waits for
 *   the work queued on the stream first); abort(NULL) does nothing. */
typedef struct fourmc_image_writer fourmc_image_writer;      /* opaque */
int  fourmc_gpu_image_writer_begin(fourmc_image_writer** w, void* d_image, uint64_t image_cap, uint32_t magic, int level,
                                   uint32_t batch_blocks, void* stream);
int  fourmc_gpu_image_writer_append(fourmc_image_writer* w, const void* d_src, uint64_t bytes);
int  fourmc_gpu_image_writer_finish(fourmc_image_writer* w, uint64_t* image_bytes);   /* frees w, whatever it returns */
void fourmc_gpu_image_writer_abort(fourmc_image_writer* w);                         /* frees w; NULL is a no-op */

/* the verdict of an image decode: which of the CLI's messages (fourmc_file.c: decode_stream) it ends with */
enum {
    FOURMC_IMG_OK                    = 0,
    FOURMC_IMG_MAGIC_UNREADABLE      = 1,   /* exit 4 */
    FOURMC_IMG_NOT_4MC               = 2,   /* exit 4 */
    FOURMC_IMG_HEADER_UNREADABLE     = 3,   /* exit 4 */
    FOURMC_IMG_VERSION               = 4,   /* exit 4 */
    FOURMC_IMG_HEADER_CHECKSUM       = 5,   /* exit 4 */
    FOURMC_IMG_BLOCK_SIZE_UNREADABLE = 6,   /* exit 2 */
    FOURMC_IMG_CSIZE_BEYOND          = 7,   /* exit 4 */
    FOURMC_IMG_DATA_UNREADABLE       = 8,   /* exit 2 */
    FOURMC_IMG_USIZE_BEYOND          = 9,   /* exit 4 */
    FOURMC_IMG_BLOCK_CHECKSUM        = 10,  /* exit 4 */
    FOURMC_IMG_CORRUPT               = 11,  /* exit 4 */
    FOURMC_IMG_FOOTER_UNREADABLE     = 12,  /* exit 1 */
    FOURMC_IMG_FOOTER_SHORT          = 13,  /* exit 2 */
    FOURMC_IMG_FOOTER_CHECKSUM       = 14,  /* exit 4 */
    FOURMC_IMG_FOOTER_VERSION        = 15,  /* exit 4 */
    FOURMC_IMG_DST_SMALL             = 16   /* exit 1: total_bytes > dst_cap, nothing decoded (the CLI has no such case) */
};
typedef struct fourmc_image_status {
    uint64_t decoded_bytes;   /* bytes at d_dst the CLI would have written before it stopped: the sum of the decoded sizes.
                               * Exception: a crafted block that decodes to fewer bytes than its usize is no error to the CLI,
                               * which writes what it decoded and closes the gap; here block i still sits at the usize prefix,
                               * so d_dst[:decoded_bytes] is then not the CLI's output although the verdict is OK           */
    uint64_t total_bytes;     /* sum of usize of every well-formed block before the framing verdict (the size query's answer)  */
    uint64_t fail_offset;     /* image offset of the header / block header / footer that ended decoding; image_bytes if none   */
    uint32_t streams, blocks; /* streams whose header passed; blocks decoded (parse only: well-formed blocks)                    */
    int32_t  exit_code;       /* 0, or the CLI's exit code for this image (1, 2, 4)                                            */
    int32_t  reason;          /* FOURMC_IMG_*                                                                                  */
} fourmc_image_status;
/* d_image[0, image_bytes) -> decoded bytes at d_dst: block i at the sum of the usizes of the blocks before it, across streams.
 * d_dst NULL: parse only (total_bytes, blocks and the framing verdict; no payload is checked).  As the CLI's loop over
 * concatenated streams, decoding ends cleanly after a stream whose blocks add up to 0 bytes, whatever follows it.  Bytes past decoded_bytes are
 * unspecified.  total_bytes > dst_cap: FOURMC_IMG_DST_SMALL, nothing written.  The decoders may read up to 64 bytes past a
 * payload, as with fourmc_gpu_4mc_decode_blocks.  env FOURMC_IMAGE_PARSE=walk forces the file-order walk (test knob). */
int fourmc_gpu_image_decompress(const void* d_image, uint64_t image_bytes, void* d_dst, uint64_t dst_cap,
                                uint32_t magic, fourmc_image_status* status, void* stream);
/* Many images with one call: a Hadoop dataset is a directory of part files of a few blocks each, and one call per image leaves
 * most of the chip idle for a launch latency per file.  All images lie in ONE device buffer and all outputs go to ONE device
 * buffer, so a single descriptor table describes every block of every image and one block decode serves them all.
 * The one rule.  After the call, items[i].status equals, field for field, what the single-image decompress call above returns
 *   for d_images + image_off, image_bytes, d_dst + dst_off, dst_cap and the same magic, and d_dst[dst_off, dst_off +
 *   decoded_bytes) holds the same bytes: for clean images, framing damage of every kind, a block that fails its XXH32 or its
 *   decode, concatenated streams, trailing bytes, the empty stream that ends a file, and FOURMC_IMG_DST_SMALL when the image's
 *   total_bytes exceeds its own dst_cap (nothing written for that image).  fail_offset is an offset in the image, not in the
 *   buffer.  A damaged image changes nothing about its neighbours.  Two items may name the same image bytes.
 * Size query.  d_dst NULL: the parse-only statuses of every item; dst_off, dst_cap and dst_bytes are ignored.
 * Writes.  Nothing outside the items' output regions; for an item, nothing outside [dst_off, dst_off + total_bytes).
 * Arguments.  Checked on the host before any device is looked for; each of these returns FOURMC_EINVAL with `items` untouched: a
 *   magic that is neither 4mc nor 4mz; items NULL with n > 0; d_images NULL with a nonzero image_bytes; an image that does not
 *   lie inside [0, images_bytes); with d_dst not NULL, an output region that does not lie inside [0, dst_bytes), or two output
 *   regions of nonzero dst_cap that overlap.  n == 0 returns FOURMC_OK and does nothing.  More than 0x7FFFFFFF blocks in all:
 *   FOURMC_EUNSUP.  No device: FOURMC_ENODEV.  On every failure `items` is left as it came.
 * Slack.  The decoders may read up to 64 bytes past a payload: inside the buffer that is the next image; behind the last image
 *   the caller keeps slack, as with the single call.
 * Settings.  FOURMC_IMAGE_PARSE=walk, FOURMC_DECODE, FOURMC_ZDECODE and the batch limits of the block decode apply as they do to
 *   the single call; the parse statistics below count each image once, under the parser that accepted it.
 * Synchronizations of `stream`: two, however many images there are (the block count the workspace is sized by, then the
 *   statuses); the size query takes one.  `items` crosses to the device once and the statuses come back once.
 * Not reproduced: .4mc and .4mz in one call, images at unrelated device pointers. */
typedef struct fourmc_image_item {      /* 72 bytes */
    uint64_t image_off, image_bytes;    /* in : the image is d_images[image_off, image_off + image_bytes)           */
    uint64_t dst_off, dst_cap;          /* in : its output region is d_dst[dst_off, dst_off + dst_cap)              */
    fourmc_image_status status;         /* out                                                                       */
} fourmc_image_item;
int fourmc_gpu_images_decompress(const void* d_images, uint64_t images_bytes, void* d_dst, uint64_t dst_bytes,
                                 uint32_t magic, fourmc_image_item* items /*host*/, uint32_t n, void* stream);
/* the exact text fourmc_file.c prints for a FOURMC_IMG_* verdict ("" for FOURMC_IMG_OK) */
const char* fourmc_gpu_image_reason_text(int reason);
/* Statistics (read-only): images fourmc_gpu_image_decompress has parsed so far with the footer-driven fast path and with the
 * file-order walk (everything the fast path does not prove: concatenations, damage, FOURMC_IMAGE_PARSE=walk). */
void fourmc_gpu_image_parse_stats(unsigned long long* fast, unsigned long long* walk);

/* ---- streaming reads of one image: append chunks of any size as they arrive, in file order ------------------------------------
 * The one rule.  After finish, *status equals, field for field, what fourmc_gpu_image_decompress returns for the concatenation of
 *   every appended chunk (N bytes in all) with the same d_dst, dst_cap and magic, and d_dst[0, decoded_bytes) holds the same bytes.
 *   This holds for every way the image is cut: empty and 1-byte appends, cuts inside the file header, a block header, a payload,
 *   the end mark, the footer's size field or its body, appends of many blocks, concatenated streams, trailing bytes and bytes
 *   after the empty stream that ends a file.  The reader never writes outside [d_dst, d_dst + dst_cap).
 *   - A check that needs bytes not yet appended waits ("magic unreadable", "cannot read next block size", "cannot read data
 *     block", "unreadable footer", "footer short"): finish decides it with N.  fail_offset is an offset in the image, not in a
 *     chunk; for an image that decodes cleanly it is N.
 *   - FOURMC_IMG_DST_SMALL is decided as image_decompress decides it: the sum of the usizes of the well-formed blocks is compared
 *     with dst_cap, and that check wins over a block that failed its checksum.  The one difference: the blocks that fit may
 *     already have been written (a block that would end past dst_cap is never decoded).
 *   - Once the verdict is final (a framing error, or the clean end after a stream whose blocks add up to 0 bytes), later appends
 *     are accepted; they count toward N and cost nothing more.  A footer may claim any size up to 4 GiB: its XXH32 is a
 *     streaming state carried across appends, and the footer is never buffered.
 *   The block decode is fourmc_gpu_4mc_decode_blocks with the magic's codec (payload XXH32, then LZ4 or zstd), in batches of
 *   batch_blocks from the reader's staging, so every setting it obeys (FOURMC_DECODE, FOURMC_ZDECODE) applies unchanged.
 * Begin.  Checks the magic and the pointers, then allocates everything the reader owns in one piece: batch_blocks staging slots of
 *   4 MiB (with the 64 bytes of slack the block decoders read past a payload), the descriptors and header offsets of one batch,
 *   the copy pieces of one walk and the device state (the walk's position, phase, partial header bytes, running totals and
 *   footer XXH32 state; the fold of the decoded batches).  A block cut by the end of a chunk waits in its own staging slot, so
 *   there is no separate carry slot.  batch_blocks 0 means 512, the writer's and the mapped file path's batch.  FOURMC_EINVAL for a
 *   bad magic or a NULL pointer (d_dst NULL included: there is no parse-only mode); FOURMC_ENODEV without a device; FOURMC_ENOMEM
 *   when the allocation fails.  On any error *r is left NULL.
 * Append.  Queues work on the reader's stream: the walk over the chunk, the copy of its payload bytes into staging, and the decode
 *   of each batch it fills.  No hipMalloc / hipFree of its own (the engine's decode workspaces may grow, as in every decode call).
 *   It synchronizes the stream once to read back what the walk found, plus once for each further batch the chunk fills.  The
 *   reader never reads outside [d_chunk, d_chunk + bytes), so chunks cut from files and sockets need no slack, and the chunk may be
 *   reused or freed once the stream has passed the append.
 * Finish.  Decodes the last partial batch, decides the checks that waited with N, folds in the first failing block in file order,
 *   writes *status and synchronizes the stream.  finish frees the reader whatever it returns.
 * Failures.  An argument check (a NULL reader, a NULL chunk of nonzero length) fails the call and leaves the reader as it was.
 *   After any other failure (FOURMC_ENOMEM from a decode workspace, FOURMC_EHIP, ...) the reader is poisoned: later appends
 *   return that first error, and finish returns it and frees.
 * Independence.  The reader owns its buffers and holds no per-stream workspace of the engine between calls, so other engine calls
 *   on the same stream may run between appends, and several readers and writers may be open at once, on one stream or several.
 *   fourmc_gpu_release_workspaces does not touch a reader's buffers.  A reader is used by one thread at a time.  abort frees the
 *   reader without a status (it waits for the work queued on the stream first); abort(NULL) does nothing. */
typedef struct fourmc_image_reader fourmc_image_reader;      /* opaque */
int  fourmc_gpu_image_reader_begin(fourmc_image_reader** r, void* d_dst, uint64_t dst_cap, uint32_t magic,
                                   uint32_t batch_blocks, void* stream);
int  fourmc_gpu_image_reader_append(fourmc_image_reader* r, const void* d_chunk, uint64_t bytes);
int  fourmc_gpu_image_reader_finish(fourmc_image_reader* r, fourmc_image_status* status);  /* frees r, whatever it returns */
void fourmc_gpu_image_reader_abort(fourmc_image_reader* r);                                /* frees r; NULL is a no-op */

/* ---- random access into single-stream images in device memory ---------------------------------------------------------------
 * The device twins of fourmc_file_block_count / fourmc_file_decode_blocks (include/fourmc.h): the image's footer index, the
 * decode of a block range, and reads of decoded byte ranges.  Every verdict is the one fourmc_file_decode_blocks reaches on the
 * same bytes written to a file (its read_index and per-block checks, in their order); the format comes from the image's header.
 * Synchronizations of `stream`: image_index 1, image_decode_blocks 2, image_read 3.  No per-block data crosses to the host, and
 * the decoders may read up to 64 bytes past a payload, as with fourmc_gpu_4mc_decode_blocks. */
/* one block: its footer entry and its block header (zeros when the header lies beyond the image).  32 bytes. */
typedef struct fourmc_image_entry {
    uint64_t image_off;   /* offset of the block's 12-byte header (the footer index, absolute)  */
    uint64_t data_off;    /* offset of its first decoded byte = sum of usize of the blocks before it */
    uint32_t usize, csize, xxh32, pad;
} fourmc_image_entry;
typedef struct fourmc_image_index_info {
    int64_t  nblocks;       /* what fourmc_file_block_count returns for the same bytes: n, or -1 / -2                    */
    int64_t  framing;       /* what fourmc_file_decode_blocks(0, n) with unlimited dst_cap would return if every payload
                             * decoded correctly: 0, or its -1 / -2 / -4 from the per-block header checks (nblocks when < 0) */
    uint64_t total_bytes;   /* sum of usize (meaningful when framing == 0)                                               */
    int32_t  is_zstd, pad;  /* 1 for a .4mz image (0 when nblocks < 0)                                                   */
} fourmc_image_index_info;
/* The index of d_image[0, image_bytes).  d_entries NULL: the summary only; else min(nblocks, entries_cap) entries. */
int fourmc_gpu_image_index(const void* d_image, uint64_t image_bytes, fourmc_image_entry* d_entries, uint64_t entries_cap,
                           fourmc_image_index_info* info, void* stream);
/* Blocks [first, first+count) into d_dst, block i at data_off[i] - data_off[first].  *result (host) is what
 * fourmc_file_decode_blocks returns for the same bytes as a file: decoded bytes, or -1 / -2 / -3 / -4 / -5; its -6 (engine error)
 * is this function's return code instead.  Nothing is written to d_dst unless every framing check of the range passes. */
int fourmc_gpu_image_decode_blocks(const void* d_image, uint64_t image_bytes, uint32_t first, uint32_t count,
                                   void* d_dst, uint64_t dst_cap, int64_t* result, void* stream);
/* Batched reads of decoded bytes: range i writes bytes [offset, offset+length) of the image's content to d_dst + dst_off.
 * `ranges` is a host array; each range's result, in order of precedence:
 *   info.nblocks if < 0, else info.framing if != 0   the image cannot be indexed: every range gets this code;
 *   0                        length == 0;
 *   -3                       offset + length > total_bytes (nothing written);
 *   -5                       dst_off + length > dst_cap (nothing written);
 *   -4                       a block the range covers failed its XXH32, failed to decode, or decoded to a size other than its
 *                            usize; the range's destination bytes are then unspecified;
 *   length                   all bytes written.
 * The blocks a range covers are those from the one holding its first byte to the one holding its last.  A block wholly inside a
 * range is decoded straight into the range's destination; a partly covered one is decoded once into a 4 MiB staging slot, however
 * many ranges share it, and the covered bytes are copied from there.  Destinations that overlap are FOURMC_EINVAL, checked
 * before any launch.  Bytes of d_dst outside every range's [dst_off, dst_off+length) are never written.  The staging stays with
 * the stream until fourmc_gpu_release_workspaces. */
typedef struct fourmc_image_range { uint64_t offset, length, dst_off; int64_t result; } fourmc_image_range;   /* 32 bytes */
int fourmc_gpu_image_read(const void* d_image, uint64_t image_bytes, fourmc_image_range* ranges, uint32_t nranges,
                          void* d_dst, uint64_t dst_cap, void* stream);

/* ---- the line records of a Hadoop split, from a single-stream image in device memory -----------------------------------------
 * What FourMcInputFormat.getSplits and FourMcLineRecordReader do between them (java/hadoop-4mc: mapreduce/FourMcInputFormat.java:
 * 159-168, mapreduce/FourMcLineRecordReader.java): a raw byte slice of the file is aligned to block headers, and the reader of the
 * aligned split skips its first line unless it starts the file, then reads lines while its position is <= the split's end - so
 * every line has exactly one owner.  Both calls obey the settings image_read obeys (FOURMC_DECODE, FOURMC_ZDECODE); no per-block
 * data crosses to the host.  Synchronizations of `stream`: image_align_slices 2 (1 for an image without blocks); image_read_records
 * 3 + one per staged tail block (usually 1; 0 when split_end is at or past the end mark; more only while a line longer than a
 * block has shown no delimiter), less when a check ends the call early; image_read_lines the same, plus one when a staged tail
 * block ends with a CR and is not the last block (the next block's first byte says whether that CR ends the line).
 * image_read_records cuts at ONE caller-chosen byte and a record includes it; the lines Hadoop's default LineReader hands to a
 * mapper (LF, lone CR and CR LF end a line, the terminator stripped, the text cut at max.line.length) are image_read_lines'.
 * Not reproduced by either: multi-stream images are refused as in the random-access group (the index code). */
typedef struct fourmc_image_slice {       /* 48 bytes */
    uint64_t start, end;                  /* in : raw byte slice [start, end) of the image, as FileInputFormat cuts it */
    uint64_t split_start, split_end;      /* out: aligned as FourMcBlockIndex.java:142-173 with fileSize = image_bytes: what
                                           *      fourmc_index_align_start / _align_end return (split_start ~0 when dropped) */
    uint32_t first_block, block_count;    /* out: blocks whose headers lie in [split_start, split_end) (0, 0 when dropped) */
    int64_t  result;                      /* out: 1 kept, 0 dropped (start found no block before end),
                                           *      or info.nblocks / info.framing when the image cannot be indexed */
} fourmc_image_slice;
/* start == 0 stays 0, so [0, e) with e <= 12 is kept with zero blocks.  An image with an empty index (zero blocks) returns each
 * slice unchanged with result = 1: the reference's "leave the default split". */
int fourmc_gpu_image_align_slices(const void* d_image, uint64_t image_bytes, fourmc_image_slice* slices /*host*/, uint32_t n,
                                  void* stream);
/* The records of the split [split_start, split_end).  split_start must be 0 or the offset of a block header; split_end a block
 * header's offset not below split_start, or any value at or past the end mark.  T: the total decoded size; ds: the decoded offset
 * of the block at split_start (0 for 0); de: that of the block at split_end (T when it is no block header).  A record is a maximal
 * run of bytes ending with `delim`, inclusive; the content's final unterminated run, if not empty, is a record too.  The split owns
 * the records whose first byte s has s <= de and (split_start == 0 or s > ds):
 *   lo = 0 when split_start == 0, else 1 + the position of the first delimiter in [ds, de) (none: the split owns nothing);
 *   hi = 1 + the position of the first delimiter at or after de (none: T);  the owned records are the records of [lo, hi).
 * Output: d_dst[0, hi - ds) = the content from ds, each block decoded where it belongs; d_starts[i] = offset in d_dst of record i,
 * d_starts[records] = data_bytes.  d_starts NULL: count only.  Nothing owned: result 0, data_off = data_bytes = 0, d_starts[0] = 0.
 * The blocks from split_end on that the last record reaches into are decoded one at a time into a staging slot kept with the
 * stream, until one shows a delimiter, and never into d_dst beyond hi: of the last one only the prefix is copied.
 * result, in order of precedence:
 *   info.nblocks if < 0, else info.framing if != 0   the image cannot be indexed;
 *   -3   a bad split offset;
 *   -4   a block from split_end on, decoded in search of hi, failed its XXH32, failed to decode or decoded to a size other
 *        than its usize (hi is then unknown);
 *   -5   hi - ds > dst_cap: data_bytes = hi - ds, the smallest dst_cap that works, and nothing is written to d_dst;
 *   -4   a block of [ds, hi) failed in one of those ways;
 *   -5   records + 1 > starts_cap with d_starts not NULL: reserved = records, and nothing is written to d_starts;
 *   the records owned (>= 0).
 * The call never writes outside [d_dst, d_dst + dst_cap) or d_starts[0, starts_cap); bytes of d_dst from data_bytes on are
 * unspecified. */
typedef struct fourmc_image_records {     /* 40 bytes */
    int64_t  result;      /* records owned (>= 0), or a negative code                               */
    uint64_t base;        /* decoded offset of d_dst[0] = ds (0 for the index codes and -3)         */
    uint64_t data_off;    /* offset in d_dst of the first owned record = lo - ds                    */
    uint64_t data_bytes;  /* d_dst[0, data_bytes) = decoded content [ds, hi)                        */
    uint64_t reserved;    /* the record count when result is the -5 of starts_cap, else 0           */
} fourmc_image_records;
int fourmc_gpu_image_read_records(const void* d_image, uint64_t image_bytes, uint64_t split_start, uint64_t split_end, uint8_t delim,
                                  void* d_dst, uint64_t dst_cap, uint64_t* d_starts, uint64_t starts_cap,
                                  fourmc_image_records* out /*host*/, void* stream);

/* The lines of the split by Hadoop's default rule, which is the reference reader's: it is built as new LineReader(stream, job)
 * and calls readLine(value, maxLineLen) (FourMcLineRecordReader.java:122,135,154), so no custom delimiter is ever read.  With D[0, T)
 * the decoded content, position p ENDS A LINE when D[p] == LF, or D[p] == CR and (p + 1 == T or D[p+1] != LF); a CR followed by LF
 * ends nothing by itself.  Lines start at 0 and behind every end; a final unterminated run is a line if not empty.  Line [s, s')
 * has a terminator of t = 2 (CR LF), 1 (LF, lone CR) or 0 bytes, and its TEXT is D[s, s + min(s' - s - t, max_line_len)): the whole
 * line is consumed however long it is, as readLine with maxBytesToConsume = Integer.MAX_VALUE does.
 * Ownership, split offsets, ds / de / lo / hi, d_dst[0, hi - ds), base, data_off, data_bytes, d_starts[0 .. lines] with
 * d_starts[lines] = data_bytes, and the result codes with their precedence are image_read_records' word for word, with "line end"
 * for "delimiter".  New: d_text_len[i] = the length of line i's text, so line i's text is d_dst[d_starts[i], d_starts[i] +
 * d_text_len[i]).  The call needs lines + 1 <= lines_cap (else the -5 with reserved = lines, and neither table is written);
 * d_starts[0 .. lines] and d_text_len[0, lines) are written, so d_text_len may hold one entry less than d_starts.  Both tables
 * NULL: count only; one without the other: FOURMC_EINVAL.  max_line_len: Hadoop's default is 0x7FFFFFFF; larger: FOURMC_EINVAL;
 * 0: every text is empty.  Nothing is written outside [d_dst, d_dst + dst_cap), d_starts[0, lines_cap) or d_text_len[0, lines_cap).
 * One deviation from the reference, by reading it (no JVM ran it): when the last decoded byte before split_end is a CR and the byte
 * behind it is not LF, the reference's LineReader must fill its buffer to look behind the CR, which pulls the whole next block
 * through FourMcInputStream and moves the file position past the split's end; its reader stops, the next split's reader skips its
 * first line as always, and the line that starts at de is read by nobody.  Here that line belongs to the earlier split: the rule
 * above is the contract, and every line has exactly one owner.
 * Not reproduced: the reference's IOException("Too many bytes before newline") for a line of 2 GiB or more; the key (the raw file
 * position after the last block read); multi-byte delimiters (textinputformat.record.delimiter, which the reference never reads);
 * multi-stream images (the index code). */
typedef struct fourmc_image_lines { int64_t result; uint64_t base, data_off, data_bytes, reserved; } fourmc_image_lines; /* as fourmc_image_records */
int fourmc_gpu_image_read_lines(const void* d_image, uint64_t image_bytes, uint64_t split_start, uint64_t split_end,
                                uint32_t max_line_len,               /* Hadoop's default: 0x7FFFFFFF; larger: FOURMC_EINVAL; 0: every text empty */
                                void* d_dst, uint64_t dst_cap,
                                uint64_t* d_starts, uint32_t* d_text_len, uint64_t lines_cap,
                                fourmc_image_lines* out /*host*/, void* stream);
/* The lines of many splits of ONE image with one call: a job that holds an image in HBM wants the lines of every split of it, or of
 * the splits one rank was given, and one call per split builds the index again, synchronizes four times or more, decodes the tail
 * block of split k alone and again as the first block of split k+1, and launches a decode and a scan that fill a corner of the chip.
 * All contents go to ONE device buffer and all tables to ONE pair of device tables, each split to a region of its own.
 * The one rule.  After the call items[i].out equals, field for field, what fourmc_gpu_image_read_lines gives for the same image,
 *   split_start, split_end and max_line_len with d_dst + dst_off, dst_cap, d_starts + table_off, d_text_len + table_off and
 *   lines_cap, and d_dst[dst_off, dst_off + out.data_bytes), d_starts[table_off .. table_off + lines] and d_text_len[table_off,
 *   table_off + lines) hold the same values; the starts are offsets in the item's own region.  This holds for every case the single
 *   call documents: ownership and lo / hi with the CR at a block's end, lines longer than a block, -3 for a bad split offset, both
 *   -4s and both -5s with their precedence, `reserved`, and data_bytes as the smallest dst_cap that works, so an item with dst_cap
 *   == 0 is a size query.  An image that cannot be indexed (a damaged footer, several streams) gives every item the index code and
 *   the call returns FOURMC_OK, as fourmc_gpu_image_read does for its ranges.  A damaged block changes nothing for the splits that
 *   do not cover it.  Two items may name the same split.
 * Count only.  d_starts and d_text_len both NULL; table_off, lines_cap and table_entries are ignored.  One without the other:
 *   FOURMC_EINVAL.
 * Writes.  Nothing outside the items' regions; for an item, nothing outside d_dst[dst_off, dst_off + dst_cap), d_starts[table_off,
 *   table_off + lines_cap) and d_text_len[table_off, table_off + lines_cap).  An item whose result is -3, an index code, the tail's
 *   -4 or the -5 of dst_cap leaves its regions untouched; the -5 of lines_cap and the body's -4 leave its tables untouched.  Regions
 *   may abut at any byte: the scan reads whole 16-byte chunks and masks, and neither writes nor counts a neighbour's byte.
 * Arguments.  Checked on the host before any device is looked for; each of these returns FOURMC_EINVAL with `items` untouched:
 *   items NULL with n > 0; d_image NULL; d_dst NULL; one table without the other; max_line_len > 0x7FFFFFFF; an output region that
 *   does not lie inside [0, dst_bytes) (dst_off + dst_cap may not wrap); two output regions of nonzero dst_cap that overlap; with
 *   tables, a table region that does not lie inside [0, table_entries), or two table regions of nonzero lines_cap that overlap.
 *   n == 0 returns FOURMC_OK and does nothing.  No device: FOURMC_ENODEV.  On every failure `items` is left as it came.
 * Groups.  A split still looking for its hi needs one staged tail block of 4 MiB + 64 bytes per round, so the items are processed
 *   in groups of at most FOURMC_SPLIT_GROUP splits (env, read at every call; default 256, which is 1 GiB of staging at the most;
 *   clamped to 1..4096; a test knob as much as a tuning knob), cut also where the tiles of one launch's grid would pass 0x7FFFFFFF.
 *   The staging stays with the stream until fourmc_gpu_release_workspaces, like the single call's slot.
 * Work per group.  One plan kernel, one lane per split.  Per tail round, for all splits still searching: one descriptor kernel, one
 *   container decode, one tail-find launch of one workgroup per split.  Then ONE container decode for the bodies of all the group's
 *   splits straight into their regions, one kernel for the staged prefixes, and one count, one finish, one write and one length
 *   launch over all the group's spans.
 * Synchronizations of `stream`: one for the call (the index summary; the index itself is built once per call, on the stream, and
 *   is read back by nobody), and per group one for the plans, one per tail round and one for the results; a group none of whose
 *   splits fits its region ends after its rounds.  The tail rounds of a group are the most tail blocks any of its splits stages:
 *   usually 1; 0 when every split_end is at or past the end mark; more only for a line longer than a block or a block-ending CR.
 *   A workspace that has to grow synchronizes once more, the first time a stream sees a call of that size.
 * Settings.  FOURMC_DECODE, FOURMC_ZDECODE and the batch limits of the block decode apply as they do to the single call.
 * Several images in one call: fourmc_gpu_images_read_lines below.
 * Not reproduced: the one-byte rule of image_read_records in batch form; sharing one decode between two items that cover the same
 *   block (each item's region gets its own copy). */
typedef struct fourmc_image_split_item {     /* 88 bytes, no padding */
    uint64_t split_start, split_end;         /* in : as fourmc_gpu_image_read_lines takes them                                  */
    uint64_t dst_off, dst_cap;               /* in : the split's content goes to d_dst[dst_off, dst_off + dst_cap)              */
    uint64_t table_off, lines_cap;           /* in : its tables are d_starts[table_off, +lines_cap), d_text_len[table_off, +lines_cap) */
    fourmc_image_lines out;                  /* out                                                                             */
} fourmc_image_split_item;
int fourmc_gpu_image_read_lines_batch(const void* d_image, uint64_t image_bytes, uint32_t max_line_len,
                                      void* d_dst, uint64_t dst_bytes,
                                      uint64_t* d_starts, uint32_t* d_text_len, uint64_t table_entries,
                                      fourmc_image_split_item* items /*host*/, uint32_t n, void* stream);
/* Statistics (read-only), as fourmc_gpu_image_parse_stats: the groups image_read_lines_batch has processed so far, the tail rounds
 * it has run and the container block-decode calls it has made (one per tail round, one per group with a body block). */
void fourmc_gpu_image_lines_batch_stats(unsigned long long* groups, unsigned long long* tail_rounds, unsigned long long* block_decodes);

/* ---- lines by number -------------------------------------------------------------------------------------------------------
 * The calls above hand out lines by split.  A consumer that samples (a shuffled text dataset, a join that fetches rows by id,
 * NLineInputFormat-style cuts by line count) wants line k, and would have to decode and scan the whole image and keep the decoded
 * copy to get it.  Here a small per-image LINE INDEX is built once, and a read decodes only the blocks its lines touch.
 * The line rule is fourmc_gpu_image_read_lines': with D[0, T) the decoded content, a LINE END is a position p that ends a line; E is
 * their number; lines = E + (T > 0 and T - 1 is no line end); line 0 starts at 0, line k > 0 one past end k - 1; line k ends at end
 * k, or at T for the final unterminated line.
 *
 * fourmc_gpu_image_line_index.  Entry b, b < nblocks, of the index:
 *   ends_before   the line ends in D[0, data_off[b]);
 *   ends          the line ends inside block b;
 *   flags bit 0   the block's last byte is a CR that ends nothing, because the next content byte is LF;
 *         bit 1   the block's first byte is an LF whose previous content byte is CR, so its terminator is 2 bytes long;
 *         bits 8..31   the offset in the block just behind its last line end (0: it has none; usize: its last byte is one) - where
 *                 the line that leaves the block starts, which lets a read decode of a long line no block it will not copy from.
 *   Entry nblocks is the sentinel {E, 0, 0}.  The seam rules look past blocks of usize 0, which fourmc_gpu_image_index accepts.
 * info->result, in order of precedence: the index codes (info.nblocks < 0, else info.framing != 0, as in the random-access group;
 *   nothing else of *info is then meaningful); -4 a block failed its XXH32, failed to decode or decoded to a size other than its
 *   usize (nothing is written to d_index); -5 nblocks + 1 > index_cap with d_index not NULL (lines and ends are filled in, nothing is
 *   written to d_index); else 0.  d_index NULL is a pure count.
 * Work.  The image is decoded once, in groups of at most FOURMC_LINES_AT_GROUP blocks (env, read at every call; default 256,
 *   clamped to 1..4096, like FOURMC_SPLIT_GROUP), each block into a staging slot of 4 MiB + 64 bytes kept with the stream.  Per
 *   group: one descriptor launch, one container decode, one count launch (a workgroup per block; a CR in the block's last byte
 *   counts as an end, and the launch records whether the last byte is CR or LF and the first LF).  One finish launch over all
 *   blocks then subtracts the CR LF seams, sets the flags and writes the 64-bit prefix, so no group needs its neighbour's bytes.
 *   Synchronizations of `stream`: 2 (the index summary, the result).
 *
 * fourmc_gpu_image_read_lines_at.  d_lines[0, n) are line numbers IN DEVICE MEMORY (a torch.randperm slice never visits the host).
 *   Request i writes row i = d_rows[i * row_bytes, (i + 1) * row_bytes): d_text_len[i] = min(text length, max_line_len), exactly what
 *   fourmc_gpu_image_read_lines puts in its d_text_len for that line; the row holds the first min(d_text_len[i], row_bytes) bytes of
 *   the text, then `pad` up to row_bytes; a caller sees truncation as d_text_len[i] > row_bytes.  Fixed-stride rows on purpose: every
 *   destination is known before any block is decoded, so rounds are independent and no block is decoded twice.
 * d_status[i]: 1 written; -3 line >= lines (the row is all pad, text_len 0); -4 a block the request needed was damaged (the row is
 *   unspecified, text_len 0; requests that do not need the block are unaffected).  Duplicate line numbers are allowed.
 * out->result: the index code if the image cannot be indexed (every status then gets that code and every text_len 0); else the
 *   number of requests with status 1, which is also out->served.  blocks_staged / rounds: the blocks this call decoded and the
 *   rounds it took.
 * The one rule.  For every k < lines, row k and text_len k equal line k of fourmc_gpu_image_read_lines(0, image_bytes, max_line_len)
 *   on the same image: d_dst[d_starts[k], + min(d_text_len[k], row_bytes)) and d_text_len[k].
 * Blocks a request needs, from the index and the footer entries alone (L = min(row_bytes, max_line_len)): bp, the block holding end
 *   k - 1 (block 0 for k = 0); be, the block holding end k (the last block with bytes for the final unterminated line); and, when
 *   be > bp, every block j between them with data_off[j] < s + L, where s = data_off[bp] + flags[bp] >> 8 is the line's start.
 *   Blocks of a long line beyond its first L bytes are not decoded, except be.
 * index_entries must equal nblocks + 1 (else FOURMC_EINVAL, after the index summary has been read).  The kernels clamp whatever they
 *   read from d_index: an index that belongs to another image may give wrong rows, but never an access outside the call's regions.
 *   Nothing is written outside d_rows[0, n * row_bytes), d_text_len[0, n) and d_status[0, n).
 * Work.  A locate launch (one lane per request: binary searches over the index, marks the needed blocks), a scan that compacts
 *   the marked blocks in ascending order, one read-back of their count.  Then rounds of at most FOURMC_LINES_AT_GROUP needed
 *   blocks, each round: one descriptor launch, one container decode, one per-tile count launch over the staged blocks (16 KiB
 *   tiles), one resolve-and-copy launch (a wave per request: rank / select over the tile counts and the 16-bit masks for the
 *   line's start and end, the copy of the piece of its text that lies in this round's blocks, the pad and the status in the round
 *   of be).  Synchronizations of `stream`: 3 (the index summary, the count of needed blocks, the result).
 * Arguments, checked on the host before any device is looked for, each FOURMC_EINVAL with the outputs untouched: d_image NULL;
 *   info / out NULL; d_lines, d_rows, d_text_len or d_status NULL with n > 0; d_index NULL for read_lines_at; row_bytes == 0;
 *   max_line_len > 0x7FFFFFFF; n * row_bytes overflowing 64 bits.  n == 0 returns FOURMC_OK.  No device: FOURMC_ENODEV.
 * Not here: the many-images form; packed output; a one-byte-delimiter form; the index inside the file (the format has no place). */
typedef struct fourmc_image_line_entry { uint64_t ends_before; uint32_t ends; uint32_t flags; } fourmc_image_line_entry; /* 16 bytes */
typedef struct fourmc_image_line_info  { int64_t result; uint64_t lines, ends, total_bytes; uint32_t nblocks, pad; } fourmc_image_line_info; /* 40 */
int fourmc_gpu_image_line_index(const void* d_image, uint64_t image_bytes,
                                fourmc_image_line_entry* d_index, uint64_t index_cap,
                                fourmc_image_line_info* info /*host*/, void* stream);
typedef struct fourmc_image_lines_at { int64_t result; uint64_t served, blocks_staged, rounds; } fourmc_image_lines_at;   /* 32 bytes */
int fourmc_gpu_image_read_lines_at(const void* d_image, uint64_t image_bytes,
                                   const fourmc_image_line_entry* d_index, uint64_t index_entries,
                                   const uint64_t* d_lines /*device*/, uint32_t n, uint32_t max_line_len,
                                   void* d_rows, uint32_t row_bytes, uint8_t pad,
                                   uint32_t* d_text_len, int32_t* d_status,
                                   fourmc_image_lines_at* out /*host*/, void* stream);
/* Statistics (read-only): the rounds fourmc_gpu_image_read_lines_at has run so far in this process, the container block-decode calls
 * it has made and the blocks it has staged. */
void fourmc_gpu_image_lines_at_stats(unsigned long long* rounds, unsigned long long* block_decodes, unsigned long long* blocks_staged);

/* ---- the lines of the splits of MANY images with one call --------------------------------------------------------------------
 * A Hadoop dataset is a directory of part files of a few blocks each (the case fourmc_gpu_images_decompress and _images_compress
 * were built for).  image_read_lines_batch takes the splits of ONE image: a job with a thousand part files in HBM makes a thousand
 * calls, each of which builds an index, synchronizes four times or more and launches decodes and scans that fill a corner of the
 * chip.  Here the images lie in ONE device buffer, image k at d_images + images[k].image_off, and every item names its image.
 * The one rule.  After the call items[i].out and the item's regions of d_dst, d_starts and d_text_len equal what
 *   fourmc_gpu_image_read_lines_batch gives for a one-item call with the image d_images + images[image].image_off of
 *   images[image].image_bytes bytes and the same split offsets and capacities - and so, by that call's rule, what
 *   fourmc_gpu_image_read_lines gives for the split.  Every case documented there carries over: ownership and lo / hi with a CR at
 *   a block's end, lines longer than a block, -3 for a bad split offset, both -4s and both -5s with their precedence, `reserved`,
 *   data_bytes as the smallest capacity that works (dst_cap == 0 is a size query), count only with both tables NULL, and what an
 *   item may write.
 * Only with several images.  The format is each image's own header's, as in the random-access group: one call may mix .4mc and
 *   .4mz.  An image that cannot be indexed (a damaged footer, several streams, fewer than 12 bytes, image_bytes == 0) gives ITS
 *   items the index code; every other item is unaffected and the call returns FOURMC_OK.  A damaged block changes nothing for the
 *   splits that do not cover it, in its own image or any other.  A split offset is judged against its own image's headers: one
 *   that is a block header of another image of the call is -3.  Two entries of `images` may name the same or overlapping bytes,
 *   and two items may name the same split.
 * Arguments.  Checked on the host before any device is looked for; each returns FOURMC_EINVAL with `items` untouched: all that
 *   image_read_lines_batch checks (d_images for d_image); images NULL with nimages > 0; an image region that does not lie inside
 *   [0, images_bytes); an item whose image >= nimages.  n == 0 returns FOURMC_OK and does nothing.  More than 0x7FFFFFFF blocks
 *   over all images: FOURMC_EUNSUP.  No device: FOURMC_ENODEV.  On every failure `items` is left as it came.
 * Slack.  The decoders may read up to 64 bytes past a payload: inside the buffer that is the next image; behind the last image
 *   the caller keeps that slack, as for fourmc_gpu_images_decompress.
 * Index.  One kernel indexes all images, one wave per image in a grid of nimages; its body is the one-image index kernel's, so
 *   the verdicts are the same by construction.  It runs twice: the first run writes only the summaries, which come back in ONE
 *   read-back (the call's first synchronization: nblocks, the code and the format of every image, which size the entry table);
 *   the second writes the entries of every indexable image that an item names, image k's at that image's first-entry index (the
 *   host's prefix sum over the block counts, uploaded with the image table).  The entries are image-relative, equal to
 *   fourmc_gpu_image_index's; the image's offset is added where descriptors are made.  A workspace that has to grow later loses
 *   the entries and the kernel runs again.
 * Groups.  As in the one-image call (the same host function runs both): the items in the order given, at most FOURMC_SPLIT_GROUP
 *   to a group with the same cut at the grid limit; per group one synchronization for the plans, one per tail round and one for
 *   the results; one plan launch with a lane per split, each request carrying its image; per round one descriptor launch and one
 *   tail-find launch for all searching splits of all images ("last block" is the last of the split's own image); the body
 *   descriptors, the prefix copy and the count / finish / write / length launches once over all the group's spans.
 * Decodes.  The host knows every item's format after the index read-back and orders a round's jobs, and a group's spans, with .4mc
 *   before .4mz: each phase is ONE fourmc_gpu_4mc_decode_blocks per format present, with d_images as its source - one call per
 *   round and one for the bodies when the dataset has one format, two when it has both.  Staging is one slot of 4 MiB + 64 bytes
 *   per searching split of the group.
 * Synchronizations of `stream`: one for the summaries, then per group as above; a workspace that has to grow synchronizes once more.
 * Statistics.  fourmc_gpu_images_lines_stats: the groups, tail rounds and block-decode calls of THIS call so far, and the launches
 *   of the index kernel (2 per call when nothing grows).  fourmc_gpu_image_lines_batch_stats is not incremented by it. */
typedef struct fourmc_image_ref { uint64_t image_off, image_bytes; } fourmc_image_ref;      /* 16 bytes */
typedef struct fourmc_images_split_item {      /* 96 bytes, no padding */
    uint32_t image, pad;                       /* in : index into `images`; pad is ignored            */
    uint64_t split_start, split_end;           /* in : offsets in THAT image, as image_read_lines takes them */
    uint64_t dst_off, dst_cap;
    uint64_t table_off, lines_cap;
    fourmc_image_lines out;                    /* out */
} fourmc_images_split_item;
int fourmc_gpu_images_read_lines(const void* d_images, uint64_t images_bytes,
                                 const fourmc_image_ref* images /*host*/, uint32_t nimages, uint32_t max_line_len,
                                 void* d_dst, uint64_t dst_bytes, uint64_t* d_starts, uint32_t* d_text_len, uint64_t table_entries,
                                 fourmc_images_split_item* items /*host*/, uint32_t n, void* stream);
void fourmc_gpu_images_lines_stats(unsigned long long* groups, unsigned long long* tail_rounds,
                                   unsigned long long* block_decodes, unsigned long long* index_launches);
/* fourmc_gpu_image_align_slices for the slices of many images: each slices[i].s comes back as that call returns it for the image
 * images[slices[i].image] alone, the index code in `result` for an image that cannot be indexed and "unchanged, result 1" for an
 * image without blocks included.  The batched index above and ONE align launch over all slices; two synchronizations whatever
 * the counts (the summaries, the results).  Arguments as above (slices for items); n == 0 returns FOURMC_OK and does nothing. */
typedef struct fourmc_images_slice { uint32_t image, pad; fourmc_image_slice s; } fourmc_images_slice;   /* 56 bytes */
int fourmc_gpu_images_align_slices(const void* d_images, uint64_t images_bytes, const fourmc_image_ref* images /*host*/,
                                   uint32_t nimages, fourmc_images_slice* slices /*host*/, uint32_t n, void* stream);

/* ---- Hadoop block streams in device memory: the files of Lz4Codec / ZstdCodec and their six siblings ----------------------------
 * The reference ships eight raw block codecs beside the .4mc / .4mz container: Lz4Codec, Lz4MediumCodec, Lz4HighCodec, Lz4UltraCodec,
 * ZstdCodec, ZstdMediumCodec, ZstdHighCodec, ZstdUltraCodec (extensions .lz4_fast .lz4_mc .lz4_hc .lz4_uc .zstd_fast .zstd_mc
 * .zstd_hc .zstd_uc).  A job that names one as its output or intermediate codec writes part files in the framing of Hadoop's
 * BlockCompressorStream (Lz4Codec.java:95-104): no header, no checksum, no index.  These calls write and read that framing.
 * Provenance.  BlockCompressorStream / BlockDecompressorStream are Hadoop's classes, not the reference's; their source was not at
 *   hand and no JVM wrote or read a file for this code.  The rules below are written from knowledge of those classes and from the
 *   reference's Lz4Codec.java, Lz4Compressor.java, jniCompressor.c, jniZstdCompressor.c and their twins.  They are the contract
 *   here, by reading, as fourmc_gpu_image_read_lines' rule is.
 * Format.  All integers are big-endian u32 at any byte offset.
 *     stream := group* [ BE32(0) ]
 *     group  := BE32(rawlen) chunk+          rawlen in 1 .. 0x7FFFFFFF
 *     chunk  := BE32(clen) payload[clen]     payload = one raw LZ4 block / one zstd frame
 * M, the most input bytes in one chunk: 4 MiB - (compressBound(4 MiB) - 4 MiB), the codec's buffer less the overhead the codec
 *   hands to BlockCompressorStream (Lz4Codec.java:102-103).  fourmc_gpu_bstream_max_input derives it from fourmc_LZ4_compressBound
 *   / fourmc_ZSTD_compressBound: 4177840 for the LZ4 codecs, 4177920 for the zstd codecs.
 * What a writer produces.  Under every pattern of write() calls a group of rawlen R has exactly ceil(R / M) chunks, every chunk but
 *   the last decoding to M bytes and the last to the rest: small writes accumulate until the next one would pass M, then ONE group
 *   of ONE chunk goes out; a single write longer than M goes out as one group with chunks of M.  A stream nothing was written to is
 *   the four bytes 00 00 00 00, and a stream whose last write took the long-write path ends with a trailing BE32(0).  Chunks are
 *   compressed with unlimited output (LZ4_compress, LZ4_compressMC, LZ4_compressHC2(level), ZSTD_compress(level), capacity = the
 *   bound): there is no stored-raw fallback and no checksum.
 * Reader rule.  At a group boundary with fewer than 4 bytes left (0, or 1 - 3: Hadoop's reader swallows the EOF there) the stream
 *   ends cleanly; rawlen == 0 ends it cleanly whatever follows; rawlen > 0x7FFFFFFF is FOURMC_BS_BAD_RAWLEN.  Inside a group: fewer
 *   than 4 bytes where a clen is due is FOURMC_BS_CLEN_UNREADABLE; clen == 0 or clen > 4 MiB is FOURMC_BS_BAD_CLEN (Lz4Decompressor
 *   would cut such an input at its 4 MiB direct buffer); a clen beyond the bytes left is FOURMC_BS_DATA_UNREADABLE.
 * The walk assumes the writer's shape.  Chunk j of a group is expected to decode to min(M, R - j M) bytes, so finding the chunks is
 *   pure header chasing, independent of the decode, and every chunk decodes straight to its final place.  The decode then proves
 *   the assumption: each chunk is decoded with dst_cap = its expected size and must return exactly that.
 * Not reproduced.  (a) Foreign chunkings: a stream chunked another way, which BlockDecompressorStream would accept but these
 *   codecs never write, gets FOURMC_BS_SHAPE (or FOURMC_BS_CORRUPT when a chunk holds more than its expected size), never wrong
 *   bytes.  (b) A group cut short by a framing error is not decoded at all, though Hadoop's reader would hand out its leading chunks
 *   before it fails: total_bytes counts whole groups only and nothing is ever written beyond it.  (c) Streaming writer and reader
 *   forms, the lines of a block stream, and .zst files (the libzstd pass-through of the file API) are not in this group. */
enum {
    FOURMC_BS_OK              = 0,
    FOURMC_BS_BAD_RAWLEN      = 1,   /* a group's rawlen has its top bit set                                          */
    FOURMC_BS_CLEN_UNREADABLE = 2,   /* fewer than 4 bytes left where a chunk's length is due                         */
    FOURMC_BS_BAD_CLEN        = 3,   /* a chunk length of 0 or above 4 MiB                                            */
    FOURMC_BS_DATA_UNREADABLE = 4,   /* a chunk length beyond the bytes left                                          */
    FOURMC_BS_CORRUPT         = 5,   /* the codec returned < 0 for a chunk (a chunk holding more than its expected size included) */
    FOURMC_BS_SHAPE           = 6,   /* a chunk decoded cleanly to fewer bytes than the writer's shape gives it      */
    FOURMC_BS_DST_SMALL       = 7    /* total_bytes > dst_cap: nothing decoded                                       */
};
typedef struct fourmc_bstream_status {   /* 40 bytes */
    uint64_t decoded_bytes;   /* the sum of the expected sizes of the chunks before the first failure: d_dst[0, decoded_bytes) is good */
    uint64_t total_bytes;     /* the sum of the rawlens of the well-formed groups (the size query's answer)                           */
    uint64_t fail_offset;     /* stream offset of the rawlen / clen field or chunk header that ended decoding; image_bytes if none     */
    uint32_t groups, chunks;  /* well-formed groups and their chunks; when a chunk failed: the groups and chunks wholly in front of it */
    int32_t  reason;          /* FOURMC_BS_*                                                                                          */
    uint32_t pad;             /* 0                                                                                                    */
} fourmc_bstream_status;
/* M for a FOURMC_CODEC_* selector, 0 for an unknown one.  Host arithmetic: no device is looked for. */
uint32_t fourmc_gpu_bstream_max_input(int codec);
/* The exact worst case of bstream_compress: 4 for an empty source, else the sum over the groups of 8 + compressBound(group length).
 * group_bytes 0 means M.  0 for an unknown codec or a group_bytes above M.  Host arithmetic. */
uint64_t fourmc_gpu_bstream_bound(uint64_t src_bytes, int codec, uint32_t group_bytes);
/* d_src[0, src_bytes) -> a block stream at d_image.  The source is cut at every group_bytes of input (0: M), the last piece short;
 * piece g becomes BE32(len_g) BE32(csize_g) payload_g, the payload what the raw codec call writes for the piece with dst_cap =
 * compressBound(len_g): fourmc_gpu_lz4_compress_fast, _mc (with its no-limit capacity), _hc(level), fourmc_gpu_zstd_compress(level).
 * For the exact encoders these are the reference's bytes; FOURMC_LZ4_ENCODE=parallel applies exactly as it does to the raw call.
 * The levels of the eight codec classes, from their *Compressor.java: LZ4 fast, MC, HC 4 (High), HC 8 (Ultra); zstd 1, 3, 6, 12.
 * Correspondence.  This is byte for byte what BlockCompressorStream writes when each write() carries one piece and a piece is longer
 *   than M / 2 (two never fit one group).  For smaller writes of w bytes each it is what the stream writes when group_bytes =
 *   floor(M / w) * w: the writes that accumulate into one group.  An empty source writes 00 00 00 00.  Pieces longer than M - the
 *   multi-chunk groups of a long write() - are never written.
 * Arguments, checked on the host before any device is looked for, the codec first: an unknown codec, a NULL d_image or image_bytes,
 *   a NULL d_src with a nonzero src_bytes, a group_bytes above M, image_cap < fourmc_gpu_bstream_bound(src_bytes, codec,
 *   group_bytes): FOURMC_EINVAL.  A zstd level outside the device's 1 .. 12: FOURMC_EUNSUP.  A codec result <= 0 or above its bound
 *   fails the call with FOURMC_EINVAL, the guard image_compress has.
 * Cost.  One synchronization of `stream` (the length and the count of bad results together).  Staging: one slot of
 *   compressBound(group_bytes) rounded up to 256 bytes per group in the engine's image workspace, for at most 512 groups at a time
 *   (the file API's batch): larger inputs are encoded in pieces of 512 groups, the 64-bit offset carried on the device. */
int fourmc_gpu_bstream_compress(const void* d_src, uint64_t src_bytes, void* d_image, uint64_t image_cap, uint64_t* image_bytes,
                                int codec, int level, uint32_t group_bytes, void* stream);
/* d_image[0, image_bytes) -> decoded bytes at d_dst, by the reader rule above.  `codec` only selects the family: any LZ4 selector
 * means LZ4, FOURMC_CODEC_ZSTD means zstd.  d_dst NULL: the size query (parse only: total_bytes, groups, chunks and the framing
 * verdict).  total_bytes > dst_cap: FOURMC_BS_DST_SMALL, nothing written; it wins over every other verdict.  Otherwise the first
 * failing chunk in file order wins over the framing verdict (the walk lists only chunks in front of the point where it stopped).
 * The call never writes outside [d_dst, d_dst + total_bytes); bytes from decoded_bytes on are unspecified.  The decoders may read up
 * to 64 bytes past a payload: the caller keeps that slack behind the image, as for .4mc.  The chunks go through
 * fourmc_gpu_lz4_decompress / fourmc_gpu_zstd_decompress, so FOURMC_DECODE, FOURMC_ZDECODE and the launch-splitting limits apply
 * unchanged.  FOURMC_EINVAL (before any device is looked for): an unknown codec, a NULL status, a NULL d_image with a nonzero
 * image_bytes.  Synchronizations of `stream`: two (the chunk count that sizes the descriptor table, then the status); the size
 * query takes one.  The files are not splittable, so one stream is one serial walk on one lane: the parallelism comes from many
 * chunks and many streams per launch, and this call is the n = 1 case of the next one, run by the same host function. */
int fourmc_gpu_bstream_decompress(const void* d_image, uint64_t image_bytes, void* d_dst, uint64_t dst_cap, int codec,
                                  fourmc_bstream_status* status, void* stream);
/* Many streams of ONE device buffer with one call, their outputs in ONE device buffer.
 * The one rule.  items[i].status and d_dst[dst_off, dst_off + decoded_bytes) equal what the single call gives for d_images +
 *   image_off, image_bytes, d_dst + dst_off, dst_cap and the same codec.  A damaged stream changes nothing for its neighbours; two
 *   items may name the same stream bytes; d_dst NULL is the size query of every item (dst_off, dst_cap and dst_bytes are ignored).
 * Arguments, as fourmc_gpu_images_decompress checks them, on the host before any device is looked for and with `items` untouched
 *   on every failure, the codec first: an unknown codec, items NULL with n > 0, d_images NULL with a nonzero image_bytes, a stream
 *   outside [0, images_bytes), with d_dst an output region outside [0, dst_bytes) or two output regions of nonzero dst_cap that
 *   overlap: FOURMC_EINVAL.  n == 0: FOURMC_OK.  More than 0x7FFFFFFF chunks in all: FOURMC_EUNSUP.  No device: FOURMC_ENODEV.
 * Work, whatever n is: the walk twice with one wave per stream (the first run leaves each stream's summary, which come back in one
 *   read-back; the host's prefix sum over the chunk counts gives each stream its slice of ONE descriptor table, which the second
 *   run fills), one block decode over all chunks of all streams, one fold with one wave per stream; two synchronizations. */
typedef struct fourmc_bstream_item {     /* 72 bytes */
    uint64_t image_off, image_bytes;     /* in : the stream is d_images[image_off, image_off + image_bytes)          */
    uint64_t dst_off, dst_cap;           /* in : its output region is d_dst[dst_off, dst_off + dst_cap)              */
    fourmc_bstream_status status;        /* out                                                                       */
} fourmc_bstream_item;
int fourmc_gpu_bstreams_decompress(const void* d_images, uint64_t images_bytes, void* d_dst, uint64_t dst_bytes, int codec,
                                   fourmc_bstream_item* items /*host*/, uint32_t n, void* stream);
/* a short fixed text for a FOURMC_BS_* verdict ("" for FOURMC_BS_OK).  The words are this library's: no CLI reads these files. */
const char* fourmc_gpu_bstream_reason_text(int reason);

/* ---- .zst streams: the files of ZstCodec (hadoop-4mc/.../ZstCodec.java) and of the zstd tool, decoded in device memory ----
 * One stream: the contract of the reference's ZSTD_decompress(dst, cap, image, image_bytes) (zstd_decompress.c:1112; the frame loop
 * :989-1078): concatenated frames and skippable frames, no dictionary, every windowLog the one-shot call takes (up to 31), and -
 * unlike the block call fourmc_gpu_zstd_decompress - a content checksum is verified (XXH64 of the frame's output, low 32 bits).
 * ZSTD_decompressStream, which ZstdStreamDecompressor uses, differs in one place: it refuses windowLog > 27.  Deviation, as in the
 * block call: a frame with a non-zero dictionary ID fails (FOURMC_ZST_FRAME).
 *
 * Verdicts, in this order.  d_dst == NULL is the size query: the walk over the headers and the entropy stage run (a .zst frame
 * need not carry its size), nothing else.  total_bytes > dst_cap: FOURMC_ZST_DST_SMALL, nothing is written, and it wins over every
 * other verdict.  Otherwise the frames are executed in file order and the first failing frame - header, entropy stage, execution
 * or checksum - gives FOURMC_ZST_FRAME with codec_result < 0.  Nothing is written outside [d_dst, d_dst + total_bytes), bytes from
 * decoded_bytes on are unspecified; one exception: a frame only the serial one-wave decoder can judge (below) is decoded by it,
 * with what follows it in its stream, into [d_dst + total_bytes, d_dst + dst_cap), and a failure there may leave bytes behind.
 *
 * How.  Every block of every frame of every stream of a call gets one lane for its entropy stage (Huffman literals, FSE
 * sequences), whatever the frame's length; then one wave per frame executes the frame's blocks in order.  A frame those stages
 * decline - an Offset_Value beyond 28 bits (needs windowLog > 27), a Huffman stream that does not end on its mark, a block of more
 * than 43691 sequences on average over a round, a frame of 2 GiB or more - is handed with the rest of its stream to the serial
 * decoder, whose result is the verdict; the size query reports such a frame as failing.  The workspace is bounded by the table
 * entries (blocks) per round: FOURMC_ZST_ROUND_BLOCKS or the setter, default what 4 GiB hold (about 8700); a call of more blocks
 * runs the entropy stage twice, once for the sizes and once per round in front of its execution.  The decoders may read up to 64
 * bytes past an image: the caller keeps that slack.  Synchronizations of `stream`: three (block count, sizes, status); the size
 * query takes two.
 *
 * Many streams: the single call is the n = 1 case and runs the same host function; each item's status and bytes equal the single
 * call's, a damaged stream changes nothing for its neighbours, two items may name the same image bytes.  FOURMC_EINVAL, checked on
 * the host before any device is looked for, with `items` untouched: NULL items, a NULL d_images with a nonzero image_bytes, an image
 * outside [0, images_bytes), and - with a destination - an output region outside [0, dst_bytes) or two regions of nonzero dst_cap
 * that overlap.  n == 0: FOURMC_OK.  More than 0x7FFFFFFF frames or blocks in all: FOURMC_EUNSUP. */
enum { FOURMC_ZST_OK = 0, FOURMC_ZST_FRAME = 1, FOURMC_ZST_DST_SMALL = 2 };
typedef struct fourmc_zst_status {      /* 48 bytes */
    uint64_t decoded_bytes;  /* sum of the sizes of the frames wholly decoded in front of the first failing frame: d_dst[0, decoded_bytes) is good */
    uint64_t total_bytes;    /* sum of the decoded sizes of the frames in front of the first frame whose header walk or entropy stage fails (all, if none): the size query's answer */
    uint64_t fail_offset;    /* image offset of the magic number of the failing frame; image_bytes if none */
    uint32_t frames, skippable, blocks, pad;   /* zstd frames, skippable frames and blocks in front of the failure */
    int32_t  reason;         /* FOURMC_ZST_* */
    int32_t  codec_result;   /* 0, or the negative value the frame decoder gave for the failing frame */
} fourmc_zst_status;
typedef struct fourmc_zst_item { uint64_t image_off, image_bytes, dst_off, dst_cap; fourmc_zst_status status; } fourmc_zst_item;   /* 80 bytes */
int fourmc_gpu_zst_decompress (const void* d_image, uint64_t image_bytes, void* d_dst, uint64_t dst_cap, fourmc_zst_status* status, void* stream);
int fourmc_gpu_zsts_decompress(const void* d_images, uint64_t images_bytes, void* d_dst, uint64_t dst_bytes, fourmc_zst_item* items /*host*/, uint32_t n, void* stream);
const char* fourmc_gpu_zst_reason_text(int reason);
/* since the last call, this device: frames the lane-per-block stages decoded, frames handed to the serial decoder, blocks of the
 * former (a test aid like the execute kernel's counters) */
void fourmc_gpu_zst_stats(unsigned long long* fast_frames, unsigned long long* serial_frames, unsigned long long* fast_blocks);
/* Tuning knob: table entries (blocks) per round of the .zst decode; 0: FOURMC_ZST_ROUND_BLOCKS, else the default.  Results are identical. */
void     fourmc_gpu_set_zst_round_blocks(uint32_t blocks);
uint32_t fourmc_gpu_get_zst_round_blocks(void);

/* ---- .zst streams written in device memory: the part files of ZstCodec, many with one call ----
 * The image written for (src, level) is, byte for byte, what the reference's C calls give: ZSTD_initCStream(cs, level), then
 * ZSTD_compressStream over the whole source with no flush and no pledged size, then ZSTD_endStream (jniZStreamCompressor.c:86-137).
 * One frame: no content size, a window descriptor, no checksum, no dictionary ID; every block but the last is a full 128 KiB block;
 * the last block is ZSTD_endStream's: the rest of the source, or - after a source that is a non-zero multiple of 128 KiB - an empty
 * 3-byte block.  The empty source gives header + empty block, 9 bytes: the reference of the tests (tests/zst_model.py zstcodec)
 * makes its ZSTD_compressStream call with zero bytes, which starts the frame with an unknown size; a caller that goes from
 * ZSTD_initCStream straight to ZSTD_endStream gets the pledged-size-0 header 20 00 instead, which is not written here.  The bytes do
 * not depend on how a writer cuts its input into compressStream calls (tests/test_zst_write_cpu.py shows it on the reference).
 * Levels.  `level` is what ZSTD_initCStream gets: 1 and 2 (strategy "fast", window 512 KiB and 1 MiB), 3 and 4 ("dfast", 2 MiB), the
 *   parameter rows for an unknown source size.  fourmc_zst_codec_level maps the value configured for ZstCodec
 *   (io.compress.zst.compression.level) as ZstCodec.java:118-122 does: <= 0 or >= 23 becomes 3, every other value is itself.  Levels
 *   5 .. 22 get FOURMC_ZSTW_LEVEL (their match finders have no external-dictionary mode on the device), any other value too.
 * Length.  A source above 0xC0000000 bytes (3 GiB) gets FOURMC_ZSTW_TOO_LONG: below it no index reaches the reference's overflow
 *   correction, which is not reproduced.
 * Capacity.  fourmc_gpu_zst_bound(n) = 6 + n + 3 * (n / 131072 + 1) holds every image (all blocks stored raw, plus the empty last
 *   block): with image_cap >= the bound every source is written, the sources of 1 and 2 bytes and those with a last block of 1 or 2
 *   bytes included.  image_cap may be smaller: an image that does not fit gets FOURMC_ZSTW_DST_SMALL with codec_result = the
 *   encoder's error (-70), image_bytes 0, the bytes of its region unspecified.  Below the bound an image is written for certain when
 *   image_cap >= its length + 131075 (one more raw block); with less room a block that would have fit compressed may be refused.
 *   Never are other bytes than the reference's reported as written.
 * Verdicts per item; a refused item (_LEVEL, _TOO_LONG: decided on the host, nothing of it reaches the device) or a failing one
 *   costs only itself.  Nothing is written outside [image_off, image_off + image_cap) of an item.
 * Arguments, checked on the host before any device is looked for, with `items` untouched: items NULL with n > 0; d_src NULL with a
 *   nonzero src_bytes; d_images NULL with a nonzero image_cap; a source outside [0, src_total) (sources of _TOO_LONG items are not
 *   looked at: they are never read); an image region outside [0, images_bytes); two regions of nonzero image_cap that overlap:
 *   FOURMC_EINVAL.  n == 0: FOURMC_OK.  Two items may name the same source bytes.
 * Work.  A stream is one chain (every block's parse depends on the tables and repeat offsets the blocks before it left), so one wave
 *   runs one stream and the parallelism is the number of streams: one launch per strategy present ("fast": levels 1, 2; "dfast": 3,
 *   4), one upload (items and jobs), one read-back (the items with their status).  Workspace per stream: what the block encoder
 *   takes for one block of its level.  Synchronizations of `stream`: one.  The single call is the n = 1 case of the same function.
 * What ZstdStreamCompressor.java does differently (read from its code, :195-270, with CompressorStream.finish; no JVM ran): with no
 *   input at all compress() returns at :227-232 before endStream is ever called, so the Java writer emits zero bytes; and when the
 *   total input is a non-zero multiple of ZSTD_CStreamInSize() = 131072 its direct buffer is empty at finish(), the same return
 *   fires and the frame is left without its last block.  The device always writes the terminated frame: in the second case the
 *   Java bytes plus 01 00 00.  The readers (zstd -d, ZstdStreamDecompressor, fourmc_gpu_zst_decompress) take both. */
enum { FOURMC_ZSTW_OK = 0, FOURMC_ZSTW_DST_SMALL = 1, FOURMC_ZSTW_LEVEL = 2, FOURMC_ZSTW_TOO_LONG = 3 };
typedef struct fourmc_zstw_status {     /* 24 bytes */
    uint64_t image_bytes;    /* length of the image; 0 unless FOURMC_ZSTW_OK */
    uint32_t blocks;         /* blocks of the frame, the empty last one included */
    int32_t  reason;         /* FOURMC_ZSTW_* */
    int32_t  codec_result;   /* 0, or the negative ZSTD error number of FOURMC_ZSTW_DST_SMALL */
    uint32_t pad;
} fourmc_zstw_status;
typedef struct fourmc_zstw_item { uint64_t src_off, src_bytes, image_off, image_cap; int32_t level, pad; fourmc_zstw_status status; } fourmc_zstw_item;   /* 64 bytes */
uint64_t fourmc_gpu_zst_bound(uint64_t src_bytes);   /* 6 + src_bytes + 3 * (src_bytes / 131072 + 1): every block raw, plus the empty last block */
int fourmc_zst_codec_level(int configured);          /* ZstCodec.java:118-122: <= 0 or >= 23 -> 3 */
int fourmc_gpu_zst_compress (const void* d_src, uint64_t src_bytes, void* d_image, uint64_t image_cap, int level, fourmc_zstw_status* status, void* stream);
int fourmc_gpu_zsts_compress(const void* d_src, uint64_t src_total, void* d_images, uint64_t images_bytes, fourmc_zstw_item* items /*host*/, uint32_t n, void* stream);
/* a short fixed text for a FOURMC_ZSTW_* verdict ("" for FOURMC_ZSTW_OK) */
const char* fourmc_gpu_zstw_reason_text(int reason);

/* ---- block streams from a job's write() calls, many per call ----------------------------------------------------------------------
 * bstream_compress above cuts its source at one fixed group_bytes.  A job's stream is shaped by the sizes of its write() calls, and
 * this call takes those: every stream the writer can write (tests/bstream_model.py restates it) is written here byte for byte, many
 * streams with one call, all chunks of all streams through the same codec launches.
 * The rule.  M = fourmc_gpu_bstream_max_input(codec); a stream's write sizes are w_0 .. w_{k-1}.  With the codecs' 4 MiB buffers the
 *   compressor never saves a user buffer, so the shape depends on the sizes alone.  At write i with nothing accumulated: if w_i > M
 *   the write is a long group, BE32(w_i) then ceil(w_i / M) chunks, all of M bytes but the last, and the next group starts at i + 1;
 *   otherwise the group takes writes i .. j for the largest j with w_i + .. + w_j <= M, is written as BE32(sum) BE32(clen) payload,
 *   and the next group starts at j + 1.  A group whose sum is 0 (zero-length writes in front of a long write, or at the end) is not
 *   written.  The stream ends with BE32(0) when no group was written at all or the last written group was a long one (only
 *   zero-length writes may follow it).  Each payload is what the raw codec call writes for the chunk's source bytes with dst_cap =
 *   the codec's bound (LZ4_compressMC: its "no limit" value), as in bstream_compress.  A stream's data is contiguous in d_src, so
 *   every chunk is a contiguous source range: nothing is gathered.
 * Schedules.  n_writes > 0: entries [writes_off, writes_off + n_writes) of d_writes, a table in DEVICE memory (a text job issues
 *   several write()s per record: a stream may have tens of millions of entries, and a device-resident caller has them already, as
 *   the line-length table of image_read_lines).  n_writes == 0: the uniform schedule, every write() write_bytes long and the last
 *   one short; write_bytes 0 is one write() of the whole source (no write at all for an empty source).
 * Verdicts, per item; an item that gets one writes nothing into its region and costs only itself:
 *   FOURMC_BSW_SUM    the write sizes do not sum to src_bytes;
 *   FOURMC_BSW_WRITE  a write size above 0x7FFFFFFF (it wins over _SUM);
 *   FOURMC_BSW_CAP    image_cap is below the exact worst case of the item's schedule (image_bytes then holds that worst case).
 *   For _SUM and _WRITE image_bytes, groups and chunks are 0.
 * The size query.  d_images NULL plans only: groups, chunks and image_bytes = the exact worst case of each item's schedule, which is
 *   4 per written group, 4 + compressBound(len) per chunk and 4 for the trailer; image_off and image_cap are ignored and _CAP is
 *   never given.  The written length never exceeds it.
 * fourmc_gpu_bstream_writes_bound(src_bytes, codec) holds for EVERY schedule over src_bytes, without a table:
 *     src_bytes + V(src_bytes) + (K + 4) * C + 4 * G + 4
 *   where compressBound(n) - n <= V(n) + K with V additive over the chunks (LZ4: n / 255 and 16; zstd: n / 256 and 64), and C, G are
 *   the most chunks and written groups any schedule has.  Two written groups in a row hold more than M bytes together when the first
 *   is a one-chunk group (the writer only closes it because the next write no longer fits; a long group is more than M by itself),
 *   and a long group of c chunks holds more than (c - 1) M bytes.  So the densest run of chunks alternates a one-chunk group of 1
 *   byte with a long group of M + 1 bytes (2 chunks): 3 chunks in M + 2 bytes; every other neighbourhood - two one-chunk groups (2 in
 *   M + 1), a longer long group (c + 1 in (c - 1) M + 2) - is sparser for M > 1.  The densest run of groups alternates writes of 1
 *   and M bytes: 2 groups in M + 1 bytes; a long group is 1 group in more than M.  Hence
 *     C = 3 floor(S / (M + 2)) + min(S mod (M + 2), 2),   G = 2 floor(S / (M + 1)) + min(S mod (M + 1), 1).
 *   tests/test_bstreams_encode_cpu.py enumerates every schedule of up to 6 writes at M = 3, 4, 5 against these counts.  0 for an
 *   unknown codec; 4 for src_bytes 0.  Host arithmetic.
 * Arguments, as fourmc_gpu_images_compress checks them, on the host before any device is looked for and with `items` untouched on
 *   every failure, the codec first: an unknown codec; items NULL with n > 0; d_src NULL with a nonzero src_bytes or d_writes NULL with
 *   a nonzero n_writes; a source outside [0, src_total), a table range outside [0, writes_total) or - unless this is the query - an
 *   image region outside [0, images_bytes); two image regions of nonzero image_cap that overlap: FOURMC_EINVAL.  A zstd level outside
 *   the device's 1 .. 12: FOURMC_EUNSUP.  n == 0: FOURMC_OK.  No device: FOURMC_ENODEV.  More than 0x7FFFFFFF chunks in all:
 *   FOURMC_EUNSUP.  A codec result outside [1, bound] fails the call with FOURMC_EINVAL, as in bstream_compress.
 * Work.  Plan: one wave per 64 table entries sums them (64-bit) and one workgroup per stream turns the tile sums into prefixes (the
 *   count / finish pattern of the line scan), which also gives _SUM and _WRITE; then one wave per stream chases the groups, each step
 *   a 64-ary search for the last prefix <= start + M over the tile prefixes and then the entries of one tile, so its serial length is
 *   the number of groups, not of writes.  The chase runs twice, as the decode walk does: for the counts, which come back in the one
 *   read-back that sizes everything else, then for the group table.  Uniform schedules are closed form.  Encode: the chunks of all
 *   streams in file order, in rounds of at most FOURMC_BSW_ROUND chunks (default 512, read at every call): one thread per chunk
 *   writes its descriptor (its staging slot is its bound rounded up to 256 bytes), the raw codec call runs over the round
 *   (FOURMC_LZ4_ENCODE=parallel and the launch-splitting limits apply unchanged), a segmented scan with 64-bit carries per stream
 *   gives every chunk its place and the pack writes group header, chunk header, payload and trailer; a last kernel, one thread per
 *   stream, leaves the lengths and writes the four bytes of a stream without a chunk.  A round may end inside a stream and inside a
 *   long group: the carries live on the device.
 * Synchronizations of `stream`: two (the plan's read-back, the results); the query takes one.
 * Writes.  Nothing outside [image_off, image_off + image_bytes) of the items that are FOURMC_BSW_OK.  Two items may name the same
 *   source bytes or table entries.  d_src, d_writes and d_images must not overlap each other (not checked). */
enum {
    FOURMC_BSW_OK    = 0,
    FOURMC_BSW_SUM   = 1,   /* the write sizes do not sum to src_bytes                    */
    FOURMC_BSW_WRITE = 2,   /* a write size above 0x7FFFFFFF                              */
    FOURMC_BSW_CAP   = 3,   /* image_cap below the exact worst case of the schedule       */
    FOURMC_BSW_LINE  = 4    /* the line writers below: a line that cannot be read         */
};
typedef struct fourmc_bstream_enc_item {   /* 72 bytes */
    uint64_t src_off, src_bytes;      /* in : d_src[src_off, +src_bytes)                                             */
    uint64_t image_off, image_cap;    /* in : the stream goes to d_images[image_off, +image_cap)                     */
    uint64_t writes_off, n_writes;    /* in : entries [writes_off, +n_writes) of d_writes are this stream's write() sizes */
    uint32_t write_bytes;             /* in : with n_writes == 0: every write() this long, the last one short;
                                              0 = one write() of the whole source                                    */
    int32_t  reason;                  /* out: FOURMC_BSW_OK / _SUM / _WRITE / _CAP                                   */
    uint64_t image_bytes;             /* out: the stream's length (size query: the exact worst case for this schedule) */
    uint32_t groups, chunks;          /* out                                                                         */
} fourmc_bstream_enc_item;
int fourmc_gpu_bstreams_compress(const void* d_src, uint64_t src_total, const uint32_t* d_writes, uint64_t writes_total,
                                 void* d_images, uint64_t images_bytes, int codec, int level,
                                 fourmc_bstream_enc_item* items /*host*/, uint32_t n, void* stream);
uint64_t fourmc_gpu_bstream_writes_bound(uint64_t src_bytes, int codec);   /* host only, any schedule */

/* ---- .4mc / .4mz images from a job's write() calls, many per call ---------------------------------------------------------------
 * fourmc_gpu_images_compress cuts a block at every 4 MiB of input, as the `4mc` command line does.  A Hadoop job that names
 * FourMcCodec, FourMzCodec or one of their six siblings as its output codec writes through FourMcOutputStream / FourMzOutputStream
 * (FourMcOutputStream.java:69-223 over Lz4Compressor.java:147-298 / ZstdCompressor, with close()), whose blocks end at write()
 * boundaries.  This call writes those files: for (data, write sizes, magic, level) the image is what that Java writes, byte for byte.
 * tests/fourmc_stream_model.py restates the Java buffer by buffer; no JVM wrote a fixture for it.
 * Block cuts, M = 4194304 (FourMcOutputStream.java:140-182).  Zero-length writes do nothing (:153).  At a write of w bytes with
 *   acc > 0 bytes accumulated and acc + w > M the accumulated bytes become a block and acc = 0 (:157-161).  A write of w > M then
 *   becomes ceil(w / M) blocks of its own, all of M bytes but the last, and the next write starts fresh (:163-173): the short rest is
 *   not joined with what follows.  A write of w <= M accumulates (:176); when acc reaches M exactly the block is written at once
 *   (:177-181).  close() writes what is accumulated (:105).  These are the chunks of the block streams above with M = 4 MiB in place
 *   of the codec's max input, and the same device planner finds them.
 * Block payload (FourMcOutputStream.java:195-223).  The compressor call is the JNI one with unlimited output: LZ4_compress,
 *   LZ4_compressMC, LZ4_compressHC2(level) into a buffer of LZ4_compressBound (jniCompressor.c:91, :123, :156), ZSTD_compress with a
 *   capacity of 1 GiB (jniZstdCompressor.c:93, :126, :160).  With u the block's length and c the call's result, the block is stored
 *   when u <= c (:204): BE32(u) BE32(u) BE32(xxh32(raw)) and the raw bytes; otherwise BE32(u) BE32(c) BE32(xxh32(payload)) and the
 *   payload.  The stream's 4 MiB byte buffer (compress(buffer, 0, buffer.length), :196) caps nothing that matters: bytesWritten is
 *   min(c, 4 MiB) (Lz4Compressor.java:248-249), and a result above 4 MiB gives u <= 4 MiB <= bytesWritten, the stored case.
 *   This is NOT the CLI's rule, which compresses into u - 1 bytes and stores when that fails.  For the LZ4 codecs the two give the
 *   same bytes; for zstd a tight capacity can change the encoder's decisions near the end of an almost incompressible block, so the
 *   device runs the raw codec call with capacity = the codec's bound, as fourmc_gpu_bstreams_compress does, and then applies u <= c.
 * Framing.  magic, 1, xxh32 of those 8 bytes (:69-80); the blocks; twelve zero bytes (:108-110); the footer size, 1, deltas, size,
 *   magic, xxh32 with size = 20 + 4 * blocks, deltas[0] = 12 and deltas[i] = offset of block i less offset of block i - 1
 *   (:113-129): the layout fourmc_gpu_image_compress writes.  A stream without a non-empty write is the 44-byte image.
 * Levels.  `level` is the CLI level of fourmc_gpu_images_compress; the eight codec classes map to it as
 *   FourMcCodec 1 (LZ4_compress), FourMcMediumCodec 2 (LZ4_compressMC), FourMcHighCodec 3 (LZ4_compressHC2 4, Lz4HighCompressor.java:47),
 *   FourMcUltraCodec 4 (LZ4_compressHC2 8, Lz4UltraCompressor.java:47), FourMzCodec 1 (ZSTD_compress 1, jniZstdCompressor.c:94),
 *   FourMzMediumCodec 2 (ZSTD_compress 3, :127), FourMzHighCodec 3 (ZSTD_compress 6, ZstdHighCompressor.java:46),
 *   FourMzUltraCodec 4 (ZSTD_compress 12, ZstdUltraCompressor.java:46).
 * Schedules: as fourmc_bstream_enc_item has them (a table of uint32 sizes in device memory, or the uniform schedule).
 * Verdicts, per item, FOURMC_BSW_*; an item that gets one writes nothing into its region and costs only itself: _SUM, _WRITE (it
 *   wins over _SUM; image_bytes, blocks and stored_blocks are then 0) and _CAP: image_cap below the exact worst case of the schedule,
 *   12 + sum over the blocks of (12 + len) + 12 + 20 + 4 * blocks = 44 + 16 * blocks + src_bytes (the stored fallback means no block
 *   exceeds its input); image_bytes and blocks then hold that worst case and the plan's count.
 * The size query.  d_images NULL plans only: blocks, and image_bytes = that worst case.  One synchronization.
 * fourmc_gpu_image_writes_bound(S) = 12 + 16 * C(S) + S + 32 holds for every schedule over S bytes, with
 *   C(S) = 3 * (S / (M + 2)) + min(S mod (M + 2), 2) the most blocks any schedule has (a 1-byte write in front of a write of M + 1:
 *   the argument of fourmc_gpu_bstream_writes_bound).
 * Arguments, checked on the host before a device is looked for, the magic first, `items` untouched: FOURMC_EINVAL for a magic that
 *   is neither 4mc nor 4mz, items NULL with n > 0, d_src NULL with a nonzero src_bytes, d_writes NULL with a nonzero n_writes, a
 *   source outside [0, src_total), a table range outside [0, writes_total), and - unless this is the query - a region outside
 *   [0, images_bytes) or two regions of nonzero image_cap that overlap.  n == 0: FOURMC_OK.  More than 0x7FFFFFFF blocks in all (known
 *   after the plan): FOURMC_EUNSUP.  No device: FOURMC_ENODEV.  A codec result outside [1, bound]: FOURMC_EINVAL after the call's work.
 * Work.  The plan of fourmc_gpu_bstreams_compress with M = 4 MiB (its kernels, launched as they are), one read-back.  Then rounds of
 *   at most FOURMC_BSW_ROUND blocks (default 512, read at every call) in file order over all streams: the block streams' descriptor
 *   kernel (staging slot = the codec's bound rounded up to 256), the raw codec launch, a seal-and-scan kernel (stored or compressed
 *   per block, a descriptor that points a stored block at its source bytes and a compressed one at its staging slot, and a segmented
 *   scan with a 64-bit carry per stream that places every block and records its offset for the footer), the XXH32 launch over those
 *   descriptors and the pack launch of the whole-image encode over them.  After the last round one workgroup per image writes the
 *   header, the end mark and the footer.  A round may end inside a stream and inside a long write.
 * Synchronizations of `stream`: two (the plan's read-back, the results); the query takes one.
 * Writes.  Nothing outside [image_off, image_off + image_bytes) of the items that are FOURMC_BSW_OK.
 * Not reproduced: a file written by a JVM as a fixture; .4mc and .4mz in one call; a streaming writer with Hadoop's cuts
 *   (fourmc_gpu_image_writer_* cuts at every 4 MiB). */
typedef struct fourmc_image_wr_item {   /* 80 bytes */
    uint64_t src_off, src_bytes;      /* in : d_src[src_off, +src_bytes), the stream's data                          */
    uint64_t image_off, image_cap;    /* in : the image goes to d_images[image_off, +image_cap)                      */
    uint64_t writes_off, n_writes;    /* in : entries [writes_off, +n_writes) of d_writes; n_writes == 0: uniform    */
    uint32_t write_bytes;             /* in : uniform schedule: every write() this long, the last short; 0 = one write() */
    int32_t  reason;                  /* out: FOURMC_BSW_OK / _SUM / _WRITE / _CAP                                   */
    uint64_t image_bytes;             /* out: the image's length (query, _CAP: the exact worst case)                 */
    uint64_t blocks, stored_blocks;   /* out: its blocks, and those written raw                                      */
} fourmc_image_wr_item;
int fourmc_gpu_images_compress_writes(const void* d_src, uint64_t src_total, const uint32_t* d_writes, uint64_t writes_total,
                                      void* d_images, uint64_t images_bytes, uint32_t magic, int level,
                                      fourmc_image_wr_item* items /*host*/, uint32_t n, void* stream);
uint64_t fourmc_gpu_image_writes_bound(uint64_t src_bytes);   /* host only, holds for every schedule */

/* ---- text lines written as the part files of a TextOutputFormat job, many per call -------------------------------------------------
 * The line readers above hand out lines in two layouts: a packed buffer with a table of starts and a table of text lengths
 * (image_read_lines, _batch, images_read_lines), or rows of a fixed stride with a table of text lengths (image_read_lines_at).  These
 * calls take lines in either layout - all of them, or the ones a table of picks names, in its order - and write them as the files a
 * job with TextOutputFormat and one of the sixteen codecs writes.
 * The writer rule.  Hadoop's TextOutputFormat.LineRecordWriter with a NullWritable / null key, over new DataOutputStream(
 *   codec.createOutputStream(fileOut)), issues for every record out.write(text, 0, len) and then out.write(NEWLINE), NEWLINE the one
 *   byte 0x0A; DataOutputStream passes both straight to the codec stream's write(b, off, len).  This is written from knowledge of
 *   Hadoop's classes: the Hadoop source is not part of this tree and no JVM wrote a fixture.  For lines of text lengths
 *   l_0 .. l_{k-1} the data is text_0 '\n' text_1 '\n' .. text_{k-1} '\n', T = sum(l_j) + k bytes, and the write schedule is
 *   [l_0, 1, l_1, 1, .., l_{k-1}, 1], 2 k entries - not one write per line: FourMcOutputStream ends blocks at write boundaries
 *   (FourMcOutputStream.java:153-181), so a block can end between a text and its LF, and a line of 4 MiB is followed by a block that
 *   holds only the LF.  An empty line is a zero-length write, which both streams ignore, and a one-byte write.  Every record gets its
 *   newline: the data always ends with LF, and an image whose last line was unterminated comes back one byte longer.  Text is copied
 *   as it is: a CR or LF inside a text is written and reads back as more lines, as with the Java writer.  No line at all is the stream
 *   with no write: the 44-byte image, or the block stream 00 00 00 00.  tests/text_output_model.py restates the rule.
 * The lines (fourmc_lines_src, in device memory, one description per call).  Table line k is d_text_len[k] bytes at
 *   d_text[d_starts[k]] - or, with d_starts NULL, at d_text[k * row_bytes], the rows of image_read_lines_at.  Output line j of an item
 *   is table line d_pick[line_off + j], or line_off + j without d_pick.  A pick may name a line more than once and in any order, two
 *   items may share picks and lines, and lines may overlap in d_text: a compaction of matching line numbers, a slice of a random
 *   permutation or the d_lines of image_read_lines_at can be passed as they are.
 * Verdicts, per item, FOURMC_BSW_*, the first that applies; an item that gets one copies nothing and costs only itself:
 *   FOURMC_BSW_WRITE  a text length above 0x7FFFFFFF (the write planner would refuse that write; it is decided before any copy);
 *   FOURMC_BSW_LINE   a line that cannot be read: a pick >= table_lines, d_starts[k] + d_text_len[k] > text_bytes, or in the row
 *                     layout d_text_len[k] > row_bytes (the reader cut that row short; writing it would silently lose text);
 *   FOURMC_BSW_CAP    lines_pack: packed_cap < T.  The writers: image_cap below the exact worst case, as the call below them says;
 *   FOURMC_BSW_SUM    is never given (the write table is made from the same lengths as the text).
 * fourmc_gpu_lines_pack writes, for every item that is OK, the data to d_packed[packed_off, +T) and the schedule to
 *   d_writes[writes_off, +2 n_lines): what fourmc_gpu_images_compress_writes, fourmc_gpu_bstreams_compress and - for .zst targets,
 *   whose files do not depend on write sizes - fourmc_gpu_zsts_compress take.  packed_bytes = T, also for _CAP; 0 for _WRITE and
 *   _LINE.  d_packed NULL is the size query: nothing is copied, no table is written, regions are not looked at.  The call returns
 *   after its one synchronization; the copy is queued on `stream` behind it.
 * The two writers are the pack into staging the call owns followed by fourmc_gpu_images_compress_writes / fourmc_gpu_bstreams_compress
 *   themselves, with d_src = the staging and d_writes = the packed table.  THE ONE RULE: for every item that is OK the image is, byte
 *   for byte, what that call writes for the data and the schedule of the writer rule, and image_bytes, blocks, stored_blocks and the
 *   size query are that call's (block streams: blocks = its chunks, stored_blocks = 0).  An item the pack refused goes below as an
 *   item that owns nothing, so its neighbours' bytes and verdicts are those of a call without it; its image_bytes, blocks and
 *   stored_blocks are 0.  text_bytes = T.  d_images NULL is the size query: nothing is copied (only the write table is made, which the
 *   planner reads) and image_bytes is the exact worst case of the schedule.  `magic`, `level`, `codec`: as those calls take them.
 * Staging, leased per stream from two registries of the line writers' own (the calls below lease theirs and may grow them) and given
 *   back by fourmc_gpu_release_workspaces: 64 bytes per item, 8 bytes per line and per 64 lines for the offsets and tile prefixes;
 *   for the writers also sum(T) bytes of text and 8 bytes per line of write sizes.
 * Arguments, checked on the host before a device is looked for, each FOURMC_EINVAL with `items` untouched and a message that names the
 *   call and the item: the magic / codec checks of the calls below, first; then src or items NULL with n > 0; d_text NULL with
 *   text_bytes > 0; d_text_len NULL with table_lines > 0; d_starts NULL and row_bytes 0 with table_lines > 0; in the row layout
 *   table_lines * row_bytes overflowing or above text_bytes; per item [line_off, +n_lines) outside pick_total (outside table_lines
 *   without a pick); and - unless this is the query - d_writes NULL (lines_pack), a region outside its buffer, a write slice
 *   [writes_off, +2 n_lines) outside writes_total, two regions of nonzero capacity or two non-empty write slices that overlap.  A zstd
 *   level outside the device's 1 .. 12 (bstreams_write_lines): FOURMC_EUNSUP.  n == 0: FOURMC_OK.  No device: FOURMC_ENODEV.  More
 *   than 2^31 - 1 chunks of 16 KiB in one call, or an item of 2^38 lines or more: FOURMC_EUNSUP.
 * Work.  Measure: one lane per output line, one wave per tile of 64 lines, resolves the pick, reads the length, checks it and scans
 *   the piece sizes l + 1; one workgroup per item turns the tile sums into 64-bit prefixes, T and the verdict; one wave places the
 *   items.  After the read-back: the same tiles give every line its 64-bit offset in its item's text and the write table.  Gather:
 *   the packed text is cut into chunks of 16 KiB, one workgroup of 256 each, whatever the lines are; a workgroup finds its chunk's
 *   first and last line by searching the tile prefixes and one tile, and every lane owns aligned 16-byte pieces of the output, which
 *   it fills from one unaligned 16-byte load when they lie inside one text and byte by byte, terminators included, where lines meet.
 *   The kernels clamp what they read from the tables a second time: tables that change during the call may give wrong text, never an
 *   access outside d_text[0, text_bytes), the item's region or its write slice.
 * Synchronizations of `stream`: lines_pack one (the items' sums and verdicts), also as the query; each writer three (that one and
 *   the two of the call below), its query two.  A lease that has to grow synchronizes once more.
 * Writes.  Nothing outside d_packed[packed_off, +T) and d_writes[writes_off, +2 n_lines) / [image_off, +image_bytes) of the items
 *   that are OK.  d_text, the tables and the outputs must not overlap each other (not checked).
 * Not reproduced: the key form of the record writer (key, separator, value, newline: four writes per record); a separator or
 *   terminator other than LF; .zst targets through a call of their own (lines_pack plus fourmc_gpu_zsts_compress gives them); .4mc
 *   and .4mz in one call; a streaming form. */
typedef struct fourmc_lines_src {
    const void*     d_text;      uint64_t text_bytes;   /* the bytes the lines point into                                      */
    const uint64_t* d_starts;                           /* line k's text starts at d_text[d_starts[k]]; NULL: at k * row_bytes  */
    uint32_t        row_bytes;                          /* the stride when d_starts is NULL (image_read_lines_at's rows)        */
    const uint32_t* d_text_len;                         /* text length without terminator, as the readers write it             */
    uint64_t        table_lines;                        /* entries of d_starts / d_text_len (rows of d_text)                    */
    const uint64_t* d_pick;      uint64_t pick_total;   /* optional: output line j of an item is table line d_pick[line_off + j];
                                                           NULL: table line line_off + j.  Duplicates and any order allowed      */
} fourmc_lines_src;
typedef struct fourmc_lines_pack_item {   /* host, 56 bytes */
    uint64_t line_off, n_lines;           /* in : entries of d_pick if given, else of the tables                         */
    uint64_t packed_off, packed_cap;      /* in : the text goes to d_packed[packed_off, +packed_cap)                     */
    uint64_t writes_off;                  /* in : its 2 * n_lines sizes go to d_writes[writes_off, ...)                   */
    int32_t  reason, pad;                 /* out: FOURMC_BSW_OK / _WRITE / _LINE / _CAP                                  */
    uint64_t packed_bytes;                /* out: T (also for the query and for _CAP)                                    */
} fourmc_lines_pack_item;
int fourmc_gpu_lines_pack(const fourmc_lines_src* src, void* d_packed, uint64_t packed_total,
                          uint32_t* d_writes, uint64_t writes_total,
                          fourmc_lines_pack_item* items /*host*/, uint32_t n, void* stream);
typedef struct fourmc_lines_wr_item {     /* host, 72 bytes */
    uint64_t line_off, n_lines;           /* in : entries of d_pick if given, else of the tables                         */
    uint64_t image_off, image_cap;        /* in : the file goes to d_images[image_off, +image_cap)                       */
    int32_t  reason, pad;                 /* out: FOURMC_BSW_* of the pack or of the writer below it                     */
    uint64_t text_bytes;                  /* out: T                                                                      */
    uint64_t image_bytes, blocks, stored_blocks;   /* out: as fourmc_image_wr_item has them; block streams: chunks, 0    */
} fourmc_lines_wr_item;
int fourmc_gpu_images_write_lines  (const fourmc_lines_src* src, void* d_images, uint64_t images_bytes, uint32_t magic, int level,
                                    fourmc_lines_wr_item* items /*host*/, uint32_t n, void* stream);
int fourmc_gpu_bstreams_write_lines(const fourmc_lines_src* src, void* d_images, uint64_t images_bytes, int codec, int level,
                                    fourmc_lines_wr_item* items /*host*/, uint32_t n, void* stream);

/* ---- host-buffer conveniences with the reference's per-block signatures ------------------- */
/* These stage one block through HBM (H2D, one launch, D2H).  They exist so the JNI entry points
 * keep their exact one-call-one-block contract (SURVEY.md §8(b) "Batching constraint").        */
int      fourmc_LZ4_compressBound(int inputSize);                       /* lz4.h:212            */
int      fourmc_LZ4_compress_default(const char* src, char* dst, int srcSize, int dstCapacity);
int      fourmc_LZ4_compressMC(const char* src, char* dst, int srcSize);
int      fourmc_LZ4_compressMC_limitedOutput(const char* src, char* dst, int srcSize, int maxOutputSize);
int      fourmc_LZ4_compress_HC(const char* src, char* dst, int srcSize, int dstCapacity, int compressionLevel);
int      fourmc_LZ4_decompress_safe(const char* src, char* dst, int compressedSize, int dstCapacity);
size_t   fourmc_ZSTD_decompress(void* dst, size_t dstCapacity, const void* src, size_t compressedSize);
size_t   fourmc_ZSTD_compress(void* dst, size_t dstCapacity, const void* src, size_t srcSize, int compressionLevel);   /* zstd.h:156 */
size_t   fourmc_ZSTD_compressBound(size_t srcSize);                                                             /* zstd.h:206 */
unsigned fourmc_XXH32(const void* input, size_t len, unsigned seed);    /* host scalar: framing bytes, JNI xxhash32 */

/* Host batch: `n` blocks described by host-side descriptors over host buffers; the engine does
 * one H2D of the inputs, one launch, one D2H of outputs + descriptors.  Used by the file API.  */
/* Page-locked host memory for staging buffers handed to the two calls below (NULL if it cannot be had: use malloc then). */
void* fourmc_host_alloc(size_t bytes);
void  fourmc_host_free(void* p);
int fourmc_host_4mc_encode(const void* src, size_t src_bytes, void* dst, size_t dst_bytes,
                           fourmc_block* blocks, uint32_t n, int codec, int level);
int fourmc_host_4mc_decode(const void* src, size_t src_bytes, void* dst, size_t dst_bytes,
                           fourmc_block* blocks, uint32_t n, int codec);
/* Encode `n` blocks and return the finished piece of the file image ("12-byte block header + payload" per block, back to
 * back: native/4mc.c:309-315, :321-327) in ONE device-to-host transfer into `image` - which may be the output file itself
 * (a shared mapping).  image_off[b]: where block b's header sits in the piece; *image_bytes: the piece's length. */
int fourmc_host_4mc_encode_image(const void* src, size_t src_bytes, fourmc_block* blocks, uint32_t n, int codec, int level,
                                 void* image, size_t image_cap, uint64_t* image_off, size_t* image_bytes);

/* ---- debug / profiling exports: the research side build only (make -C 4mc_amd/csrc research -> libhadoop-4mc-research.so,
 * -DFOURMC_RESEARCH); the drop-in library does not export them ------------------------------------------------------------ */
#ifdef FOURMC_RESEARCH
/* Profiling aid (not part of the reference boundary): copy a range of the engine's per-block device
 * workspace to the host; the zstd kernels leave per-phase cycle counters there (tools/zstd_timing.py). */
int fourmc_gpu_debug_read_workspace(void* host, size_t offset, size_t bytes);
/* Test aid: blocks the 4mz execute kernel completed / handed back to the one-wave kernel since the last call. */
int  fourmc_gpu_debug_zstd_exec_counts(unsigned long long* executed, unsigned long long* handed_back);
/* Test aid: runs only the parser kernel of the block-parallel LZ4 decoder on `n` blocks and copies the first `bytes` of
 * the workspace (block 0's slot first: header, window descriptors, token positions) to `host`; layout[0..2] = slot bytes,
 * descriptor offset, token offset. */
int fourmc_gpu_debug_lz4_parse(const void* d_src, const void* d_dst, fourmc_block* d_blocks, uint32_t n, int container_mode,
                               void* host, size_t bytes, size_t* layout);
/* Timing aid (tools/records_scan.py): the delimiter scan and compaction of fourmc_gpu_image_read_records alone, over bytes already
 * decoded: d[0, len) as the content of a split that starts the file; *records (host) = the records, d_starts as there (NULL: count
 * only; -5 in *records when starts_cap is too small).  Synchronizes once. */
int fourmc_gpu_debug_records_scan(const void* d, uint64_t len, uint8_t delim, uint64_t* d_starts, uint64_t starts_cap,
                                  int64_t* records, void* stream);
/* The same for fourmc_gpu_image_read_lines: count, finish, write and the length pass; *lines (host) = the lines. */
int fourmc_gpu_debug_lines_scan(const void* d, uint64_t len, uint32_t max_line_len, uint64_t* d_starts, uint32_t* d_text_len,
                                uint64_t lines_cap, int64_t* lines, void* stream);
/* one-block host calls (LZ4_* / ZSTD_* twins, JNI) made so far, and the launches that served them (concurrent calls share one) */
void fourmc_debug_one_block_counters(unsigned long long* calls, unsigned long long* launches);

#endif

#ifdef __cplusplus
}
#endif
#endif
