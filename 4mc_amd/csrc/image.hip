// 4mc_amd/csrc/image.hip — the container layer of whole .4mc / .4mz file images in HBM (fourmc_gpu_image_*).
//
// The codecs, the payload XXH32 and the packing are the existing kernels; what is here is the framing around them:
//   encode  descriptors from the input size (4 MiB blocks, the last one short), the exclusive scan of 12 + csize into the
//           64-bit image offsets (native/4mc.c:293), and the file header, end mark and footer (framing.c, native/4mc.c:330-361)
//           with the footer's XXH32 computed here;
//   decode  two parsers of an image into block descriptors, and the reduction of the per-block results and the framing
//           verdict into the status the CLI's decode_stream (fourmc_file.c) would end with.
// Parsers.  The fast path proves a single stream from its footer: the footer's deltas give every block header's offset, and
// one lane per block checks that header and that it ends where the next one starts; the last one must end at the end mark.
// The walk is decode_stream's loop on one lane, in file order, for everything else (a damaged or lying footer, a truncated
// image, trailing bytes, a concatenation of streams).  Both write the same summary and, after the engine has allocated for the
// count it read back, the same descriptors.  Header fields are big-endian u32 at any byte offset.
// Streaming writes reuse the encode half: a batch's descriptors may start inside a chunk or in the writer's carry slot, and its scan
// runs on from the offset the previous batch left in the writer's device index.
// Many images (fourmc_gpu_images_decompress): the same parsers and reduction, one wave per image of one buffer, and a plan that
// gives every image its slice of one descriptor table.
// Many images, the encode (fourmc_gpu_images_compress): the same descriptors, scan and tail, one wave or workgroup per image, over
// slices of one descriptor table and one dense offset table that the engine has laid out from the sizes.
// Images from write() sizes (fourmc_gpu_images_compress_writes): blocks cut as Hadoop's FourMcOutputStream cuts them, planned and
// described by the block streams' kernels (bstream.hip); here the seal (stored or compressed, by the stream's rule) with the
// segmented scan across rounds, and the tail per image.
// Random access (second half): the footer index of a single stream, block-range decodes and byte-range reads, each with the
// verdict fourmc_file_decode_blocks (fourmc_file.c) reaches on the same bytes as a file.
// Streaming reads (last part): the walk restated to stop at the end of each appended chunk and resume at the next, the gather of
// payload bytes into staging slots, the fold of each decoded batch and the finish that decides what waited for more bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"
#include "devcopy.h"
#include "devframe.h"       // be32 / put_be32, scan_add / wave_total

namespace {

constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
constexpr uint32_t kBlock = FOURMC_BLOCKSIZE;

__device__ __forceinline__ uint32_t le32(const uint8_t* p)
{ return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24); }
__device__ __forceinline__ uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// XXH32 on one lane (xxhash.c:392-415): framing bytes (a footer, a file header) and, on the error path only, the payload whose
// checksum decides between two messages (fourmc_file.c:521-525)
__device__ uint32_t xxh32_lane(const uint8_t* p, uint64_t len, uint32_t seed)
{
    uint64_t left = len;
    uint32_t h;
    if (len >= 16) {
        uint32_t v0 = seed + P1 + P2, v1 = seed + P2, v2 = seed, v3 = seed - P1;
        for (; left >= 16; left -= 16, p += 16) {
            v0 = rotl(v0 + le32(p) * P2, 13) * P1;      v1 = rotl(v1 + le32(p + 4) * P2, 13) * P1;
            v2 = rotl(v2 + le32(p + 8) * P2, 13) * P1;  v3 = rotl(v3 + le32(p + 12) * P2, 13) * P1;
        }
        h = rotl(v0, 1) + rotl(v1, 7) + rotl(v2, 12) + rotl(v3, 18);
    } else h = seed + P5;
    h += uint32_t(len);
    for (; left >= 4; left -= 4, p += 4) h = rotl(h + le32(p) * P3, 17) * P4;
    for (; left; left--, p++) h = rotl(h + uint32_t(*p) * P5, 11) * P1;
    h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16;
    return h;
}

// ------------------------------------------------------------------------------------------------------------- encode
// block b of an item's n: src0 + b * 4 MiB of the source, dst0 + b * 4 MiB of the staging, src_len = what is left of src_bytes, at
// most 4 MiB.  The item's descriptors are blocks[0, n): a single image and a writer's batch pass the table, one image of many its slice.
__device__ __forceinline__ void enc_desc(fourmc_block* __restrict__ blocks, uint64_t src0, uint64_t dst0, uint64_t src_bytes, uint32_t n,
                                         uint32_t b)
{
    if (b >= n) return;
    const uint64_t at = uint64_t(b) * kBlock;
    fourmc_block d;
    d.src_off = src0 + at; d.dst_off = dst0 + at;
    d.src_len = uint32_t(src_bytes - at < kBlock ? src_bytes - at : kBlock);
    d.dst_cap = d.src_len; d.result = 0; d.xxh32 = 0;
    blocks[b] = d;
}
__global__ __launch_bounds__(256)
void image_enc_desc_kernel(fourmc_block* __restrict__ blocks, uint64_t src_bytes, uint32_t n)
{ enc_desc(blocks, 0, 0, src_bytes, n, blockIdx.x * 256 + threadIdx.x); }
// a batch of the streaming writer: its blocks start at src0 of its chunk (or of the carry slot) and at dst0 of its staging
__global__ __launch_bounds__(256)
void image_wr_desc_kernel(fourmc_block* __restrict__ blocks, uint64_t src0, uint64_t dst0, uint64_t src_bytes, uint32_t n)
{ enc_desc(blocks, src0, dst0, src_bytes, n, blockIdx.x * 256 + threadIdx.x); }

// off[b] = start + sum_{j<b} (12 + csize_j), b = 0..n-1, on one wave, 64 blocks per step with a 64-bit carry; returns what off[n]
// would be (where the end mark goes).  `start` is where the first block header lies: 12 in a single image (native/4mc.c:293).  A
// result outside [1, src_len] cannot come from the container encode; it is counted in *bad (every lane gets the wave's count; the
// engine fails the call) and clamped so that the pack and the footer stay inside the bound the engine checked the capacity against.
__device__ __forceinline__ uint64_t enc_scan(fourmc_block* __restrict__ blocks, uint64_t* __restrict__ off, uint32_t n, uint64_t start,
                                             uint32_t* bad_out)
{
    const int lane = threadIdx.x;
    uint64_t carry = start;
    uint32_t bad = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 64) {
        const uint32_t b = b0 + uint32_t(lane);
        uint32_t step = 0;
        if (b < n) {
            const fourmc_block d = blocks[b];
            int32_t r = d.result;
            if (r <= 0 || uint32_t(r) > d.src_len) { bad++; r = r <= 0 ? 0 : int32_t(d.src_len); blocks[b].result = r; }
            step = 12u + uint32_t(r);
        }
        const uint32_t incl = scan_add(step);
        if (b < n) off[b] = carry + (incl - step);
        carry += wave_total(incl);
    }
    for (int o = 32; o; o >>= 1) bad += uint32_t(__shfl_xor(int(bad), o));
    *bad_out = bad;
    return carry;
}
// A single image: the scan from 12, off[n] and the summary.
// kWriter: one batch of the streaming writer.  `off` is its device index at the batch's first block number; the scan starts from
// off[0], the running image offset the previous batch left there as its off[n] (12 before the first), and adds its bad results to
// the running count.
template <bool kWriter>
__global__ __launch_bounds__(64)
void image_enc_scan_kernel(fourmc_block* __restrict__ blocks, uint64_t* __restrict__ off, uint32_t n, fourmc_image_enc_summary* sum)
{
    uint32_t bad = 0;
    const uint64_t carry = enc_scan(blocks, off, n, kWriter ? off[0] : 12, &bad);
    if (threadIdx.x == 0) {
        off[n] = carry;
        if (kWriter) {
            sum->bad_blocks += bad;
        } else {
            sum->image_bytes = carry + 12 + 20 + 4ull * n;
            sum->bad_blocks = bad;
        }
    }
}

// file header at 0 of `image`, end mark at `end`, footer behind it (framing.c: fourmc_frame_header / fourmc_frame_footer), on one
// workgroup of 256.  off[0, n): the block headers' offsets, counted from `base` bytes in front of the image (0: in-image offsets);
// end: the in-image offset of the end mark.  Only differences of off[] and off[0] - base (the 12 of the first header) are written.
__device__ __forceinline__ void enc_tail(uint8_t* __restrict__ image, const uint64_t* __restrict__ off, uint32_t n, uint64_t end,
                                         uint64_t base, uint32_t magic)
{
    const uint32_t t = threadIdx.x;
    uint8_t* foot = image + end + 12;
    const uint32_t fsz = 20u + 4u * n;
    if (t == 0) {
        put_be32(image, magic); put_be32(image + 4, 1);
        put_be32(foot, fsz); put_be32(foot + 4, 1);
        put_be32(foot + 8 + 4 * n, fsz); put_be32(foot + 12 + 4 * n, magic);
    }
    if (t < 12) image[end + t] = 0;
    for (uint32_t i = t; i < n; i += 256)                 // delta to the previous block; the first one absolute in the image
        put_be32(foot + 8 + 4 * i, uint32_t(i ? off[i] - off[i - 1] : off[0] - base));
    __threadfence();
    __syncthreads();
    if (t == 0) {
        put_be32(image + 8, xxh32_lane(image, 8, 0));
        put_be32(foot + fsz - 4, xxh32_lane(foot, fsz - 4, 0));
    }
}
__global__ __launch_bounds__(256)
void image_enc_tail_kernel(uint8_t* __restrict__ image, const uint64_t* __restrict__ off, uint32_t n, uint32_t magic)
{ enc_tail(image, off, n, off[n], 0, magic); }

// ---- many images (fourmc_gpu_images_compress): the three steps above for n images at once.  ONE descriptor table, with offsets
// relative to the common source and to one staging, describes every block of every image, so one container encode serves them all;
// the dense offset table holds offsets absolute in d_images, so one pack does too.
// Descriptors, one wave per image over its slice (the engine's argument loop has computed the slices: fourmc_image_enc_plan).
__global__ __launch_bounds__(64)
void images_enc_desc_kernel(const fourmc_image_enc_plan* __restrict__ plans, fourmc_block* __restrict__ blocks)
{
    const fourmc_image_enc_plan pl = plans[blockIdx.x];
    for (uint32_t b0 = 0; b0 < pl.nblocks; b0 += 64)
        enc_desc(blocks + pl.first, pl.src_off, pl.stage_off, pl.src_bytes, pl.nblocks, b0 + threadIdx.x);
}
// Scan, one wave per image: its first block header lies at image_off + 12 of d_images.  end[i]: where its end mark goes (absolute);
// res[i]: its length and its bad results.  An image without blocks has its end mark at 12.
__global__ __launch_bounds__(64)
void images_enc_scan_kernel(const fourmc_image_enc_plan* __restrict__ plans, fourmc_block* __restrict__ blocks, uint64_t* __restrict__ off,
                            uint64_t* __restrict__ end, fourmc_image_enc_result* __restrict__ res)
{
    const uint32_t i = blockIdx.x;
    const fourmc_image_enc_plan pl = plans[i];
    uint32_t bad = 0;
    const uint64_t carry = enc_scan(blocks + pl.first, off + pl.first, pl.nblocks, pl.image_off + 12, &bad);
    if (threadIdx.x == 0) {
        end[i] = carry;
        res[i].image_bytes = carry - pl.image_off + 12 + 20 + 4ull * pl.nblocks;
        res[i].bad_blocks = bad;
    }
}
// Tail, one workgroup per image: the footer's first delta is the in-image 12, whatever image_off is
__global__ __launch_bounds__(256)
void images_enc_tail_kernel(uint8_t* __restrict__ images, const fourmc_image_enc_plan* __restrict__ plans, const uint64_t* __restrict__ off,
                            const uint64_t* __restrict__ end, uint32_t magic)
{
    const uint32_t i = blockIdx.x;
    const fourmc_image_enc_plan pl = plans[i];
    enc_tail(images + pl.image_off, off + pl.first, pl.nblocks, end[i] - pl.image_off, pl.image_off, magic);
}

// ---- images from write() sizes (fourmc_gpu_images_compress_writes): the blocks are the chunks of the block streams' plan at
// M = 4 MiB and come in rounds, with that plan's descriptors and side entries (bstream.hip: bsw_desc_kernel); the raw codec call has
// run over them with the codec's bound as the capacity.
// Seal and scan, one wave over the round's m blocks.  Seal (FourMcOutputStream.java:204): a block whose result c is not below its
// length u is stored.  seal[b] names the bytes that go behind block b's header from ONE base address, so that one XXH32 launch and
// one pack launch serve stored and compressed blocks alike: dst_off = the source bytes (src_delta + src_off) or the staging slot
// (stage_delta + dst_off), result = their number (u or c), src_len = u.  Scan: idx[b] = the block header's absolute offset in
// d_images = its stream's image_off + 12 + the bytes of the stream's blocks in front of it: those of earlier rounds in
// run[stream].bytes, those of this round by the wave's prefix sum less its value at the segment's head (a stream's blocks are
// consecutive).  A result outside [1, bound] is counted in *bad and the block stored, so nothing leaves the worst case the engine
// checked the capacity against.
__global__ __launch_bounds__(64)
void imgw_seal_kernel(const fourmc_block* __restrict__ blocks, const fourmc_bsw_side* __restrict__ side, uint32_t m, int zstd,
                      const fourmc_bstream_enc_item* __restrict__ items, uint64_t src_delta, uint64_t stage_delta,
                      fourmc_block* __restrict__ seal, uint64_t* __restrict__ idx, fourmc_imgw_run* __restrict__ run,
                      uint64_t* __restrict__ bad_out)
{
    const int lane = threadIdx.x;
    uint32_t run_stream = 0xFFFFFFFFu, bad = 0;
    uint64_t run_bytes = 0, run_stored = 0;
    for (uint32_t b0 = 0; b0 < m; b0 += 64) {
        const uint32_t b = b0 + uint32_t(lane);
        const bool valid = b < m;
        uint32_t step = 0, st = 0xFFFFFFFFu, stored = 0;
        if (valid) {
            const fourmc_block d = blocks[b];
            st = side[b].stream;
            const bool wrong = d.result <= 0 || uint32_t(d.result) > fourmc_bstream_block_bound(zstd, d.src_len);
            bad += wrong;
            stored = wrong || d.src_len <= uint32_t(d.result);
            fourmc_block q;
            q.src_off = d.src_off; q.src_len = d.src_len;
            q.dst_off = stored ? src_delta + d.src_off : stage_delta + d.dst_off;
            q.result = int32_t(stored ? d.src_len : uint32_t(d.result));
            q.dst_cap = uint32_t(q.result); q.xxh32 = 0;
            seal[b] = q;
            step = 12u + uint32_t(q.result);
        }
        const uint32_t incl = scan_add(step), incl_s = scan_add(stored);
        const uint32_t before = uint32_t(__shfl_up(int(st), 1)), after = uint32_t(__shfl_down(int(st), 1));
        const unsigned long long heads = __ballot(valid && (lane == 0 || before != st));
        const int h = 63 - __builtin_clzll((heads & (~0ull >> (63 - lane))) | 1ull);       // the head of this lane's segment
        const uint32_t excl_h = uint32_t(__shfl(int(incl - step), h)), excl_sh = uint32_t(__shfl(int(incl_s - stored), h));
        uint64_t end = 0, end_s = 0;
        if (valid) {
            const bool cont = h == 0 && st == run_stream;                                  // the segment began in an earlier step
            const uint64_t pos = (cont ? run_bytes : run[st].bytes) + (incl - step - excl_h);
            idx[b] = items[st].image_off + 12 + pos;
            end = pos + step;
            end_s = (cont ? run_stored : run[st].stored) + (incl_s - excl_sh);
        }
        const int last = 63 - __builtin_clzll(__ballot(valid));
        if (valid && (lane == last || after != st)) { fourmc_imgw_run r; r.bytes = end; r.stored = end_s; run[st] = r; }
        run_stream = uint32_t(__shfl(int(st), last));
        run_bytes = uint64_t(__shfl((long long)end, last));
        run_stored = uint64_t(__shfl((long long)end_s, last));
    }
    for (int o = 32; o; o >>= 1) bad += uint32_t(__shfl_xor(int(bad), o));
    if (lane == 0) *bad_out += bad;
}
// Tail, one workgroup per stream that is written: its block offsets are its slice of idx (absolute, so the footer's first delta is
// the in-image 12), its end mark lies behind its last block
__global__ __launch_bounds__(256)
void imgw_tail_kernel(uint8_t* __restrict__ images, const fourmc_bstream_enc_item* __restrict__ items,
                      const fourmc_bsw_plan* __restrict__ plans, const fourmc_bsw_slice* __restrict__ slices,
                      const uint64_t* __restrict__ idx, const fourmc_imgw_run* __restrict__ run, uint32_t magic,
                      fourmc_imgw_result* __restrict__ res)
{
    const uint32_t i = blockIdx.x;
    const fourmc_bsw_plan pl = plans[i];
    if (pl.reason != FOURMC_BSW_OK) {
        if (threadIdx.x == 0) { fourmc_imgw_result r; r.image_bytes = 0; r.stored = 0; res[i] = r; }
        return;
    }
    const fourmc_imgw_run rn = run[i];
    const uint64_t image_off = items[i].image_off, end = 12 + rn.bytes;
    enc_tail(images + image_off, idx + slices[i].chunk0, uint32_t(pl.chunks), end, image_off, magic);
    if (threadIdx.x == 0) { fourmc_imgw_result r; r.image_bytes = end + 12 + 20 + 4 * pl.chunks; r.stored = rn.stored; res[i] = r; }
}

// ------------------------------------------------------------------------------------------------------------- decode
// The fast path, one wave.  `blocks` NULL: check only (summary); else write the descriptors of the image it accepted.
// The three bases place one image among many (images_parse_kernel): the image starts at src_base of the buffer the block decode
// reads from, its output at dst_base of the buffer it writes to, its descriptors at blocks + desc_base.  A single image has zeros.
__device__ __forceinline__ void parse_fast(const uint8_t* __restrict__ img, uint64_t N, uint32_t magic, fourmc_image_parse* ps,
                                           fourmc_block* __restrict__ blocks, uint64_t src_base, uint64_t dst_base, uint64_t desc_base)
{
    const int lane = threadIdx.x;
    // the footer at the end: [size][version 1][k deltas][size][magic][xxh32]
    if (N < 44) return;
    const uint32_t fsz = be32(img + N - 12);
    if (fsz < 20 || ((fsz - 20) & 3) || uint64_t(fsz) > N - 24) return;
    const uint64_t F = N - fsz;
    if (be32(img + F) != fsz || be32(img + F + 4) != 1 || be32(img + N - 8) != magic) return;
    if (be32(img) != magic || be32(img + 4) != 1 || be32(img + 8) != xxh32_lane(img, 8, 0)) return;
    const uint64_t eos = F - 12;
    if (be32(img + eos) | be32(img + eos + 4) | be32(img + eos + 8)) return;
    const uint32_t k = (fsz - 20) / 4;
    if (k == 0 && eos != 12) return;
    // every block: its header at off_i (prefix of the deltas), inside [12, eos), not an end mark, sizes the CLI accepts without a
    // message, and its payload ends where the next header (or the end mark) starts
    uint64_t carry = 0, ucarry = 0;
    bool ok = true;
    for (uint32_t i0 = 0; i0 < k && ok; i0 += 64) {
        const uint32_t i = i0 + uint32_t(lane);
        const bool have = i < k;
        const uint32_t delta = have ? be32(img + F + 8 + 4ull * i) : 0u;
        const uint32_t incl = scan_add(delta);
        const uint64_t at = carry + incl;                 // absolute offset of header i
        const uint32_t dtot = wave_total(incl);
        // the start of block i + 1: the next lane's offset, or - for the wave's last block - the next delta, or the end mark
        uint64_t next = eos;
        if (have && i + 1 < k) next = at + be32(img + F + 8 + 4ull * (i + 1));
        bool good = true;
        uint32_t usize = 0, csize = 0, sum = 0;
        if (have) {
            if (i == 0 && at != 12) good = false;
            if (at < 12 || at + 12 > eos) good = false;
            if (good) {
                usize = be32(img + at); csize = be32(img + at + 4); sum = be32(img + at + 8);
                if ((usize | csize | sum) == 0 || csize > kBlock || (usize != csize && usize > kBlock) || at + 12 + csize != next) good = false;
            }
        }
        ok = __ballot(have && !good) == 0;
        const uint32_t uincl = scan_add(have ? usize : 0u);
        if (ok && blocks && have) {
            fourmc_block d;
            d.src_off = src_base + at + 12; d.dst_off = dst_base + ucarry + (uincl - usize);
            d.src_len = csize; d.dst_cap = usize; d.result = 0; d.xxh32 = sum;
            blocks[desc_base + i] = d;
        }
        carry += dtot; ucarry += wave_total(uincl);
    }
    if (!ok) return;
    if (lane == 0 && !blocks) {
        if (xxh32_lane(img + F, fsz - 4, 0) != be32(img + N - 4)) return;
        ps->nblocks = k; ps->total = ucarry; ps->streams = 1; ps->reason = FOURMC_IMG_OK; ps->fail_offset = N;
        ps->fast = 1;
    }
}
__global__ __launch_bounds__(64)
void image_parse_fast_kernel(const uint8_t* __restrict__ img, uint64_t N, uint32_t magic, fourmc_image_parse* ps,
                             fourmc_block* __restrict__ blocks)
{ parse_fast(img, N, magic, ps, blocks, 0, 0, 0); }

// decode_stream's per-field checks (fourmc_file.c:473-592), shared by the whole-image walk and the streaming reader's walk.  Each
// one is decided once the bytes it reads are there; the checks of "unreadable" kinds (N - p < k) are the callers'.
// the file header after its magic: version, then the header checksum (computed over its first 8 bytes)
__device__ __forceinline__ int32_t file_header_verdict(uint32_t version, uint32_t stored, uint32_t computed)
{
    if (version != 1) return FOURMC_IMG_VERSION;
    if (stored != computed) return FOURMC_IMG_HEADER_CHECKSUM;
    return FOURMC_IMG_OK;
}
__device__ __forceinline__ bool end_mark(uint32_t usize, uint32_t csize, uint32_t sum) { return (usize | csize | sum) == 0; }
__device__ __forceinline__ bool csize_beyond(uint32_t csize) { return csize > kBlock; }
__device__ __forceinline__ bool usize_beyond(uint32_t usize, uint32_t csize) { return usize != csize && usize > kBlock; }
// an oversized usize ends with one of two messages: the payload's XXH32 decides (fourmc_file.c:521-525)
__device__ __forceinline__ int32_t usize_verdict(uint32_t payload_hash, uint32_t sum)
{ return payload_hash != sum ? FOURMC_IMG_BLOCK_CHECKSUM : FOURMC_IMG_USIZE_BEYOND; }
// the footer once all fsz bytes are there: its checksum (over fsz - 4 bytes), then its version
__device__ __forceinline__ int32_t footer_verdict(uint32_t computed, uint32_t stored, uint32_t version)
{
    if (computed != stored) return FOURMC_IMG_FOOTER_CHECKSUM;
    if (version != 1) return FOURMC_IMG_FOOTER_VERSION;
    return FOURMC_IMG_OK;
}

// The walk: decode_stream (fourmc_file.c:473-592) and decompress_file's loop over concatenated streams on one lane, the checks in
// their order.  That loop (`do got = decode_stream(..); while (got)`, fourmc_file.c:606-609, native/4mc.c:908-912) ends after a
// stream that decoded 0 bytes, whatever follows it: the walk ends cleanly after a stream whose blocks add up to 0 usize.  count mode (blocks NULL): nothing to do when the fast path has accepted the image; else the summary.  fill mode:
// the same walk, writing the descriptors of the blocks it counted.  The bases: as parse_fast's.
__device__ __forceinline__ void parse_walk(const uint8_t* __restrict__ img, uint64_t N, uint32_t magic, fourmc_image_parse* ps,
                                           fourmc_block* __restrict__ blocks, uint64_t src_base, uint64_t dst_base, uint64_t desc_base)
{
    if (threadIdx.x != 0) return;
    if (!blocks && ps->fast) return;
    uint64_t p = 0, nb = 0, total = 0;
    uint32_t streams = 0;
    int32_t reason = FOURMC_IMG_OK;
    uint64_t at = 0;
    for (;;) {
        at = p;
        if (N == p) break;                                                       // clean end: no byte after a footer
        if (N - p < 4)                     { reason = FOURMC_IMG_MAGIC_UNREADABLE; break; }
        if (be32(img + p) != magic)        { reason = FOURMC_IMG_NOT_4MC; break; }
        if (N - p < 12)                    { reason = FOURMC_IMG_HEADER_UNREADABLE; break; }
        if ((reason = file_header_verdict(be32(img + p + 4), be32(img + p + 8), xxh32_lane(img + p, 8, 0)))) break;
        p += 12; streams++;
        const uint64_t stream_total0 = total;
        for (;;) {
            at = p;
            if (N - p < 12)                { reason = FOURMC_IMG_BLOCK_SIZE_UNREADABLE; break; }
            const uint32_t usize = be32(img + p), csize = be32(img + p + 4), sum = be32(img + p + 8);
            p += 12;
            if (end_mark(usize, csize, sum)) break;
            if (csize_beyond(csize))       { reason = FOURMC_IMG_CSIZE_BEYOND; break; }
            if (N - p < csize)             { reason = FOURMC_IMG_DATA_UNREADABLE; break; }
            if (usize_beyond(usize, csize)) { reason = usize_verdict(xxh32_lane(img + p, csize, 0), sum); break; }
            if (blocks) {
                fourmc_block d;
                d.src_off = src_base + p; d.dst_off = dst_base + total; d.src_len = csize; d.dst_cap = usize; d.result = 0; d.xxh32 = sum;
                blocks[desc_base + nb] = d;
            }
            nb++; total += usize; p += csize;
        }
        if (reason != FOURMC_IMG_OK) break;
        at = p;                                                                  // footer (fourmc_file.c:562-588)
        if (N - p < 4)                     { reason = FOURMC_IMG_FOOTER_UNREADABLE; break; }
        const uint32_t fsz = be32(img + p);
        if (fsz < 8 || N - p < fsz)        { reason = FOURMC_IMG_FOOTER_SHORT; break; }
        if ((reason = footer_verdict(xxh32_lane(img + p, fsz - 4, 0), be32(img + p + fsz - 4), be32(img + p + 4)))) break;
        p += fsz;
        if (total == stream_total0) break;                                       // an empty stream ends the file
    }
    if (!blocks) {
        ps->nblocks = nb; ps->total = total; ps->streams = streams; ps->reason = reason;
        ps->fail_offset = reason == FOURMC_IMG_OK ? N : at;
    }
}
__global__ __launch_bounds__(64)
void image_parse_walk_kernel(const uint8_t* __restrict__ img, uint64_t N, uint32_t magic, fourmc_image_parse* ps,
                             fourmc_block* __restrict__ blocks)
{ parse_walk(img, N, magic, ps, blocks, 0, 0, 0); }

// image_reduce's scan, one wave: the index of the first block whose result is negative (n if none) and *done, the sum of the
// positive results before it
__device__ __forceinline__ uint32_t first_failing(const fourmc_block* __restrict__ blocks, uint32_t n, uint64_t* done_out)
{
    const int lane = threadIdx.x;
    uint64_t done = 0;
    uint32_t first = n;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + uint32_t(lane);
        const int32_t r = i < n ? blocks[i].result : 0;
        const unsigned long long badm = __ballot(i < n && r < 0);
        uint64_t mine = (i < n && r > 0) ? uint64_t(r) : 0;
        if (badm) {
            const uint32_t l = uint32_t(__builtin_ctzll(badm));
            if (uint32_t(lane) >= l) mine = 0;
            first = i0 + l;
        }
        for (int o = 32; o; o >>= 1) mine += uint64_t(__shfl_xor((long long)mine, o));
        done += mine;
        if (badm) break;
    }
    *done_out = done;
    return first;
}
__device__ __forceinline__ int32_t block_reason(int32_t result)
{ return result == FOURMC_BLK_BADSUM ? FOURMC_IMG_BLOCK_CHECKSUM : FOURMC_IMG_CORRUPT; }

// The verdict: the first block that failed its checksum or its decode ends decoding there (file order puts it before any
// framing error, which the parsers only ever report behind the last block they counted); otherwise the parser's verdict.
// `blocks` is the image's own slice of the descriptors; src_base: where the image starts in the buffer their src_off count from.
__device__ __forceinline__ void reduce_verdict(const fourmc_block* __restrict__ blocks, uint32_t n, const fourmc_image_parse* ps,
                                               fourmc_image_status* st, uint64_t src_base)
{
    uint64_t done = 0;
    const uint32_t first = first_failing(blocks, n, &done);
    if (threadIdx.x) return;
    st->decoded_bytes = done;
    st->total_bytes = ps->total;
    st->streams = ps->streams;
    st->blocks = first;
    if (first < n) {
        st->reason = block_reason(blocks[first].result);
        st->exit_code = 4;
        st->fail_offset = blocks[first].src_off - 12 - src_base;
    } else {
        st->reason = ps->reason;
        st->exit_code = fourmc_image_exit_code(ps->reason);
        st->fail_offset = ps->fail_offset;
    }
}
__global__ __launch_bounds__(64)
void image_reduce_kernel(const fourmc_block* __restrict__ blocks, uint32_t n, const fourmc_image_parse* ps, fourmc_image_status* st)
{ reduce_verdict(blocks, n, ps, st, 0); }

// ------------------------------------------------------------------------------------------------------------- many images
// fourmc_gpu_images_decompress: the three steps above for n images of one buffer at once, so that ONE descriptor table with offsets
// relative to two base pointers describes every block of every image and one container decode serves them all.
// Parse, one wave per image.  Count mode (desc NULL): the fast path, then - in the same launch - the walk when it did not accept
// the image; ps[i] is the image's summary.  Fill mode: the parser that accepted the image writes its descriptors at
// desc + first[i]; an image that ends FOURMC_IMG_DST_SMALL has none (what fourmc_gpu_image_decompress' host code decides).
__device__ __forceinline__ bool dst_small(const fourmc_image_parse& s, const fourmc_image_item& it) { return s.total > it.dst_cap; }

__global__ __launch_bounds__(64)
void images_parse_kernel(const uint8_t* __restrict__ images, const fourmc_image_item* __restrict__ items, uint32_t magic, int fast,
                         fourmc_image_parse* ps, const uint64_t* __restrict__ first, fourmc_block* __restrict__ desc)
{
    const uint32_t i = blockIdx.x;
    const fourmc_image_item it = items[i];
    const uint8_t* img = images + it.image_off;
    if (!desc) {
        if (threadIdx.x == 0) ps[i] = fourmc_image_parse{};
        if (fast) parse_fast(img, it.image_bytes, magic, ps + i, nullptr, 0, 0, 0);
        parse_walk(img, it.image_bytes, magic, ps + i, nullptr, 0, 0, 0);    // lane 0 reads what lane 0 wrote: ps[i].fast
        return;
    }
    const fourmc_image_parse s = ps[i];
    if (dst_small(s, it) || s.nblocks == 0) return;
    if (s.fast) parse_fast(img, it.image_bytes, magic, ps + i, desc, it.image_off, it.dst_off, first[i]);
    else parse_walk(img, it.image_bytes, magic, ps + i, desc, it.image_off, it.dst_off, first[i]);
}

// Plan, one workgroup: first[i] = the exclusive prefix of the images' descriptor counts (none for FOURMC_IMG_DST_SMALL), the total
// and the parsers' counts for the engine's first read-back; for the size query (every well-formed block counts, no destination is
// looked at) the final statuses too.  A plain pass in chunks of kPlanThreads images with a carry, not decoupled look-back: its
// workgroups would spin on their predecessors' flags (records.hip), and n images are a few KiB of counts.
constexpr uint32_t kPlanThreads = 256;
__global__ __launch_bounds__(kPlanThreads)
void images_plan_kernel(const fourmc_image_item* __restrict__ items, uint32_t n, const fourmc_image_parse* __restrict__ ps, int query,
                        uint64_t* __restrict__ first, fourmc_images_summary* __restrict__ sum, fourmc_image_status* __restrict__ status)
{
    __shared__ uint64_t wsum[kPlanThreads / 64];
    __shared__ uint32_t taken[2];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t < 2) taken[t] = 0;
    uint64_t carry = 0;
    uint32_t nfast = 0, nwalk = 0;
    for (uint64_t i0 = 0; i0 < n; i0 += kPlanThreads) {
        const uint64_t i = i0 + t;
        uint64_t c = 0;
        if (i < n) {
            const fourmc_image_parse s = ps[i];
            if (s.fast) nfast++; else nwalk++;
            if (query) {
                c = s.nblocks;
                fourmc_image_status r = {};
                r.total_bytes = s.total; r.streams = s.streams; r.blocks = uint32_t(s.nblocks);
                r.reason = s.reason; r.exit_code = fourmc_image_exit_code(s.reason); r.fail_offset = s.fail_offset;
                status[i] = r;
            } else c = dst_small(s, items[i]) ? 0 : s.nblocks;
        }
        uint64_t incl = c;
        for (int o = 1; o < 64; o <<= 1) { const uint64_t v = uint64_t(__shfl_up((unsigned long long)incl, o)); if (int(lane) >= o) incl += v; }
        __syncthreads();                                   // the previous chunk's totals have been read
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint64_t base = 0, total = 0;
        for (uint32_t j = 0; j < kPlanThreads / 64; j++) { if (j < w) base += wsum[j]; total += wsum[j]; }
        if (i < n) first[i] = carry + base + (incl - c);
        carry += total;
    }
    if (nfast) atomicAdd(&taken[0], nfast);
    if (nwalk) atomicAdd(&taken[1], nwalk);
    __syncthreads();
    if (t == 0) { sum->nblocks = carry; sum->fast = taken[0]; sum->walk = taken[1]; }
}

// Reduce, one wave per image over its slice of the descriptors: image_reduce_kernel's verdict with the fail offset counted from
// the image's start, or the FOURMC_IMG_DST_SMALL status fourmc_gpu_image_decompress builds on the host.
__global__ __launch_bounds__(64)
void images_reduce_kernel(const fourmc_image_item* __restrict__ items, const fourmc_image_parse* __restrict__ ps,
                          const uint64_t* __restrict__ first, const fourmc_block* __restrict__ desc, fourmc_image_status* __restrict__ status)
{
    const uint32_t i = blockIdx.x;
    const fourmc_image_item it = items[i];
    const fourmc_image_parse s = ps[i];
    if (dst_small(s, it)) {
        if (threadIdx.x) return;
        fourmc_image_status r = {};
        r.total_bytes = s.total; r.streams = s.streams;
        r.reason = FOURMC_IMG_DST_SMALL; r.exit_code = fourmc_image_exit_code(FOURMC_IMG_DST_SMALL);
        status[i] = r;
        return;
    }
    reduce_verdict(desc + first[i], uint32_t(s.nblocks), ps + i, status + i, it.image_off);
}

// ------------------------------------------------------------------------------------------------------------- random access
// The footer index and the block-range / byte-range reads.  Every check is fourmc_file.c's read_index and the per-block loop of
// fourmc_file_decode_blocks, in their order; the offsets are its 64-bit prefix sums of the footer's deltas.
constexpr uint32_t kSlot = FOURMC_BLOCKSIZE;            // staging slot per partly covered block

// 64-bit inclusive prefix of u32 values: their two 16-bit halves through scan_add (64 x 0xffff cannot overflow a lane)
__device__ __forceinline__ uint64_t scan_add64(uint32_t v)
{ return uint64_t(scan_add(v & 0xffffu)) + (uint64_t(scan_add(v >> 16)) << 16); }
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int l)
{
    return (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v >> 32)), l))) << 32) |
           uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), l));
}
__device__ __forceinline__ uint64_t up_u64(uint64_t v)  // lane l gets lane l-1's value (lane 0 its own)
{ return uint64_t(__shfl_up((unsigned long long)v, 1)); }

// read_index on every lane (the same addresses: one request): n, or -1 / -2; *F: the footer's offset, *fsz: the tail's size field
__device__ int64_t index_header(const uint8_t* img, uint64_t N, uint32_t* magic, uint64_t* F, uint64_t* fsz)
{
    if (N < 12) return -1;
    const uint32_t m = be32(img);
    if (m != FOURMC_MAGIC_4MC && m != FOURMC_MAGIC_4MZ) return -2;
    if (be32(img + 4) != 1 || be32(img + 8) != xxh32_lane(img, 8, 0)) return -2;
    const uint64_t fs = be32(img + N - 12);
    if (fs < 20 || fs + 24 > N) return -2;
    const uint8_t* foot = img + N - fs;                  // fourmc_frame_parse_footer(foot, fs): its size field may be below fs
    const uint32_t size = be32(foot);
    if (size < 20 || size > fs || ((size - 20) & 3)) return -2;
    if (be32(foot + size - 4) != xxh32_lane(foot, size - 4, 0)) return -2;
    if (be32(foot + 4) != 1) return -2;
    if (be32(foot + size - 12) != size || be32(foot + size - 8) != m) return -2;
    *magic = m; *F = N - fs; *fsz = fs;
    return (size - 20) / 4;
}

// The index, one wave, 64 blocks per step: offsets and data offsets by scan, each block's header where the footer puts it, and the
// verdict of fourmc_file_decode_blocks(0, n) with unlimited capacity - the first block, in order, that fails a check.
__device__ __forceinline__ void image_index_body(const uint8_t* __restrict__ img, uint64_t N, fourmc_image_index_dev* __restrict__ idx,
                                                 fourmc_image_entry* __restrict__ ent, uint64_t cap)
{
    const int lane = threadIdx.x;
    uint32_t magic = 0;
    uint64_t F = 0, fsz = 0;
    const int64_t n = index_header(img, N, &magic, &F, &fsz);
    if (n < 0) {
        if (lane == 0) { idx->info.nblocks = n; idx->info.framing = n; idx->info.total_bytes = 0; idx->info.is_zstd = 0; idx->info.pad = 0; idx->data_end = 0; }
        return;
    }
    const uint32_t k = uint32_t(n);
    const uint64_t end = N - fsz - 12;                   // the end of the last block: where the end mark starts
    int64_t framing = 0;
    if (k && !(uint64_t(be32(img + F + 8)) < end)) framing = -1;          // lo < hi, else nothing is read
    uint64_t carry = 0, ucarry = 0, prev_off = 0;
    uint32_t prev_csize = 0, prev_read = 0;
    for (uint32_t i0 = 0; i0 < k; i0 += 64) {
        const uint32_t i = i0 + uint32_t(lane);
        const bool have = i < k;
        const uint32_t delta = have ? be32(img + F + 8 + 4ull * i) : 0u;
        const uint64_t incl = scan_add64(delta);
        const uint64_t off = carry + incl;
        const bool readable = have && off + 12 <= N;
        uint32_t usize = 0, csize = 0, sum = 0;
        if (readable) { usize = be32(img + off); csize = be32(img + off + 4); sum = be32(img + off + 8); }
        uint64_t poff = up_u64(off);
        uint32_t pcs = uint32_t(__shfl_up(int(csize), 1)), prd = uint32_t(__shfl_up(int(readable), 1));
        if (lane == 0) { poff = prev_off; pcs = prev_csize; prd = prev_read; }
        const bool chain = i == 0 || (prd && off == poff + 12 + pcs);   // the index and the block headers agree
        int32_t code = 0;
        if (!chain || off + 12 > end) code = -2;
        else if (csize > kBlock || usize > kBlock || off + 12 + csize > end) code = -4;
        const uint64_t uincl = scan_add64(usize);
        if (ent && have && i < cap) {
            fourmc_image_entry e;
            e.image_off = off; e.data_off = ucarry + uincl - usize; e.usize = usize; e.csize = csize; e.xxh32 = sum; e.pad = 0;
            ent[i] = e;
        }
        const unsigned long long bad = __ballot(have && code != 0);
        if (bad && framing == 0) framing = __shfl(code, int(__builtin_ctzll(bad)));
        carry += lane_u64(incl, 63); ucarry += lane_u64(uincl, 63);
        prev_off = lane_u64(off, 63);
        prev_csize = uint32_t(__builtin_amdgcn_readlane(int(csize), 63));
        prev_read = uint32_t(__builtin_amdgcn_readlane(int(readable), 63));
    }
    if (lane == 0) {
        idx->info.nblocks = n; idx->info.framing = framing; idx->info.total_bytes = ucarry;
        idx->info.is_zstd = magic == FOURMC_MAGIC_4MZ; idx->info.pad = 0;
        idx->data_end = end;
    }
}

__global__ __launch_bounds__(64)
void image_index_kernel(const uint8_t* __restrict__ img, uint64_t N, fourmc_image_index_dev* __restrict__ idx,
                        fourmc_image_entry* __restrict__ ent, uint64_t cap)
{ image_index_body(img, N, idx, ent, cap); }

// The index of many images (fourmc_gpu_images_read_lines / _images_align_slices): blockIdx.x's wave is the kernel above on image
// blockIdx.x, its summary to idx[blockIdx.x] and - when entries are asked for - its first tab[].cap entries from ent[tab[].ent0]
// on, image-relative as fourmc_gpu_image_index writes them.  cap 0: the summary only (an image nobody asks, or one that cannot
// be indexed).
__global__ __launch_bounds__(64)
void images_index_kernel(const uint8_t* __restrict__ base, const fourmc_images_tab* __restrict__ tab,
                         fourmc_image_index_dev* __restrict__ idx, fourmc_image_entry* __restrict__ ent)
{
    const fourmc_images_tab t = tab[blockIdx.x];
    image_index_body(base + t.image_off, t.image_bytes, idx + blockIdx.x, ent ? ent + t.ent0 : nullptr, ent ? uint64_t(t.cap) : 0);
}

// fourmc_file_decode_blocks(first, count, dst_cap) after read_index, one wave: lo / hi, then its loop's checks (-2 index and
// headers disagree, -4 sizes, -5 capacity) per block, the first failure in order deciding.  Then the descriptors, block i at
// data_off[i] - data_off[first]; all-zero descriptors (nothing read, nothing written) when a check failed.
__global__ __launch_bounds__(64)
void image_span_kernel(const fourmc_image_entry* __restrict__ ent, const fourmc_image_index_dev* __restrict__ idx, uint64_t N,
                       uint32_t first, uint32_t count, uint64_t dst_cap, fourmc_image_span* __restrict__ span,
                       fourmc_block* __restrict__ desc)
{
    const int lane = threadIdx.x;
    const uint64_t n = uint64_t(idx->info.nblocks);
    const uint64_t lo = ent[first].image_off;
    const uint64_t hi = uint64_t(first) + count < n ? ent[first + count].image_off : idx->data_end;
    const uint64_t d0 = ent[first].data_off;
    int64_t code = (lo < hi && hi <= N) ? 0 : -1;
    for (uint32_t b0 = 0; b0 < count && code == 0; b0 += 64) {
        const uint32_t b = b0 + uint32_t(lane);
        int32_t c = 0;
        if (b < count) {
            const fourmc_image_entry e = ent[first + b];
            bool chain = true;
            if (b) {
                const fourmc_image_entry p = ent[first + b - 1];
                chain = p.image_off + 12 <= N && e.image_off == p.image_off + 12 + p.csize;
            }
            if (!chain || e.image_off + 12 > hi) c = -2;
            else if (e.csize > kBlock || e.usize > kBlock || e.image_off + 12 + e.csize > hi) c = -4;
            else if (e.data_off - d0 + e.usize > dst_cap) c = -5;
        }
        const unsigned long long bad = __ballot(c != 0);
        if (bad) code = __shfl(c, int(__builtin_ctzll(bad)));
    }
    for (uint32_t b0 = 0; b0 < count; b0 += 64) {
        const uint32_t b = b0 + uint32_t(lane);
        if (b >= count) break;
        fourmc_block d = {};
        if (code == 0) {
            const fourmc_image_entry e = ent[first + b];
            d.src_off = e.image_off + 12; d.dst_off = e.data_off - d0; d.src_len = e.csize; d.dst_cap = e.usize; d.xxh32 = e.xxh32;
        }
        desc[b] = d;
    }
    if (lane == 0) {
        const uint64_t last = uint64_t(first) + count - 1;
        span->framing = code;
        span->out = code == 0 ? ent[last].data_off + ent[last].usize - d0 : 0;
    }
}

// the file function's ending: its framing code, else -4 for any block whose result is not its usize, else the bytes
__global__ __launch_bounds__(64)
void image_span_reduce_kernel(const fourmc_block* __restrict__ desc, uint32_t count, const fourmc_image_span* __restrict__ span,
                              int64_t* __restrict__ result)
{
    const int lane = threadIdx.x;
    int64_t r = span->framing;
    if (r == 0) {
        bool bad = false;
        for (uint32_t b = uint32_t(lane); b < count; b += 64) {
            const fourmc_block d = desc[b];
            bad |= d.result < 0 || uint32_t(d.result) != d.dst_cap;
        }
        r = __ballot(bad) ? -4 : int64_t(span->out);
    }
    if (lane == 0) *result = r;
}

// first block whose data ends beyond `pos` (data_off + usize is non-decreasing); n if none
__device__ uint32_t block_after(const fourmc_image_entry* ent, uint32_t n, uint64_t pos)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ent[mid].data_off + ent[mid].usize > pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ __forceinline__ bool partial(const fourmc_image_entry& e, uint64_t a, uint64_t z)
{ return e.data_off < a || e.data_off + e.usize > z; }

// One lane per range (the image's framing is 0 here): the early results, the covering blocks [b0, b1], how many of them lie wholly
// inside (decoded straight into the destination), and a flag on each partly covered one (decoded once into staging).  Result
// `length` marks a range still to be read.
__global__ __launch_bounds__(256)
void image_plan_kernel(const fourmc_image_entry* __restrict__ ent, uint32_t n, const fourmc_image_index_dev* __restrict__ idx,
                       fourmc_image_range* __restrict__ ranges, uint32_t nranges, uint64_t dst_cap, fourmc_image_rplan* __restrict__ rp,
                       uint32_t* __restrict__ flags, fourmc_image_plan* __restrict__ plan)
{
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nranges) return;
    const fourmc_image_range q = ranges[r];
    fourmc_image_rplan p = {};
    const uint64_t total = idx->info.total_bytes;
    int64_t res = int64_t(q.length);
    if (q.length == 0) res = 0;
    else if (q.offset > total || q.length > total - q.offset) res = -3;
    else if (q.dst_off > dst_cap || q.length > dst_cap - q.dst_off) res = -5;
    if (res > 0) {
        const uint64_t a = q.offset, z = q.offset + q.length;
        p.b0 = block_after(ent, n, a);
        p.b1 = block_after(ent, n, z - 1);
        const bool s0 = partial(ent[p.b0], a, z), s1 = p.b1 != p.b0 && partial(ent[p.b1], a, z);
        p.nd = p.b1 - p.b0 + 1 - s0 - s1;
        uint32_t piece = 0;
        if (s0) { flags[p.b0] = 1; const fourmc_image_entry e = ent[p.b0]; piece = uint32_t(min(z, e.data_off + e.usize) - max(a, e.data_off)); }
        if (s1) { flags[p.b1] = 1; const fourmc_image_entry e = ent[p.b1]; piece = max(piece, uint32_t(z - e.data_off)); }
        if (piece) atomicMax(&plan->max_piece, piece);
    }
    ranges[r].result = res;
    rp[r] = p;
}

// Two exclusive scans in one workgroup each: block 0 the direct counts of the ranges into their first descriptor, block 1 the staging
// flags into slot numbers (in place).  Each thread sums a contiguous run; a wave scan plus the 16 wave totals in LDS order them.
template <class Get, class Put>
__device__ uint64_t block_scan(uint32_t m, Get get, Put put)
{
    __shared__ uint64_t wsum[16];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t per = uint32_t((uint64_t(m) + 1023) / 1024), a = min(m, t * per), z = uint32_t(min(uint64_t(m), uint64_t(a) + per));
    uint64_t mine = 0;
    for (uint32_t i = a; i < z; i++) mine += get(i);
    uint64_t incl = mine;                                  // 64-bit wave scan: the counts of one thread may exceed 32 bits
    for (int o = 1; o < 64; o <<= 1) { const uint64_t v = uint64_t(__shfl_up((unsigned long long)incl, o)); if (int(lane) >= o) incl += v; }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint64_t base = 0, total = 0;
    for (uint32_t j = 0; j < 16; j++) { if (j < w) base += wsum[j]; total += wsum[j]; }
    uint64_t run = base + incl - mine;
    for (uint32_t i = a; i < z; i++) { const uint64_t v = get(i); put(i, run); run += v; }
    return total;
}
__global__ __launch_bounds__(1024)
void image_plan_scan_kernel(fourmc_image_rplan* __restrict__ rp, uint32_t nranges, uint32_t* __restrict__ flags, uint32_t n,
                            fourmc_image_plan* __restrict__ plan)
{
    if (blockIdx.x == 0) {
        const uint64_t t = block_scan(nranges, [&](uint32_t i) { return uint64_t(rp[i].nd); }, [&](uint32_t i, uint64_t v) { rp[i].dbase = v; });
        if (threadIdx.x == 0) plan->ndirect = t;
    } else {
        const uint64_t t = block_scan(n, [&](uint32_t i) { return uint64_t(flags[i]); }, [&](uint32_t i, uint64_t v) { flags[i] = uint32_t(v); });
        if (threadIdx.x == 0) plan->nstaged = uint32_t(t);
    }
}

// Descriptors.  Blocks [0, nranges): one wave per range writes its direct descriptors.  Blocks from nranges on: one lane per image
// block writes the staged descriptor of each flagged block (the slots are the scanned flags: a block is flagged iff the next slot
// number differs).
__global__ __launch_bounds__(64)
void image_read_desc_kernel(const fourmc_image_entry* __restrict__ ent, uint32_t n, const fourmc_image_range* __restrict__ ranges,
                            uint32_t nranges, const fourmc_image_rplan* __restrict__ rp, const uint32_t* __restrict__ slot,
                            uint32_t nstaged, uint64_t ndirect, uint64_t dst_delta, uint64_t stage_delta, fourmc_block* __restrict__ desc)
{
    const uint32_t lane = threadIdx.x;
    if (blockIdx.x < nranges) {
        const uint32_t r = blockIdx.x;
        const fourmc_image_range q = ranges[r];
        if (q.result <= 0) return;
        const fourmc_image_rplan p = rp[r];
        const uint64_t a = q.offset, z = q.offset + q.length;
        const uint32_t s0 = partial(ent[p.b0], a, z) ? 1u : 0u;
        for (uint32_t j = lane; j < p.nd; j += 64) {
            const fourmc_image_entry e = ent[p.b0 + s0 + j];
            fourmc_block d;
            d.src_off = e.image_off + 12; d.dst_off = dst_delta + q.dst_off + (e.data_off - a);
            d.src_len = e.csize; d.dst_cap = e.usize; d.result = 0; d.xxh32 = e.xxh32;
            desc[p.dbase + j] = d;
        }
        return;
    }
    const uint32_t b = (blockIdx.x - nranges) * 64 + lane;
    if (b >= n) return;
    const uint32_t s = slot[b], next = b + 1 < n ? slot[b + 1] : nstaged;
    if (next == s) return;
    const fourmc_image_entry e = ent[b];
    fourmc_block d;
    d.src_off = e.image_off + 12; d.dst_off = stage_delta + uint64_t(s) * kSlot;
    d.src_len = e.csize; d.dst_cap = e.usize; d.result = 0; d.xxh32 = e.xxh32;
    desc[ndirect + s] = d;
}

// The covered bytes of each (range, staged block) piece from its slot to the destination: one wave per 64 KiB chunk of a piece;
// blockIdx.x = 2 * range + (0: the first covering block, 1: the last), blockIdx.y = chunk.
constexpr uint32_t kChunk = 64 * 1024;
__global__ __launch_bounds__(64)
void image_read_copy_kernel(const fourmc_image_entry* __restrict__ ent, const fourmc_image_range* __restrict__ ranges,
                            const fourmc_image_rplan* __restrict__ rp, const uint32_t* __restrict__ slot,
                            const uint8_t* __restrict__ stage, uint8_t* __restrict__ dst)
{
    const uint32_t r = blockIdx.x >> 1, which = blockIdx.x & 1;
    const fourmc_image_range q = ranges[r];
    if (q.result <= 0) return;
    const fourmc_image_rplan p = rp[r];
    const uint64_t a = q.offset, z = q.offset + q.length;
    const uint32_t b = which ? p.b1 : p.b0;
    if (which && p.b1 == p.b0) return;
    const fourmc_image_entry e = ent[b];
    if (!partial(e, a, z)) return;
    const uint64_t from = max(a, e.data_off), to = min(z, e.data_off + e.usize);
    const uint64_t c0 = from + uint64_t(blockIdx.y) * kChunk;
    if (c0 >= to) return;
    const int len = int(min(to - c0, uint64_t(kChunk)));
    wave_copy(dst + q.dst_off + (c0 - a), stage + uint64_t(slot[b]) * kSlot + (c0 - e.data_off), len, int(threadIdx.x));
}

// Per range, one wave: -4 when any covering block's result is not its usize
__global__ __launch_bounds__(64)
void image_read_reduce_kernel(const fourmc_image_entry* __restrict__ ent, fourmc_image_range* __restrict__ ranges,
                              const fourmc_image_rplan* __restrict__ rp, const uint32_t* __restrict__ slot,
                              const fourmc_block* __restrict__ desc, uint64_t ndirect)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    const fourmc_image_range q = ranges[r];
    if (q.result <= 0) return;
    const fourmc_image_rplan p = rp[r];
    const uint64_t a = q.offset, z = q.offset + q.length;
    auto bad = [](const fourmc_block& d) { return d.result < 0 || uint32_t(d.result) != d.dst_cap; };
    bool b = false;
    for (uint32_t j = lane; j < p.nd; j += 64) b |= bad(desc[p.dbase + j]);
    if (lane == 0 && partial(ent[p.b0], a, z)) b |= bad(desc[ndirect + slot[p.b0]]);
    if (lane == 1 && p.b1 != p.b0 && partial(ent[p.b1], a, z)) b |= bad(desc[ndirect + slot[p.b1]]);
    if (__ballot(b) && lane == 0) ranges[r].result = -4;
}

// ------------------------------------------------------------------------------------------------------------- streaming reads
// The reader's walk is the whole-image walk restated so that it stops at the end of the appended bytes and carries on at the next
// append: its state (fourmc_image_rd_state) lives in device memory, a unit in progress (a header, a payload, a footer) is carried
// by what it has received so far, and every check is decided as soon as the bytes it reads are there.  A check that needs bytes
// not yet appended waits: the finish kernel decides it with N = everything appended.  Payload bytes go from the chunk straight
// into the block's staging slot (assigned when its header completes), so a block cut by the end of a chunk waits in its own slot.
enum : uint32_t { RD_FHDR = 0, RD_BHDR = 1, RD_PAY = 2, RD_BADPAY = 3, RD_FSIZE = 4, RD_FBODY = 5 };
constexpr uint32_t kNoSlot = ~0u;
constexpr uint64_t kRdSlot = FOURMC_BLOCKSIZE;           // staging slot stride of the reader

__device__ __forceinline__ uint32_t avalanche(uint32_t h)
{ h ^= h >> 15; h *= P2; h ^= h >> 13; h *= P3; h ^= h >> 16; return h; }
__device__ __forceinline__ void xxh_round4(uint32_t* v, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    v[0] = rotl(v[0] + a * P2, 13) * P1; v[1] = rotl(v[1] + b * P2, 13) * P1;
    v[2] = rotl(v[2] + c * P2, 13) * P1; v[3] = rotl(v[3] + d * P2, 13) * P1;
}
// 16 bytes held as two little-endian words: byte k at bits 8 (k % 8) of word k / 8
__device__ __forceinline__ void put_byte(uint64_t* w, uint32_t k, uint8_t b) { w[k >> 3] |= uint64_t(b) << (8 * (k & 7)); }
__device__ __forceinline__ uint32_t word_le32(const uint64_t* w, uint32_t k)   // k = 0, 4, 8, 12
{ return uint32_t(w[k >> 3] >> (8 * (k & 7))); }
__device__ __forceinline__ uint32_t word_be32(const uint64_t* w, uint32_t k) { return __builtin_bswap32(word_le32(w, k)); }

// streaming XXH32 (seed 0): xxh32_lane's result for the concatenation of every update
__device__ __forceinline__ void xs_reset(fourmc_image_rd_state& S)
{
    S.xv[0] = P1 + P2; S.xv[1] = P2; S.xv[2] = 0; S.xv[3] = 0u - P1;
    S.xlen = 0; S.xbn = 0; S.xbuf[0] = S.xbuf[1] = 0;
}
__device__ void xs_update(fourmc_image_rd_state& S, const uint8_t* p, uint64_t n)
{
    S.xlen += n;
    while (S.xbn && n) {
        put_byte(S.xbuf, S.xbn, *p++); n--;
        if (++S.xbn == 16) {
            xxh_round4(S.xv, word_le32(S.xbuf, 0), word_le32(S.xbuf, 4), word_le32(S.xbuf, 8), word_le32(S.xbuf, 12));
            S.xbn = 0; S.xbuf[0] = S.xbuf[1] = 0;
        }
    }
    for (; n >= 16; n -= 16, p += 16) xxh_round4(S.xv, le32(p), le32(p + 4), le32(p + 8), le32(p + 12));
    for (; n; n--) put_byte(S.xbuf, S.xbn++, *p++);
}
__device__ uint32_t xs_digest(const fourmc_image_rd_state& S)
{
    uint32_t h = S.xlen >= 16 ? rotl(S.xv[0], 1) + rotl(S.xv[1], 7) + rotl(S.xv[2], 12) + rotl(S.xv[3], 18) : P5;
    h += uint32_t(S.xlen);
    uint32_t k = 0;
    for (; k + 4 <= S.xbn; k += 4) h = rotl(h + word_le32(S.xbuf, k) * P3, 17) * P4;
    for (; k < S.xbn; k++) h = rotl(h + uint32_t(uint8_t(S.xbuf[k >> 3] >> (8 * (k & 7)))) * P5, 11) * P1;
    return avalanche(h);
}

__device__ __forceinline__ void rd_enter(fourmc_image_rd_state& S, uint32_t phase)
{ S.phase = phase; S.at = S.pos; S.have = 0; S.part[0] = S.part[1] = 0; S.got = 0; }
__device__ __forceinline__ void rd_final(fourmc_image_rd_state& S, int32_t reason) { S.final_ = 1; S.reason = reason; }

// One lane.  Consumes chunk[i, L) until the chunk ends, the batch is full or the verdict is final; the chunk is read only inside
// [c, c + L).  A block whose payload is complete gets its descriptor in its slot; its payload bytes in this chunk become a copy piece.
__global__ __launch_bounds__(64)
void image_rd_walk_kernel(const uint8_t* __restrict__ c, uint64_t L, uint64_t i, fourmc_image_rd_state* __restrict__ st,
                          uint32_t magic, uint64_t dst_cap, uint32_t batch, uint8_t* __restrict__ stage,
                          fourmc_block* __restrict__ desc, uint64_t* __restrict__ at_out, fourmc_image_piece* __restrict__ pc)
{
    if (threadIdx.x != 0) return;
    fourmc_image_rd_state S = *st;
    uint32_t np = 0;
    uint64_t maxp = 0;
    while (!S.final_ && S.batch_n < batch) {
        // a payload with all its bytes completes without another one (an empty payload right after its header)
        if ((S.phase == RD_PAY || S.phase == RD_BADPAY) && S.got == S.csize) {
            if (S.phase == RD_BADPAY) { rd_final(S, usize_verdict(xs_digest(S), S.sum)); break; }
            if (S.slot != kNoSlot) {
                fourmc_block d;
                d.src_off = uint64_t(S.slot) * kRdSlot; d.dst_off = S.total; d.src_len = S.csize; d.dst_cap = S.usize;
                d.result = 0; d.xxh32 = S.sum;
                desc[S.slot] = d;
                at_out[S.slot] = S.at;
                S.batch_n++;
            }
            S.nblocks++; S.total += S.usize;
            rd_enter(S, RD_BHDR);
            continue;
        }
        if (i == L) break;
        const uint64_t left = L - i;
        if (S.phase == RD_FHDR || S.phase == RD_BHDR || S.phase == RD_FSIZE) {
            const uint32_t want = S.phase == RD_FSIZE ? 4u : 12u;
            while (S.have < want && i < L) { put_byte(S.part, S.have++, c[i++]); S.pos++; }
            if (S.phase == RD_FHDR) {
                if (S.have >= 4 && word_be32(S.part, 0) != magic) { rd_final(S, FOURMC_IMG_NOT_4MC); break; }
                if (S.have < 12) continue;
                const uint32_t w0 = word_le32(S.part, 0), w1 = word_le32(S.part, 4);      // XXH32 of the first 8 bytes
                const uint32_t hsum = avalanche(rotl(rotl(P5 + 8 + w0 * P3, 17) * P4 + w1 * P3, 17) * P4);
                if (const int32_t r = file_header_verdict(word_be32(S.part, 4), word_be32(S.part, 8), hsum)) { rd_final(S, r); break; }
                S.streams++; S.stream_total0 = S.total;
                rd_enter(S, RD_BHDR);
            } else if (S.phase == RD_BHDR) {
                if (S.have < 12) continue;
                const uint32_t usize = word_be32(S.part, 0), csize = word_be32(S.part, 4), sum = word_be32(S.part, 8);
                if (end_mark(usize, csize, sum)) { rd_enter(S, RD_FSIZE); continue; }
                if (csize_beyond(csize)) { rd_final(S, FOURMC_IMG_CSIZE_BEYOND); break; }
                S.usize = usize; S.csize = csize; S.sum = sum; S.got = 0;
                if (usize_beyond(usize, csize)) { S.phase = RD_BADPAY; xs_reset(S); continue; }
                S.phase = RD_PAY;
                S.slot = usize <= dst_cap && S.total <= dst_cap - usize ? S.batch_n : kNoSlot;   // else DST_SMALL decides
            } else {
                if (S.have < 4) continue;
                S.fsz = word_be32(S.part, 0);
                if (S.fsz < 8) { rd_final(S, FOURMC_IMG_FOOTER_SHORT); break; }
                xs_reset(S);
                S.xbuf[0] = uint32_t(S.part[0]); S.xbn = 4; S.xlen = 4;                  // the size field opens the hashed bytes
                S.phase = RD_FBODY; S.got = 4;
            }
            continue;
        }
        if (S.phase == RD_PAY || S.phase == RD_BADPAY) {
            const uint64_t take = min(uint64_t(S.csize) - S.got, left);
            if (S.phase == RD_BADPAY) xs_update(S, c + i, take);
            else if (S.slot != kNoSlot) {
                fourmc_image_piece q;
                q.src = uint64_t(uintptr_t(c + i)); q.dst = uint64_t(uintptr_t(stage + uint64_t(S.slot) * kRdSlot + S.got));
                q.len = take; q.pad = 0;
                pc[np++] = q;
                maxp = max(maxp, take);
            }
            S.got += take; i += take; S.pos += take;
            continue;
        }
        // RD_FBODY: footer bytes [got, fsz): XXH32 over [0, fsz - 4), the version at [4, 8), the checksum at [fsz - 4, fsz)
        const uint64_t fsz = S.fsz, a = S.got, take = min(fsz - a, left), z = a + take;
        const uint64_t hz = min(z, fsz - 4);
        if (a < hz) xs_update(S, c + i, hz - a);
        for (uint64_t q = max(a, uint64_t(4)); q < min(z, uint64_t(8)); q++) put_byte(S.part, uint32_t(q), c[i + (q - a)]);
        for (uint64_t q = max(a, fsz - 4); q < z; q++) put_byte(S.part, uint32_t(8 + q - (fsz - 4)), c[i + (q - a)]);
        S.got = z; i += take; S.pos += take;
        if (S.got < fsz) continue;
        if (const int32_t r = footer_verdict(xs_digest(S), word_be32(S.part, 8), word_be32(S.part, 4))) { rd_final(S, r); break; }
        if (S.total == S.stream_total0) { rd_final(S, FOURMC_IMG_OK); break; }     // an empty stream ends the file
        rd_enter(S, RD_FHDR);
    }
    S.cpos = i; S.npieces = np; S.max_piece = uint32_t(maxp);
    *st = S;
}

// The copy pieces of one walk: one wave per 64 KiB of a piece; blockIdx.x = piece, blockIdx.y = its 64 KiB step
__global__ __launch_bounds__(64)
void image_rd_gather_kernel(const fourmc_image_piece* __restrict__ pc)
{
    const fourmc_image_piece q = pc[blockIdx.x];
    const uint64_t c0 = uint64_t(blockIdx.y) * kChunk;
    if (c0 >= q.len) return;
    wave_copy(reinterpret_cast<uint8_t*>(uintptr_t(q.dst)) + c0, reinterpret_cast<const uint8_t*>(uintptr_t(q.src)) + c0,
              int(min(q.len - c0, uint64_t(kChunk))), int(threadIdx.x));
}

// image_reduce's rule across batches: the first failing block (in file order) and the decoded bytes before it; the batch empties
__global__ __launch_bounds__(64)
void image_rd_fold_kernel(const fourmc_block* __restrict__ desc, const uint64_t* __restrict__ at, uint32_t n,
                          fourmc_image_rd_state* __restrict__ st)
{
    const uint64_t base = st->decoded;
    if (st->first_reason == 0) {
        uint64_t done = 0;
        const uint32_t first = first_failing(desc, n, &done);
        if (threadIdx.x == 0) {
            st->done += done;
            if (first < n) { st->first = uint32_t(base + first); st->first_at = at[first]; st->first_reason = block_reason(desc[first].result); }
        }
    }
    if (threadIdx.x == 0) { st->decoded = base + n; st->batch_n = 0; }
}

// The checks that waited for bytes, decided with N; then the status image_decompress writes for the same bytes
__global__ __launch_bounds__(64)
void image_rd_finish_kernel(const fourmc_image_rd_state* __restrict__ st, uint64_t N, uint64_t dst_cap, fourmc_image_status* __restrict__ out)
{
    if (threadIdx.x != 0) return;
    const fourmc_image_rd_state S = *st;
    int32_t reason = S.reason;
    if (!S.final_) {
        switch (S.phase) {
            case RD_FHDR:   reason = S.have == 0 ? FOURMC_IMG_OK : S.have < 4 ? FOURMC_IMG_MAGIC_UNREADABLE : FOURMC_IMG_HEADER_UNREADABLE; break;
            case RD_BHDR:   reason = FOURMC_IMG_BLOCK_SIZE_UNREADABLE; break;
            case RD_FSIZE:  reason = FOURMC_IMG_FOOTER_UNREADABLE; break;
            case RD_FBODY:  reason = FOURMC_IMG_FOOTER_SHORT; break;
            default:        reason = FOURMC_IMG_DATA_UNREADABLE; break;
        }
    }
    fourmc_image_status r = {};
    r.total_bytes = S.total; r.streams = S.streams;
    if (S.total > dst_cap) {
        r.reason = FOURMC_IMG_DST_SMALL; r.exit_code = fourmc_image_exit_code(FOURMC_IMG_DST_SMALL);
    } else if (S.first_reason) {
        r.decoded_bytes = S.done; r.blocks = S.first; r.reason = S.first_reason; r.exit_code = 4; r.fail_offset = S.first_at;
    } else {
        r.decoded_bytes = S.done; r.blocks = uint32_t(S.nblocks); r.reason = reason; r.exit_code = fourmc_image_exit_code(reason);
        r.fail_offset = reason == FOURMC_IMG_OK ? N : S.at;
    }
    *out = r;
}

} // namespace

extern "C" {

hipError_t fourmc_launch_image_enc_desc(fourmc_block* d_blocks, uint64_t src_bytes, uint32_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(image_enc_desc_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_blocks, src_bytes, n);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_enc_frame(void* d_image, fourmc_block* d_blocks, uint64_t* d_off, uint32_t n, uint32_t magic,
                                         const void* d_staging, fourmc_image_enc_summary* d_sum, hipStream_t s)
{
    hipLaunchKernelGGL(image_enc_scan_kernel<false>, dim3(1), dim3(64), 0, s, d_blocks, d_off, n, d_sum);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = fourmc_launch_pack_image(d_staging, d_image, d_blocks, d_off, n, s)) return e;
    hipLaunchKernelGGL(image_enc_tail_kernel, dim3(1), dim3(256), 0, s, static_cast<uint8_t*>(d_image), d_off, n, magic);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_wr_desc(fourmc_block* d_blocks, uint64_t src0, uint64_t dst0, uint64_t src_bytes, uint32_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(image_wr_desc_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_blocks, src0, dst0, src_bytes, n);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_wr_batch(void* d_image, fourmc_block* d_blocks, uint64_t* d_off, uint32_t n, const void* d_staging,
                                        fourmc_image_enc_summary* d_sum, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(image_enc_scan_kernel<true>, dim3(1), dim3(64), 0, s, d_blocks, d_off, n, d_sum);
    if (hipError_t e = hipGetLastError()) return e;
    return fourmc_launch_pack_image(d_staging, d_image, d_blocks, d_off, n, s);
}

hipError_t fourmc_launch_image_wr_tail(void* d_image, const uint64_t* d_off, uint32_t n, uint32_t magic, hipStream_t s)
{
    hipLaunchKernelGGL(image_enc_tail_kernel, dim3(1), dim3(256), 0, s, static_cast<uint8_t*>(d_image), d_off, n, magic);
    return hipGetLastError();
}

hipError_t fourmc_launch_images_enc_desc(const fourmc_image_enc_plan* d_plans, uint32_t n, fourmc_block* d_blocks, uint32_t nblocks,
                                         hipStream_t s)
{
    if (n == 0 || nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(images_enc_desc_kernel, dim3(n), dim3(64), 0, s, d_plans, d_blocks);
    return hipGetLastError();
}

hipError_t fourmc_launch_images_enc_frame(void* d_images, const fourmc_image_enc_plan* d_plans, uint32_t n, fourmc_block* d_blocks,
                                          uint32_t nblocks, uint64_t* d_off, uint64_t* d_end, uint32_t magic, const void* d_staging,
                                          fourmc_image_enc_result* d_res, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(images_enc_scan_kernel, dim3(n), dim3(64), 0, s, d_plans, d_blocks, d_off, d_end, d_res);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = fourmc_launch_pack_image(d_staging, d_images, d_blocks, d_off, nblocks, s)) return e;
    hipLaunchKernelGGL(images_enc_tail_kernel, dim3(n), dim3(256), 0, s, static_cast<uint8_t*>(d_images), d_plans, d_off, d_end, magic);
    return hipGetLastError();
}

hipError_t fourmc_launch_imgw_seal(const fourmc_block* d_blocks, const fourmc_bsw_side* d_side, uint32_t m, int zstd,
                                   const fourmc_bstream_enc_item* d_items, uint64_t src_delta, uint64_t stage_delta,
                                   fourmc_block* d_seal, uint64_t* d_idx, fourmc_imgw_run* d_run, uint64_t* d_bad, hipStream_t s)
{
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(imgw_seal_kernel, dim3(1), dim3(64), 0, s, d_blocks, d_side, m, zstd, d_items, src_delta, stage_delta, d_seal,
                       d_idx, d_run, d_bad);
    return hipGetLastError();
}

hipError_t fourmc_launch_imgw_tail(void* d_images, const fourmc_bstream_enc_item* d_items, const fourmc_bsw_plan* d_plans,
                                   const fourmc_bsw_slice* d_slices, const uint64_t* d_idx, const fourmc_imgw_run* d_run, uint32_t n,
                                   uint32_t magic, fourmc_imgw_result* d_res, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(imgw_tail_kernel, dim3(n), dim3(256), 0, s, static_cast<uint8_t*>(d_images), d_items, d_plans, d_slices, d_idx,
                       d_run, magic, d_res);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_parse(const void* d_image, uint64_t image_bytes, uint32_t magic, int fast, int walk,
                                     fourmc_image_parse* d_ps, fourmc_block* d_blocks, hipStream_t s)
{
    const uint8_t* img = static_cast<const uint8_t*>(d_image);
    if (fast) {
        hipLaunchKernelGGL(image_parse_fast_kernel, dim3(1), dim3(64), 0, s, img, image_bytes, magic, d_ps, d_blocks);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (walk) {
        hipLaunchKernelGGL(image_parse_walk_kernel, dim3(1), dim3(64), 0, s, img, image_bytes, magic, d_ps, d_blocks);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t fourmc_launch_image_reduce(const fourmc_block* d_blocks, uint32_t n, const fourmc_image_parse* d_ps,
                                      fourmc_image_status* d_status, hipStream_t s)
{
    hipLaunchKernelGGL(image_reduce_kernel, dim3(1), dim3(64), 0, s, d_blocks, n, d_ps, d_status);
    return hipGetLastError();
}

hipError_t fourmc_launch_images_parse(const void* d_images, const fourmc_image_item* d_items, uint32_t n, uint32_t magic, int fast,
                                      fourmc_image_parse* d_ps, const uint64_t* d_first, fourmc_block* d_desc, hipStream_t s)
{
    hipLaunchKernelGGL(images_parse_kernel, dim3(n), dim3(64), 0, s, static_cast<const uint8_t*>(d_images), d_items, magic, fast, d_ps,
                       d_first, d_desc);
    return hipGetLastError();
}

hipError_t fourmc_launch_images_plan(const fourmc_image_item* d_items, uint32_t n, const fourmc_image_parse* d_ps, int query,
                                     uint64_t* d_first, fourmc_images_summary* d_sum, fourmc_image_status* d_status, hipStream_t s)
{
    hipLaunchKernelGGL(images_plan_kernel, dim3(1), dim3(kPlanThreads), 0, s, d_items, n, d_ps, query, d_first, d_sum, d_status);
    return hipGetLastError();
}

hipError_t fourmc_launch_images_reduce(const fourmc_image_item* d_items, uint32_t n, const fourmc_image_parse* d_ps,
                                       const uint64_t* d_first, const fourmc_block* d_desc, fourmc_image_status* d_status, hipStream_t s)
{
    hipLaunchKernelGGL(images_reduce_kernel, dim3(n), dim3(64), 0, s, d_items, d_ps, d_first, d_desc, d_status);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_index(const void* d_image, uint64_t image_bytes, fourmc_image_index_dev* d_idx,
                                     fourmc_image_entry* d_ent, uint64_t cap, hipStream_t s)
{
    hipLaunchKernelGGL(image_index_kernel, dim3(1), dim3(64), 0, s, static_cast<const uint8_t*>(d_image), image_bytes, d_idx, d_ent, cap);
    return hipGetLastError();
}

hipError_t fourmc_launch_images_index(const void* d_images, const fourmc_images_tab* d_tab, uint32_t nimages,
                                      fourmc_image_index_dev* d_idx, fourmc_image_entry* d_ent, hipStream_t s)
{
    if (!nimages) return hipSuccess;
    hipLaunchKernelGGL(images_index_kernel, dim3(nimages), dim3(64), 0, s, static_cast<const uint8_t*>(d_images), d_tab, d_idx, d_ent);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_span(const fourmc_image_entry* d_ent, const fourmc_image_index_dev* d_idx, uint64_t image_bytes,
                                    uint32_t first, uint32_t count, uint64_t dst_cap, fourmc_image_span* d_span,
                                    fourmc_block* d_desc, hipStream_t s)
{
    hipLaunchKernelGGL(image_span_kernel, dim3(1), dim3(64), 0, s, d_ent, d_idx, image_bytes, first, count, dst_cap, d_span, d_desc);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_span_reduce(const fourmc_block* d_desc, uint32_t count, const fourmc_image_span* d_span,
                                           int64_t* d_result, hipStream_t s)
{
    hipLaunchKernelGGL(image_span_reduce_kernel, dim3(1), dim3(64), 0, s, d_desc, count, d_span, d_result);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_plan(const fourmc_image_entry* d_ent, uint32_t n, const fourmc_image_index_dev* d_idx,
                                    fourmc_image_range* d_ranges, uint32_t nranges, uint64_t dst_cap, fourmc_image_rplan* d_rp,
                                    uint32_t* d_flags, fourmc_image_plan* d_plan, hipStream_t s)
{
    if (nranges) {
        hipLaunchKernelGGL(image_plan_kernel, dim3((nranges + 255) / 256), dim3(256), 0, s, d_ent, n, d_idx, d_ranges, nranges,
                           dst_cap, d_rp, d_flags, d_plan);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(image_plan_scan_kernel, dim3(2), dim3(1024), 0, s, d_rp, nranges, d_flags, n, d_plan);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_read_desc(const fourmc_image_entry* d_ent, uint32_t n, const fourmc_image_range* d_ranges,
                                         uint32_t nranges, const fourmc_image_rplan* d_rp, const uint32_t* d_slot, uint32_t nstaged,
                                         uint64_t ndirect, uint64_t dst_delta, uint64_t stage_delta, fourmc_block* d_desc, hipStream_t s)
{
    const uint32_t grid = nranges + (nstaged ? (n + 63) / 64 : 0);
    if (!grid) return hipSuccess;
    hipLaunchKernelGGL(image_read_desc_kernel, dim3(grid), dim3(64), 0, s, d_ent, n, d_ranges, nranges, d_rp, d_slot, nstaged,
                       ndirect, dst_delta, stage_delta, d_desc);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_read_copy(const fourmc_image_entry* d_ent, const fourmc_image_range* d_ranges, uint32_t nranges,
                                         const fourmc_image_rplan* d_rp, const uint32_t* d_slot, const void* d_stage, void* d_dst,
                                         uint32_t max_piece, hipStream_t s)
{
    if (!nranges || !max_piece) return hipSuccess;
    hipLaunchKernelGGL(image_read_copy_kernel, dim3(2 * nranges, (max_piece + kChunk - 1) / kChunk), dim3(64), 0, s, d_ent, d_ranges,
                       d_rp, d_slot, static_cast<const uint8_t*>(d_stage), static_cast<uint8_t*>(d_dst));
    return hipGetLastError();
}

hipError_t fourmc_launch_image_read_reduce(const fourmc_image_entry* d_ent, fourmc_image_range* d_ranges, uint32_t nranges,
                                           const fourmc_image_rplan* d_rp, const uint32_t* d_slot, const fourmc_block* d_desc,
                                           uint64_t ndirect, hipStream_t s)
{
    if (!nranges) return hipSuccess;
    hipLaunchKernelGGL(image_read_reduce_kernel, dim3(nranges), dim3(64), 0, s, d_ent, d_ranges, d_rp, d_slot, d_desc, ndirect);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_rd_walk(const void* d_chunk, uint64_t bytes, uint64_t start, fourmc_image_rd_state* d_st,
                                       uint32_t magic, uint64_t dst_cap, uint32_t batch, void* d_stage, fourmc_block* d_desc,
                                       uint64_t* d_at, fourmc_image_piece* d_pc, hipStream_t s)
{
    hipLaunchKernelGGL(image_rd_walk_kernel, dim3(1), dim3(64), 0, s, static_cast<const uint8_t*>(d_chunk), bytes, start, d_st, magic,
                       dst_cap, batch, static_cast<uint8_t*>(d_stage), d_desc, d_at, d_pc);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_rd_gather(const fourmc_image_piece* d_pc, uint32_t npieces, uint64_t max_piece, hipStream_t s)
{
    if (!npieces || !max_piece) return hipSuccess;
    hipLaunchKernelGGL(image_rd_gather_kernel, dim3(npieces, uint32_t((max_piece + kChunk - 1) / kChunk)), dim3(64), 0, s, d_pc);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_rd_fold(const fourmc_block* d_desc, const uint64_t* d_at, uint32_t n, fourmc_image_rd_state* d_st,
                                       hipStream_t s)
{
    hipLaunchKernelGGL(image_rd_fold_kernel, dim3(1), dim3(64), 0, s, d_desc, d_at, n, d_st);
    return hipGetLastError();
}

hipError_t fourmc_launch_image_rd_finish(const fourmc_image_rd_state* d_st, uint64_t image_bytes, uint64_t dst_cap,
                                         fourmc_image_status* d_status, hipStream_t s)
{
    hipLaunchKernelGGL(image_rd_finish_kernel, dim3(1), dim3(64), 0, s, d_st, image_bytes, dst_cap, d_status);
    return hipGetLastError();
}

} // extern "C"
