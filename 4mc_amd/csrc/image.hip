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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"

namespace {

constexpr uint32_t P1 = 2654435761u, P2 = 2246822519u, P3 = 3266489917u, P4 = 668265263u, P5 = 374761393u;
constexpr uint32_t kBlock = FOURMC_BLOCKSIZE;

__device__ __forceinline__ uint32_t be32(const uint8_t* p)
{ return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | uint32_t(p[3]); }
__device__ __forceinline__ uint32_t le32(const uint8_t* p)
{ return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24); }
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v)
{ p[0] = uint8_t(v >> 24); p[1] = uint8_t(v >> 16); p[2] = uint8_t(v >> 8); p[3] = uint8_t(v); }
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

// wave64 inclusive prefix sum: 4 row_shr steps scan each row of 16 lanes, row_bcast15 / row_bcast31 carry the row totals
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dpp0(uint32_t v)
{ return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), CTRL, ROWMASK, 0xf, false)); }
__device__ __forceinline__ uint32_t scan_add(uint32_t v)
{
    v += dpp0<0x111, 0xf>(v); v += dpp0<0x112, 0xf>(v); v += dpp0<0x114, 0xf>(v); v += dpp0<0x118, 0xf>(v);
    v += dpp0<0x142, 0xa>(v);
    v += dpp0<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ uint32_t wave_total(uint32_t incl) { return uint32_t(__builtin_amdgcn_readlane(int(incl), 63)); }

// ------------------------------------------------------------------------------------------------------------- encode
__global__ __launch_bounds__(256)
void image_enc_desc_kernel(fourmc_block* __restrict__ blocks, uint64_t src_bytes, uint32_t n)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const uint64_t at = uint64_t(b) * kBlock;
    fourmc_block d;
    d.src_off = at; d.dst_off = at;
    d.src_len = uint32_t(src_bytes - at < kBlock ? src_bytes - at : kBlock);
    d.dst_cap = d.src_len; d.result = 0; d.xxh32 = 0;
    blocks[b] = d;
}

// off[b] = 12 + sum_{j<b} (12 + csize_j), b = 0..n (off[n]: where the end mark goes); one wave, 64 blocks per step with a 64-bit
// carry.  A result outside [1, src_len] cannot come from the container encode; it is counted (the engine fails the call) and
// clamped so that the pack and the footer stay inside the bound the engine checked the capacity against.
__global__ __launch_bounds__(64)
void image_enc_scan_kernel(fourmc_block* __restrict__ blocks, uint64_t* __restrict__ off, uint32_t n, fourmc_image_enc_summary* sum)
{
    const int lane = threadIdx.x;
    uint64_t carry = 12;
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
    if (lane == 0) {
        off[n] = carry;
        sum->image_bytes = carry + 12 + 20 + 4ull * n;
        sum->bad_blocks = bad;
    }
}

// file header at 0, end mark at off[n], footer behind it (framing.c: fourmc_frame_header / fourmc_frame_footer)
__global__ __launch_bounds__(256)
void image_enc_tail_kernel(uint8_t* __restrict__ image, const uint64_t* __restrict__ off, uint32_t n, uint32_t magic)
{
    const uint32_t t = threadIdx.x;
    const uint64_t end = off[n];
    uint8_t* foot = image + end + 12;
    const uint32_t fsz = 20u + 4u * n;
    if (t == 0) {
        put_be32(image, magic); put_be32(image + 4, 1);
        put_be32(foot, fsz); put_be32(foot + 4, 1);
        put_be32(foot + 8 + 4 * n, fsz); put_be32(foot + 12 + 4 * n, magic);
    }
    if (t < 12) image[end + t] = 0;
    for (uint32_t i = t; i < n; i += 256)                 // delta to the previous block; the first one absolute
        put_be32(foot + 8 + 4 * i, uint32_t(i ? off[i] - off[i - 1] : off[0]));
    __threadfence();
    __syncthreads();
    if (t == 0) {
        put_be32(image + 8, xxh32_lane(image, 8, 0));
        put_be32(foot + fsz - 4, xxh32_lane(foot, fsz - 4, 0));
    }
}

// ------------------------------------------------------------------------------------------------------------- decode
// The fast path, one wave.  `blocks` NULL: check only (summary); else write the descriptors of the image it accepted.
__global__ __launch_bounds__(64)
void image_parse_fast_kernel(const uint8_t* __restrict__ img, uint64_t N, uint32_t magic, fourmc_image_parse* ps,
                             fourmc_block* __restrict__ blocks)
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
            d.src_off = at + 12; d.dst_off = ucarry + (uincl - usize);
            d.src_len = csize; d.dst_cap = usize; d.result = 0; d.xxh32 = sum;
            blocks[i] = d;
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

// The walk: decode_stream (fourmc_file.c:473-592) and decompress_file's loop over concatenated streams on one lane, the checks in
// their order.  That loop (`do got = decode_stream(..); while (got)`, fourmc_file.c:606-609, native/4mc.c:908-912) ends after a
// stream that decoded 0 bytes, whatever follows it: the walk ends cleanly after a stream whose blocks add up to 0 usize.  count mode (blocks NULL): nothing to do when the fast path has accepted the image; else the summary.  fill mode:
// the same walk, writing the descriptors of the blocks it counted.
__global__ __launch_bounds__(64)
void image_parse_walk_kernel(const uint8_t* __restrict__ img, uint64_t N, uint32_t magic, fourmc_image_parse* ps,
                             fourmc_block* __restrict__ blocks)
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
        if (be32(img + p + 4) != 1)        { reason = FOURMC_IMG_VERSION; break; }
        if (be32(img + p + 8) != xxh32_lane(img + p, 8, 0)) { reason = FOURMC_IMG_HEADER_CHECKSUM; break; }
        p += 12; streams++;
        const uint64_t stream_total0 = total;
        for (;;) {
            at = p;
            if (N - p < 12)                { reason = FOURMC_IMG_BLOCK_SIZE_UNREADABLE; break; }
            const uint32_t usize = be32(img + p), csize = be32(img + p + 4), sum = be32(img + p + 8);
            p += 12;
            if ((usize | csize | sum) == 0) break;
            if (csize > kBlock)            { reason = FOURMC_IMG_CSIZE_BEYOND; break; }
            if (N - p < csize)             { reason = FOURMC_IMG_DATA_UNREADABLE; break; }
            if (usize != csize && usize > kBlock) {
                reason = xxh32_lane(img + p, csize, 0) != sum ? FOURMC_IMG_BLOCK_CHECKSUM : FOURMC_IMG_USIZE_BEYOND;
                break;
            }
            if (blocks) {
                fourmc_block d;
                d.src_off = p; d.dst_off = total; d.src_len = csize; d.dst_cap = usize; d.result = 0; d.xxh32 = sum;
                blocks[nb] = d;
            }
            nb++; total += usize; p += csize;
        }
        if (reason != FOURMC_IMG_OK) break;
        at = p;                                                                  // footer (fourmc_file.c:562-588)
        if (N - p < 4)                     { reason = FOURMC_IMG_FOOTER_UNREADABLE; break; }
        const uint32_t fsz = be32(img + p);
        if (fsz < 8 || N - p < fsz)        { reason = FOURMC_IMG_FOOTER_SHORT; break; }
        if (xxh32_lane(img + p, fsz - 4, 0) != be32(img + p + fsz - 4)) { reason = FOURMC_IMG_FOOTER_CHECKSUM; break; }
        if (be32(img + p + 4) != 1)        { reason = FOURMC_IMG_FOOTER_VERSION; break; }
        p += fsz;
        if (total == stream_total0) break;                                       // an empty stream ends the file
    }
    if (!blocks) {
        ps->nblocks = nb; ps->total = total; ps->streams = streams; ps->reason = reason;
        ps->fail_offset = reason == FOURMC_IMG_OK ? N : at;
    }
}

// The verdict: the first block that failed its checksum or its decode ends decoding there (file order puts it before any
// framing error, which the parsers only ever report behind the last block they counted); otherwise the parser's verdict.
__global__ __launch_bounds__(64)
void image_reduce_kernel(const fourmc_block* __restrict__ blocks, uint32_t n, const fourmc_image_parse* ps, fourmc_image_status* st)
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
    if (lane) return;
    st->decoded_bytes = done;
    st->total_bytes = ps->total;
    st->streams = ps->streams;
    st->blocks = first;
    if (first < n) {
        const int32_t r = blocks[first].result;
        st->reason = r == FOURMC_BLK_BADSUM ? FOURMC_IMG_BLOCK_CHECKSUM : FOURMC_IMG_CORRUPT;
        st->exit_code = 4;
        st->fail_offset = blocks[first].src_off - 12;
    } else {
        st->reason = ps->reason;
        st->exit_code = fourmc_image_exit_code(ps->reason);
        st->fail_offset = ps->fail_offset;
    }
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
    hipLaunchKernelGGL(image_enc_scan_kernel, dim3(1), dim3(64), 0, s, d_blocks, d_off, n, d_sum);
    if (hipError_t e = hipGetLastError()) return e;
    if (hipError_t e = fourmc_launch_pack_image(d_staging, d_image, d_blocks, d_off, n, s)) return e;
    hipLaunchKernelGGL(image_enc_tail_kernel, dim3(1), dim3(256), 0, s, static_cast<uint8_t*>(d_image), d_off, n, magic);
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

} // extern "C"
