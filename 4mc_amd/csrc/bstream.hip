// 4mc_amd/csrc/bstream.hip — the framing of Hadoop block streams in HBM (fourmc_gpu_bstream_*): the part files Lz4Codec, ZstdCodec
// and their six siblings write through BlockCompressorStream (Lz4Codec.java:95-104).  The format and the reader rule are stated in
// include/fourmc_gpu.h; they are written from knowledge of Hadoop's classes and from the reference's codec and compressor classes,
// not from a file a JVM wrote.
//
//   stream := group* [ BE32(0) ]      group := BE32(rawlen) chunk+      chunk := BE32(clen) payload[clen]
//
// The codecs are the existing raw block kernels; what is here is the framing around them:
//   decode  the walk, one wave per stream with lane 0 chasing the length fields in file order (the files have no index, so a stream
//           is one serial chain: two dependent reads per group), run twice - first for each stream's summary, then, once the host
//           has given every stream its slice of one descriptor table, for one fourmc_block per chunk - and the fold of the decoded
//           chunks and the walk's verdict into the status, one wave per stream;
//   encode  descriptors from the input size (groups of group_bytes, the last one short), the scan of 8 + csize into 64-bit stream
//           offsets carried across staging pieces, and the pack that writes each group's 8-byte header and copies its payload out
//           of the staging slot.
// The walk assumes the writer's shape: chunk j of a group of rawlen R decodes to min(M, R - j M) bytes.  That is what makes it pure
// header chasing; the decode proves it (dst_cap = the expected size, and the result must equal it).
// Only vector stores and plain C++; no atomics across workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"
#include "devcopy.h"
#include "devframe.h"

namespace {

constexpr uint32_t kMaxClen = FOURMC_BLOCKSIZE;          // Lz4Decompressor's direct buffer: a longer chunk would be cut there

// ------------------------------------------------------------------------------------------------------------- decode
// The reader rule on one lane.  Count mode (desc NULL): the summary of the whole stream into *out.  Fill mode: the same chase over
// the groups the summary counted, writing chunk k's descriptor at desc[k] and its header offset and group number at side[k]; it
// checks nothing again but never passes the counts it was given, so a stream whose bytes changed between the runs cannot write
// outside its slice.  src_base / dst_base: where the stream and its output lie in the buffers the block decode works on.
// Only whole groups count: a group cut short by a framing error contributes no chunk and no byte of total.
__device__ __forceinline__ void bs_walk(const uint8_t* __restrict__ img, uint64_t N, uint32_t M, fourmc_bstream_walk* out,
                                        const fourmc_bstream_walk* have, fourmc_block* __restrict__ desc,
                                        fourmc_bstream_side* __restrict__ side, uint64_t src_base, uint64_t dst_base)
{
    uint64_t p = 0, total = 0, groups = 0, chunks = 0, fail = N;
    int32_t reason = FOURMC_BS_OK;
    const uint64_t group_limit = desc ? have->groups : ~0ull, chunk_limit = desc ? have->chunks : ~0ull;
    while (groups < group_limit) {
        if (N - p < 4) break;                                   // 0 bytes: the end; 1 - 3: the EOF Hadoop's reader swallows
        const uint32_t R = be32(img + p);
        if (R == 0) break;                                      // the writer's trailing zero, or the empty stream
        if (R > 0x7FFFFFFFu) { reason = FOURMC_BS_BAD_RAWLEN; fail = p; break; }
        uint64_t q = p + 4, k = chunks;
        uint32_t done = 0;
        while (done < R) {
            if (N - q < 4)          { reason = FOURMC_BS_CLEN_UNREADABLE; fail = q; break; }
            const uint32_t clen = be32(img + q);
            if (clen == 0 || clen > kMaxClen) { reason = FOURMC_BS_BAD_CLEN; fail = q; break; }
            if (N - q - 4 < clen)   { reason = FOURMC_BS_DATA_UNREADABLE; fail = q; break; }
            const uint32_t expect = R - done < M ? R - done : M;
            if (desc) {
                if (k >= chunk_limit) { reason = -1; break; }
                fourmc_block d;
                d.src_off = src_base + q + 4; d.dst_off = dst_base + total + done; d.src_len = clen; d.dst_cap = expect;
                d.result = 0; d.xxh32 = 0;
                desc[k] = d;
                fourmc_bstream_side sd; sd.at = q; sd.group = groups;
                side[k] = sd;
            }
            k++; done += expect; q += 4ull + clen;
        }
        if (reason != FOURMC_BS_OK) break;
        p = q; chunks = k; total += R; groups++;
    }
    if (!desc) {
        out->chunks = chunks; out->groups = groups; out->total = total; out->fail_offset = fail; out->reason = reason; out->pad = 0;
    }
}

// an item whose decoded size does not fit its region is not decoded at all: it has no descriptors (the host's prefix sum gives it
// none) and its status is FOURMC_BS_DST_SMALL
__device__ __forceinline__ bool bs_dst_small(const fourmc_bstream_walk& w, const fourmc_bstream_item& it) { return w.total > it.dst_cap; }

// one wave per stream; desc NULL: run 1 (ws[i] = the summary), else run 2 (the descriptors of the summary ws[i] holds, at first[i])
__global__ __launch_bounds__(64)
void bstream_walk_kernel(const uint8_t* __restrict__ images, const fourmc_bstream_item* __restrict__ items, uint32_t M,
                         fourmc_bstream_walk* __restrict__ ws, const uint64_t* __restrict__ first, fourmc_block* __restrict__ desc,
                         fourmc_bstream_side* __restrict__ side)
{
    if (threadIdx.x != 0) return;
    const uint32_t i = blockIdx.x;
    const fourmc_bstream_item it = items[i];
    const uint8_t* img = images + it.image_off;
    if (!desc) { bs_walk(img, it.image_bytes, M, ws + i, nullptr, nullptr, nullptr, 0, 0); return; }
    const fourmc_bstream_walk w = ws[i];
    if (bs_dst_small(w, it) || w.chunks == 0) return;
    bs_walk(img, it.image_bytes, M, nullptr, &w, desc + first[i], side + first[i], it.image_off, it.dst_off);
}

// The fold, one wave per stream over its slice: the first chunk in file order whose result is not its expected size ends decoding
// there - the codec's sign says whether it is damage (CORRUPT: a negative result, which a chunk holding more than its expected size
// gives too) or a foreign chunking (SHAPE: a clean decode to fewer bytes).  It lies in front of any framing error, which the walk
// only reports behind the last chunk it listed; without one the walk's verdict stands.
__global__ __launch_bounds__(64)
void bstream_fold_kernel(const fourmc_bstream_item* __restrict__ items, const fourmc_bstream_walk* __restrict__ ws,
                         const uint64_t* __restrict__ first, const fourmc_block* __restrict__ desc,
                         const fourmc_bstream_side* __restrict__ side, fourmc_bstream_status* __restrict__ status)
{
    const uint32_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const fourmc_bstream_item it = items[i];
    const fourmc_bstream_walk w = ws[i];
    fourmc_bstream_status st = {};
    st.total_bytes = w.total;
    if (bs_dst_small(w, it)) {
        if (lane) return;
        st.reason = FOURMC_BS_DST_SMALL; st.fail_offset = it.image_bytes;
        status[i] = st;
        return;
    }
    const uint32_t n = uint32_t(w.chunks);
    const fourmc_block* blocks = desc + first[i];
    uint64_t done = 0;
    uint32_t bad_at = n;
    for (uint32_t c0 = 0; c0 < n; c0 += 64) {
        const uint32_t c = c0 + uint32_t(lane);
        int32_t r = 0; uint32_t cap = 0;
        if (c < n) { r = blocks[c].result; cap = blocks[c].dst_cap; }
        const unsigned long long badm = __ballot(c < n && (r < 0 || uint32_t(r) != cap));
        uint64_t mine = c < n ? uint64_t(cap) : 0;
        if (badm) {
            const uint32_t l = uint32_t(__builtin_ctzll(badm));
            if (uint32_t(lane) >= l) mine = 0;
            bad_at = c0 + l;
        }
        for (int o = 32; o; o >>= 1) mine += uint64_t(__shfl_xor((long long)mine, o));
        done += mine;
        if (badm) break;
    }
    if (lane) return;
    st.decoded_bytes = done;
    if (bad_at < n) {
        const int32_t r = blocks[bad_at].result;
        st.reason = (r < 0 || uint32_t(r) > blocks[bad_at].dst_cap) ? FOURMC_BS_CORRUPT : FOURMC_BS_SHAPE;
        st.fail_offset = side[first[i] + bad_at].at;
        st.groups = uint32_t(side[first[i] + bad_at].group);
        st.chunks = bad_at;
    } else {
        st.reason = w.reason; st.fail_offset = w.fail_offset; st.groups = uint32_t(w.groups); st.chunks = n;
    }
    status[i] = st;
}

// ------------------------------------------------------------------------------------------------------------- encode
// group b of a staging piece: src0 + b * group_bytes of the source (src_bytes: what the piece holds from src0 on), slot b of the
// staging, dst_cap = the codec's bound for its length - or 0xFFFFFFFF, LZ4_compressMC's "no limit" (the slot still holds the bound)
__global__ __launch_bounds__(256)
void bstream_enc_desc_kernel(fourmc_block* __restrict__ blocks, uint64_t src0, uint64_t src_bytes, uint32_t group_bytes,
                             uint32_t stride, uint32_t n, int zstd, int nolimit)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const uint64_t at = uint64_t(b) * group_bytes;
    fourmc_block d;
    d.src_off = src0 + at; d.dst_off = uint64_t(b) * stride;
    d.src_len = uint32_t(src_bytes - at < group_bytes ? src_bytes - at : group_bytes);
    d.dst_cap = nolimit ? 0xFFFFFFFFu : fourmc_bstream_block_bound(zstd, d.src_len);
    d.result = 0; d.xxh32 = 0;
    blocks[b] = d;
}

// off[b] = where group b's header goes: the running stream offset sum->image_bytes (0 before the first piece) plus the 8 + csize of
// the piece's groups before it, on one wave with a 64-bit carry; the carry goes back into *sum for the next piece.  A result <= 0 or
// above the codec's bound cannot come from an encoder that was given the bound; it is counted (the engine fails the call) and
// clamped, so that the pack stays inside the capacity the engine checked against fourmc_gpu_bstream_bound.
__global__ __launch_bounds__(64)
void bstream_enc_scan_kernel(fourmc_block* __restrict__ blocks, uint64_t* __restrict__ off, uint32_t n, int zstd,
                             fourmc_bstream_enc_summary* sum)
{
    const int lane = threadIdx.x;
    uint64_t carry = sum->image_bytes;
    uint32_t bad = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += 64) {
        const uint32_t b = b0 + uint32_t(lane);
        uint32_t step = 0;
        if (b < n) {
            const fourmc_block d = blocks[b];
            const uint32_t bound = fourmc_bstream_block_bound(zstd, d.src_len);
            int32_t r = d.result;
            if (r <= 0 || uint32_t(r) > bound) { bad++; r = r <= 0 ? 0 : int32_t(bound); blocks[b].result = r; }
            step = 8u + uint32_t(r);
        }
        const uint32_t incl = scan_add(step);
        if (b < n) off[b] = carry + (incl - step);
        carry += wave_total(incl);
    }
    for (int o = 32; o; o >>= 1) bad += uint32_t(__shfl_xor(int(bad), o));
    if (lane == 0) { sum->image_bytes = carry; sum->bad += bad; }
}

// one workgroup per group: BE32(len) BE32(csize) at off[b], then the payload out of the staging slot, a quarter to each wave
// (pack.hip's 12-byte twin)
__global__ __launch_bounds__(256)
void bstream_pack_kernel(const uint8_t* __restrict__ staging, uint8_t* __restrict__ image, const fourmc_block* __restrict__ blocks,
                         const uint64_t* __restrict__ off)
{
    const fourmc_block blk = blocks[blockIdx.x];
    const uint32_t csize = blk.result > 0 ? uint32_t(blk.result) : 0u;
    uint8_t* out = image + off[blockIdx.x];
    const uint32_t t = threadIdx.x;
    if (t < 8) out[t] = uint8_t((t < 4 ? blk.src_len : csize) >> (8 * (3 - (t & 3))));
    const uint32_t part = (((csize + 3) / 4) + 15) & ~15u;
    const uint32_t w = t >> 6, from = w * part;
    if (from >= csize) return;
    const uint32_t len = csize - from < part ? csize - from : part;
    wave_copy(out + 8 + from, staging + blk.dst_off + from, int(len), int(t & 63));
}

} // namespace

extern "C" {

hipError_t fourmc_launch_bstream_walk(const void* d_images, const fourmc_bstream_item* d_items, uint32_t n, uint32_t max_input,
                                      fourmc_bstream_walk* d_ws, const uint64_t* d_first, fourmc_block* d_desc,
                                      fourmc_bstream_side* d_side, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bstream_walk_kernel, dim3(n), dim3(64), 0, s, static_cast<const uint8_t*>(d_images), d_items, max_input, d_ws,
                       d_first, d_desc, d_side);
    return hipGetLastError();
}

hipError_t fourmc_launch_bstream_fold(const fourmc_bstream_item* d_items, uint32_t n, const fourmc_bstream_walk* d_ws,
                                      const uint64_t* d_first, const fourmc_block* d_desc, const fourmc_bstream_side* d_side,
                                      fourmc_bstream_status* d_status, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bstream_fold_kernel, dim3(n), dim3(64), 0, s, d_items, d_ws, d_first, d_desc, d_side, d_status);
    return hipGetLastError();
}

hipError_t fourmc_launch_bstream_enc_desc(fourmc_block* d_blocks, uint64_t src0, uint64_t src_bytes, uint32_t group_bytes,
                                          uint32_t stride, uint32_t n, int zstd, int nolimit, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bstream_enc_desc_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_blocks, src0, src_bytes, group_bytes, stride,
                       n, zstd, nolimit);
    return hipGetLastError();
}

hipError_t fourmc_launch_bstream_enc_pack(void* d_image, fourmc_block* d_blocks, uint64_t* d_off, uint32_t n, int zstd,
                                          const void* d_staging, fourmc_bstream_enc_summary* d_sum, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bstream_enc_scan_kernel, dim3(1), dim3(64), 0, s, d_blocks, d_off, n, zstd, d_sum);
    hipLaunchKernelGGL(bstream_pack_kernel, dim3(n), dim3(256), 0, s, static_cast<const uint8_t*>(d_staging),
                       static_cast<uint8_t*>(d_image), d_blocks, d_off);
    return hipGetLastError();
}

} // extern "C"
