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
//           of the staging slot;
//   encode from write() sizes (fourmc_gpu_bstreams_compress, "the writer's grouping" below): the plan that turns each stream's
//           table of write sizes into groups and chunks - tile sums and their prefixes by full-chip kernels, then one wave per
//           stream chasing the groups with a 64-ary search per step - the descriptors of a round of chunks, the segmented scan of
//           their places with one 64-bit carry per stream, and the pack that also writes group headers of multi-chunk groups, the
//           trailer and the empty stream.
// The walk assumes the writer's shape: chunk j of a group of rawlen R decodes to min(M, R - j M) bytes.  That is what makes it pure
// header chasing; the decode proves it (dst_cap = the expected size, and the result must equal it).
// Only vector stores and plain C++; no atomics across workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"
#include "devcopy.h"
#include "devframe.h"
#include "bswscan.h"

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

// ------------------------------------------------------------------------------------------- encode: the writer's grouping
// BlockCompressorStream's rule over a stream's write() sizes w_0 .. w_{k-1} (include/fourmc_gpu.h): at write i with nothing
// accumulated, w_i > M is a long group of ceil(w_i / M) chunks; otherwise the group takes writes i .. j for the largest j whose sum
// stays <= M and is one chunk; a group of sum 0 is not written.  A group is long exactly when its rawlen is above M.
// (kBswTile, scan_add64 and bsw_owner: bswscan.h, shared with lines_pack.hip)
constexpr uint64_t kBswBadBit = 1ull << 63;              // in a tile's sum, before the finish: an entry above 0x7FFFFFFF

__device__ __forceinline__ uint32_t bsw_slot(int zstd, uint32_t len) { return (fourmc_bstream_block_bound(zstd, len) + 255u) & ~255u; }

// one wave per tile of 64 entries, over the tiles of all streams: sums[tile] = the sum of its entries, kBswBadBit set when one of
// them is above 0x7FFFFFFF
__global__ __launch_bounds__(256)
void bsw_tile_kernel(const uint32_t* __restrict__ writes, const fourmc_bstream_enc_item* __restrict__ items,
                     const uint64_t* __restrict__ tile0, uint32_t n, uint64_t ntiles, uint64_t* __restrict__ sums)
{
    const uint64_t gt = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gt >= ntiles) return;
    const uint32_t i = bsw_owner(tile0, 1, n, gt);
    const fourmc_bstream_enc_item it = items[i];
    const uint64_t e = (gt - tile0[i]) * kBswTile + uint64_t(lane);
    const uint32_t w = e < it.n_writes ? writes[it.writes_off + e] : 0u;
    uint64_t sum = w;
    for (int o = 32; o; o >>= 1) sum += uint64_t(__shfl_xor((long long)sum, o));
    const bool bad = __ballot(w > 0x7FFFFFFFu) != 0;
    if (lane == 0) sums[gt] = sum | (bad ? kBswBadBit : 0);
}

// One workgroup per stream with a table: its tile sums become their inclusive 64-bit prefixes in place, and the total and the bad
// bits give the verdict (_WRITE over _SUM).  Each thread owns a run of consecutive tiles.
__global__ __launch_bounds__(1024)
void bsw_finish_kernel(const fourmc_bstream_enc_item* __restrict__ items, const uint64_t* __restrict__ tile0,
                       uint64_t* __restrict__ sums, fourmc_bsw_plan* __restrict__ plans)
{
    __shared__ uint64_t part[1024];
    __shared__ uint32_t any_bad;
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const fourmc_bstream_enc_item it = items[i];
    if (it.n_writes == 0) return;
    uint64_t* mine = sums + tile0[i];
    const uint64_t T = tile0[i + 1] - tile0[i], per = (T + 1023) / 1024;
    const uint64_t lo = per * t < T ? per * t : T, hi = lo + per < T ? lo + per : T;
    if (t == 0) any_bad = 0;
    __syncthreads();
    uint64_t acc = 0;
    bool bad = false;
    for (uint64_t k = lo; k < hi; k++) { const uint64_t v = mine[k]; bad |= (v & kBswBadBit) != 0; acc += v & ~kBswBadBit; }
    if (bad) any_bad = 1;                                // every writer stores the same value
    part[t] = acc;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t add = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    uint64_t run = part[t] - acc;                        // exclusive: the tiles in front of this thread's run
    for (uint64_t k = lo; k < hi; k++) { run += mine[k] & ~kBswBadBit; mine[k] = run; }
    if (t == 0) {
        fourmc_bsw_plan pl = {};
        pl.reason = any_bad ? FOURMC_BSW_WRITE : part[1023] != it.src_bytes ? FOURMC_BSW_SUM : FOURMC_BSW_OK;
        plans[i] = pl;
    }
}

// what the chase and the closed form count per stream
struct BswCount {
    uint64_t groups = 0, chunks = 0, worst = 0, stage = 0;
    bool last_long = false;
    __device__ __forceinline__ void group(int zstd, uint32_t M, uint64_t R, uint64_t times)
    {   // `times` groups of rawlen R each
        const uint64_t k = (R + M - 1) / M;
        const uint32_t rest = uint32_t(R - (k - 1) * M);
        groups += times; chunks += times * k;
        worst += times * (4 + (k - 1) * (4ull + fourmc_bstream_block_bound(zstd, M)) + 4ull + fourmc_bstream_block_bound(zstd, rest));
        stage += times * ((k - 1) * bsw_slot(zstd, M) + bsw_slot(zstd, rest));
        last_long = R > M;
    }
};

// The uniform schedule (n_writes == 0) in closed form: every group holds `unit` bytes - the writes of w <= M bytes that fit one
// chunk, or one long write - and the last one the rest.  0 for no write at all.
__device__ __forceinline__ uint64_t bsw_uniform_unit(const fourmc_bstream_enc_item& it, uint32_t M)
{
    if (it.src_bytes == 0) return 0;
    const uint64_t w = it.write_bytes && it.write_bytes < it.src_bytes ? it.write_bytes : it.src_bytes;
    return w > M ? w : (M / w) * w;
}

// One wave per stream.  Count mode (groups NULL): plans[i] = the stream's counts, its exact worst case and its staging bytes.
// Fill mode: the same chase writes group g of the stream to groups[slices[i].group0 + g], never past the count it was given.
// Each step finds how many entries have an inclusive prefix <= start + M: a 64-ary search over the tile prefixes (lanes probe 64
// evenly spaced tiles of the range left, which shrinks 64-fold per probe), then the scan of the one tile the boundary falls in.
__global__ __launch_bounds__(64)
void bsw_chase_kernel(const uint32_t* __restrict__ writes, const fourmc_bstream_enc_item* __restrict__ items,
                      const uint64_t* __restrict__ tile0, const uint64_t* __restrict__ prefix, uint32_t M, int zstd,
                      fourmc_bsw_plan* __restrict__ plans, const fourmc_bsw_slice* __restrict__ slices,
                      fourmc_bsw_group* __restrict__ groups)
{
    const uint32_t i = blockIdx.x;
    const int lane = threadIdx.x;
    const fourmc_bstream_enc_item it = items[i];
    BswCount n;
    if (it.n_writes == 0) {                              // closed form; the descriptors use it too, so fill mode has nothing to do
        if (groups || lane) return;
        fourmc_bsw_plan pl = {};
        const uint64_t unit = bsw_uniform_unit(it, M);
        const uint64_t w = it.write_bytes && it.write_bytes < it.src_bytes ? it.write_bytes : it.src_bytes;
        if (w > 0x7FFFFFFFull) { pl.reason = FOURMC_BSW_WRITE; plans[i] = pl; return; }
        if (unit) {
            const uint64_t full = it.src_bytes / unit, rest = it.src_bytes % unit;
            if (full) n.group(zstd, M, unit, full);
            if (rest) n.group(zstd, M, rest, 1);
        }
        pl.groups = n.groups; pl.chunks = n.chunks; pl.trailer = n.groups == 0 || n.last_long;
        pl.worst = n.worst + 4 * pl.trailer; pl.stage = n.stage; pl.reason = FOURMC_BSW_OK;
        plans[i] = pl;
        return;
    }
    const fourmc_bsw_plan have = plans[i];
    if (have.reason != FOURMC_BSW_OK) return;            // the finish left the verdict and zero counts
    const uint64_t* P = prefix + tile0[i];
    const uint32_t* W = writes + it.writes_off;
    const uint64_t nw = it.n_writes, T = tile0[i + 1] - tile0[i];
    fourmc_bsw_group* out = groups ? groups + slices[i].group0 : nullptr;
    uint64_t c = 0, start = 0;                           // entries consumed, and their bytes
    while (c < nw) {
        const uint64_t target = start + M;
        uint64_t a = c / kBswTile, b = T;                // the first tile whose end prefix is above target lies in [a, b]
        while (b - a > 64) {
            const uint64_t stride = (b - a + 63) / 64;
            uint64_t at = a + (uint64_t(lane) + 1) * stride - 1;
            if (at >= b) at = b - 1;
            const uint32_t k = uint32_t(__popcll(__ballot(P[at] <= target)));
            if (k == 64) { a = b; break; }
            a += k * stride;
            if (a + stride < b) b = a + stride;
        }
        {
            const uint64_t at = a + uint64_t(lane);
            a += uint32_t(__popcll(__ballot(at < b && P[at] <= target)));
        }
        uint64_t cnt = nw, end = P[T - 1], wc = 0;       // the boundary tile: a (a == T: every entry fits)
        if (a < T) {
            const uint64_t e = a * kBswTile + uint64_t(lane);
            const uint32_t w = e < nw ? W[e] : 0u;
            const uint64_t base = a ? P[a - 1] : 0;
            const uint64_t incl = base + scan_add64(w, lane);
            const uint32_t k = uint32_t(__popcll(__ballot(e < nw && incl <= target)));
            cnt = a * kBswTile + k;
            end = k ? uint64_t(__shfl((long long)incl, int(k) - 1)) : base;
            wc = k < 64 ? uint64_t(uint32_t(__shfl(int(w), int(k)))) : 0;        // the first entry that does not fit
        }
        uint64_t R;
        if (cnt > c) { R = end - start; c = cnt; }       // writes c .. cnt - 1 accumulate
        else         { R = wc; c++; }                     // nothing fits: entry c is longer than M
        if (R) {
            if (out && n.groups < have.groups && lane == 0) {
                fourmc_bsw_group g; g.src = start; g.stage = n.stage; g.rawlen = uint32_t(R); g.chunk0 = uint32_t(n.chunks);
                out[n.groups] = g;
            }
            n.group(zstd, M, R, 1);
        }
        start += R;
    }
    if (groups || lane) return;
    fourmc_bsw_plan pl = {};
    pl.groups = n.groups; pl.chunks = n.chunks; pl.trailer = n.groups == 0 || n.last_long;
    pl.worst = n.worst + 4 * pl.trailer; pl.stage = n.stage; pl.reason = FOURMC_BSW_OK;
    plans[i] = pl;
}

// where chunk gc (counted over all streams in file order) lies: its stream, its group's rawlen, its number in the group, its source
// bytes and its staging offset (counted over all streams)
struct BswChunk { uint32_t stream, rawlen, j, len; uint64_t src, stage; bool last; };
__device__ __forceinline__ BswChunk bsw_locate(uint64_t gc, const fourmc_bstream_enc_item* __restrict__ items,
                                               const fourmc_bsw_plan* __restrict__ plans, const fourmc_bsw_slice* __restrict__ slices,
                                               const fourmc_bsw_group* __restrict__ groups, uint32_t n, uint32_t M, int zstd)
{
    BswChunk c;
    c.stream = bsw_owner(&slices[0].chunk0, sizeof(fourmc_bsw_slice) / 8, n, gc);
    const fourmc_bstream_enc_item it = items[c.stream];
    const fourmc_bsw_slice sl = slices[c.stream];
    const uint64_t k = gc - sl.chunk0;                   // the chunk's number in its stream
    uint64_t gsrc, gstage, R;
    if (it.n_writes == 0) {
        const uint64_t unit = bsw_uniform_unit(it, M), per = (unit + M - 1) / M, g = k / per;
        c.j = uint32_t(k % per);
        gsrc = g * unit;
        R = it.src_bytes - gsrc < unit ? it.src_bytes - gsrc : unit;
        gstage = g * ((per - 1) * bsw_slot(zstd, M) + bsw_slot(zstd, uint32_t(unit - (per - 1) * M)));
    } else {
        const fourmc_bsw_group* G = groups + sl.group0;
        uint64_t lo = 0, hi = plans[c.stream].groups;    // G[lo].chunk0 <= k < G[hi].chunk0
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (G[mid].chunk0 <= k) lo = mid; else hi = mid;
        }
        const fourmc_bsw_group g = G[lo];
        c.j = uint32_t(k - g.chunk0);
        gsrc = g.src; gstage = g.stage; R = g.rawlen;
    }
    c.rawlen = uint32_t(R);
    const uint64_t done = uint64_t(c.j) * M;
    c.len = uint32_t(R - done < M ? R - done : M);
    c.src = it.src_off + gsrc + done;
    c.stage = sl.stage0 + gstage + uint64_t(c.j) * bsw_slot(zstd, M);
    c.last = k + 1 == plans[c.stream].chunks;
    return c;
}

// one thread per chunk of a round (chunks c0 .. c0 + m - 1): its descriptor, its staging slot counted from the round's first chunk,
// and the side entry the scan and the pack read
__global__ __launch_bounds__(256)
void bsw_desc_kernel(const fourmc_bstream_enc_item* __restrict__ items, const fourmc_bsw_plan* __restrict__ plans,
                     const fourmc_bsw_slice* __restrict__ slices, const fourmc_bsw_group* __restrict__ groups, uint32_t n, uint32_t M,
                     int zstd, int nolimit, uint64_t c0, uint32_t m, fourmc_block* __restrict__ blocks,
                     fourmc_bsw_side* __restrict__ side)
{
    __shared__ uint64_t stage0;
    if (threadIdx.x == 0) stage0 = bsw_locate(c0, items, plans, slices, groups, n, M, zstd).stage;
    __syncthreads();
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= m) return;
    const BswChunk c = bsw_locate(c0 + b, items, plans, slices, groups, n, M, zstd);
    fourmc_block d;
    d.src_off = c.src; d.dst_off = c.stage - stage0; d.src_len = c.len;
    d.dst_cap = nolimit ? 0xFFFFFFFFu : fourmc_bstream_block_bound(zstd, c.len);
    d.result = 0; d.xxh32 = 0;
    blocks[b] = d;
    fourmc_bsw_side sd;
    sd.stream = c.stream; sd.rawlen = c.j == 0 ? c.rawlen : 0u; sd.trailer = c.last && plans[c.stream].trailer ? 1u : 0u; sd.pad = 0;
    side[b] = sd;
}

// off[b] = where chunk b's bytes go in d_images: its stream's image_off, the stream offset carry[stream] left by the rounds before
// and the steps of the stream's chunks in front of it in this round - 4 + csize, and 4 more for the first chunk of a group, which
// carries the group header.  One wave; the chunks of a stream are consecutive, so the segmented sum is the wave's prefix sum less
// its value at the segment's head.  The end offset goes back into carry[stream] for the next round.  Bad codec results are counted
// and clamped as in bstream_enc_scan_kernel.
__global__ __launch_bounds__(64)
void bsw_scan_kernel(fourmc_block* __restrict__ blocks, const fourmc_bsw_side* __restrict__ side, uint32_t m, int zstd,
                     const fourmc_bstream_enc_item* __restrict__ items, uint64_t* __restrict__ carry, uint64_t* __restrict__ off,
                     fourmc_bstream_enc_summary* sum)
{
    const int lane = threadIdx.x;
    uint32_t run_stream = 0xFFFFFFFFu, bad = 0;
    uint64_t run_off = 0;
    for (uint32_t b0 = 0; b0 < m; b0 += 64) {
        const uint32_t b = b0 + uint32_t(lane);
        const bool valid = b < m;
        uint32_t step = 0, st = 0xFFFFFFFFu;
        if (valid) {
            const fourmc_block d = blocks[b];
            const fourmc_bsw_side sd = side[b];
            const uint32_t bound = fourmc_bstream_block_bound(zstd, d.src_len);
            int32_t r = d.result;
            if (r <= 0 || uint32_t(r) > bound) { bad++; r = r <= 0 ? 0 : int32_t(bound); blocks[b].result = r; }
            step = (sd.rawlen ? 8u : 4u) + uint32_t(r);
            st = sd.stream;
        }
        const uint32_t incl = scan_add(step);
        const uint32_t before = uint32_t(__shfl_up(int(st), 1)), after = uint32_t(__shfl_down(int(st), 1));
        const unsigned long long heads = __ballot(valid && (lane == 0 || before != st));
        const int h = 63 - __builtin_clzll((heads & (~0ull >> (63 - lane))) | 1ull);       // the head of this lane's segment
        const uint32_t excl_h = uint32_t(__shfl(int(incl - step), h));
        uint64_t end = 0;
        if (valid) {
            const uint64_t base = h == 0 && st == run_stream ? run_off : carry[st];
            const uint64_t pos = base + (incl - step - excl_h);
            off[b] = items[st].image_off + pos;
            end = pos + step;
        }
        const int last = 63 - __builtin_clzll(__ballot(valid));
        if (valid && (lane == last || after != st)) carry[st] = end;
        run_stream = uint32_t(__shfl(int(st), last));
        run_off = uint64_t(__shfl((long long)end, last));
    }
    for (int o = 32; o; o >>= 1) bad += uint32_t(__shfl_xor(int(bad), o));
    if (lane == 0) sum->bad += bad;
}

// one workgroup per chunk: [BE32(rawlen) for the first chunk of a group] BE32(csize) payload [BE32(0) behind the last chunk of a
// stream that ends with the trailer]; bstream_pack_kernel is its one-chunk-group case
__global__ __launch_bounds__(256)
void bsw_pack_kernel(const uint8_t* __restrict__ staging, uint8_t* __restrict__ images, const fourmc_block* __restrict__ blocks,
                     const fourmc_bsw_side* __restrict__ side, const uint64_t* __restrict__ off)
{
    const fourmc_block blk = blocks[blockIdx.x];
    const fourmc_bsw_side sd = side[blockIdx.x];
    const uint32_t csize = blk.result > 0 ? uint32_t(blk.result) : 0u;
    const uint32_t head = sd.rawlen ? 8u : 4u;
    uint8_t* out = images + off[blockIdx.x];
    const uint32_t t = threadIdx.x;
    if (t < head) out[t] = uint8_t((head == 8 && t < 4 ? sd.rawlen : csize) >> (8 * (3 - (t & 3))));
    if (sd.trailer && t >= 64 && t < 68) out[head + csize + (t - 64)] = 0;
    const uint32_t part = (((csize + 3) / 4) + 15) & ~15u;
    const uint32_t w = t >> 6, from = w * part;
    if (from >= csize) return;
    const uint32_t len = csize - from < part ? csize - from : part;
    wave_copy(out + head + from, staging + blk.dst_off + from, int(len), int(t & 63));
}

// one thread per stream: the length of every stream that was written (its carry, and the trailer), and the four bytes of a stream
// with no chunk at all
__global__ __launch_bounds__(256)
void bsw_result_kernel(const fourmc_bstream_enc_item* __restrict__ items, const fourmc_bsw_plan* __restrict__ plans,
                       const uint64_t* __restrict__ carry, uint32_t n, uint8_t* __restrict__ images, uint64_t* __restrict__ bytes)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const fourmc_bsw_plan pl = plans[i];
    if (pl.reason != FOURMC_BSW_OK) { bytes[i] = 0; return; }
    if (pl.chunks == 0) {
        uint8_t* out = images + items[i].image_off;
        out[0] = 0; out[1] = 0; out[2] = 0; out[3] = 0;
        bytes[i] = 4;
        return;
    }
    bytes[i] = carry[i] + 4 * pl.trailer;
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

hipError_t fourmc_launch_bsw_sums(const uint32_t* d_writes, const fourmc_bstream_enc_item* d_items, const uint64_t* d_tile0, uint32_t n,
                                  uint64_t ntiles, uint64_t* d_sums, fourmc_bsw_plan* d_plans, hipStream_t s)
{
    if (n == 0 || ntiles == 0) return hipSuccess;
    hipLaunchKernelGGL(bsw_tile_kernel, dim3(uint32_t((ntiles + 3) / 4)), dim3(256), 0, s, d_writes, d_items, d_tile0, n, ntiles, d_sums);
    hipLaunchKernelGGL(bsw_finish_kernel, dim3(n), dim3(1024), 0, s, d_items, d_tile0, d_sums, d_plans);
    return hipGetLastError();
}

hipError_t fourmc_launch_bsw_chase(const uint32_t* d_writes, const fourmc_bstream_enc_item* d_items, const uint64_t* d_tile0,
                                   const uint64_t* d_prefix, uint32_t n, uint32_t max_input, int zstd, fourmc_bsw_plan* d_plans,
                                   const fourmc_bsw_slice* d_slices, fourmc_bsw_group* d_groups, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bsw_chase_kernel, dim3(n), dim3(64), 0, s, d_writes, d_items, d_tile0, d_prefix, max_input, zstd, d_plans,
                       d_slices, d_groups);
    return hipGetLastError();
}

hipError_t fourmc_launch_bsw_desc(const fourmc_bstream_enc_item* d_items, const fourmc_bsw_plan* d_plans, const fourmc_bsw_slice* d_slices,
                                  const fourmc_bsw_group* d_groups, uint32_t n, uint32_t max_input, int zstd, int nolimit, uint64_t c0,
                                  uint32_t m, fourmc_block* d_blocks, fourmc_bsw_side* d_side, hipStream_t s)
{
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(bsw_desc_kernel, dim3((m + 255) / 256), dim3(256), 0, s, d_items, d_plans, d_slices, d_groups, n, max_input, zstd,
                       nolimit, c0, m, d_blocks, d_side);
    return hipGetLastError();
}

hipError_t fourmc_launch_bsw_pack(void* d_images, const fourmc_bstream_enc_item* d_items, fourmc_block* d_blocks,
                                  const fourmc_bsw_side* d_side, uint64_t* d_off, uint32_t m, int zstd, const void* d_staging,
                                  uint64_t* d_carry, fourmc_bstream_enc_summary* d_sum, hipStream_t s)
{
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(bsw_scan_kernel, dim3(1), dim3(64), 0, s, d_blocks, d_side, m, zstd, d_items, d_carry, d_off, d_sum);
    hipLaunchKernelGGL(bsw_pack_kernel, dim3(m), dim3(256), 0, s, static_cast<const uint8_t*>(d_staging),
                       static_cast<uint8_t*>(d_images), d_blocks, d_side, d_off);
    return hipGetLastError();
}

hipError_t fourmc_launch_bsw_result(const fourmc_bstream_enc_item* d_items, const fourmc_bsw_plan* d_plans, const uint64_t* d_carry,
                                    uint32_t n, void* d_images, uint64_t* d_bytes, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bsw_result_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_items, d_plans, d_carry, n,
                       static_cast<uint8_t*>(d_images), d_bytes);
    return hipGetLastError();
}

} // extern "C"
