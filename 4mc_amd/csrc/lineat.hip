// 4mc_amd/csrc/lineat.hip — lines by number (fourmc_gpu_image_line_index / _image_read_lines_at).
//
// The index is one entry per block: the line ends in front of the block, those inside it, and what the block's two seams look
// like.  It is built from per-block facts alone: the count launch takes every staged block for itself (a CR in its last byte is an
// end, nothing is in front of its first byte) and notes its first and last byte; the finish launch, one workgroup over all blocks,
// takes the CR LF seams back out and scans.  No group of blocks needs its neighbour's bytes.
// A read is rank / select over the same masks records.hip cuts lines with (linescan.h: ends16 through step_ends): the index says
// which block holds end k - 1 and end k and which rank they have there, the per-tile counts of the staged block say which 16 KiB
// tile, a wave scan over the tile's popcounts says which lane and step, and the rank inside the 16-bit mask is the position.
// Every launch is a plain launch: nothing here waits for another workgroup.  The staged blocks are 16-byte aligned, so a block is
// a Span with head 0 and its chunks never leave its slot.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"

namespace {
#include "linescan.h"

constexpr uint32_t kSlotTiles = FOURMC_BLOCKSIZE / FOURMC_RECORDS_TILE;   // tile counts per staging slot
constexpr uint32_t kNone = ~0u;

// the slot's descriptor: block list[j] (first + j without a list) into slot j
__global__ __launch_bounds__(256)
void lineat_desc_kernel(const fourmc_image_entry* __restrict__ ent, const uint32_t* __restrict__ list, uint32_t first, uint32_t m,
                        uint64_t stride, fourmc_block* __restrict__ desc)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const fourmc_image_entry e = ent[list ? list[j] : first + j];
    fourmc_block d;
    d.src_off = e.image_off + 12; d.dst_off = uint64_t(j) * stride; d.src_len = e.csize; d.dst_cap = e.usize; d.result = 0; d.xxh32 = e.xxh32;
    desc[j] = d;
}

// ------------------------------------------------------------------------------------------------------------- the index
// One workgroup of 8 waves per staged block, a wave per tile and round: the block's ends by itself, and the offset behind the
// last of them that is not a CR in the block's last byte (whether THAT one is an end is the next block's first byte).
__global__ __launch_bounds__(512)
void lineat_block_count_kernel(const uint8_t* __restrict__ stage, uint64_t stride, const fourmc_image_entry* __restrict__ ent,
                               uint32_t first, const fourmc_block* __restrict__ desc, fourmc_lineat_blk* __restrict__ blk)
{
    __shared__ uint32_t s_cnt, s_last;
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t b = first + blockIdx.x;
    const uint32_t usize = ent[b].usize;
    const bool bad = block_bad(desc[blockIdx.x]);
    const uint8_t* d = stage + uint64_t(blockIdx.x) * stride;
    if (t == 0) { s_cnt = 0; s_last = 0; }
    __syncthreads();
    uint32_t info = bad ? 4u : 0u;
    if (!bad && usize) {
        const uint32_t lastb = d[usize - 1];
        info |= (lastb == 13u ? 1u : 0u) | (d[0] == 10u ? 2u : 0u) | (lastb == 10u ? 8u : 0u);
        const Span sp(d, usize);
        const uint32_t ntiles = uint32_t((sp.nchunks + kTileChunks - 1) / kTileChunks);
        const uint32_t cr_chunk = lastb == 13u ? (usize - 1) / 16 : kNone, cr_bit = 1u << ((usize - 1) & 15);
        uint32_t k = 0, last = 0, two;
        for (uint32_t tile = w; tile < ntiles; tile += 8) {
            const uint32_t c0 = tile * kTileChunks + lane;
            const bool inner = sp.inner(tile);
            for (uint32_t i0 = 0; i0 < kSteps; i0 += 4) {             // 4 KiB of the wave in flight
                uint4 v[4];
                if (inner) { for (uint32_t j = 0; j < 4; j++) v[j] = sp.base[c0 + 64 * (i0 + j)]; }
                else { for (uint32_t j = 0; j < 4; j++) v[j] = clean_chunk(sp, c0 + 64 * (i0 + j)); }
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    const uint32_t c = c0 + 64 * (i0 + j);
                    uint32_t m = step_ends<false>(sp, c, v[j], lane, two);
                    k += __popc(m);
                    if (c == cr_chunk) m &= ~cr_bit;
                    if (m) last = max(last, 16 * c + 32 - uint32_t(__builtin_clz(m)));
                }
            }
        }
        for (int o = 32; o; o >>= 1) { k += uint32_t(__shfl_xor(int(k), o)); last = max(last, uint32_t(__shfl_xor(int(last), o))); }
        if (lane == 0) { atomicAdd(&s_cnt, k); atomicMax(&s_last, last); }
    }
    __syncthreads();
    if (t == 0) { fourmc_lineat_blk r; r.cnt = s_cnt; r.info = info | (s_last << 8); blk[b] = r; }
}

// what block b's seams do to its own count: its entry without the prefix
struct Seams { uint32_t ends, flags; };
__device__ __forceinline__ Seams seams_of(const fourmc_image_entry* __restrict__ ent, const fourmc_lineat_blk* __restrict__ blk, uint32_t nb,
                                          uint32_t b)
{
    Seams r = {0, 0};
    const uint32_t usize = ent[b].usize;
    if (!usize) return r;
    const fourmc_lineat_blk me = blk[b];
    bool open_cr = false, lf_of_cr = false;
    if (me.info & 1u) {                                          // the next content byte: past blocks without bytes
        uint32_t j = b + 1;
        while (j < nb && ent[j].usize == 0) j++;
        open_cr = j < nb && (blk[j].info & 2u);
    }
    if (me.info & 2u) {
        uint32_t j = b;
        while (j > 0 && ent[j - 1].usize == 0) j--;
        lf_of_cr = j > 0 && (blk[j - 1].info & 1u);
    }
    r.ends = me.cnt - (open_cr ? 1u : 0u);
    const uint32_t behind = (me.info & 1u) && !open_cr ? usize : min(me.info >> 8, usize);
    r.flags = (open_cr ? 1u : 0u) | (lf_of_cr ? 2u : 0u) | (behind << 8);
    return r;
}

// One workgroup: each thread a contiguous run of blocks; a 64-bit wave scan and the 16 wave totals order the runs (records.hip:
// finish_body).
__global__ __launch_bounds__(1024)
void lineat_index_finish_kernel(const fourmc_image_entry* __restrict__ ent, const fourmc_lineat_blk* __restrict__ blk, uint32_t nb,
                                uint64_t total_bytes, fourmc_image_line_entry* __restrict__ index, uint64_t cap,
                                fourmc_lineat_sum* __restrict__ sum)
{
    __shared__ uint64_t wsum[16];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t per = (nb + 1023) / 1024;
    const uint32_t a = uint32_t(min(uint64_t(nb), uint64_t(t) * per)), z = uint32_t(min(uint64_t(nb), uint64_t(a) + per));
    uint64_t mine = 0;
    bool bad = false;
    for (uint32_t b = a; b < z; b++) { mine += seams_of(ent, blk, nb, b).ends; bad |= (blk[b].info & 4u) != 0; }
    const int any_bad = __syncthreads_or(bad);
    uint64_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) { const uint64_t v = uint64_t(__shfl_up((unsigned long long)incl, o)); if (int(lane) >= o) incl += v; }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint64_t run = 0, ends = 0;
    for (uint32_t j = 0; j < 16; j++) { if (j < w) run += wsum[j]; ends += wsum[j]; }
    run += incl - mine;
    const bool fits = uint64_t(nb) + 1 <= cap;
    if (index && fits && !any_bad) {
        for (uint32_t b = a; b < z; b++) {
            const Seams s = seams_of(ent, blk, nb, b);
            fourmc_image_line_entry e; e.ends_before = run; e.ends = s.ends; e.flags = s.flags;
            index[b] = e;
            run += s.ends;
        }
    }
    if (t != 0) return;
    fourmc_lineat_sum r = {};
    r.total = total_bytes;
    if (any_bad) { r.result = -4; *sum = r; return; }
    uint32_t l = nb;                                              // the last block with bytes: is the content's last byte an end
    while (l > 0 && ent[l - 1].usize == 0) l--;
    const bool open_end = l > 0 && !(blk[l - 1].info & 9u);
    r.ends = ends; r.lines = ends + (open_end ? 1 : 0);
    if (index && !fits) r.result = -5;
    else if (index) { fourmc_image_line_entry e; e.ends_before = ends; e.ends = 0; e.flags = 0; index[nb] = e; }
    *sum = r;
}

// ------------------------------------------------------------------------------------------------------------- the read
__global__ __launch_bounds__(256)
void lineat_fill_kernel(int32_t* __restrict__ status, uint32_t* __restrict__ tlen, uint32_t n, int32_t code)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    status[i] = code; tlen[i] = 0;
}

// the block holding line end number k: the last b < nb with ends_before[b] <= k.  Whatever the index holds, the answer is a block.
__device__ __forceinline__ uint32_t holder(const fourmc_image_line_entry* __restrict__ index, uint32_t nb, uint64_t k)
{
    uint32_t lo = 0, hi = nb;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (index[mid].ends_before <= k) lo = mid + 1; else hi = mid;
    }
    return lo ? lo - 1 : 0;
}
__device__ __forceinline__ uint32_t rank32(uint64_t r) { return r < 0xFFFFFFFEull ? uint32_t(r) : 0xFFFFFFFEu; }

// One lane per request.  A line that leaves bp starts behind bp's last end, which the index holds: its start is known here, and
// with it the blocks between bp and be that its first L bytes reach into.  A line inside one block is found when that block is staged.
__global__ __launch_bounds__(256)
void lineat_locate_kernel(const fourmc_image_entry* __restrict__ ent, uint32_t nb, uint64_t total, const fourmc_image_line_entry* __restrict__ index,
                          const uint64_t* __restrict__ lines, uint32_t n, uint32_t L, fourmc_lineat_req* __restrict__ req,
                          uint32_t* __restrict__ flags, uint32_t* __restrict__ tlen, int32_t* __restrict__ status)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = lines[i], E = index[nb].ends_before;
    tlen[i] = 0;
    fourmc_lineat_req q = {};
    if (k > E || total == 0 || nb == 0) { status[i] = -3; req[i] = q; return; }
    if (k == E) {                                                 // the final unterminated line, if there is one: the last block says
        uint32_t l = nb;
        while (l > 1 && ent[l - 1].usize == 0) l--;
        q.be = l - 1; q.je = kNone;
    } else {
        q.be = holder(index, nb, k); q.je = rank32(k - min(k, index[q.be].ends_before));
    }
    if (k) {
        q.bp = min(holder(index, nb, k - 1), q.be); q.js = rank32(k - 1 - min(k - 1, index[q.bp].ends_before));
        q.start = q.be > q.bp ? ent[q.bp].data_off + min(index[q.bp].flags >> 8, ent[q.bp].usize) : ~uint64_t(0);
    }
    flags[q.bp] = 1; flags[q.be] = 1;
    if (L) for (uint32_t j = q.bp + 1; j < q.be && ent[j].data_off < q.start + L; j++) if (ent[j].usize) flags[j] = 1;
    req[i] = q; status[i] = 0;
}

__device__ __forceinline__ void wave_fill(uint8_t* __restrict__ dst, uint32_t from, uint32_t to, uint8_t pad, uint32_t lane)
{ for (uint32_t x = from + lane; x < to; x += 64) dst[x] = pad; }

// a wave per request: the rows of the refused ones are all pad
__global__ __launch_bounds__(64 * kWaves)
void lineat_refuse_kernel(const int32_t* __restrict__ status, uint32_t n, uint8_t* __restrict__ rows, uint32_t row_bytes, uint8_t pad)
{
    const uint32_t i = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= n || status[i] != -3) return;
    wave_fill(rows + uint64_t(i) * row_bytes, 0, row_bytes, pad, threadIdx.x & 63);
}

// One workgroup: the marked blocks in ascending order.
__global__ __launch_bounds__(1024)
void lineat_compact_kernel(const uint32_t* __restrict__ flags, uint32_t nb, uint32_t* __restrict__ list, fourmc_lineat_counts* __restrict__ counts)
{
    __shared__ uint32_t wsum[16];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    uint32_t base = 0;
    for (uint64_t i0 = 0; i0 < nb; i0 += 1024) {
        const uint64_t i = i0 + t;
        const bool f = i < nb && flags[i] != 0;
        const unsigned long long bal = __ballot(f);
        if (lane == 0) wsum[w] = uint32_t(__popcll(bal));
        __syncthreads();
        uint32_t off = base, all = 0;
        for (uint32_t j = 0; j < 16; j++) { if (j < w) off += wsum[j]; all += wsum[j]; }
        if (f) list[off + uint32_t(__popcll(bal & ((1ull << lane) - 1)))] = uint32_t(i);
        base += all;
        __syncthreads();
    }
    if (t == 0) counts->needed = base;
}

// one wave per tile of every slot of the round; tiles behind a block's end count nothing
__global__ __launch_bounds__(64 * kWaves)
void lineat_tiles_kernel(const uint8_t* __restrict__ stage, uint64_t stride, const fourmc_image_entry* __restrict__ ent,
                         const uint32_t* __restrict__ list, uint32_t* __restrict__ tcnt)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t tile = blockIdx.x * kWaves + (threadIdx.x >> 6), slot = blockIdx.y;
    if (tile >= kSlotTiles) return;
    const Span sp(stage + uint64_t(slot) * stride, ent[list[slot]].usize);
    const uint32_t k = uint64_t(tile) * kTileChunks < sp.nchunks ? lines_count_tile(sp, tile, lane) : 0u;
    if (lane == 0) tcnt[slot * kSlotTiles + tile] = k;
}

// The j-th (from 0) line end of the block staged at d, taken by itself, by its tile counts: its offset, or kNone when the block
// has no more than j.  two: the end is the LF of a CR LF that lies inside the block.  Every lane gets the same answer.
__device__ __forceinline__ uint32_t select_end(const uint8_t* __restrict__ d, uint32_t usize, const uint32_t* __restrict__ tc, uint32_t j,
                                               uint32_t lane, uint32_t& two)
{
    const Span sp(d, usize);
    const uint32_t ntiles = uint32_t((sp.nchunks + kTileChunks - 1) / kTileChunks);
    uint32_t run = 0, tile = kNone;
    for (uint32_t t0 = 0; t0 < ntiles; t0 += 64) {
        const uint32_t c = t0 + lane < ntiles ? tc[t0 + lane] : 0u;
        const uint32_t incl = scan_add(c);
        const unsigned long long hit = __ballot(run + incl > j);
        if (hit) {
            const int l = __builtin_ctzll(hit);
            tile = t0 + uint32_t(l);
            j -= run + uint32_t(__shfl(int(incl - c), l));
            break;
        }
        run += wave_total(incl);
    }
    if (tile == kNone) return kNone;
    const uint32_t c0 = tile * kTileChunks + lane;
    run = 0;
    for (uint32_t i = 0; i < kSteps; i++) {
        const uint32_t c = c0 + 64 * i;
        uint32_t tw;
        const uint32_t m = step_ends<true>(sp, c, clean_chunk(sp, c), lane, tw);
        const uint32_t k = __popc(m), incl = scan_add(k);
        const unsigned long long hit = __ballot(run + incl > j);
        if (hit) {
            const int l = __builtin_ctzll(hit);
            uint32_t mm = m;
            const uint32_t r = min(j - (run + incl - k), 15u);       // the rank inside the mask (only lane l's is meant)
            for (uint32_t x = 0; x < r; x++) mm &= mm - 1;
            const uint32_t bit = mm ? uint32_t(__builtin_ctz(mm)) : 0u;
            two = uint32_t(__shfl(int((tw >> bit) & 1u), l));
            return uint32_t(__shfl(int(16 * c + bit), l));
        }
        run += wave_total(incl);
    }
    return kNone;
}

// this round's slot of block b
__device__ __forceinline__ uint32_t slot_of(const uint32_t* __restrict__ list, uint32_t m, uint32_t b)
{
    uint32_t lo = 0, hi = m;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (list[mid] < b) lo = mid + 1; else hi = mid; }
    return lo;                                                    // the first slot whose block is >= b; m: none
}

// One wave per request that is still open (status 0).  With the round's blocks list[0, m), ascending:
//   bp staged and the start not known: the start is behind end js of bp;
//   be staged: the end is end je of be, or the content's end; the text length, the pad and the status;
//   every staged block between bp and be: the piece of the first `cut` text bytes that lies in it goes to the row, cut = L until the
//   round of be says how long the text is.  A byte an earlier round copied behind the text's end (the CR of a CR LF over a seam) is
//   under that round's pad.
// A damaged block that the request needs ends it with -4, in whichever round it is met first.
__global__ __launch_bounds__(64 * kWaves)
void lineat_resolve_kernel(const uint8_t* __restrict__ stage, uint64_t stride, const fourmc_image_entry* __restrict__ ent,
                           const fourmc_image_line_entry* __restrict__ index, const uint32_t* __restrict__ list,
                           const fourmc_block* __restrict__ desc, uint32_t m, const uint32_t* __restrict__ tcnt,
                           fourmc_lineat_req* __restrict__ req, uint32_t n, uint32_t max_len, uint8_t* __restrict__ rows, uint32_t row_bytes,
                           uint8_t pad, uint32_t* __restrict__ tlen, int32_t* __restrict__ status)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (i >= n || status[i] != 0) return;
    fourmc_lineat_req q = req[i];
    if (q.be < list[0] || q.bp > list[m - 1]) return;
    uint8_t* __restrict__ row = rows + uint64_t(i) * row_bytes;
    const uint32_t sp_ = slot_of(list, m, q.bp), se = slot_of(list, m, q.be);
    const bool has_bp = sp_ < m && list[sp_] == q.bp, has_be = se < m && list[se] == q.be;
    if ((has_bp && block_bad(desc[sp_])) || (has_be && block_bad(desc[se]))) { if (lane == 0) status[i] = -4; return; }
    uint32_t two = 0;
    if (has_bp && q.start == ~uint64_t(0)) {
        const fourmc_image_entry e = ent[q.bp];
        const uint32_t p = select_end(stage + uint64_t(sp_) * stride, e.usize, tcnt + sp_ * kSlotTiles, q.js, lane, two);
        q.start = e.data_off + (p == kNone ? e.usize : p + 1);
        if (lane == 0) req[i].start = q.start;
    }
    if (q.start == ~uint64_t(0)) return;                         // an index that is not this image's: bp comes no more
    uint32_t cut = min(row_bytes, max_len), text = 0;
    if (has_be) {
        const fourmc_image_entry e = ent[q.be];
        const uint8_t* d = stage + uint64_t(se) * stride;
        uint64_t text_end = e.data_off + e.usize;
        if (q.je == kNone) {
            const uint32_t c = e.usize ? d[e.usize - 1] : 10u;
            if (c == 10u || c == 13u) {                           // the content ends with a line end: there is no line E
                wave_fill(row, 0, row_bytes, pad, lane);
                if (lane == 0) status[i] = -3;
                return;
            }
        } else {
            const uint32_t p = select_end(d, e.usize, tcnt + se * kSlotTiles, q.je, lane, two);
            if (p != kNone) {
                const uint32_t t = p == 0 && d[0] == 10u && (index[q.be].flags & 2u) ? 2u : 1u + two;
                text_end = e.data_off + p + 1 - min(uint64_t(t), e.data_off + p + 1);
            }
        }
        const uint64_t len = text_end > q.start ? text_end - q.start : 0;
        text = uint32_t(min(len, uint64_t(max_len)));
        cut = min(text, row_bytes);
    }
    for (uint32_t s = sp_; s < m && list[s] <= q.be; s++) {
        const fourmc_image_entry e = ent[list[s]];
        const uint64_t lo = max(q.start, e.data_off), hi = min(q.start + cut, e.data_off + e.usize);
        if (lo >= hi) continue;
        if (block_bad(desc[s])) { if (lane == 0) status[i] = -4; return; }
        const uint8_t* __restrict__ src = stage + uint64_t(s) * stride + (lo - e.data_off);
        uint8_t* __restrict__ dst = row + (lo - q.start);
        const uint32_t len = uint32_t(hi - lo);
        uint32_t x = lane;
        for (; x + 192 < len; x += 256) {                        // four loads in flight
            const uint8_t b0 = src[x], b1 = src[x + 64], b2 = src[x + 128], b3 = src[x + 192];
            dst[x] = b0; dst[x + 64] = b1; dst[x + 128] = b2; dst[x + 192] = b3;
        }
        for (; x < len; x += 64) dst[x] = src[x];
    }
    if (!has_be) return;
    wave_fill(row, cut, row_bytes, pad, lane);
    if (lane == 0) { tlen[i] = text; status[i] = 1; }
}

__global__ __launch_bounds__(256)
void lineat_served_kernel(const int32_t* __restrict__ status, uint32_t n, fourmc_lineat_counts* __restrict__ counts)
{
    uint32_t k = 0;
    for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += uint64_t(gridDim.x) * 256) k += status[i] == 1;
    for (int o = 32; o; o >>= 1) k += uint32_t(__shfl_xor(int(k), o));
    if ((threadIdx.x & 63) == 0 && k) atomicAdd(&counts->served, k);
}

} // namespace

extern "C" {

hipError_t fourmc_launch_lineat_desc(const fourmc_image_entry* d_ent, const uint32_t* d_list, uint32_t first, uint32_t m, uint64_t stride,
                                     fourmc_block* d_desc, hipStream_t s)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(lineat_desc_kernel, dim3((m + 255) / 256), dim3(256), 0, s, d_ent, d_list, first, m, stride, d_desc);
    return hipGetLastError();
}

hipError_t fourmc_launch_lineat_block_count(const void* d_stage, uint64_t stride, const fourmc_image_entry* d_ent, uint32_t first,
                                            const fourmc_block* d_desc, uint32_t m, fourmc_lineat_blk* d_blk, hipStream_t s)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(lineat_block_count_kernel, dim3(m), dim3(512), 0, s, static_cast<const uint8_t*>(d_stage), stride, d_ent, first,
                       d_desc, d_blk);
    return hipGetLastError();
}

hipError_t fourmc_launch_lineat_index_finish(const fourmc_image_entry* d_ent, const fourmc_lineat_blk* d_blk, uint32_t nb, uint64_t total,
                                             fourmc_image_line_entry* d_index, uint64_t cap, fourmc_lineat_sum* d_sum, hipStream_t s)
{
    hipLaunchKernelGGL(lineat_index_finish_kernel, dim3(1), dim3(1024), 0, s, d_ent, d_blk, nb, total, d_index, cap, d_sum);
    return hipGetLastError();
}

hipError_t fourmc_launch_lineat_fill(int32_t* d_status, uint32_t* d_text_len, uint32_t n, int32_t code, hipStream_t s)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(lineat_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_status, d_text_len, n, code);
    return hipGetLastError();
}

hipError_t fourmc_launch_lineat_locate(const fourmc_image_entry* d_ent, uint32_t nb, uint64_t total, const fourmc_image_line_entry* d_index,
                                       const uint64_t* d_lines, uint32_t n, uint32_t L, fourmc_lineat_req* d_req, uint32_t* d_flags,
                                       uint8_t* d_rows, uint32_t row_bytes, uint8_t pad, uint32_t* d_text_len, int32_t* d_status, hipStream_t s)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(lineat_locate_kernel, dim3((n + 255) / 256), dim3(256), 0, s, d_ent, nb, total, d_index, d_lines, n, L, d_req, d_flags,
                       d_text_len, d_status);
    if (hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(lineat_refuse_kernel, dim3((n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, d_status, n, d_rows, row_bytes, pad);
    return hipGetLastError();
}

hipError_t fourmc_launch_lineat_compact(const uint32_t* d_flags, uint32_t nb, uint32_t* d_list, fourmc_lineat_counts* d_counts, hipStream_t s)
{
    hipLaunchKernelGGL(lineat_compact_kernel, dim3(1), dim3(1024), 0, s, d_flags, nb, d_list, d_counts);
    return hipGetLastError();
}

hipError_t fourmc_launch_lineat_tiles(const void* d_stage, uint64_t stride, const fourmc_image_entry* d_ent, const uint32_t* d_list, uint32_t m,
                                      uint32_t* d_tcnt, hipStream_t s)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(lineat_tiles_kernel, dim3(kSlotTiles / kWaves, m), dim3(64 * kWaves), 0, s, static_cast<const uint8_t*>(d_stage), stride,
                       d_ent, d_list, d_tcnt);
    return hipGetLastError();
}

hipError_t fourmc_launch_lineat_resolve(const void* d_stage, uint64_t stride, const fourmc_image_entry* d_ent, const fourmc_image_line_entry* d_index,
                                        const uint32_t* d_list, const fourmc_block* d_desc, uint32_t m, const uint32_t* d_tcnt,
                                        fourmc_lineat_req* d_req, uint32_t n, uint32_t max_line_len, uint8_t* d_rows, uint32_t row_bytes,
                                        uint8_t pad, uint32_t* d_text_len, int32_t* d_status, hipStream_t s)
{
    if (!n || !m) return hipSuccess;
    hipLaunchKernelGGL(lineat_resolve_kernel, dim3((n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, static_cast<const uint8_t*>(d_stage),
                       stride, d_ent, d_index, d_list, d_desc, m, d_tcnt, d_req, n, max_line_len, d_rows, row_bytes, pad, d_text_len, d_status);
    return hipGetLastError();
}

hipError_t fourmc_launch_lineat_served(const int32_t* d_status, uint32_t n, fourmc_lineat_counts* d_counts, hipStream_t s)
{
    if (!n) return hipSuccess;
    const uint32_t most = (n + 255) / 256;
    hipLaunchKernelGGL(lineat_served_kernel, dim3(most < 1024 ? most : 1024), dim3(256), 0, s, d_status, n, d_counts);
    return hipGetLastError();
}

} // extern "C"
