// 4mc_amd/csrc/records.hip — the line records of a Hadoop split (fourmc_gpu_image_align_slices / _image_read_records).
//
// Alignment and planning are index work, one lane per slice or one lane in all: binary searches over the footer index
// (FourMcBlockIndex.java:92-173).  The hot path is the delimiter scan over the decoded bytes of a split, count - scan - write:
//   count   one wave per 16 KiB tile: 16 bytes per lane and step, a 16-bit match mask per lane, popcounts summed over the wave;
//   finish  one workgroup: the tile counts into their 64-bit exclusive prefix in place, the first delimiter (which a split that
//           does not start the file drops), the body blocks' verdict, and the ownership rule into the call's result;
//   write   the count kernel's walk again; a wave prefix of the popcounts (DPP) puts each lane's starts behind the tile's base.
// The data is read twice and every start written once.  A single pass with decoupled look-back would read it once, but its
// workgroups spin on their predecessors' flags; two plain launches need no forward-progress assumption, and the second read of
// a split costs far less than its decode did ("Line records").
// The bytes are addressed in 16-byte chunks from the destination rounded DOWN to 16: aligned loads never leave the pages the
// destination's own bytes lie in, and the bytes of the first and last chunk that are not the destination's are masked out.
//
// fourmc_gpu_image_read_lines cuts the same bytes by Hadoop's default LineReader rule (LF, lone CR, CR LF) with sibling kernels
// below "the scan, by lines": the same two passes over another mask, a terminator length per line from the write pass, and a
// third small pass over the table that turns it into the text length.  The one-byte kernels are as they were.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"

namespace {

#include "linescan.h"                                           // the chunk view, the masks, the wave's walk over a tile

// ------------------------------------------------------------------------------------------------------------- index work
// first block whose header offset is >= pos; n if none (findNextPosition, FourMcBlockIndex.java:87-104)
__device__ uint32_t next_block(const fourmc_image_entry* ent, uint32_t n, uint64_t pos)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ent[mid].image_off >= pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// alignSliceStartToIndex / alignSliceEndToIndex (FourMcBlockIndex.java:142-173), fileSize = image_bytes
__device__ __forceinline__ fourmc_image_slice align_slice(const fourmc_image_entry* __restrict__ ent, uint32_t n, uint64_t image_bytes,
                                                          fourmc_image_slice q)
{
    const uint32_t j = next_block(ent, n, q.end);
    q.split_end = j < n ? ent[j].image_off : image_bytes;
    uint32_t first = 0;
    bool kept = true;
    q.split_start = 0;
    if (q.start != 0) {
        first = next_block(ent, n, q.start);
        kept = first < n && ent[first].image_off < q.end;
        q.split_start = kept ? ent[first].image_off : ~uint64_t(0);
    }
    q.first_block = kept ? first : 0;
    q.block_count = kept ? j - first : 0;
    q.result = kept ? 1 : 0;
    return q;
}

// one lane per slice
__global__ __launch_bounds__(256)
void image_align_kernel(const fourmc_image_entry* __restrict__ ent, uint32_t n, uint64_t image_bytes,
                        fourmc_image_slice* __restrict__ slices, uint32_t nslices)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nslices) return;
    slices[i] = align_slice(ent, n, image_bytes, slices[i]);
}

// one lane per slice of any of the images
__global__ __launch_bounds__(256)
void images_align_kernel(const fourmc_image_entry* __restrict__ ent, const fourmc_images_tab* __restrict__ tab,
                         fourmc_images_slice* __restrict__ slices, uint32_t nslices)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nslices) return;
    const fourmc_images_tab t = tab[slices[i].image];
    if (t.nblocks) slices[i].s = align_slice(ent + t.ent0, t.nblocks, t.image_bytes, slices[i].s);
}

// the split's offsets into blocks and decoded offsets
__device__ __forceinline__ fourmc_records_plan plan_split(const fourmc_image_entry* __restrict__ ent, uint32_t n,
                                                          const fourmc_image_index_dev* __restrict__ idx, uint64_t split_start, uint64_t split_end)
{
    fourmc_records_plan p = {};
    p.total = idx->info.total_bytes;
    p.de = p.total; p.b1 = n;
    if (split_start != 0) {
        const uint32_t b = next_block(ent, n, split_start);
        if (b < n && ent[b].image_off == split_start) { p.b0 = b; p.ds = ent[b].data_off; }
        else p.code = -3;
    }
    if (split_end < idx->data_end) {
        const uint32_t b = next_block(ent, n, split_end);
        if (b < n && ent[b].image_off == split_end && split_end >= split_start) { p.b1 = b; p.de = ent[b].data_off; }
        else p.code = -3;
    }
    return p;
}

// one lane
__global__ __launch_bounds__(64)
void records_plan_kernel(const fourmc_image_entry* __restrict__ ent, uint32_t n, const fourmc_image_index_dev* __restrict__ idx,
                         uint64_t split_start, uint64_t split_end, fourmc_records_plan* __restrict__ plan)
{
    if (threadIdx.x != 0) return;
    *plan = plan_split(ent, n, idx, split_start, split_end);
}

__global__ __launch_bounds__(256)
void records_desc_kernel(const fourmc_image_entry* __restrict__ ent, uint32_t first, uint32_t count, uint64_t ds, int to_stage,
                         fourmc_block* __restrict__ desc)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= count) return;
    const fourmc_image_entry e = ent[first + b];
    fourmc_block d;
    d.src_off = e.image_off + 12; d.dst_off = to_stage ? 0 : e.data_off - ds; d.src_len = e.csize; d.dst_cap = e.usize; d.result = 0; d.xxh32 = e.xxh32;
    desc[b] = d;
}


// One workgroup over a staged block (16-byte aligned): its verdict, and its first delimiter, 16 KiB per step until one shows.
__global__ __launch_bounds__(1024)
void records_tail_find_kernel(const uint8_t* __restrict__ stage, const fourmc_block* __restrict__ desc,
                              const fourmc_image_entry* __restrict__ ent, uint32_t b, uint8_t delim, fourmc_records_tail* __restrict__ out)
{
    __shared__ uint32_t first;
    const fourmc_block d = *desc;
    const fourmc_image_entry e = ent[b];
    fourmc_records_tail r = {};
    r.data_off = e.data_off;
    if (block_bad(d)) {
        r.code = -4;
        if (threadIdx.x == 0) *out = r;
        return;
    }
    const Span sp(stage, e.usize);
    const uint32_t pat = pattern(delim);
    if (threadIdx.x == 0) first = ~0u;
    __syncthreads();
    for (uint64_t c0 = 0; c0 < sp.nchunks; c0 += 1024) {
        const uint64_t c = c0 + threadIdx.x;
        const uint32_t m = sp.mask(c, pat);
        if (m) atomicMin(&first, uint32_t(16 * c) + uint32_t(__builtin_ctz(m)));
        if (__syncthreads_or(m != 0)) break;
    }
    if (threadIdx.x == 0) {
        if (first != ~0u) { r.found = 1; r.hi = e.data_off + first + 1; }
        *out = r;
    }
}

// ------------------------------------------------------------------------------------------------------------- the scan
// one wave per tile: the delimiters of its 16 KiB
__global__ __launch_bounds__(64 * kWaves)
void records_count_kernel(const uint8_t* __restrict__ d, uint64_t len, uint32_t pat, uint64_t* __restrict__ cnt, uint64_t ntiles)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const Span sp(d, len);
    const uint64_t c0 = tile * kTileChunks + lane;
    uint32_t k = 0;
    if (sp.inner(tile)) {
        for (uint32_t i = 0; i < kSteps; i += 4) {                 // 4 KiB of the wave in flight
            const uint4 v0 = sp.base[c0 + 64 * i], v1 = sp.base[c0 + 64 * (i + 1)];
            const uint4 v2 = sp.base[c0 + 64 * (i + 2)], v3 = sp.base[c0 + 64 * (i + 3)];
            k += __popc(match16(v0, pat)) + __popc(match16(v1, pat)) + __popc(match16(v2, pat)) + __popc(match16(v3, pat));
        }
    } else {
        for (uint32_t i = 0; i < kSteps; i++) k += __popc(sp.mask(c0 + 64 * i, pat));
    }
    for (int o = 32; o; o >>= 1) k += uint32_t(__shfl_xor(int(k), o));
    if (lane == 0) cnt[tile] = k;
}

// One workgroup.  cnt[0, ntiles) becomes its exclusive prefix; then the ownership rule on the total, the first delimiter's
// position and the last byte (fourmc_gpu.h).  `body` = de - ds: a split that does not start the file owns something only when
// its first delimiter lies below it.  The start before the first record of a file and the end behind an unterminated last
// record have no delimiter in front of them: they are written here.
// LINES: the delimiters are the line ends of ends16 (pat unused), and the unterminated last line's terminator length, 0, goes
// to tlen; the one-byte kernel is the instantiation without, to the instruction what it was before the rule had a sibling.
template <bool LINES>
__device__ __forceinline__
void finish_body(const uint8_t* __restrict__ d, uint64_t len, uint32_t pat, uint64_t* __restrict__ cnt, uint64_t ntiles,
                 const fourmc_block* __restrict__ desc, uint32_t ndesc, int first_split, uint64_t ds, uint64_t body,
                 uint64_t* __restrict__ starts, uint64_t starts_cap, uint32_t* __restrict__ tlen, fourmc_records_state* __restrict__ st)
{
    __shared__ uint64_t wsum[16];
    __shared__ unsigned long long tile0;
    __shared__ uint32_t in_tile;
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) { tile0 = ~0ull; in_tile = ~0u; }
    bool bad = false;
    for (uint32_t i = t; i < ndesc; i += 1024) bad |= block_bad(desc[i]);
    const int any_bad = __syncthreads_or(bad);
    // each thread a contiguous run of tiles; a 64-bit wave scan and the 16 wave totals order the runs
    const uint64_t per = (ntiles + 1023) / 1024, a = min(ntiles, t * per), z = min(ntiles, a + per);
    uint64_t mine = 0, nz = ~0ull;
    for (uint64_t i = a; i < z; i++) { const uint64_t c = cnt[i]; if (c && nz == ~0ull) nz = i; mine += c; }
    if (nz != ~0ull) atomicMin(&tile0, (unsigned long long)nz);
    uint64_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) { const uint64_t v = uint64_t(__shfl_up((unsigned long long)incl, o)); if (int(lane) >= o) incl += v; }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint64_t run = 0, total = 0;
    for (uint32_t j = 0; j < 16; j++) { if (j < w) run += wsum[j]; total += wsum[j]; }
    run += incl - mine;
    for (uint64_t i = a; i < z; i++) { const uint64_t c = cnt[i]; cnt[i] = run; run += c; }
    // the first delimiter: in the first tile that counted one
    const Span sp(d, len);
    if (total) {
        const uint64_t c = uint64_t(tile0) * kTileChunks + t;
        const uint32_t m = LINES ? ends_of(sp, c) : sp.mask(c, pat);
        if (m) atomicMin(&in_tile, 16 * t + uint32_t(__builtin_ctz(m)));
    }
    __syncthreads();
    if (t != 0) return;
    fourmc_records_state s = {};
    s.r.base = ds;
    if (any_bad) { s.r.result = -4; *st = s; return; }
    const bool open_end = len > 0 && (LINES ? d[len - 1] != 10 && d[len - 1] != 13 : d[len - 1] != uint8_t(pat));   // an unterminated last record
    uint64_t lo = 0, records = 0;
    if (first_split) records = total + (open_end ? 1 : 0);
    else if (total) {
        const uint64_t p0 = uint64_t(tile0) * FOURMC_RECORDS_TILE + in_tile - sp.head;
        if (p0 < body) { lo = p0 + 1; records = total - 1 + (open_end ? 1 : 0); }
    }
    if (starts && records + 1 > starts_cap) {
        s.r.result = -5; s.r.data_off = records ? lo : 0; s.r.data_bytes = len; s.r.reserved = records;
    } else if (records == 0) {
        if (starts) starts[0] = 0;
    } else {
        s.r.result = int64_t(records); s.r.data_off = lo; s.r.data_bytes = len;
        if (starts) {
            s.write = 1; s.shift = first_split ? 1 : 0;
            if (first_split) starts[0] = 0;
            if (open_end) { starts[records] = len; if (LINES) tlen[records - 1] = 0; }
        }
    }
    *st = s;
}

__global__ __launch_bounds__(1024)
void records_finish_kernel(const uint8_t* __restrict__ d, uint64_t len, uint32_t pat, uint64_t* __restrict__ cnt, uint64_t ntiles,
                           const fourmc_block* __restrict__ desc, uint32_t ndesc, int first_split, uint64_t ds, uint64_t body,
                           uint64_t* __restrict__ starts, uint64_t starts_cap, fourmc_records_state* __restrict__ st)
{ finish_body<false>(d, len, pat, cnt, ntiles, desc, ndesc, first_split, ds, body, starts, starts_cap, nullptr, st); }

// the count kernel's walk; the start behind delimiter number r of d goes to starts[shift + r]
__global__ __launch_bounds__(64 * kWaves)
void records_write_kernel(const uint8_t* __restrict__ d, uint64_t len, uint32_t pat, const uint64_t* __restrict__ base, uint64_t ntiles,
                          const fourmc_records_state* __restrict__ st, uint64_t* __restrict__ starts)
{
    if (!st->write) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const Span sp(d, len);
    const uint64_t c0 = tile * kTileChunks + lane;
    uint64_t run = base[tile] + st->shift;
    const bool inner = sp.inner(tile);
    for (uint32_t i0 = 0; i0 < kSteps; i0 += 4) {
        uint32_t m[4];
        if (inner) {
            const uint4 v0 = sp.base[c0 + 64 * i0], v1 = sp.base[c0 + 64 * (i0 + 1)];
            const uint4 v2 = sp.base[c0 + 64 * (i0 + 2)], v3 = sp.base[c0 + 64 * (i0 + 3)];
            m[0] = match16(v0, pat); m[1] = match16(v1, pat); m[2] = match16(v2, pat); m[3] = match16(v3, pat);
        } else {
            for (uint32_t j = 0; j < 4; j++) m[j] = sp.mask(c0 + 64 * (i0 + j), pat);
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t k = __popc(m[j]);
            const uint32_t incl = scan_add(k);
            uint64_t o = run + (incl - k);
            const uint64_t at = 16 * (c0 + 64 * (i0 + j)) + 1 - sp.head;      // the start behind byte 0 of the chunk
            for (uint32_t mm = m[j]; mm; mm &= mm - 1) starts[o++] = at + uint32_t(__builtin_ctz(mm));
            run += wave_total(incl);
        }
    }
}

// ------------------------------------------------------------------------------------------------------ the scan, by lines
// one wave per tile
__global__ __launch_bounds__(64 * kWaves)
void lines_count_kernel(const uint8_t* __restrict__ d, uint64_t len, uint64_t* __restrict__ cnt, uint64_t ntiles)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const Span sp(d, len);
    const uint32_t k = lines_count_tile(sp, tile, lane);
    if (lane == 0) cnt[tile] = k;
}

__global__ __launch_bounds__(1024)
void lines_finish_kernel(const uint8_t* __restrict__ d, uint64_t len, uint64_t* __restrict__ cnt, uint64_t ntiles,
                         const fourmc_block* __restrict__ desc, uint32_t ndesc, int first_split, uint64_t ds, uint64_t body,
                         uint64_t* __restrict__ starts, uint64_t starts_cap, uint32_t* __restrict__ tlen, fourmc_records_state* __restrict__ st)
{ finish_body<true>(d, len, 0, cnt, ntiles, desc, ndesc, first_split, ds, body, starts, starts_cap, tlen, st); }

// The count kernel's walk.  Line end number r of d closes line shift + r - 1 and opens line shift + r: the start behind it goes
// to starts[shift + r] and its terminator's length (2 for the LF of a CR LF, else 1) to tlen[shift + r - 1]; the end a split that
// does not start the file drops (shift 0, r 0) closes a line the split does not own.
__device__ __forceinline__ void lines_write_tile(const Span& sp, uint64_t tile, uint32_t lane, uint64_t run,
                                                 uint64_t* __restrict__ starts, uint32_t* __restrict__ tlen)
{
    const uint64_t c0 = tile * kTileChunks + lane;
    const bool inner = sp.inner(tile);
    for (uint32_t i0 = 0; i0 < kSteps; i0 += 4) {
        uint32_t m[4], two[4];
        if (inner) {
            const uint4 v0 = sp.base[c0 + 64 * i0], v1 = sp.base[c0 + 64 * (i0 + 1)];
            const uint4 v2 = sp.base[c0 + 64 * (i0 + 2)], v3 = sp.base[c0 + 64 * (i0 + 3)];
            m[0] = step_ends<true>(sp, c0 + 64 * i0, v0, lane, two[0]); m[1] = step_ends<true>(sp, c0 + 64 * (i0 + 1), v1, lane, two[1]);
            m[2] = step_ends<true>(sp, c0 + 64 * (i0 + 2), v2, lane, two[2]); m[3] = step_ends<true>(sp, c0 + 64 * (i0 + 3), v3, lane, two[3]);
        } else {
            for (uint32_t j = 0; j < 4; j++) m[j] = step_ends<true>(sp, c0 + 64 * (i0 + j), clean_chunk(sp, c0 + 64 * (i0 + j)), lane, two[j]);
        }
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            const uint32_t k = __popc(m[j]);
            const uint32_t incl = scan_add(k);
            uint64_t o = run + (incl - k);
            const uint64_t at = 16 * (c0 + 64 * (i0 + j)) + 1 - sp.head;      // the start behind byte 0 of the chunk
            for (uint32_t mm = m[j]; mm; mm &= mm - 1) {
                const uint32_t bit = uint32_t(__builtin_ctz(mm));
                starts[o] = at + bit;
                if (o) tlen[o - 1] = 1 + ((two[j] >> bit) & 1u);
                o++;
            }
            run += wave_total(incl);
        }
    }
}

__global__ __launch_bounds__(64 * kWaves)
void lines_write_kernel(const uint8_t* __restrict__ d, uint64_t len, const uint64_t* __restrict__ base, uint64_t ntiles,
                        const fourmc_records_state* __restrict__ st, uint64_t* __restrict__ starts, uint32_t* __restrict__ tlen)
{
    if (!st->write) return;
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const Span sp(d, len);
    lines_write_tile(sp, tile, lane, base[tile] + st->shift, starts, tlen);
}

// tlen[i], the terminator's length of line i, into the length of its text, cut at max_len.  The line count is on the device
// only, so a fixed grid strides over it.
__device__ __forceinline__ void lines_len_body(const fourmc_records_state* __restrict__ st, const uint64_t* __restrict__ starts,
                                               uint32_t* __restrict__ tlen, uint32_t max_len)
{
    if (!st->write) return;
    const uint64_t n = uint64_t(st->r.result), step = uint64_t(gridDim.x) * 256;
    for (uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += step) {
        const uint64_t text = starts[i + 1] - starts[i] - tlen[i];
        tlen[i] = uint32_t(text < max_len ? text : max_len);
    }
}

__global__ __launch_bounds__(256)
void lines_len_kernel(const fourmc_records_state* __restrict__ st, const uint64_t* __restrict__ starts, uint32_t* __restrict__ tlen,
                      uint32_t max_len)
{ lines_len_body(st, starts, tlen, max_len); }

// records_tail_find_kernel by lines: the first line end of a staged block.  A CR in the block's last byte ends a line only if
// the next block does not open with LF, which this block cannot say unless it is the last (found = 2, hi behind the block).
// `pending`: the block BEHIND such a CR; its first byte decides (hi behind the LF, or still behind the CR), an empty block
// leaves the question open.  One workgroup of 1024.
__device__ __forceinline__
void lines_tail_find_body(const uint8_t* __restrict__ stage, const fourmc_block* __restrict__ desc,
                          const fourmc_image_entry* __restrict__ ent, uint32_t b, int last_block, int pending,
                          fourmc_records_tail* __restrict__ out)
{
    __shared__ uint32_t first;
    const fourmc_block d = *desc;
    const fourmc_image_entry e = ent[b];
    fourmc_records_tail r = {};
    r.data_off = e.data_off;
    if (block_bad(d)) {
        r.code = -4;
        if (threadIdx.x == 0) *out = r;
        return;
    }
    if (pending) {
        if (threadIdx.x == 0) {
            if (e.usize == 0) { r.found = 2; r.hi = e.data_off; }
            else { r.found = 1; r.hi = e.data_off + (stage[0] == 10 ? 1 : 0); }
            *out = r;
        }
        return;
    }
    const Span sp(stage, e.usize);
    if (threadIdx.x == 0) first = ~0u;
    __syncthreads();
    for (uint64_t c0 = 0; c0 < sp.nchunks; c0 += 1024) {
        const uint64_t c = c0 + threadIdx.x;
        const uint32_t m = ends_of(sp, c);
        if (m) atomicMin(&first, uint32_t(16 * c) + uint32_t(__builtin_ctz(m)));
        if (__syncthreads_or(m != 0)) break;
    }
    if (threadIdx.x == 0) {
        if (first != ~0u) {
            const bool open = !last_block && first == e.usize - 1 && stage[first] == 13;
            r.found = open ? 2 : 1; r.hi = e.data_off + first + 1;
        }
        *out = r;
    }
}

__global__ __launch_bounds__(1024)
void lines_tail_find_kernel(const uint8_t* __restrict__ stage, const fourmc_block* __restrict__ desc,
                            const fourmc_image_entry* __restrict__ ent, uint32_t b, int last_block, int pending,
                            fourmc_records_tail* __restrict__ out)
{ lines_tail_find_body(stage, desc, ent, b, last_block, pending, out); }

// ------------------------------------------------------------------------------------- many splits with one call, by lines
// fourmc_gpu_image_read_lines_batch: the kernels above with one more index.  A group of splits is a table of spans (kernels.h:
// fourmc_lines_span), each with its own destination, tables, descriptors and state; the tiles of all spans are numbered through,
// first[k] being span k's first tile, and a wave finds its span by a binary search over `first`.  Inside its span a wave is the
// single call's wave: the same Span, the same walk, the same seam loads, so a span's bytes are cut as the single call cuts them
// whatever lies in front of and behind its region.
template <class T>
__device__ __forceinline__ uint32_t span_of(const T* __restrict__ first, uint32_t ns, T key)     // the last k with first[k] <= key
{
    uint32_t lo = 0, hi = ns;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return uint32_t(__builtin_amdgcn_readfirstlane(int(lo - 1)));
}

// one lane per split
__global__ __launch_bounds__(256)
void lines_batch_plan_kernel(const fourmc_image_entry* __restrict__ ent, const fourmc_images_tab* __restrict__ tab,
                             const fourmc_image_index_dev* __restrict__ idx, const fourmc_split_req* __restrict__ req, uint32_t m,
                             fourmc_records_plan* __restrict__ plan)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const fourmc_split_req q = req[i];
    const fourmc_images_tab t = tab[q.image];
    plan[i] = plan_split(ent + t.ent0, t.nblocks, idx + q.image, q.split_start, q.split_end);
}

// one lane per searching split: its next tail block into its staging slot
__global__ __launch_bounds__(256)
void lines_batch_tail_desc_kernel(const fourmc_image_entry* __restrict__ ent, const fourmc_tail_job* __restrict__ job, uint32_t nj,
                                  uint64_t stride, fourmc_block* __restrict__ desc)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nj) return;
    const fourmc_image_entry e = ent[job[j].e];
    fourmc_block d;
    d.src_off = job[j].src_base + e.image_off + 12; d.dst_off = uint64_t(job[j].slot) * stride; d.src_len = e.csize; d.dst_cap = e.usize; d.result = 0; d.xxh32 = e.xxh32;
    desc[j] = d;
}

// one workgroup per searching split, over that split's slot
__global__ __launch_bounds__(1024)
void lines_batch_tail_find_kernel(const uint8_t* __restrict__ stage, uint64_t stride, const fourmc_block* __restrict__ desc,
                                  const fourmc_image_entry* __restrict__ ent, const fourmc_tail_job* __restrict__ job,
                                  fourmc_records_tail* __restrict__ out)
{
    const fourmc_tail_job q = job[blockIdx.x];
    lines_tail_find_body(stage + uint64_t(q.slot) * stride, desc + blockIdx.x, ent, q.e, q.last_block, q.pending, out + blockIdx.x);
}

// one lane per body block of the group: block b0 + i of its span, at its decoded offset in the span's region
__global__ __launch_bounds__(256)
void lines_batch_body_desc_kernel(const fourmc_image_entry* __restrict__ ent, const fourmc_lines_span* __restrict__ spans,
                                  const uint32_t* __restrict__ first, uint32_t ns, uint32_t ndesc, const uint8_t* __restrict__ d_dst,
                                  fourmc_block* __restrict__ desc)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= ndesc) return;
    uint32_t lo = 0, hi = ns;
    while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2; if (first[mid] <= i) lo = mid + 1; else hi = mid; }
    const fourmc_lines_span& sp = spans[lo - 1];
    const fourmc_image_entry e = ent[sp.e0 + (i - sp.desc0)];
    fourmc_block d;
    d.src_off = sp.src_base + e.image_off + 12; d.dst_off = uint64_t(sp.dst - d_dst) + (e.data_off - sp.ds); d.src_len = e.csize; d.dst_cap = e.usize;
    d.result = 0; d.xxh32 = e.xxh32;
    desc[i] = d;
}

// blockIdx.y: the span; its staged prefix to where it belongs.  The slot is 16-byte aligned: whole chunks when the destination is too.
__global__ __launch_bounds__(256)
void lines_batch_copy_kernel(const fourmc_lines_span* __restrict__ spans)
{
    const fourmc_lines_span& sp = spans[blockIdx.y];
    const uint64_t n = sp.copy_len;
    if (!n) return;
    const uint8_t* __restrict__ src = sp.stage;
    uint8_t* __restrict__ dst = sp.dst + sp.copy_off;
    const uint64_t t = uint64_t(blockIdx.x) * 256 + threadIdx.x, step = uint64_t(gridDim.x) * 256;
    uint64_t done = 0;
    if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const uint64_t nv = n / 16;
        for (uint64_t i = t; i < nv; i += step) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        done = nv * 16;
    }
    for (uint64_t i = done + t; i < n; i += step) dst[i] = src[i];
}

// one wave per tile of the group
__global__ __launch_bounds__(64 * kWaves)
void lines_batch_count_kernel(const fourmc_lines_span* __restrict__ spans, const uint64_t* __restrict__ first, uint32_t ns,
                              uint64_t* __restrict__ cnt, uint64_t ntiles)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const fourmc_lines_span& s = spans[span_of(first, ns, tile)];
    const Span sp(s.dst, s.len);
    const uint32_t k = lines_count_tile(sp, tile - s.tile0, lane);
    if (lane == 0) cnt[tile] = k;
}

// one workgroup per span: its counts into their prefix, its verdict, its state
__global__ __launch_bounds__(1024)
void lines_batch_finish_kernel(const fourmc_lines_span* __restrict__ spans, uint64_t* __restrict__ cnt,
                               const fourmc_block* __restrict__ desc, fourmc_records_state* __restrict__ st)
{
    const fourmc_lines_span& s = spans[blockIdx.x];
    finish_body<true>(s.dst, s.len, 0, cnt + s.tile0, s.ntiles, desc + s.desc0, s.ndesc, s.first_split, s.ds, s.body, s.starts,
                      s.lines_cap, s.tlen, st + blockIdx.x);
}

__global__ __launch_bounds__(64 * kWaves)
void lines_batch_write_kernel(const fourmc_lines_span* __restrict__ spans, const uint64_t* __restrict__ first, uint32_t ns,
                              const uint64_t* __restrict__ cnt, uint64_t ntiles, const fourmc_records_state* __restrict__ st)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t tile = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const uint32_t k = span_of(first, ns, tile);
    if (!st[k].write) return;
    const fourmc_lines_span& s = spans[k];
    const Span sp(s.dst, s.len);
    lines_write_tile(sp, tile - s.tile0, lane, cnt[tile] + st[k].shift, s.starts, s.tlen);
}

// blockIdx.y: the span
__global__ __launch_bounds__(256)
void lines_batch_len_kernel(const fourmc_lines_span* __restrict__ spans, const fourmc_records_state* __restrict__ st, uint32_t max_len)
{
    const fourmc_lines_span& s = spans[blockIdx.y];
    lines_len_body(st + blockIdx.y, s.starts, s.tlen, max_len);
}

} // namespace

extern "C" {

hipError_t fourmc_launch_image_align(const fourmc_image_entry* d_ent, uint32_t n, uint64_t image_bytes,
                                     fourmc_image_slice* d_slices, uint32_t nslices, hipStream_t s)
{
    if (!nslices) return hipSuccess;
    hipLaunchKernelGGL(image_align_kernel, dim3((nslices + 255) / 256), dim3(256), 0, s, d_ent, n, image_bytes, d_slices, nslices);
    return hipGetLastError();
}

hipError_t fourmc_launch_images_align(const fourmc_image_entry* d_ent, const fourmc_images_tab* d_tab, fourmc_images_slice* d_slices,
                                      uint32_t nslices, hipStream_t s)
{
    if (!nslices) return hipSuccess;
    hipLaunchKernelGGL(images_align_kernel, dim3((nslices + 255) / 256), dim3(256), 0, s, d_ent, d_tab, d_slices, nslices);
    return hipGetLastError();
}

hipError_t fourmc_launch_records_plan(const fourmc_image_entry* d_ent, uint32_t n, const fourmc_image_index_dev* d_idx,
                                      uint64_t split_start, uint64_t split_end, fourmc_records_plan* d_plan, hipStream_t s)
{
    hipLaunchKernelGGL(records_plan_kernel, dim3(1), dim3(64), 0, s, d_ent, n, d_idx, split_start, split_end, d_plan);
    return hipGetLastError();
}

hipError_t fourmc_launch_records_desc(const fourmc_image_entry* d_ent, uint32_t first, uint32_t count, uint64_t ds, int to_stage,
                                      fourmc_block* d_desc, hipStream_t s)
{
    if (!count) return hipSuccess;
    hipLaunchKernelGGL(records_desc_kernel, dim3((count + 255) / 256), dim3(256), 0, s, d_ent, first, count, ds, to_stage, d_desc);
    return hipGetLastError();
}

hipError_t fourmc_launch_records_tail_find(const void* d_stage, const fourmc_block* d_desc, const fourmc_image_entry* d_ent,
                                           uint32_t b, uint8_t delim, fourmc_records_tail* d_tail, hipStream_t s)
{
    hipLaunchKernelGGL(records_tail_find_kernel, dim3(1), dim3(1024), 0, s, static_cast<const uint8_t*>(d_stage), d_desc, d_ent, b,
                       delim, d_tail);
    return hipGetLastError();
}

uint64_t fourmc_records_tiles(const void* d, uint64_t len)
{
    if (!len) return 0;
    const Span sp(d, len);
    return (sp.nchunks + kTileChunks - 1) / kTileChunks;
}

hipError_t fourmc_launch_records_count(const void* d, uint64_t len, uint8_t delim, uint64_t* d_cnt, uint64_t ntiles, hipStream_t s)
{
    if (!ntiles) return hipSuccess;
    hipLaunchKernelGGL(records_count_kernel, dim3(uint32_t((ntiles + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s,
                       static_cast<const uint8_t*>(d), len, uint32_t(delim) * 0x01010101u, d_cnt, ntiles);
    return hipGetLastError();
}

hipError_t fourmc_launch_records_finish(const void* d, uint64_t len, uint8_t delim, uint64_t* d_cnt, uint64_t ntiles,
                                        const fourmc_block* d_desc, uint32_t ndesc, int first_split, uint64_t ds, uint64_t body,
                                        uint64_t* d_starts, uint64_t starts_cap, fourmc_records_state* d_st, hipStream_t s)
{
    hipLaunchKernelGGL(records_finish_kernel, dim3(1), dim3(1024), 0, s, static_cast<const uint8_t*>(d), len,
                       uint32_t(delim) * 0x01010101u, d_cnt, ntiles, d_desc, ndesc, first_split, ds, body, d_starts, starts_cap, d_st);
    return hipGetLastError();
}

hipError_t fourmc_launch_records_write(const void* d, uint64_t len, uint8_t delim, const uint64_t* d_cnt, uint64_t ntiles,
                                       const fourmc_records_state* d_st, uint64_t* d_starts, hipStream_t s)
{
    if (!ntiles) return hipSuccess;
    hipLaunchKernelGGL(records_write_kernel, dim3(uint32_t((ntiles + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s,
                       static_cast<const uint8_t*>(d), len, uint32_t(delim) * 0x01010101u, d_cnt, ntiles, d_st, d_starts);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_tail_find(const void* d_stage, const fourmc_block* d_desc, const fourmc_image_entry* d_ent,
                                         uint32_t b, int last_block, int pending, fourmc_records_tail* d_tail, hipStream_t s)
{
    hipLaunchKernelGGL(lines_tail_find_kernel, dim3(1), dim3(1024), 0, s, static_cast<const uint8_t*>(d_stage), d_desc, d_ent, b,
                       last_block, pending, d_tail);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_count(const void* d, uint64_t len, uint64_t* d_cnt, uint64_t ntiles, hipStream_t s)
{
    if (!ntiles) return hipSuccess;
    hipLaunchKernelGGL(lines_count_kernel, dim3(uint32_t((ntiles + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s,
                       static_cast<const uint8_t*>(d), len, d_cnt, ntiles);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_finish(const void* d, uint64_t len, uint64_t* d_cnt, uint64_t ntiles, const fourmc_block* d_desc,
                                      uint32_t ndesc, int first_split, uint64_t ds, uint64_t body, uint64_t* d_starts,
                                      uint64_t starts_cap, uint32_t* d_tlen, fourmc_records_state* d_st, hipStream_t s)
{
    hipLaunchKernelGGL(lines_finish_kernel, dim3(1), dim3(1024), 0, s, static_cast<const uint8_t*>(d), len, d_cnt, ntiles, d_desc,
                       ndesc, first_split, ds, body, d_starts, starts_cap, d_tlen, d_st);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_write(const void* d, uint64_t len, uint32_t max_line_len, const uint64_t* d_cnt, uint64_t ntiles,
                                     const fourmc_records_state* d_st, uint64_t* d_starts, uint32_t* d_tlen, hipStream_t s)
{
    if (ntiles) {
        hipLaunchKernelGGL(lines_write_kernel, dim3(uint32_t((ntiles + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s,
                           static_cast<const uint8_t*>(d), len, d_cnt, ntiles, d_st, d_starts, d_tlen);
        if (hipError_t e = hipGetLastError()) return e;
    }
    // one thread per line up to 2048 workgroups (a line of text per ~100 bytes: the grid is full from ~50 MB on), strides above
    const uint64_t most = len / 256 + 1;
    hipLaunchKernelGGL(lines_len_kernel, dim3(uint32_t(most < 2048 ? most : 2048)), dim3(256), 0, s, d_st, d_starts, d_tlen, max_line_len);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_batch_plan(const fourmc_image_entry* d_ent, const fourmc_images_tab* d_tab, const fourmc_image_index_dev* d_idx,
                                          const fourmc_split_req* d_req, uint32_t m, fourmc_records_plan* d_plan, hipStream_t s)
{
    if (!m) return hipSuccess;
    hipLaunchKernelGGL(lines_batch_plan_kernel, dim3((m + 255) / 256), dim3(256), 0, s, d_ent, d_tab, d_idx, d_req, m, d_plan);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_batch_tail_desc(const fourmc_image_entry* d_ent, const fourmc_tail_job* d_job, uint32_t nj,
                                               uint64_t stride, fourmc_block* d_desc, hipStream_t s)
{
    if (!nj) return hipSuccess;
    hipLaunchKernelGGL(lines_batch_tail_desc_kernel, dim3((nj + 255) / 256), dim3(256), 0, s, d_ent, d_job, nj, stride, d_desc);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_batch_tail_find(const void* d_stage, uint64_t stride, const fourmc_block* d_desc,
                                               const fourmc_image_entry* d_ent, const fourmc_tail_job* d_job, uint32_t nj,
                                               fourmc_records_tail* d_tail, hipStream_t s)
{
    if (!nj) return hipSuccess;
    hipLaunchKernelGGL(lines_batch_tail_find_kernel, dim3(nj), dim3(1024), 0, s, static_cast<const uint8_t*>(d_stage), stride, d_desc,
                       d_ent, d_job, d_tail);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_batch_body_desc(const fourmc_image_entry* d_ent, const fourmc_lines_span* d_spans,
                                               const uint32_t* d_first_desc, uint32_t ns, uint32_t ndesc, const void* d_dst,
                                               fourmc_block* d_desc, hipStream_t s)
{
    if (!ndesc) return hipSuccess;
    hipLaunchKernelGGL(lines_batch_body_desc_kernel, dim3((ndesc + 255) / 256), dim3(256), 0, s, d_ent, d_spans, d_first_desc, ns, ndesc,
                       static_cast<const uint8_t*>(d_dst), d_desc);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_batch_copy(const fourmc_lines_span* d_spans, uint32_t ns, uint64_t longest, hipStream_t s)
{
    if (!ns || !longest) return hipSuccess;
    const uint64_t most = (longest + 4095) / 4096;                 // 16 bytes per thread
    hipLaunchKernelGGL(lines_batch_copy_kernel, dim3(uint32_t(most < 64 ? most : 64), ns), dim3(256), 0, s, d_spans);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_batch_count(const fourmc_lines_span* d_spans, const uint64_t* d_first_tile, uint32_t ns,
                                           uint64_t* d_cnt, uint64_t ntiles, hipStream_t s)
{
    if (!ntiles) return hipSuccess;
    hipLaunchKernelGGL(lines_batch_count_kernel, dim3(uint32_t((ntiles + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s, d_spans,
                       d_first_tile, ns, d_cnt, ntiles);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_batch_finish(const fourmc_lines_span* d_spans, uint32_t ns, uint64_t* d_cnt, const fourmc_block* d_desc,
                                            fourmc_records_state* d_st, hipStream_t s)
{
    if (!ns) return hipSuccess;
    hipLaunchKernelGGL(lines_batch_finish_kernel, dim3(ns), dim3(1024), 0, s, d_spans, d_cnt, d_desc, d_st);
    return hipGetLastError();
}

hipError_t fourmc_launch_lines_batch_write(const fourmc_lines_span* d_spans, const uint64_t* d_first_tile, uint32_t ns,
                                           const uint64_t* d_cnt, uint64_t ntiles, uint64_t longest, uint32_t max_line_len,
                                           const fourmc_records_state* d_st, hipStream_t s)
{
    if (!ns) return hipSuccess;
    if (ntiles) {
        hipLaunchKernelGGL(lines_batch_write_kernel, dim3(uint32_t((ntiles + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, s, d_spans,
                           d_first_tile, ns, d_cnt, ntiles, d_st);
        if (hipError_t e = hipGetLastError()) return e;
    }
    // per span one thread per line at a line of text per ~32 bytes, up to 256 workgroups; strides above
    const uint64_t most = longest / 8192 + 1;
    hipLaunchKernelGGL(lines_batch_len_kernel, dim3(uint32_t(most < 256 ? most : 256), ns), dim3(256), 0, s, d_spans, d_st, max_line_len);
    return hipGetLastError();
}

} // extern "C"
