// 4mc_amd/csrc/lines_pack.hip — lines in the readers' table layouts, gathered into the text a TextOutputFormat job writes
// (fourmc_gpu_lines_pack and the two line writers; include/fourmc_gpu.h has the writer rule).  Every output line j of an item is the
// piece text_j '\n' of len_j + 1 bytes; an item's packed text is its pieces in order, and its write table is len_j, 1 per line.
//
//   measure  one lane per output line, one wave per tile of 64 lines over all items (bstream.hip's tile pattern, its scan and its
//            search: bswscan.h): the pick, the length, the two checks, the piece size; the wave's 64-bit scan leaves every line's
//            offset inside its tile (8 bytes of scratch per line) and the tile's sum with two flag bits.  One workgroup per item
//            turns its tile sums into prefixes with a leading 0 and gives T and the verdict.  One wave then walks the items: _CAP,
//            each item's first chunk of the gather, and - for the writers, which own the staging - its place behind the item before.
//   table    the same tiles again, for the items that are OK: tile prefix + offset in the tile = the line's 64-bit offset in its
//            item's text, and from two neighbours the write table.  From here on only the scratch says where a line lies and how
//            long it is: the caller's tables are read again for the source position alone, and that is clamped to the text.
//   gather   output-centric: the packed text of the good items, seen from the 16-byte boundary below each item's first byte, is cut
//            into chunks of kLpChunk bytes, one workgroup of 256 each.  Two waves find the lines of the chunk's first and last byte
//            (tile prefixes, then the 64 offsets of one tile).  Every lane owns aligned 16-byte pieces of the output: it finds its
//            first byte's line between those two, and then either the piece lies inside one text - one 16-byte load at the source's
//            own alignment, one aligned 16-byte store - or it walks the lines byte by byte, placing the terminators it owns.  Pieces
//            cut by the item's ends are stored bytewise, so items may abut at any byte.
// A workgroup's cost is bounded by its chunk, whatever the lines are: a line of 4 MiB is 256 chunks, 200 000 lines of 40 bytes 500.
// Only vector stores and plain C++; no atomics across workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"
#include "devcopy.h"
#include "bswscan.h"

namespace {

constexpr uint32_t kLpChunk = 16384;                     // output bytes per workgroup of the gather
constexpr uint64_t kLpWriteBit = 1ull << 63;             // in a tile's sum, before the finish: a text length above 0x7FFFFFFF
constexpr uint64_t kLpLineBit = 1ull << 62;              // ... a line that cannot be read
constexpr uint64_t kLpBits = kLpWriteBit | kLpLineBit;

// the table line of output line j of an item; table_lines for a pick that names none
__device__ __forceinline__ uint64_t lp_pick(const fourmc_lines_src& src, const fourmc_lp_item& it, uint64_t j)
{
    const uint64_t k = src.d_pick ? src.d_pick[it.line_off + j] : it.line_off + j;
    return k < src.table_lines ? k : src.table_lines;
}

// where table line k's text starts, never beyond the text
__device__ __forceinline__ uint64_t lp_start(const fourmc_lines_src& src, uint64_t k)
{
    if (k >= src.table_lines) return src.text_bytes;
    const uint64_t st = src.d_starts ? src.d_starts[k] : k * src.row_bytes;
    return st < src.text_bytes ? st : src.text_bytes;
}

// one wave per tile of 64 output lines, over the tiles of all items: off[off0 + j] = the bytes of the tile's pieces in front of line
// j, sums[tile0 + i + 1 + tile] = the tile's bytes with the flag bits of its lines (a flagged line counts as no bytes)
__global__ __launch_bounds__(256)
void lp_tile_kernel(fourmc_lines_src src, const fourmc_lp_item* __restrict__ items, uint32_t n, uint64_t ntiles,
                    uint64_t* __restrict__ sums, uint64_t* __restrict__ off)
{
    const uint64_t gt = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gt >= ntiles) return;
    const uint32_t i = bsw_owner(&items[0].tile0, sizeof(fourmc_lp_item) / 8, n, gt);
    const fourmc_lp_item it = items[i];
    const uint64_t tl = gt - it.tile0, j = tl * kBswTile + uint64_t(lane);
    uint64_t piece = 0;
    bool bad_write = false, bad_line = false;
    if (j < it.n_lines) {
        const uint64_t k = lp_pick(src, it, j);
        if (k >= src.table_lines) bad_line = true;
        else {
            const uint32_t len = src.d_text_len[k];
            const uint64_t st = src.d_starts ? src.d_starts[k] : k * src.row_bytes;
            if (len > 0x7FFFFFFFu) bad_write = true;
            else if ((!src.d_starts && len > src.row_bytes) || st > src.text_bytes || len > src.text_bytes - st) bad_line = true;
            else piece = uint64_t(len) + 1;
        }
    }
    const uint64_t incl = scan_add64(piece, lane);
    if (j < it.n_lines) off[it.off0 + j] = incl - piece;
    const uint64_t total = uint64_t(__shfl((long long)incl, 63));
    const bool w = __ballot(bad_write) != 0, l = __ballot(bad_line) != 0;
    if (lane == 0) sums[it.tile0 + i + 1 + tl] = total | (w ? kLpWriteBit : 0) | (l ? kLpLineBit : 0);
}

// One workgroup per item: its tile sums become their inclusive 64-bit prefixes in place behind a leading 0, and the total and the
// flag bits give T and the verdict (_WRITE over _LINE).  Each thread owns a run of consecutive tiles, as in bsw_finish_kernel.
__global__ __launch_bounds__(1024)
void lp_finish_kernel(const fourmc_lp_item* __restrict__ items, uint64_t* __restrict__ sums, fourmc_lp_sum* __restrict__ out)
{
    __shared__ uint64_t part[1024];
    __shared__ uint32_t any_write, any_line;
    const uint32_t i = blockIdx.x, t = threadIdx.x;
    const fourmc_lp_item it = items[i];
    uint64_t* mine = sums + it.tile0 + i + 1;
    const uint64_t T = items[i + 1].tile0 - it.tile0, per = (T + 1023) / 1024;
    const uint64_t lo = per * t < T ? per * t : T, hi = lo + per < T ? lo + per : T;
    if (t == 0) { any_write = 0; any_line = 0; mine[-1] = 0; }
    __syncthreads();
    uint64_t acc = 0;
    bool w = false, l = false;
    for (uint64_t k = lo; k < hi; k++) { const uint64_t v = mine[k]; w |= (v & kLpWriteBit) != 0; l |= (v & kLpLineBit) != 0; acc += v & ~kLpBits; }
    if (w) any_write = 1;                                // every writer stores the same value
    if (l) any_line = 1;
    part[t] = acc;
    __syncthreads();
    for (uint32_t o = 1; o < 1024; o <<= 1) {
        const uint64_t add = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    uint64_t run = part[t] - acc;                        // exclusive: the tiles in front of this thread's run
    for (uint64_t k = lo; k < hi; k++) { run += mine[k] & ~kLpBits; mine[k] = run; }
    if (t == 0) {
        fourmc_lp_sum s = {};
        s.reason = any_write ? FOURMC_BSW_WRITE : any_line ? FOURMC_BSW_LINE : FOURMC_BSW_OK;
        s.bytes = s.reason == FOURMC_BSW_OK ? part[1023] : 0;
        out[i] = s;
    }
}

// One wave over the items in order.  mode 1: an item's place is its own packed_off, and a packed_cap below T is _CAP; mode 2: the
// item lies behind the good items before it, from byte 0 on (the writers' staging).  chunk0 = the first gather chunk of the item,
// counted over all items that are OK; out[n] holds the totals.  base16: the low four address bits of the packed buffer.
__global__ __launch_bounds__(64)
void lp_place_kernel(const fourmc_lp_item* __restrict__ items, uint32_t n, int mode, uint32_t base16, fourmc_lp_sum* __restrict__ out)
{
    const int lane = threadIdx.x;
    uint64_t bytes0 = 0, chunk0 = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
        const uint32_t i = i0 + uint32_t(lane);
        uint64_t T = 0, cap = 0, at = 0;
        int32_t reason = FOURMC_BSW_OK;
        if (i < n) {
            const fourmc_lp_item it = items[i];
            T = out[i].bytes; reason = out[i].reason; cap = it.packed_cap; at = it.packed_off;
            if (mode == 1 && reason == FOURMC_BSW_OK && cap < T) reason = FOURMC_BSW_CAP;
        }
        const uint64_t good = reason == FOURMC_BSW_OK ? T : 0;
        const uint64_t incl = scan_add64(good, lane);
        if (mode == 2) at = bytes0 + incl - good;
        const uint64_t head = (uint64_t(base16) + at) & 15;
        const uint64_t chunks = good ? (head + good + kLpChunk - 1) / kLpChunk : 0;
        const uint64_t cincl = scan_add64(chunks, lane);
        if (i < n) { out[i].reason = reason; out[i].packed_off = at; out[i].chunk0 = chunk0 + cincl - chunks; }
        bytes0 += uint64_t(__shfl((long long)incl, 63));
        chunk0 += uint64_t(__shfl((long long)cincl, 63));
    }
    if (lane == 0) { fourmc_lp_sum s = {}; s.bytes = bytes0; s.packed_off = bytes0; s.chunk0 = chunk0; out[n] = s; }
}

// The tiles again, for the items that are OK: off[off0 + j] becomes line j's offset in the item's text (entry n_lines: T), and the
// write table gets len_j, 1 - the length from two neighbouring offsets, so that table and text cannot disagree
__global__ __launch_bounds__(256)
void lp_table_kernel(const fourmc_lp_item* __restrict__ items, const fourmc_lp_sum* __restrict__ sums, uint32_t n, uint64_t ntiles,
                     const uint64_t* __restrict__ prefix, uint64_t* __restrict__ off, uint32_t* __restrict__ writes)
{
    const uint64_t gt = uint64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (gt >= ntiles) return;
    const uint32_t i = bsw_owner(&items[0].tile0, sizeof(fourmc_lp_item) / 8, n, gt);
    if (sums[i].reason != FOURMC_BSW_OK) return;
    const fourmc_lp_item it = items[i];
    const uint64_t* P = prefix + it.tile0 + i;
    const uint64_t tl = gt - it.tile0, j = tl * kBswTile + uint64_t(lane);
    const bool valid = j < it.n_lines;
    const uint64_t full = valid ? P[tl] + off[it.off0 + j] : 0;
    const uint64_t down = uint64_t(__shfl_down((long long)full, 1));
    if (!valid) return;
    const uint64_t next = lane < 63 && j + 1 < it.n_lines ? down : P[tl + 1];
    off[it.off0 + j] = full;
    if (j + 1 == it.n_lines) off[it.off0 + it.n_lines] = next;
    if (writes) {
        uint32_t* w = writes + it.writes_off + 2 * j;
        w[0] = uint32_t(next - full - 1); w[1] = 1;
    }
}

// One workgroup per chunk (see the head of the file).  O: the item's n_lines + 1 offsets; P: its tile prefixes with the leading 0.
__global__ __launch_bounds__(256)
void lp_gather_kernel(fourmc_lines_src src, const fourmc_lp_item* __restrict__ items, const fourmc_lp_sum* __restrict__ sums, uint32_t n,
                      const uint64_t* __restrict__ prefix, const uint64_t* __restrict__ off, uint8_t* __restrict__ packed)
{
    __shared__ uint64_t ends[2];
    const uint32_t i = bsw_owner(&sums[0].chunk0, sizeof(fourmc_lp_sum) / 8, n, blockIdx.x);
    const fourmc_lp_item it = items[i];
    const fourmc_lp_sum sm = sums[i];
    const uint64_t T = sm.bytes, nl = it.n_lines;
    if (sm.reason != FOURMC_BSW_OK || T == 0 || nl == 0) return;
    uint8_t* out = packed + sm.packed_off;
    const uint64_t head = reinterpret_cast<uintptr_t>(out) & 15;
    const uint64_t v0 = (uint64_t(blockIdx.x) - sm.chunk0) * kLpChunk;     // counted from the 16-byte boundary below the item
    if (v0 >= head + T) return;
    const uint64_t t0 = v0 > head ? v0 - head : 0, t1 = v0 + kLpChunk - head < T ? v0 + kLpChunk - head : T;
    const uint64_t* O = off + it.off0;
    const uint64_t* P = prefix + it.tile0 + i;
    const uint32_t tiles = uint32_t((nl + kBswTile - 1) / kBswTile);
    const uint32_t t = threadIdx.x;
    const int lane = t & 63;
    if (t < 128) {                                       // wave 0: the line of the chunk's first byte; wave 1: of its last
        const uint64_t x = t < 64 ? t0 : t1 - 1;
        const uint64_t tl = bsw_owner(P, 1, tiles, x);
        const uint64_t e = tl * kBswTile + uint64_t(lane);
        const uint32_t k = uint32_t(__popcll(__ballot(e < nl && O[e] <= x)));
        if (lane == 0) ends[t >> 6] = tl * kBswTile + (k ? k - 1 : 0);
    }
    __syncthreads();
    const uint64_t ja = ends[0], jb = ends[1] < nl ? ends[1] : nl - 1;
    const uint8_t* text = static_cast<const uint8_t*>(src.d_text);
    for (uint32_t q = 0; q < kLpChunk / 16 / 256; q++) {
        const uint64_t pv = v0 + 16ull * (q * 256 + t);
        if (pv + 16 <= head || pv >= head + T) continue;
        const uint64_t lo = pv > head ? pv - head : 0;   // the piece's first byte that belongs to the item
        const bool whole = pv >= head && pv + 16 <= head + T;
        uint64_t a = ja, b = jb + 1;                     // O[a] <= lo < O[b]
        while (b - a > 1) {
            const uint64_t mid = a + (b - a) / 2;
            if (O[mid] <= lo) a = mid; else b = mid;
        }
        uint64_t j = a, cur = O[j], nxt = O[j + 1];
        uint64_t start = lp_start(src, lp_pick(src, it, j));
        if (whole && lo + 16 < nxt) {                    // sixteen bytes of one text
            const uint64_t s = start + (lo - cur);
            if (s + 16 <= src.text_bytes) {
                *reinterpret_cast<uint4*>(out + lo) = ld16u(text + s);
                continue;
            }
        }
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const uint64_t vp = pv + uint64_t(k);
            uint32_t byte = 0;
            if (vp >= head && vp < head + T) {
                const uint64_t pos = vp - head;
                while (pos >= nxt && j + 1 < nl) { j++; cur = nxt; nxt = O[j + 1]; start = lp_start(src, lp_pick(src, it, j)); }
                if (pos + 1 == nxt) byte = 0x0A;
                else { const uint64_t s = start + (pos - cur); byte = s < src.text_bytes ? text[s] : 0u; }
                if (!whole) out[pos] = uint8_t(byte);
            }
            w[k >> 2] |= byte << (8 * (k & 3));
        }
        if (whole) *reinterpret_cast<uint4*>(out + lo) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

} // namespace

extern "C" {

hipError_t fourmc_launch_lp_measure(const fourmc_lines_src* src, const fourmc_lp_item* d_items, uint32_t n, uint64_t ntiles, int mode,
                                    uint32_t base16, uint64_t* d_prefix, uint64_t* d_off, fourmc_lp_sum* d_sums, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    if (ntiles) hipLaunchKernelGGL(lp_tile_kernel, dim3(uint32_t((ntiles + 3) / 4)), dim3(256), 0, s, *src, d_items, n, ntiles, d_prefix, d_off);
    hipLaunchKernelGGL(lp_finish_kernel, dim3(n), dim3(1024), 0, s, d_items, d_prefix, d_sums);
    hipLaunchKernelGGL(lp_place_kernel, dim3(1), dim3(64), 0, s, d_items, n, mode, base16, d_sums);
    return hipGetLastError();
}

hipError_t fourmc_launch_lp_copy(const fourmc_lines_src* src, const fourmc_lp_item* d_items, const fourmc_lp_sum* d_sums, uint32_t n,
                                 uint64_t ntiles, uint64_t nchunks, const uint64_t* d_prefix, uint64_t* d_off, void* d_packed,
                                 uint32_t* d_writes, hipStream_t s)
{
    if (n == 0 || ntiles == 0) return hipSuccess;
    hipLaunchKernelGGL(lp_table_kernel, dim3(uint32_t((ntiles + 3) / 4)), dim3(256), 0, s, d_items, d_sums, n, ntiles, d_prefix, d_off, d_writes);
    if (d_packed && nchunks)
        hipLaunchKernelGGL(lp_gather_kernel, dim3(uint32_t(nchunks)), dim3(256), 0, s, *src, d_items, d_sums, n, d_prefix, d_off,
                           static_cast<uint8_t*>(d_packed));
    return hipGetLastError();
}

} // extern "C"
