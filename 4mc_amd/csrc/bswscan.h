// 4mc_amd/csrc/bswscan.h - the two wave-level pieces of the write planner (bstream.hip) that the line packer (lines_pack.hip) uses
// too: tables cut into tiles of 64 entries, 64-bit sums per tile, and the search for the owner of a position among ascending firsts.
#ifndef FOURMC_BSWSCAN_H
#define FOURMC_BSWSCAN_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

constexpr uint32_t kBswTile = 64;                        // table entries per tile: one wave reads a tile in one step

// wave64 inclusive prefix sum of 64-bit values
__device__ __forceinline__ uint64_t scan_add64(uint64_t v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t up = uint64_t(__shfl_up((long long)v, o));
        if (lane >= o) v += up;
    }
    return v;
}

// the largest i in [0, n) with first[i * stride8] <= x, for a table of n + 1 ascending 64-bit values whose first is 0 and whose last
// is above x (entries of equal value are items that own nothing: the last of them owns x)
__device__ __forceinline__ uint32_t bsw_owner(const uint64_t* __restrict__ first, uint32_t stride8, uint32_t n, uint64_t x)
{
    uint32_t lo = 0, hi = n;                             // first[lo] <= x < first[hi]
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first[size_t(mid) * stride8] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

} // namespace
#endif
