// 4mc_amd/csrc/lz4emit.h - sequence records of the exact LZ4 fast encoder (K2) and the routine that turns them into
// LZ4 bytes (native/lz4/lz4.c:1083-1200 token / literal length / literals / offset / match length, :1266-1293 last
// literals).  K2's parse writes one record per sequence and never touches the output; lz4_emit.hip writes the bytes
// after the parse, all records of a launch in parallel.  K2 itself uses the routine only when a block has more
// sequences than its record area holds (blocks above FOURMC_BLOCKSIZE): it drains the area into the output and goes on.
#ifndef FOURMC_LZ4EMIT_H
#define FOURMC_LZ4EMIT_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "devenc.h"

namespace {

// One record, 16 bytes: x = output position of the token, y = source position of the literals (the previous match's
// end), z = literal length, w = offset | kRecLast.  The match length is the next record's y - (y + z + 4); the last
// record of a block (kRecLast) is the last literals and has no match.
constexpr uint32_t kRecLast    = 0x80000000u;
constexpr uint32_t kRecRawCopy = 0xFFFFFFFFu;   // record count of a container block stored raw (it did not fit)
constexpr uint32_t kRecSlack   = 128;           // records one dense window can add, at most (each consumes >= 4 input bytes)

// Workspace of a launch of m blocks: m record counts, then m record areas of `reccap` records each.
__host__ __device__ __forceinline__ size_t lz4rec_count_bytes(uint32_t m) { return (size_t(m) * 4u + 255u) & ~size_t(255); }
__host__ __device__ __forceinline__ size_t lz4rec_area_bytes(uint32_t reccap) { return size_t(reccap) * 16u; }

struct __attribute__((packed, aligned(1))) U2B { uint16_t v; };
__device__ __forceinline__ U16B ld16u(const uint8_t* p) { return *reinterpret_cast<const U16B*>(p); }
__device__ __forceinline__ void st16u(uint8_t* p, U16B v) { *reinterpret_cast<U16B*>(p) = v; }
__device__ __forceinline__ void st8u(uint8_t* p, uint64_t v) { reinterpret_cast<U8B*>(p)->v = v; }
__device__ __forceinline__ void st4u(uint8_t* p, uint32_t v) { reinterpret_cast<U4B*>(p)->v = v; }
__device__ __forceinline__ void st2u(uint8_t* p, uint16_t v) { reinterpret_cast<U2B*>(p)->v = v; }
__device__ __forceinline__ uint16_t ld2u(const uint8_t* p) { return reinterpret_cast<const U2B*>(p)->v; }

// k bytes from s to d by one lane: 16-byte pieces, then 8 / 4 / 2 / 1 (exact: nothing outside [d, d+k) is written)
__device__ __forceinline__ void copy_lane(uint8_t* d, const uint8_t* s, uint32_t k)
{
    uint32_t j = 0;
    for (; j + 16 <= k; j += 16) st16u(d + j, ld16u(s + j));
    if (k & 8) { st8u(d + j, ld8(s + j)); j += 8; }
    if (k & 4) { st4u(d + j, ld4(s + j)); j += 4; }
    if (k & 2) { st2u(d + j, ld2u(s + j)); j += 2; }
    if (k & 1) d[j] = s[j];
}

// k bytes of 255 by one lane
__device__ __forceinline__ void fill_ff(uint8_t* d, uint32_t k)
{
    uint32_t j = 0;
    for (; j + 16 <= k; j += 16) st16u(d + j, U16B{~0ull, ~0ull});
    if (k & 8) { st8u(d + j, ~0ull); j += 8; }
    if (k & 4) { st4u(d + j, ~0u); j += 4; }
    if (k & 2) { st2u(d + j, 0xFFFF); j += 2; }
    if (k & 1) d[j] = 255;
}

// length continuation bytes of `rest` by one lane: rest/255 bytes of 255, then rest%255; returns their number
__device__ __forceinline__ uint32_t put_len(uint8_t* d, uint32_t rest)
{
    const uint32_t n255 = rest / 255;
    if (n255) fill_ff(d, n255);
    d[n255] = uint8_t(rest - n255 * 255);
    return n255 + 1;
}

// k bytes from s to d by NT threads (t = thread index): 16-byte pieces, four in flight per thread while they last
template <int NT>
__device__ __forceinline__ void copy_group(uint8_t* d, const uint8_t* s, uint32_t k, int t)
{
    constexpr uint32_t S = 16u * NT;
    uint32_t j = 16u * uint32_t(t);
    for (; j + 3 * S + 16 <= k; j += 4 * S) {
        const U16B a = ld16u(s + j), b = ld16u(s + j + S), c = ld16u(s + j + 2 * S), e = ld16u(s + j + 3 * S);
        st16u(d + j, a); st16u(d + j + S, b); st16u(d + j + 2 * S, c); st16u(d + j + 3 * S, e);
    }
    for (; j + 16 <= k; j += S) st16u(d + j, ld16u(s + j));
    if (j < k) copy_lane(d + j, s + j, k - j);          // the one thread whose piece runs past the end
}

// Writes the LZ4 bytes of records [i0, i0+64) ∩ [i0, cnt), one per lane, in a wavefront.  `tail` is the source position
// after the match of record cnt-1 when that record is not the last one (a drain inside the parse).  Literal runs up to
// 64 bytes are copied by their own lane, longer ones by the whole wavefront, one after the other.
__device__ __forceinline__ void emit_records(const uint4* rec, uint32_t i0, uint32_t cnt, uint32_t tail,
                                             const uint8_t* src, uint8_t* dst, int lane)
{
    const uint32_t i = i0 + uint32_t(lane);
    const bool act = i < cnt;
    uint4 r = make_uint4(0, 0, 0, kRecLast);
    uint32_t nxt = 0;
    if (act) { r = rec[i]; nxt = i + 1 < cnt ? rec[i + 1].y : tail; }
    const bool last = (r.w & kRecLast) != 0;
    const uint32_t lit = r.z, mcode = last ? 0u : nxt - r.y - lit - 4;
    uint32_t p = r.x;
    bool longlit = false;
    if (act) {
        dst[p++] = uint8_t((min(lit, 15u) << 4) | min(mcode, 15u));
        if (lit >= 15) p += put_len(dst + p, lit - 15);
        longlit = lit > 64;
        if (!longlit) copy_lane(dst + p, src + r.y, lit);
        if (!last) {
            const uint32_t q = p + lit;
            st2u(dst + q, uint16_t(r.w));
            if (mcode >= 15) put_len(dst + q + 2, mcode - 15);
        }
    }
    for (unsigned long long lng = __ballot(longlit); lng; lng &= lng - 1) {
        const int l = __builtin_ctzll(lng);
        const uint32_t lp = uint32_t(__builtin_amdgcn_readlane(int(p), l)), ls = uint32_t(__builtin_amdgcn_readlane(int(r.y), l));
        copy_group<64>(dst + lp, src + ls, uint32_t(__builtin_amdgcn_readlane(int(lit), l)), lane);
    }
}

} // namespace
#endif
