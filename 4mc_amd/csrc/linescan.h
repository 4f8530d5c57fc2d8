// 4mc_amd/csrc/linescan.h — the device side of the 16-byte-chunk scans that records.hip and lineat.hip share: the wave prefix sum,
// the one-byte match masks, the line-end masks of Hadoop's default rule (ends16), the chunk view of a byte range (Span) and the
// wave's walk over one 16 KiB tile.  Device code only, every function inline; each .hip file that includes it gets its own copy
// inside its own unnamed namespace, so include it INSIDE that namespace.
#ifndef FOURMC_LINESCAN_H
#define FOURMC_LINESCAN_H

constexpr uint32_t kTileChunks = FOURMC_RECORDS_TILE / 16;     // 16-byte chunks of one wave's tile
constexpr uint32_t kSteps = kTileChunks / 64;                  // steps of 64 lanes x 16 bytes
constexpr uint32_t kWaves = 4;                                 // tiles per workgroup

// wave64 inclusive prefix sum (image.hip: scan_add)
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

// bit k: byte k of the word equals the pattern's byte.  x = w ^ pat has a zero byte there; bit 7 of each byte of t says "not
// zero" without a carry between bytes; the multiply gathers bits 0, 8, 16, 24 into bits 24..27 (no two products share a bit).
__device__ __forceinline__ uint32_t match4(uint32_t w, uint32_t pat)
{
    const uint32_t x = w ^ pat;
    const uint32_t t = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;
    return (((~t & 0x80808080u) >> 7) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t match16(const uint4& v, uint32_t pat)
{ return match4(v.x, pat) | (match4(v.y, pat) << 4) | (match4(v.z, pat) << 8) | (match4(v.w, pat) << 12); }

// d[0, len) as chunks: chunk c holds the bytes [16 c - head, 16 c - head + 16) of d
struct Span {
    const uint4* base;
    uint32_t head;          // bytes of chunk 0 before d[0]
    uint64_t end;           // head + len
    uint64_t nchunks;
    __host__ __device__ Span(const void* d, uint64_t len)
    {
        const uintptr_t p = reinterpret_cast<uintptr_t>(d);
        head = uint32_t(p & 15); base = reinterpret_cast<const uint4*>(p - head);
        end = head + len; nchunks = (end + 15) / 16;
    }
    // the bytes of chunk c < nchunks that are d's
    __device__ __forceinline__ uint32_t valid(uint64_t c) const
    {
        const uint64_t a = 16 * c;
        uint32_t m = 0xffffu;
        if (a < head) m = (m << (head - a)) & 0xffffu;
        if (end - a < 16) m &= 0xffffu >> (16 - (end - a));
        return m;
    }
    // a tile whose every chunk lies wholly inside d
    __device__ __forceinline__ bool inner(uint64_t tile) const
    { return (tile > 0 || head == 0) && (tile + 1) * uint64_t(FOURMC_RECORDS_TILE) <= end; }
    __device__ __forceinline__ uint32_t mask(uint64_t c, uint32_t pat) const
    { return c < nchunks ? match16(base[c], pat) & valid(c) : 0u; }
};

__device__ __forceinline__ uint32_t pattern(uint8_t delim) { return uint32_t(delim) * 0x01010101u; }

// ---- line ends by Hadoop's default rule: LF | (CR & ~(LF one byte further)) ------------------------------------------------
constexpr uint32_t kLF4 = 0x0a0a0a0au, kCR4 = 0x0d0d0d0du;
// bit 7 of byte k: byte k of x is zero (match4's test, before its gather)
__device__ __forceinline__ uint32_t zero_flags(uint32_t x)
{ return ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }
__device__ __forceinline__ uint32_t gather4(uint32_t z) { return ((z >> 7) * 0x01020408u) >> 24; }
__device__ __forceinline__ uint32_t gather16(uint32_t z0, uint32_t z1, uint32_t z2, uint32_t z3)
{ return gather4(z0) | (gather4(z1) << 4) | (gather4(z2) << 8) | (gather4(z3) << 12); }
// what a chunk shows its neighbours: bit 7 = its byte 0 is LF (the chunk below needs it for a CR in its byte 15) ...
__device__ __forceinline__ uint32_t lf_first(const uint4& v) { return zero_flags(v.x ^ kLF4) & 0x80u; }
// ... and bit 7 = its byte 15 is CR (the chunk above needs it for the terminator length of an LF in its byte 0)
__device__ __forceinline__ uint32_t cr_last(const uint4& v) { return zero_flags(v.w ^ kCR4) >> 24; }
// The line ends of one chunk, bit k for byte k.  The flags of LF and CR are combined per 32-bit word BEFORE the gather: a CR's
// flag is cleared by the LF flag one byte up, which for byte 3 of a word is byte 0 of the next word and for byte 15 is `nx`
// (bit 7: byte 0 of the next chunk is LF).  WITH_T: also `two`, the ends that are the LF of a CR LF (terminator length 2); an LF
// in byte 0 asks `pv` (bit 7: byte 15 of the chunk before is CR).  Count and write call this one function, so they cannot differ.
template <bool WITH_T>
__device__ __forceinline__ uint32_t ends16(const uint4& v, uint32_t nx, uint32_t pv, uint32_t& two)
{
    const uint32_t l0 = zero_flags(v.x ^ kLF4), l1 = zero_flags(v.y ^ kLF4), l2 = zero_flags(v.z ^ kLF4), l3 = zero_flags(v.w ^ kLF4);
    const uint32_t c0 = zero_flags(v.x ^ kCR4), c1 = zero_flags(v.y ^ kCR4), c2 = zero_flags(v.z ^ kCR4), c3 = zero_flags(v.w ^ kCR4);
    const uint32_t e0 = l0 | (c0 & ~((l0 >> 8) | (l1 << 24))), e1 = l1 | (c1 & ~((l1 >> 8) | (l2 << 24)));
    const uint32_t e2 = l2 | (c2 & ~((l2 >> 8) | (l3 << 24))), e3 = l3 | (c3 & ~((l3 >> 8) | (nx << 24)));
    if (WITH_T)
        two = gather16(l0 & ((c0 << 8) | pv), l1 & ((c1 << 8) | (c0 >> 24)), l2 & ((c2 << 8) | (c1 >> 24)), l3 & ((c3 << 8) | (c2 >> 24)));
    return gather16(e0, e1, e2, e3);
}
// bytes of a word whose bit in the low 4 bits of `m` is clear become 0, which is neither CR nor LF
__device__ __forceinline__ uint32_t keep4(uint32_t w, uint32_t m) { return w & ((((m & 15u) * 0x00204081u) & 0x01010101u) * 0xffu); }
// chunk c with the bytes that are not d's zeroed; all zero from nchunks on
__device__ __forceinline__ uint4 clean_chunk(const Span& sp, uint64_t c)
{
    uint4 v = {0, 0, 0, 0};
    if (c < sp.nchunks) {
        const uint32_t m = sp.valid(c);
        v = sp.base[c];
        v.x = keep4(v.x, m); v.y = keep4(v.y, m >> 4); v.z = keep4(v.z, m >> 8); v.w = keep4(v.w, m >> 12);
    }
    return v;
}
// One byte of d by its chunk position, 0 outside d.  The byte behind d's last byte is never read: a CR in the last position ends
// a line, which is what the caller's choice of the span's end (hi, or the content's end) says.
__device__ __forceinline__ uint32_t span_byte(const Span& sp, uint64_t at)
{ return at >= sp.head && at < sp.end ? uint32_t(reinterpret_cast<const uint8_t*>(sp.base)[at]) : 0u; }
// the line ends of chunk c, for one thread by itself (finish, tail find)
__device__ __forceinline__ uint32_t ends_of(const Span& sp, uint64_t c)
{
    if (c >= sp.nchunks) return 0u;
    uint32_t two;
    return ends16<false>(clean_chunk(sp, c), span_byte(sp, 16 * (c + 1)) == 10u ? 0x80u : 0u, 0u, two);
}

__device__ __forceinline__ bool block_bad(const fourmc_block& d) { return d.result < 0 || uint32_t(d.result) != d.dst_cap; }

// One wave step of the walk both passes make: lane l holds chunk c in `v` (the caller loads it as it lies in an inner tile and
// through clean_chunk in an edge tile; that is all the two differ in) and gets the LF flag of chunk c + 1's byte 0 from lane l + 1's registers.  Lane 63's neighbour is lane 0 of the next step, of the
// next tile or of another workgroup: it loads that one byte itself, so every seam is the same seam.  WITH_T: the CR flag of
// chunk c - 1's byte 15 comes up the same way, and lane 0 loads its byte.
template <bool WITH_T>
__device__ __forceinline__ uint32_t step_ends(const Span& sp, uint64_t c, const uint4& v, uint32_t lane, uint32_t& two)
{
    uint32_t nx = uint32_t(__shfl_down(int(lf_first(v)), 1)), pv = 0;
    if (lane == 63) nx = span_byte(sp, 16 * (c + 1)) == 10u ? 0x80u : 0u;
    if (WITH_T) {
        pv = uint32_t(__shfl_up(int(cr_last(v)), 1));
        if (lane == 0) pv = c && span_byte(sp, 16 * c - 1) == 13u ? 0x80u : 0u;
    }
    return ends16<WITH_T>(v, nx, pv, two);
}

// one wave over one tile: the line ends of its 16 KiB, in every lane
__device__ __forceinline__ uint32_t lines_count_tile(const Span& sp, uint64_t tile, uint32_t lane)
{
    const uint64_t c0 = tile * kTileChunks + lane;
    uint32_t k = 0, two;
    if (sp.inner(tile)) {
        for (uint32_t i = 0; i < kSteps; i += 4) {                 // 4 KiB of the wave in flight
            const uint4 v0 = sp.base[c0 + 64 * i], v1 = sp.base[c0 + 64 * (i + 1)];
            const uint4 v2 = sp.base[c0 + 64 * (i + 2)], v3 = sp.base[c0 + 64 * (i + 3)];
            k += __popc(step_ends<false>(sp, c0 + 64 * i, v0, lane, two)) + __popc(step_ends<false>(sp, c0 + 64 * (i + 1), v1, lane, two))
               + __popc(step_ends<false>(sp, c0 + 64 * (i + 2), v2, lane, two)) + __popc(step_ends<false>(sp, c0 + 64 * (i + 3), v3, lane, two));
        }
    } else {
        for (uint32_t i = 0; i < kSteps; i++) k += __popc(step_ends<false>(sp, c0 + 64 * i, clean_chunk(sp, c0 + 64 * i), lane, two));
    }
    for (int o = 32; o; o >>= 1) k += uint32_t(__shfl_xor(int(k), o));
    return k;
}

#endif
