// 4mc_amd/csrc/lz4hc_opt_encode.hip - batched LZ4 HC block encode at levels 9..12 on gfx950, BYTE-IDENTICAL to LZ4_compress_HC
// of the reference (native/lz4/lz4hc.c:958-973): level 9 is the hash chain with pattern analysis (:553-788, 256 attempts,
// :565), levels 10..12 the optimal parser (:1330-1626) over LZ4HC_FindLongerMatch (:1308-1326, pattern analysis and chain swap).
//
// ONE wavefront owns one block.  Unlike levels 1..8 (lz4hc_encode.hip, a builder wave running ahead of the parser), the chain walk
// here depends on the running `longest` (chain swap, :317-338) and on the parse (pattern analysis jumps, the optimal parser's
// minLen), so nothing can be prepared ahead: the wave runs the reference's serial parse (lz4hc_opt_core.h, shared with the CPU
// model tools/model/lz4hc_opt_model.c) with every lane holding the same values, and the lanes work together where the reference
// loops over independent items:
//   * insertion: positions [nextToUpdate, ip) 64 per step; lanes that share a hash chain to each other by lane distance
//     (the delta clamp at 65535 applied to the one that reads the old head), only the last of a hash becomes the head;
//   * LZ4_count / countBack / the pattern run counts: 16 bytes per lane per step;
//   * the chain-swap scan: 64 deltas read at once, the step/accel recurrence resolved from registers;
//   * the optimal parser's price updates: one table position per lane;
//   * sequence emission: literal copy and length bytes.
// The candidate-to-candidate walk stays serial.
//
// Memory: the 64 Ki x u16 chain ring (128 KiB) lives in LDS: every chain step is a dependent ds_read.  The 32 Ki x u32 hash heads
// (128 KiB) and the 4104 price records (16 B each) live in the block's HBM workspace slot.  Stores that one lane makes and another
// lane reads later (heads in the insert, records in the price updates) are followed by a workgroup fence; records written by the
// uniform code are written by every lane with the same value, so each lane reads back its own store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"
#include "devenc.h"

namespace {

#define HO_FN __device__ static __forceinline__
#include "lz4hc_opt_core.h"

constexpr int    kScore = 1024;
constexpr size_t kHeadBytes = size_t(4) << HO_HASHLOG;
constexpr size_t kOptBytes = (size_t(HO_OPT_RECS) * sizeof(HOpt) + 255) & ~size_t(255);
constexpr size_t kWorkBytes = kHeadBytes + kOptBytes;

struct __attribute__((packed, aligned(1))) U2B { uint16_t v; };

__device__ __forceinline__ uint32_t uni(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
__device__ __forceinline__ void wg_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); }

HO_FN uint32_t ho_ld32(const HO* c, uint32_t p) { return uni(ld4(c->src + p)); }
HO_FN uint32_t ho_ld16(const HO* c, uint32_t p) { return uni(reinterpret_cast<const U2B*>(c->src + p)->v); }
HO_FN uint32_t ho_chain(const HO* c, uint32_t idx) { return uni(c->chain[idx & 0xFFFFu]); }
HO_FN uint32_t ho_head(const HO* c, uint32_t h) { return uni(c->heads[h]); }

// LZ4HC_Insert (:120-141), 64 positions per step.  Inside a step the serial order only matters between positions with the same
// hash: each chains to its nearest predecessor in the step (a lane distance < 64, no clamp needed), the first one of a hash reads
// the old head (delta clamped to 65535), the last one becomes the new head.  Lanes that share a bucket are found with the LDS
// scoreboard, their exact predecessor with one ballot per distinct hash.
HO_FN void ho_insert(HO* c, uint32_t upto)
{
    const int lane = c->lane;
    while (c->ntu < upto) {
        const uint32_t pos = c->ntu + uint32_t(lane);
        const bool on = pos < upto;
        const uint32_t h = on ? ho_hash(ld4(c->src + pos)) : 0xFFFFFFFFu;
        int prev = -1; bool last = on;
        if (on) atomicMin(&c->score[h & (kScore - 1)], uint32_t(lane));
        const bool lost = on && c->score[h & (kScore - 1)] != uint32_t(lane);     // an earlier lane sits in my bucket
        if (on) c->score[h & (kScore - 1)] = 0xFFFFFFFFu;
        for (unsigned long long rem = __ballot(lost); rem; ) {
            const uint32_t hv = uint32_t(__builtin_amdgcn_readlane(int(h), __builtin_ctzll(rem)));
            const unsigned long long m = __ballot(h == hv);
            if (h == hv) {
                const unsigned long long lower = m & ~(~0ull << lane), upper = m & (~1ull << lane);
                if (lower) prev = 63 - __builtin_clzll(lower);
                last = upper == 0;
            }
            rem &= ~m;
        }
        if (on) {
            uint32_t delta;
            if (prev >= 0) delta = uint32_t(lane - prev);
            else { delta = pos + HO_IDX0 - c->heads[h]; if (delta > HO_MAXD) delta = HO_MAXD; }
            c->chain[pos & 0xFFFFu] = uint16_t(delta);
            if (last) c->heads[h] = pos + HO_IDX0;
        }
        wg_fence();                                              // the next step's first lane of a hash reads this head
        c->ntu = min(upto, c->ntu + 64u);
    }
}

// equal bytes at a / b (b < a), a stops at lim
HO_FN uint32_t ho_count(const HO* c, uint32_t a, uint32_t b, uint32_t lim)
{
    const uint8_t* s = c->src;
    const int lane = c->lane;
    uint32_t n = 0;
    for (;;) {
        if (a + 1024 <= lim) {
            const U16B x = *reinterpret_cast<const U16B*>(s + a + 16 * lane);
            const U16B y = *reinterpret_cast<const U16B*>(s + b + 16 * lane);
            const uint64_t d0 = x.a ^ y.a, d1 = x.b ^ y.b;
            const uint32_t eq = d0 ? uint32_t(__builtin_ctzll(d0) >> 3) : (d1 ? 8u + uint32_t(__builtin_ctzll(d1) >> 3) : 16u);
            const unsigned long long bad = __ballot(eq < 16);
            if (bad) { const int l = __builtin_ctzll(bad); return n + 16 * l + uint32_t(__builtin_amdgcn_readlane(int(eq), l)); }
            n += 1024; a += 1024; b += 1024;
        } else {
            const uint32_t i = a + uint32_t(lane);
            const bool same = i < lim && s[i] == s[b + lane];
            const unsigned long long bad = ~__ballot(same);
            if (bad) return n + uint32_t(__builtin_ctzll(bad));
            n += 64; a += 64; b += 64;
        }
    }
}

// equal bytes going back from a / b (exclusive), at most maxn (maxn <= b < a)
HO_FN uint32_t ho_count_back(const HO* c, uint32_t a, uint32_t b, uint32_t maxn)
{
    const uint8_t* s = c->src;
    const int lane = c->lane;
    uint32_t n = 0;
    for (;;) {
        const uint32_t j = n + uint32_t(lane) + 1;
        const bool same = j <= maxn && s[a - j] == s[b - j];
        const unsigned long long bad = ~__ballot(same);
        if (bad) return n + uint32_t(__builtin_ctzll(bad));
        n += 64;
    }
}

// bytes equal to `byte` from a on, stopping at lim (LZ4HC_countPattern with a one-byte pattern: the only pattern :345-346 lets in)
HO_FN uint32_t ho_run(const HO* c, uint32_t a, uint32_t byte, uint32_t lim)
{
    const uint8_t* s = c->src;
    const int lane = c->lane;
    const uint64_t rep = 0x0101010101010101ull * byte;
    uint32_t n = 0;
    if (a >= lim) return 0;
    for (;;) {
        if (a + 1024 <= lim) {
            const U16B x = *reinterpret_cast<const U16B*>(s + a + 16 * lane);
            const uint64_t d0 = x.a ^ rep, d1 = x.b ^ rep;
            const uint32_t eq = d0 ? uint32_t(__builtin_ctzll(d0) >> 3) : (d1 ? 8u + uint32_t(__builtin_ctzll(d1) >> 3) : 16u);
            const unsigned long long bad = __ballot(eq < 16);
            if (bad) { const int l = __builtin_ctzll(bad); return n + 16 * l + uint32_t(__builtin_amdgcn_readlane(int(eq), l)); }
            n += 1024; a += 1024;
        } else {
            const uint32_t i = a + uint32_t(lane);
            const bool same = i < lim && s[i] == byte;
            const unsigned long long bad = ~__ballot(same);
            if (bad) return n + uint32_t(__builtin_ctzll(bad));
            n += 64; a += 64;
        }
    }
}

// bytes equal to `byte` going back from a (exclusive) down to position 0 (LZ4HC_reverseCountPattern, one-byte pattern)
HO_FN uint32_t ho_run_back(const HO* c, uint32_t a, uint32_t byte)
{
    const uint8_t* s = c->src;
    const int lane = c->lane;
    uint32_t n = 0;
    for (;;) {
        const uint32_t j = n + uint32_t(lane) + 1;
        const bool same = j <= a && s[a - j] == byte;
        const unsigned long long bad = ~__ballot(same);
        if (bad) return n + uint32_t(__builtin_ctzll(bad));
        n += 64;
    }
}

// chain swap scan (:319-333): 64 deltas per LDS read, the step/accel recurrence walks them out of a register
HO_FN uint32_t ho_swap_scan(const HO* c, uint32_t matchIndex, int end, uint32_t* mcp)
{
    uint32_t dist = 1;
    int pos = 0, step = 1, accel = 1 << 4, base = -64;
    uint32_t d = 0;
    for (; pos < end; pos += step) {
        if (pos - base >= 64) { base = pos; d = c->chain[(matchIndex + uint32_t(base) + uint32_t(c->lane)) & 0xFFFFu]; }
        const uint32_t cd = uint32_t(__builtin_amdgcn_readlane(int(d), pos - base));
        step = accel++ >> 4;
        if (cd > dist) { dist = cd; *mcp = uint32_t(pos); accel = 1 << 4; }
    }
    return dist;
}

HO_FN HOpt ho_opt_get(const HO* c, int i)
{
    const int4 v = *reinterpret_cast<const int4*>(c->opt + i);
    HOpt r; r.price = int(uni(uint32_t(v.x))); r.off = int(uni(uint32_t(v.y))); r.mlen = int(uni(uint32_t(v.z))); r.litlen = int(uni(uint32_t(v.w)));
    return r;
}
HO_FN void ho_opt_put(HO* c, int i, HOpt r) { *reinterpret_cast<int4*>(c->opt + i) = make_int4(r.price, r.off, r.mlen, r.litlen); }

// :1393-1416 - positions 0..3 literals, 4..matchML the first match; one position per lane
HO_FN void ho_opt_first(HO* c, int llen, int matchML, int off)
{
    wg_fence();                                                  // the previous parse's uniform stores land before these
    for (int p = c->lane; p <= matchML; p += 64) {
        int4 r;
        if (p < HO_MINMATCH) r = make_int4(ho_lit_price(llen + p), 0, 1, llen + p);
        else r = make_int4(ho_seq_price(llen, p), off, p, llen);
        *reinterpret_cast<int4*>(c->opt + p) = r;
    }
    wg_fence();
}

// :1465-1513 - the literal extensions cur+1..cur+3 and the match positions cur+4..cur+matchML are all distinct and read only
// opt[cur] / opt[cur - ll] (below them), and last_match_pos only changes at ml == matchML: one position per lane, in any order
HO_FN int ho_opt_match(HO* c, int cur, int matchML, int off, int last)
{
    const HOpt base = ho_opt_get(c, cur);
    const int before = (base.mlen == 1 && cur > base.litlen) ? ho_opt_get(c, cur - base.litlen).price : 0;
    int newlast = last;
    for (int k = 1 + c->lane; k <= matchML; k += 64) {
        const int pos = cur + k;
        const int4 old = *reinterpret_cast<const int4*>(c->opt + pos);
        if (k < HO_MINMATCH) {
            const int price = base.price - ho_lit_price(base.litlen) + ho_lit_price(base.litlen + k);
            if (price < old.x) *reinterpret_cast<int4*>(c->opt + pos) = make_int4(price, 0, 1, base.litlen + k);
        } else {
            int ll, price;
            if (base.mlen == 1) { ll = base.litlen; price = before + ho_seq_price(ll, k); }
            else { ll = 0; price = base.price + ho_seq_price(0, k); }
            if (pos > last + HO_TRAIL || price <= old.x) {
                if (k == matchML && last < pos) newlast = pos;
                *reinterpret_cast<int4*>(c->opt + pos) = make_int4(price, off, k, ll);
            }
        }
    }
    wg_fence();
    return int(__builtin_amdgcn_readlane(newlast, (matchML - 1) & 63));     // the lane that held k == matchML
}

// LZ4HC_encodeSequence (:467-548)
HO_FN int ho_emit(HO* c, uint32_t* ipp, uint32_t* anchorp, int ml, uint32_t match)
{
    const int lane = c->lane;
    const uint32_t ip = *ipp, anchor = *anchorp;
    const uint32_t lit = ip - anchor;
    const uint32_t token_pos = c->op;
    uint32_t op = token_pos + 1, tok;
    if (c->limited && int64_t(op) + lit / 255 + lit + (2 + 1 + HO_LASTLIT) > c->cap) return 1;
    if (lit >= 15) { tok = 0xF0; op += emit_len(c->dst + op, lit - 15, lane); }
    else tok = lit << 4;
    copy_bytes(c->dst + op, c->src + anchor, lit, lane);
    op += lit;
    const uint32_t off = ip - match;
    if (lane == 0) { c->dst[op] = uint8_t(off); c->dst[op + 1] = uint8_t(off >> 8); }
    op += 2;
    const uint32_t mcode = uint32_t(ml) - HO_MINMATCH;
    if (c->limited && int64_t(op) + mcode / 255 + (1 + HO_LASTLIT) > c->cap) return 1;
    if (mcode >= 15) { tok += 15; op += emit_len(c->dst + op, mcode - 15, lane); }
    else tok += mcode;
    if (lane == 0) c->dst[token_pos] = uint8_t(tok);
    c->op = op;
    *ipp = ip + uint32_t(ml);
    *anchorp = *ipp;
    return 0;
}

HO_FN int ho_last(HO* c, uint32_t anchor)
{
    const int lane = c->lane;
    const uint32_t run = c->n - anchor, add = (run + 255 - 15) / 255;
    uint32_t op = c->op;
    if (c->limited && int64_t(op) + 1 + add + run > c->cap) return 0;
    if (run >= 15) { if (lane == 0) c->dst[op] = 0xF0; op++; op += emit_len(c->dst + op, run - 15, lane); }
    else { if (lane == 0) c->dst[op] = uint8_t(run << 4); op++; }
    copy_bytes(c->dst + op, c->src + anchor, run, lane);
    return int(op + run);
}

__global__ __launch_bounds__(64)
void lz4hc_opt_encode_kernel(const uint8_t* __restrict__ src_base, uint8_t* dst_base, fourmc_block* blocks,
                             uint32_t nblocks, uint8_t* work_base, int level, int container_mode)
{
    __shared__ uint16_t chain[65536];
    __shared__ uint32_t score[kScore];
    const uint32_t b = blockIdx.x;
    if (b >= nblocks) return;
    const int lane = threadIdx.x;
    const fourmc_block blk = uniform_block(blocks[b]);
    const uint32_t n = blk.src_len;
    uint8_t* work = work_base + size_t(b) * kWorkBytes;
    HO c;
    c.src = src_base + blk.src_off; c.dst = dst_base + blk.dst_off; c.n = n;
    c.cap = container_mode ? (n ? int64_t(n) - 1 : 0) : int64_t(blk.dst_cap);     // (an empty block: 0, not -1; as every encoder)
    c.limited = c.cap < int64_t(n) + n / 255 + 16;              // LZ4_compressBound (lz4hc.c:945)
    c.chain = chain; c.score = score; c.lane = lane;
    c.heads = reinterpret_cast<uint32_t*>(work);
    c.opt = reinterpret_cast<HOpt*>(work + kHeadBytes);
    c.ntu = 0; c.op = 0;
    {   // LZ4HC_clearTables: heads 0, chain 0xFFFF
        uint4* h = reinterpret_cast<uint4*>(work);
        for (uint32_t i = lane; i < uint32_t(kHeadBytes / 16); i += 64) h[i] = make_uint4(0, 0, 0, 0);
        uint4* ch = reinterpret_cast<uint4*>(chain);
        for (uint32_t i = lane; i < 65536u * 2 / 16; i += 64) ch[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
        for (int i = lane; i < kScore; i += 64) score[i] = 0xFFFFFFFFu;
        wg_fence();
        __syncthreads();
    }
    int r = ho_compress(&c, level);
    if (container_mode && r <= 0) { copy_bytes(c.dst, c.src, n, lane); r = int(n); }
    if (lane == 0) blocks[b].result = r;
}

} // namespace

extern "C" size_t fourmc_lz4hc_opt_work_bytes(uint32_t n) { return size_t(n) * kWorkBytes; }

extern "C" hipError_t fourmc_launch_lz4hc_opt_encode(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                                     void* d_work, int level, int container_mode, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    if (level < 9 || level > 12) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lz4hc_opt_encode_kernel, dim3(n), dim3(64), 0, stream,
                       static_cast<const uint8_t*>(d_src), static_cast<uint8_t*>(d_dst), d_blocks, n,
                       static_cast<uint8_t*>(d_work), level, container_mode);
    return hipGetLastError();
}
