// 4mc_amd/csrc/lz4_par_encode.hip - K2p: the RATIO-TOLERANCE LZ4 block encoder (not the default: `lz4_encode.hip` reproduces the
// reference parse byte for byte and stays the encoder of the CLI, the JNI names and the headline figure).
//
// What it replaces is the same call as K2 (native/4mc.c:301, native/jniCompressor.c:91 -> native/lz4/lz4.c:1435 -> :910-1302),
// under north_star's clause "otherwise compression ratio is reported within a stated tolerance": the payload is ONE valid LZ4
// block that the reference's LZ4_decompress_safe (lz4.c:2345) decodes to the input, but not the reference's parse.  The
// reference parse is a chain (each table read depends on every earlier decision); this one has no chain longer than a window:
//   * a 4 MiB block is 64 segments of 64 KiB, one wavefront each, 18 waves per CU (an NENT x u16 table per wave in LDS:
//     8 KiB, + 512 bytes of staging).  A segment's matches stay inside the segment (offsets < 64 Ki by construction);
//   * a window is 64 consecutive positions, lane l <-> position wb + l.  EVERY position enters the table (the table does not
//     depend on the parse), in four groups of 16 lanes, a group reading before it writes, so that a lane sees the positions
//     of the groups before it - candidates 16 and more bytes back are never missed, nearer ones are picked up by the
//     lanes behind (the match extends);
//   * one candidate per position (the table's, or the position 1, 2 or 4 back when it holds the same 4 bytes), ONE 16-byte gather per lane (4 bytes before the candidate, 12 from it) against the lane's
//     own bytes (the window is loaded once as 22 dwords and handed out with ds_bpermute): match length 0..12 forwards and
//     0..4 backwards;
//   * a position is skipped when one of the next three positions holds a longer match (by 1, 2, 3 - what a lazy parser finds
//     one search at a time is a DPP shift here);
//   * a scalar walk takes the first eligible lane at or after the cursor: a match that reached the 12 bytes is extended by the
//     whole wave (256 bytes per step), the bytes behind it go back over pending literals, the sequence's bytes leave from the
//     lanes that hold them (literals: one byte store per lane; token, lengths and offset from scalars);
//   * the segments' sequences lie in a workspace; the stitch kernel adds the literals a segment ended with to the first
//     sequence of the next one that has a sequence, and writes the block's last literals (lz4.c:1265-1290 rules: last 5 bytes
//     literals, no match starting in the last 12) - one LZ4 block, no new format.
// `tools/model/lz4p_model.c` is the executable statement of the same rules (sizes on the S-mix: 2.2 % above the reference
// parse at NENT = 4096); `tests/test_gpu_lz4par_encode.py` holds the tolerance and the reference decoder's verdict.
// HBM traffic per block: n read (candidates re-read from L1/L2), csize written to the workspace, read and written once more by
// the stitch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"
#include "devenc.h"

#ifndef FOURMC_PAR_NENT
#define FOURMC_PAR_NENT 4096
#endif

namespace {

constexpr int      kSeg       = 65536;                 // bytes of a segment
constexpr int      kSegs      = 64;                    // segments of a block (what lies beyond goes out as literals)
constexpr int      kNent      = FOURMC_PAR_NENT;       // table entries per wave (u16): 8 KiB + 512 B of staging, 18 waves per CU
constexpr int      kFwd       = 12;                    // bytes compared forwards in the lanes (4 backwards)
constexpr uint32_t kSegStride = 66048;                 // workspace bytes of a segment: 65536 + 65536/255 + 16, rounded up to 256
constexpr int      kStage     = 512;                   // staging area of a wave: 256 bytes leave at a time, a sequence adds < 200
constexpr uint32_t kMetaBytes = kSegs * 8;             // {bytes written, literals left} per segment
static_assert((kNent * 2) % 16 == 0, "table is zeroed 16 bytes at a time");

__device__ __forceinline__ uint32_t U(uint32_t v) { return uint32_t(__builtin_amdgcn_readfirstlane(int(v))); }
__device__ __forceinline__ uint32_t rdl(uint32_t v, uint32_t l) { return uint32_t(__builtin_amdgcn_readlane(int(v), int(l))); }
__device__ __forceinline__ uint32_t bperm(uint32_t v, uint32_t srclane) { return uint32_t(__builtin_amdgcn_ds_bpermute(int(srclane << 2), int(v))); }
// lane l <- lane l + 1 (lane 63 <- 0)
__device__ __forceinline__ int next_lane(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x130, 0xf, 0xf, false); }
// index of the lowest set bit, 0xFFFFFFFF for 0 (what the instruction returns; `x ? ctz(x) : -1` costs a compare and a select more)
__device__ __forceinline__ uint32_t ffbl(uint32_t x) { uint32_t r; asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x)); return r; }

__device__ __forceinline__ uint4 ld16(const uint8_t* p)
{
    const U16B t = *reinterpret_cast<const U16B*>(p);
    return make_uint4(uint32_t(t.a), uint32_t(t.a >> 32), uint32_t(t.b), uint32_t(t.b >> 32));
}

struct SegMeta { uint32_t len, tail; };

__device__ __forceinline__ uint8_t* seg_area(uint8_t* work, uint32_t nblocks, uint32_t b, uint32_t k)
{ return work + size_t(nblocks) * kMetaBytes + (size_t(b) * kSegs + k) * kSegStride; }
__device__ __forceinline__ SegMeta* seg_meta(uint8_t* work, uint32_t b) { return reinterpret_cast<SegMeta*>(work + size_t(b) * kMetaBytes); }

// --------------------------------------------------------------------------------------------------------------- segments
// Sequence bytes collect in an LDS staging area and leave 256 bytes at a time (16 lanes x 16 bytes, aligned): a wave's loads and
// stores share one in-order counter, and a store per sequence in front of every candidate gather made each window wait for its
// stores to be acknowledged.
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return uint32_t(uintptr_t((const __attribute__((address_space(3))) void*)p)); }
// lanes of `mask` store the low byte of val at LDS address vaddr (the mask comes from scalars: no vector compare)
template <int OFF>
__device__ __forceinline__ void put_lanes(uint32_t vaddr, uint32_t val, unsigned long long mask)
{ asm volatile("s_mov_b64 exec, %0\n\tds_write_b8 %1, %2 offset:%3\n\ts_mov_b64 exec, -1" :: "s"(mask), "v"(vaddr), "v"(val), "i"(OFF) : "memory"); }
__device__ __forceinline__ uint32_t prev_lane(uint32_t v) { return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), 0x138, 0xf, 0xf, false)); }   // lane l <- lane l - 1 (lane 0 <- 0)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dppz(uint32_t v) { return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), CTRL, ROWMASK, 0xf, false)); }
__device__ __forceinline__ uint32_t scan_max(uint32_t v)       // inclusive prefix maximum over the wave
{
    v = max(v, dppz<0x111, 0xf>(v)); v = max(v, dppz<0x112, 0xf>(v)); v = max(v, dppz<0x114, 0xf>(v)); v = max(v, dppz<0x118, 0xf>(v));
    v = max(v, dppz<0x142, 0xa>(v)); v = max(v, dppz<0x143, 0xc>(v));
    return v;
}
__device__ __forceinline__ uint32_t scan_add_incl(uint32_t v)
{
    v += dppz<0x111, 0xf>(v); v += dppz<0x112, 0xf>(v); v += dppz<0x114, 0xf>(v); v += dppz<0x118, 0xf>(v);
    v += dppz<0x142, 0xa>(v); v += dppz<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ unsigned long long lane_range(int lo, int cnt)      // lanes [lo, lo + cnt), cnt 0..64
{ return (cnt >= 64 ? ~0ull : ((1ull << cnt) - 1)) << lo; }

struct Win { uint32_t prev4, cur0, cur1, cur2; int c; bool valid; uint4 gv; };

__global__ __launch_bounds__(64)
void lz4_par_segment_kernel(const uint8_t* __restrict__ src_base, const fourmc_block* __restrict__ blocks, uint32_t nblocks,
                            uint8_t* __restrict__ work)
{
    __shared__ __attribute__((aligned(16))) uint16_t tab[kNent];
    __shared__ __attribute__((aligned(16))) uint8_t stg[kStage];
    const int lane = threadIdx.x;
    const uint32_t gseg = blockIdx.x, b = gseg / kSegs, k = gseg % kSegs;
    if (b >= nblocks) return;
    const fourmc_block blk = uniform_block(blocks[b]);
    const uint8_t* in = src_base + blk.src_off;
    const int n = int(min(blk.src_len, 0x7E000000u));
    const int s0 = int(k) * kSeg;
    SegMeta* meta = seg_meta(work, b) + k;
    if (s0 >= n) { if (lane == 0) { meta->len = 0; meta->tail = 0; } return; }
    const int s1 = min(s0 + kSeg, n);
    uint8_t* out = seg_area(work, nblocks, b, k);
    for (int i = lane; i < kNent * 2 / 16; i += 64) reinterpret_cast<uint4*>(tab)[i] = make_uint4(0, 0, 0, 0);

    const int pmax = min(s1 - 4, n - 32);             // the last position that may start a match (reads stay inside the block)
    const int mend = min(s1, n - 5);                  // matches end at or before (lz4.c:1265: the last 5 bytes are literals)
    const uint32_t sh8 = uint32_t(lane & 3) * 8, j0 = uint32_t(lane) >> 2, lane8 = uint32_t(lane) * 8;
    const uint32_t sbase = lds_addr(stg), vstg = sbase + uint32_t(lane);
    uint32_t flushed = 0, pend = 0;                   // sequence bytes in the workspace / in the staging area
    int sp = s0;                                      // cursor: end of the last match = start of the pending literals
    uint32_t prevbyte = 0;                            // the previous window's byte of this lane

    // dword `lane` of [wb - 4, wb + 84)
    // (every lane loads, from a clamped address: a load the wave might skip would make the number of loads in flight unknown to
    // the compiler, and every wait a wait for all of them)
    const uint32_t lane4 = 4u * uint32_t(min(lane, 21));
    // The address is clamped into the block and nothing else: a lane that gets other bytes than its own that way is either one of
    // the block's first 4 positions looking back (their candidates are refused: c < 4) or lies behind pmax + 12.
    auto load_win = [&](int wb) -> uint32_t { return ld4(in + uint32_t(min(max(wb - 4 + int(lane4), 0), n - 4))); };
    // first half of a window: the lanes' bytes, the table, the candidate gather (nothing here depends on the parse)
    auto stage_a = [&](int wb, uint32_t wd) -> Win {
        Win w;
        const int p = wb + lane;
        const uint32_t d1 = bperm(wd, j0 + 1), d2 = bperm(wd, j0 + 2);
        w.cur0 = __builtin_amdgcn_alignbit(d2, d1, sh8);
        const bool act = p <= pmax;
        // (two 24-bit multiplies: full rate; a 32-bit multiply issues for four instructions' time and hashes no better here)
        const uint32_t hh = (uint32_t(__umul24(w.cur0, 0x9E3779u)) + uint32_t(__umul24(w.cur0 >> 8, 0x85EBCAu))) >> 16;   // (__umul24 returns int)
        const uint32_t ta = lds_addr(tab) + (((hh * uint32_t(kNent)) >> 16) << 1);
        // the table, four groups of 16 lanes, each group reading before it writes (LDS operations of a wave execute in order),
        // and the other three dwords the lane needs; one wait for all of it
        const unsigned long long am = __ballot(act);
        uint32_t c0, c1, c2, c3, d0, d3, d4;
        asm volatile(
            "s_mov_b64 exec, %[m0]\n\tds_read_u16 %[c0], %[a]\n\tds_write_b16 %[a], %[v]\n\t"
            "s_mov_b64 exec, %[m1]\n\tds_read_u16 %[c1], %[a]\n\tds_write_b16 %[a], %[v]\n\t"
            "s_mov_b64 exec, %[m2]\n\tds_read_u16 %[c2], %[a]\n\tds_write_b16 %[a], %[v]\n\t"
            "s_mov_b64 exec, %[m3]\n\tds_read_u16 %[c3], %[a]\n\tds_write_b16 %[a], %[v]\n\t"
            "s_mov_b64 exec, -1\n\t"
            "ds_bpermute_b32 %[d0], %[j], %[wd]\n\tds_bpermute_b32 %[d3], %[j], %[wd] offset:12\n\tds_bpermute_b32 %[d4], %[j], %[wd] offset:16\n\t"
            "s_waitcnt lgkmcnt(0)"
            : [c0] "=&v"(c0), [c1] "=&v"(c1), [c2] "=&v"(c2), [c3] "=&v"(c3), [d0] "=&v"(d0), [d3] "=&v"(d3), [d4] "=&v"(d4)
            : [a] "v"(ta), [v] "v"(uint32_t(p - s0)), [j] "v"(j0 << 2), [wd] "v"(wd),
              [m0] "s"(am & 0xFFFFull), [m1] "s"(am & 0xFFFF0000ull), [m2] "s"(am & 0xFFFF00000000ull), [m3] "s"(am & 0xFFFF000000000000ull)
            : "memory");
        w.prev4 = __builtin_amdgcn_alignbit(d1, d0, sh8);
        w.cur1 = __builtin_amdgcn_alignbit(d3, d2, sh8); w.cur2 = __builtin_amdgcn_alignbit(d4, d3, sh8);
        const uint32_t c16 = lane < 32 ? (lane < 16 ? c0 : c1) : (lane < 48 ? c2 : c3);     // (a register is only defined in its group)
        w.c = s0 + int(c16);
        // the same 4 bytes 1, 2 or 4 positions back (the lane holds them): the nearest goes before what the table said - a
        // lane does not see its own group's positions in the table, and runs and 4-byte strides are what that loses most
        const uint32_t b1 = __builtin_amdgcn_alignbit(w.cur0, w.prev4, 24), b2 = __builtin_amdgcn_alignbit(w.cur0, w.prev4, 16);
        w.c = w.cur0 == w.prev4 ? p - 4 : w.c;
        w.c = w.cur0 == b2 ? p - 2 : w.c;
        w.c = w.cur0 == b1 ? p - 1 : w.c;
        w.valid = act && w.c < p && w.c >= 4;
#ifdef K2P_MAXDIST
        w.valid = w.valid && p - w.c < K2P_MAXDIST;       // (timing experiment: what the far candidates' reads cost)
#endif
        w.gv = ld16(in + uint32_t(w.valid ? w.c - 4 : 0));
        return w;
    };
    auto flush256 = [&]() {
        if (lane < 16) *reinterpret_cast<uint4*>(out + flushed + 16 * lane) = *reinterpret_cast<const uint4*>(stg + 16 * lane);
        const uint32_t rem = pend - 256;
        if (uint32_t(4 * lane) < rem) { const uint32_t t = *reinterpret_cast<const uint32_t*>(stg + 256 + 4 * lane); *reinterpret_cast<uint32_t*>(stg + 4 * lane) = t; }
        flushed += 256; pend = rem;
    };
    // the general routes (long literal runs, long lengths): through the staging area too, a piece at a time
    auto stage_len = [&](uint32_t r) {
        uint32_t n255 = r / 255; const uint32_t last = r - n255 * 255;
        while (n255) {
            const uint32_t c = min(n255, 64u);
            if (uint32_t(lane) < c) stg[pend + lane] = 255;
            pend += c; n255 -= c;
            if (pend >= 256) flush256();
        }
        if (lane == 0) stg[pend] = uint8_t(last);
        pend += 1;
        if (pend >= 256) flush256();
    };
    auto stage_copy = [&](const uint8_t* from, uint32_t cnt) {
        while (cnt) {
            const uint32_t c = min(cnt, 128u);
            if (uint32_t(lane) < c) stg[pend + lane] = from[lane];
            if (uint32_t(lane) + 64 < c) stg[pend + 64 + lane] = from[64 + lane];
            pend += c; cnt -= c; from += c;
            if (pend >= 256) flush256();
        }
    };

    if (pmax < s0) { if (lane == 0) { meta->len = 0; meta->tail = uint32_t(s1 - s0); } return; }      // (n >= 36 from here on)
    int wb = s0;
    uint32_t wdn = load_win(s0 + 64);
    Win cur = stage_a(s0, load_win(s0));
    for (bool more = true; more; ) {
        // the next window's first half runs ahead of this window's walk (past the last window: a window without positions)
        const int wbn = wb + 64;
        const bool more_n = wbn < s1 && wbn <= pmax;
        const uint32_t wdnn = load_win(wbn + 64);
        const Win nxt = stage_a(wbn, wdn);

        // second half: match lengths, who is eligible
        const int p = wb + lane;
        const uint32_t xb = cur.prev4 ^ cur.gv.x;
        int bk = int(min(uint32_t(__clz(int(xb))), 32u) >> 3);                     // equal bytes before p, 0..4
        const uint32_t bits = min(min(ffbl(cur.cur0 ^ cur.gv.y), ffbl(cur.cur1 ^ cur.gv.z) | 32u), min(ffbl(cur.cur2 ^ cur.gv.w) | 64u, 96u));
        int mlen = int(bits >> 3);                                                 // equal bytes from p, 0..12
        if (wb + 63 + kFwd > mend) mlen = max(min(mlen, mend - p), 0);
        if (!cur.valid) mlen = 0;
        if (!cur.valid) bk = 0;
        // a position waits when one of the next three has a longer match
        const int m1 = next_lane(mlen), m2 = next_lane(m1), m3 = next_lane(m2);
        const bool elig = mlen >= 4 && max(m1, max(m2 - 1, m3 - 2)) <= mlen;
        const unsigned long long E = __ballot(elig);

        // the walk: which eligible lanes become sequences.  Scalar, and nothing but the cursor: a wave's scalar instructions are
        // what its SIMD runs out of first (four waves share one scalar issue slot every fourth clock), so everything that can
        // be said for all the window's sequences at once is said by the lanes afterwards.
        const int sp_in = sp;
        unsigned long long C = 0;
        int mlx = mlen;                               // the chosen lanes' lengths, extended
        for (;;) {
            const int rel = max(sp - wb, 0);
            if (rel >= 64) break;
            const unsigned long long em = (E >> rel) << rel;
            if (!em) break;
            const int l = __builtin_ctzll(em);
            const int pp = wb + l;
            int ml = int(rdl(uint32_t(mlen), l));
            if (ml == kFwd) {
                // the whole wave compares on: 4 bytes per lane, 256 per step
                const int cc = int(rdl(uint32_t(cur.c), l));
                int e = kFwd;
                bool open = true;
                while (open) {
                    const int q = pp + e + 4 * lane;
                    uint32_t x = 1;
                    if (q + 4 <= n) x = ld4(in + q) ^ ld4(in + cc + e + 4 * lane);
                    const unsigned long long ne = __ballot(x != 0);
                    if (ne) { const int fl = __builtin_ctzll(ne); e += 4 * fl + int(__builtin_ctz(rdl(x, fl)) >> 3); break; }
                    e += 256;
                    if (pp + e >= mend) break;
                }
                ml = min(e, mend - pp);
                asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0" : "+v"(mlx) : "s"(ml), "s"(l) : "m0");
            }
            C |= 1ull << l;
            sp = pp + ml;
        }
        if (C) {
            // the sequences of the window, all at once: lane i of C is a sequence
            uint32_t cm; asm("v_cndmask_b32 %0, 0, -1, %1" : "=v"(cm) : "s"(C));
            const uint32_t endv = uint32_t(p + mlx) & cm;
            const uint32_t einc = scan_max(endv);                                       // end of the last match at or before the lane
            const int prevend = max(int(prev_lane(einc)), sp_in);                       // ... before the lane
            const int back = min(bk, p - prevend);
            const int start = p - back, ll = start - prevend, mt = mlx + back - 4;
            const unsigned long long slow = __ballot((uint32_t(max(ll, mt)) & cm) >= 15u + 255u);
            if (slow == 0 && sp_in >= wb - 64) {
                const uint32_t hdr = ll >= 15 ? 2u : 1u, tb = mt >= 15 ? 3u : 2u;
                const uint32_t size = (hdr + uint32_t(ll) + tb) & cm;
                const uint32_t sinc = scan_add_incl(size);
                const uint32_t o = pend + sinc - size;                                  // where the sequence starts in the staging area
                const uint32_t a1 = sbase + o, a2 = a1 + hdr + uint32_t(ll);
                const uint32_t off = uint32_t(p - cur.c);
                put_lanes<0>(a1, uint32_t(min(ll, 15)) << 4 | uint32_t(min(mt, 15)), C);
                put_lanes<1>(a1, uint32_t(ll - 15), __ballot(ll >= 15) & C);
                put_lanes<0>(a2, off, C);
                put_lanes<1>(a2, off >> 8, C);
                put_lanes<2>(a2, uint32_t(mt - 15), __ballot(mt >= 15) & C);
                // literals: a lane no match covers belongs to the next sequence of the window, if there is one
                const uint32_t pack = ((o + hdr - uint32_t(prevend - wb)) & 0xFFFFu) | uint32_t(start - wb + 4) << 16;
                const unsigned long long up = C >> lane;
                const uint32_t nextidx = uint32_t(lane) + min(ffbl(uint32_t(up)), ffbl(uint32_t(up >> 32)) | 32u);
                const uint32_t pk = bperm(pack, nextidx & 63u);
                const bool lit = p >= max(int(einc), sp_in) && up != 0 && lane + 4 < int(pk >> 16);
                put_lanes<0>(vstg + uint32_t(int(int16_t(pk))), cur.cur0, __ballot(lit));
                if (sp_in < wb) {
                    // what the previous window left belongs to the first sequence
                    const uint32_t pk0 = rdl(pack, uint32_t(__builtin_ctzll(C)));
                    const int lo = sp_in - (wb - 64), hi = min(int(pk0 >> 16) - 4, 0) + 64;
                    put_lanes<0>(vstg + uint32_t(int(int16_t(pk0)) - 64), prevbyte, lane_range(lo, hi - lo));
                }
                pend += rdl(sinc, 63);
                if (pend >= 256) flush256();
            } else {
                // the general route (long literal runs, long lengths), a sequence at a time from memory
                int spx = sp_in;
                for (unsigned long long m = C; m; m &= m - 1) {
                    const int l = __builtin_ctzll(m);
                    const int pp = wb + l, ml = int(rdl(uint32_t(mlx), l)), cc = int(rdl(uint32_t(cur.c), l));
                    const int bb = min(int(rdl(uint32_t(bk), l)), pp - spx);
                    const int st = pp - bb, sll = st - spx, smt = ml + bb - 4;
                    const uint32_t soff = uint32_t(pp - cc);
                    if (lane == 0) stg[pend] = uint8_t(uint32_t(min(sll, 15)) << 4 | uint32_t(min(smt, 15)));
                    pend += 1;
                    if (sll >= 15) stage_len(uint32_t(sll - 15));
                    stage_copy(in + spx, uint32_t(sll));
                    if (lane < 2) stg[pend + lane] = uint8_t(soff >> lane8);
                    pend += 2;
                    if (smt >= 15) stage_len(uint32_t(smt - 15));
                    if (pend >= 256) flush256();
                    spx = pp + ml;
                }
            }
        }
        prevbyte = cur.cur0;
        cur = nxt; wdn = wdnn; wb = wbn; more = more_n;

    }
    for (uint32_t i = lane; i < pend; i += 64) out[flushed + i] = stg[i];
    if (lane == 0) { meta->len = flushed + pend; meta->tail = uint32_t(s1 - sp); }
}

// ----------------------------------------------------------------------------------------------------------------- stitch
__device__ __forceinline__ uint32_t len_bytes(uint32_t ll) { return ll >= 15 ? (ll - 15) / 255 + 1 : 0; }

// container_mode = 0: result = bytes of the LZ4 block, 0 when it does not fit dst_cap (the convention of LZ4_compress_default).
// container_mode = 1: one iteration of fourMCcompressFilename's loop (native/4mc.c:301-329): capacity src_len - 1, a block
//   that does not fit is stored raw (payload = input, result = src_len).
__global__ __launch_bounds__(256)
void lz4_par_stitch_kernel(const uint8_t* __restrict__ src_base, uint8_t* __restrict__ dst_base, fourmc_block* blocks,
                           uint32_t nblocks, int container_mode, uint8_t* __restrict__ work)
{
    const int lane = threadIdx.x & 63;
    const uint32_t wave = U(threadIdx.x >> 6);
    const uint32_t gseg = blockIdx.x * 4 + wave, b = gseg / kSegs, k = gseg % kSegs;
    if (b >= nblocks) return;
    const fourmc_block blk = uniform_block(blocks[b]);
    const uint8_t* in = src_base + blk.src_off;
    uint8_t* dst = dst_base + blk.dst_off;
    const uint32_t n = blk.src_len;
    const int64_t cap = container_mode ? (n ? int64_t(n) - 1 : 0) : int64_t(blk.dst_cap);     // (an empty block: 0, not -1; as every encoder)
    if (n > 0x7E000000u) { if (k == 0 && lane == 0) blocks[b].result = 0; return; }        // lz4.c:1324

    // lane j <-> segment j of the block
    const SegMeta mj = seg_meta(work, b)[lane];
    const bool has = mj.len != 0;
    const uint32_t pin = scan_add_incl(mj.tail), pex = pin - mj.tail;                // literals left by the segments before j
    const unsigned long long H = __ballot(has);
    const unsigned long long below = H & ((1ull << lane) - 1);
    const int prev = below ? 63 - __builtin_clzll(below) : -1;                      // the last segment before j with a sequence
    const uint32_t pprev = bperm(pex, uint32_t(max(prev, 0)));
    const uint32_t carry = pex - (prev >= 0 ? pprev : 0u);                           // literals that join j's first sequence
    // j's first sequence: token, old and new literal length
    const uint8_t* sj = seg_area(work, nblocks, b, uint32_t(lane));
    uint32_t tok = 0, ll0 = 0, q = 0;
    if (has) {
        tok = sj[0]; ll0 = tok >> 4; q = 1;
        if (ll0 == 15) { uint32_t bb; do { bb = sj[q++]; ll0 += bb; } while (bb == 255); }
    }
    const uint32_t nll = ll0 + carry, nh = 1 + len_bytes(nll);
    const uint32_t size = has ? nh + carry + (mj.len - q) : 0u;
    const uint32_t oin = scan_add_incl(size), oex = oin - size;
    const uint32_t body = rdl(oin, 63);
    // the block's last literals
    const int last = H ? 63 - __builtin_clzll(H) : -1;
    const uint32_t covered = min(n, uint32_t(kSegs) * kSeg);
    const uint32_t endlit = rdl(pin, 63) - (last >= 0 ? rdl(pex, uint32_t(max(last, 0))) : 0u) + (n - covered);
    const uint64_t total = uint64_t(body) + 1 + len_bytes(endlit) + endlit;
    const bool fits = int64_t(total) <= cap;

    if (!fits) {
        if (container_mode) {                                  // stored: this wave's 64 KiB of the input
            const uint32_t a = k * kSeg;
            if (a < n) copy_bytes(dst + a, in + a, min(uint32_t(kSeg), n - a), lane);
            if (k == kSegs - 1 && covered < n) copy_bytes(dst + covered, in + covered, n - covered, lane);
        }
        if (k == 0 && lane == 0) blocks[b].result = container_mode ? int32_t(n) : 0;
        return;
    }
    // this wave's segment
    const uint32_t k_has = uint32_t((H >> k) & 1);
    if (k_has) {
        const uint32_t ko = rdl(oex, k), kc = rdl(carry, k), kq = rdl(q, k), kll = rdl(nll, k), ktok = rdl(tok, k), knh = rdl(nh, k);
        const uint32_t klen = rdl(mj.len, k);
        uint8_t* o = dst + ko;
        if (lane == 0) o[0] = uint8_t(min(kll, 15u) << 4 | (ktok & 15));
        if (kll >= 15) emit_len(o + 1, kll - 15, lane);
        o += knh;
        if (kc) copy_bytes(o, in + size_t(k) * kSeg - kc, kc, lane);
        copy_bytes(o + kc, seg_area(work, nblocks, b, k) + kq, klen - kq, lane);
    }
    if (k == 0) {
        uint8_t* o = dst + body;
        if (lane == 0) o[0] = uint8_t(min(endlit, 15u) << 4);
        uint32_t h = 1;
        if (endlit >= 15) h += emit_len(o + 1, endlit - 15, lane);
        copy_bytes(o + h, in + n - endlit, endlit, lane);
        if (lane == 0) blocks[b].result = int32_t(total);
    }
}

} // namespace

extern "C" size_t fourmc_lz4_par_work_bytes(uint32_t n)
{ return size_t(n) * (kMetaBytes + size_t(kSegs) * kSegStride) + 256; }

extern "C" hipError_t fourmc_launch_lz4_encode_par(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                                   int container_mode, void* d_work, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    const dim3 grid(n * (kSegs / 4)), wg(256);
    hipLaunchKernelGGL(lz4_par_segment_kernel, dim3(n * kSegs), dim3(64), 0, stream, static_cast<const uint8_t*>(d_src), d_blocks, n,
                       static_cast<uint8_t*>(d_work));
    hipLaunchKernelGGL(lz4_par_stitch_kernel, grid, wg, 0, stream, static_cast<const uint8_t*>(d_src),
                       static_cast<uint8_t*>(d_dst), d_blocks, n, container_mode, static_cast<uint8_t*>(d_work));
    return hipGetLastError();
}
