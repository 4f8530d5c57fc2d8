// 4mc_amd/csrc/zst.hip - .zst files (what ZstCodec and the zstd tool write) decoded in device memory, many per call.
//
// Contract: ZSTD_decompress(dst, cap, image, image_bytes) of the reference (native/zstd/decompress/zstd_decompress.c:1112, the
// multi-frame loop :989-1078, one frame :901-987): concatenated frames and skippable frames, no dictionary, any windowLog the
// one-shot call takes, content checksums verified.
//
// A frame is a chain of blocks of 128 KiB or less whose ENTROPY stage is independent: tables repeat only by reference and repeat
// offsets are resolved at execution (zstd_decode.hip says so for the 64 blocks of a 4mz payload).  Here that is taken to every
// block of every frame of every stream of a call:
//   walk      one wave per stream chases frame headers and the 3-byte block headers; the first pass counts (the host reads that
//             back once), the second fills one frame table and one block table for the whole call
//   headers   one lane per block: literals header and sequence count
//   scan      one wave over the table: prefix sums give every block its exact slice of the literal and the sequence area, and a
//             running maximum gives every block the block that DEFINES each table it only refers to (treeless literals, Repeat
//             mode), however far back in its frame: the lane rebuilds such a table from the defining block's bytes in the image,
//             so no wave waits for another
//   entropy   one lane per block, one wave per 64 consecutive table entries (they may span frames and streams): Huffman
//             literals into the literal area, sequences as 8-byte triples (kSeqArea's layout) into the sequence area; the block's
//             decoded size is its literals plus its match lengths
//   sizes     one wave per stream: frame sizes, 64-bit output offsets, the first frame the stages above could not take, the
//             DST_SMALL verdict
//   execute   one wave per frame runs the frame's blocks in order (step 2 of zstd_decode_frame_v2: repeat offsets, the
//             wave-wide batch copier), frames and streams in parallel, 64-bit output offsets
//   checksum  one wave per frame that carries one: XXH64 of its output
//   serial    a frame the stages above declined goes, with what follows it in its stream, to the one-wave decoder of
//             zstd_dev.h, whose result is the verdict (it carries the reference's rules)
//   status    one lane per stream folds all of that into a fourmc_zst_status
// headers .. execute run per ROUND of at most `round_blocks` table entries, which bounds the workspace; across rounds a frame
// carries its repeat offsets and its output position in the frame table.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "fourmc_gpu.h"
#include "kernels.h"
#include "devcopy.h"
#include "zstd_dev.h"

namespace {

constexpr size_t   kZstState   = (sizeof(ZState) + 255) & ~size_t(255);    // a lane's tables
constexpr uint32_t kZstSeqPer  = (uint32_t(kBlockMax) + 2) / 3;            // sequences a block of 128 KiB of output can hold (match >= 3)
constexpr size_t   kZstPerBlock = kZstState + size_t(kBlockMax) + size_t(kZstSeqPer) * 8;
constexpr int      kSumBad     = -2;                                       // a frame's result: checksum mismatch
constexpr uint64_t kFrameMax   = 0x7FFFFFFFull - 128;                      // the execute stage counts a frame's bytes in an int

struct ZstStream {                       // one per stream
    uint64_t fail_off;                   // walk: offset of the magic number of the frame it failed at (image_bytes: none)
    uint64_t total;                      // sizes: bytes of the frames in front of the first declined frame
    uint32_t frames, skips, blocks;      // walk: complete frames, skippable frames in front of the failure, blocks of complete frames
    uint32_t walked;                     // walk: blocks including those of a frame that failed later
    uint32_t frame0, block0;             // host: the stream's first entry in the frame and the block table
    int32_t  walk_bad;
    uint32_t n_ok;                       // sizes: frames in front of the first declined one (== frames: none)
    uint32_t exec;                       // sizes: 1 = there is a destination and it is large enough
    int32_t  serial_r;                   // serial: result of the one-wave decoder over the declined frame and what follows it
    uint32_t serial_ran, pad;
};
struct ZstFrame {
    uint64_t src_off, end_off;           // magic number / first byte behind the frame, from the stream's start
    uint64_t fcs;                        // Frame_Content_Size or ~0
    uint64_t out_off, out_size;          // sizes: from the stream's first output byte
    uint32_t blk0, nblk, stream, skips_before;
    uint32_t has_sum; int32_t result;    // result: 0, or < 0 from the execute / checksum stage
    uint32_t rep[3]; int32_t op;         // carried across rounds
};
struct ZstBlock {
    uint64_t src;                        // content, from the images' base
    uint64_t lit_pre, seq_pre;           // scan: exclusive prefix sums over the whole table (a round subtracts its first entry's)
    uint32_t size, frame, fblk0;         // Block_Size, frame (table index), the frame's first block
    uint32_t lsize, lcsize, nseq, spos, out_size;
    uint32_t def_huf, def_ll, def_of, def_ml;   // 1 + the defining block's table index, 0: none in this frame
    uint8_t  type, ltype, lh, one, modes, bad, last, pad;
};

__device__ unsigned long long g_zst_counts[3];               // fast frames, serial frames, fast blocks (test aid)

__device__ __forceinline__ uint32_t rd32(const uint8_t* p)
{ return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24); }

// ------------------------------------------------------------------------------------------------ walk
// The rules are those of the serial decoder (zstd_dev.h) and so the reference's: a frame the walk fails, the reference fails.
__global__ __launch_bounds__(64)
void zst_walk_kernel(const uint8_t* __restrict__ img, const fourmc_zst_item* __restrict__ items, uint32_t n, ZstStream* st,
                     ZstFrame* fr, ZstBlock* bk, int fill)
{
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const int lane = threadIdx.x;
    const uint64_t base = items[i].image_off, len = items[i].image_bytes;
    const uint8_t* const p = img + base;
    const uint32_t f0 = fill ? st[i].frame0 : 0u, b0 = fill ? st[i].block0 : 0u;
    uint64_t ip = 0, fail = len;
    uint32_t frames = 0, skips = 0, blocks = 0, walked = 0;
    bool bad = false;
    while (len - ip >= 5) {                                            // ZSTD_startingInputLength
        const uint64_t at = ip;
        const uint32_t magic = rd32(p + ip);
        if ((magic & 0xFFFFFFF0u) == 0x184D2A50u) {                    // skippable frame
            if (len - ip < 8) { bad = true; fail = at; break; }
            const uint32_t sz = rd32(p + ip + 4);
            if (uint64_t(sz) > len - ip - 8) { bad = true; fail = at; break; }
            ip += 8 + uint64_t(sz); skips++;
            continue;
        }
        bool fbad = magic != 0xFD2FB528u || len - ip < 9;              // ZSTD_FRAMEHEADERSIZE_MIN + ZSTD_blockHeaderSize
        uint64_t fcs = ~0ull; int has_sum = 0;
        if (!fbad) {
            const uint32_t fhd = p[ip + 4];
            const int fcs_id = fhd >> 6, single = (fhd >> 5) & 1, did = fhd & 3;
            has_sum = (fhd >> 2) & 1;
            const int did_sz = did == 3 ? 4 : did, fcs_sz = fcs_id == 0 ? single : (1 << fcs_id);
            const int hsize = 5 + (single ? 0 : 1) + did_sz + fcs_sz;
            if ((fhd & 0x08) || len - ip < uint64_t(hsize) + 3) fbad = true;
            else {
                uint64_t hp = ip + 5;
                if (!single) { const uint32_t wb = p[hp++]; if (int(wb >> 3) + 10 > 31) fbad = true; }
                uint32_t dict = 0;
                for (int k = 0; k < did_sz; k++) dict |= uint32_t(p[hp++]) << (8 * k);
                if (dict != 0) fbad = true;                            // no dictionaries on the device
                if (fcs_id == 0) { if (single) fcs = p[hp++]; }
                else { fcs = 0; for (int k = 0; k < fcs_sz; k++) fcs |= uint64_t(p[hp++]) << (8 * k); if (fcs_id == 1) fcs += 256; }
                ip += uint64_t(hsize);
            }
        }
        const uint32_t blk0 = walked;
        while (!fbad) {
            if (len - ip < 3) { fbad = true; break; }
            const uint32_t bh = uint32_t(p[ip]) | (uint32_t(p[ip + 1]) << 8) | (uint32_t(p[ip + 2]) << 16);
            ip += 3;
            const uint32_t last = bh & 1, btype = (bh >> 1) & 3, bsize = bh >> 3, content = btype == 1 ? 1u : bsize;
            if (btype == 3 || uint64_t(content) > len - ip) { fbad = true; break; }
            if (btype == 2 && (bsize >= uint32_t(kBlockMax) || bsize < 2)) { fbad = true; break; }
            if (fill && lane == 0) {
                ZstBlock e = {};
                e.src = base + ip; e.size = bsize; e.frame = f0 + frames; e.fblk0 = b0 + blk0; e.type = uint8_t(btype); e.last = uint8_t(last);
                e.out_size = btype == 2 ? 0u : bsize;
                bk[b0 + walked] = e;
            }
            walked++; ip += content;
            if (last) break;
        }
        if (!fbad && has_sum) { if (len - ip < 4) fbad = true; else ip += 4; }
        if (fbad) { bad = true; fail = at; break; }
        if (fill && lane == 0) {
            ZstFrame f = {};
            f.src_off = at; f.end_off = ip; f.fcs = fcs; f.blk0 = b0 + blk0; f.nblk = walked - blk0; f.stream = i; f.skips_before = skips;
            f.has_sum = uint32_t(has_sum); f.rep[0] = 1; f.rep[1] = 4; f.rep[2] = 8;
            fr[f0 + frames] = f;
        }
        frames++; blocks = walked;
    }
    if (!bad && ip != len) { bad = true; fail = ip; }                  // 1 to 4 bytes behind the last frame
    if (!fill && lane == 0) {
        ZstStream s = {};
        s.fail_off = fail; s.frames = frames; s.skips = skips; s.blocks = blocks; s.walked = walked; s.walk_bad = bad ? 1 : 0;
        st[i] = s;
    }
}

// ------------------------------------------------------------------------------------------------ headers
__global__ __launch_bounds__(256)
void zst_headers_kernel(const uint8_t* __restrict__ img, ZstBlock* bk, uint32_t nb)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nb) return;
    if (bk[i].type != 2) return;
    const uint8_t* const bp = img + bk[i].src;
    const int bend = int(bk[i].size);
    LitHdr h; h.ltype = 0; h.lh = 0; h.lsize = 0; h.lcsize = 0; h.one = false;
    int spos = 0, nseq = 0; uint32_t modes = 0;
    bool ok = parse_lit_hdr(bp, bend, h);
    if (ok) { spos = int(h.lh + h.lcsize); ok = parse_seq_hdr(bp, bend, spos, nseq, modes); }
    bk[i].lsize = h.lsize; bk[i].lcsize = h.lcsize; bk[i].nseq = uint32_t(nseq); bk[i].spos = uint32_t(spos);
    bk[i].ltype = uint8_t(h.ltype); bk[i].lh = uint8_t(h.lh); bk[i].one = h.one ? 1 : 0; bk[i].modes = uint8_t(modes); bk[i].bad = ok ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------ scan
__global__ __launch_bounds__(64)
void zst_scan_kernel(ZstBlock* bk, uint32_t nb)
{
    const int lane = threadIdx.x;
    uint64_t lit_c = 0, seq_c = 0;
    uint32_t c_h = 0, c_t[3] = {0, 0, 0};
    for (uint32_t base = 0; base < nb; base += 64) {
        const uint32_t i = base + uint32_t(lane);
        const bool live = i < nb;
        const uint32_t j = live ? i : nb - 1;
        const bool comp = live && bk[j].type == 2 && !bk[j].bad;
        const uint32_t ltype = bk[j].ltype, nseq = comp ? bk[j].nseq : 0u, modes = bk[j].modes, fblk0 = bk[j].fblk0;
        const uint32_t need = (comp && ltype >= 2) ? ((bk[j].lsize + 63u) & ~63u) : 0u;
        const uint32_t li = scan_add(need), si = scan_add(nseq);
        const uint64_t lit_pre = lit_c + li - need, seq_pre = seq_c + si - nseq;
        lit_c += uint32_t(__builtin_amdgcn_readlane(int(li), 63));
        seq_c += uint32_t(__builtin_amdgcn_readlane(int(si), 63));
        uint32_t h = max(scan_max((comp && ltype == 2) ? i + 1 : 0u), c_h);
        c_h = uint32_t(__builtin_amdgcn_readlane(int(h), 63));
        uint32_t d[3];
        for (int t = 0; t < 3; t++) {
            const bool def = comp && nseq > 0 && ((modes >> (6 - 2 * t)) & 3) != 3;
            d[t] = max(scan_max(def ? i + 1 : 0u), c_t[t]);
            c_t[t] = uint32_t(__builtin_amdgcn_readlane(int(d[t]), 63));
        }
        if (live) {
            bk[i].lit_pre = lit_pre; bk[i].seq_pre = seq_pre;
            bk[i].def_huf = (h && h - 1 >= fblk0) ? h : 0u;
            bk[i].def_ll = (d[0] && d[0] - 1 >= fblk0) ? d[0] : 0u;
            bk[i].def_of = (d[1] && d[1] - 1 >= fblk0) ? d[1] : 0u;
            bk[i].def_ml = (d[2] && d[2] - 1 >= fblk0) ? d[2] : 0u;
        }
    }
}

// ------------------------------------------------------------------------------------------------ entropy
struct ZstLds { uint32_t llb[36], mlb[56]; uint8_t llx[36], mlx[56]; };

// the sequences of one block as (ll, ml, Offset_Value) triples: v2_sequences_lane of zstd_decode.hip, with the defining block of a
// Repeat-mode table taken from the block table (it may lie anywhere earlier in the frame).  *mlsum: the sum of the match lengths
__device__ __forceinline__ bool zst_sequences_lane(ZState* zl, const ZstLds* z, const uint8_t* img, const ZstBlock* bk, const ZstBlock& e,
                                                   const uint8_t* bp, uint32_t* out, uint64_t* mlsum)
{
    const int bend = int(e.size), nseq = int(e.nseq);
    const uint32_t modes = e.modes;
    const uint32_t defs[3] = {e.def_ll, e.def_of, e.def_ml};
    int logs[3] = {0, 0, 0};
    int pos = int(e.spos);
    for (int t = 0; t < 3; t++) {
        const int mode = int((modes >> (6 - 2 * t)) & 3);
        if (mode != 3) { const int lg = build_seq_table_lane(zl, bp, bend, pos, t, mode); if (lg < 0) return false; logs[t] = lg; continue; }
        if (!defs[t]) return false;                                    // Repeat mode with nothing to repeat
        const ZstBlock& dj = bk[defs[t] - 1];
        const uint8_t* bj = img + dj.src; const int be = int(dj.size);
        int pj = int(dj.spos);
        const uint32_t mj = dj.modes;
        for (int u = 0; u < t; u++) if (!skip_seq_table(zl, bj, be, pj, u, int((mj >> (6 - 2 * u)) & 3))) return false;
        const int lg = build_seq_table_lane(zl, bj, be, pj, t, int((mj >> (6 - 2 * t)) & 3));
        if (lg < 0) return false;
        logs[t] = lg;
    }
    const int ll_log = logs[0], of_log = logs[1], ml_log = logs[2];
    uint2* const cl = reinterpret_cast<uint2*>(zl->huf);               // {FSE entry, baseline | extra bits << 20} per LL / ML state
    uint2* const cm = cl + 512;
    for (int u = 0; u < (1 << ll_log); u++) { const uint32_t en = zl->ll[u], c = en & 0xff; if (c > 35) return false; cl[u] = make_uint2(en, z->llb[c] | (uint32_t(z->llx[c]) << 20)); }
    for (int u = 0; u < (1 << ml_log); u++) { const uint32_t en = zl->ml[u], c = en & 0xff; if (c > 52) return false; cm[u] = make_uint2(en, z->mlb[c] | (uint32_t(z->mlx[c]) << 20)); }
    BitsBack bs;
    if (!bs.init(bp + pos, bend - pos)) return false;
    uint32_t sl = bs.read(ll_log), so = bs.read(of_log), sm = bs.read(ml_log);
    uint64_t sum = 0;
    for (int n = 0; n < nseq; n++) {
        const uint2 cle = cl[sl], cme = cm[sm];
        const uint32_t el = cle.x, eo = zl->of[so], em = cme.x;
        const uint32_t lv = cle.y, mv = cme.y;
        const uint32_t ocode = eo & 0xff;
        if (ocode > 31) return false;
        const uint32_t ov = (1u << ocode) + bs.read_fast(int(ocode));  // Offset_Value: 1..3 repeat codes, else offset + 3
        const uint32_t mlen = (mv & 0xFFFFF) + bs.read_fast(int(mv >> 20));
        const uint32_t llen = (lv & 0xFFFFF) + bs.read_fast(int(lv >> 20));
        sl = (el >> 16) + bs.read(int((el >> 8) & 0xff));
        sm = (em >> 16) + bs.read(int((em >> 8) & 0xff));
        so = (eo >> 16) + bs.read(int((eo >> 8) & 0xff));
        if (ov >> 28) return false;                                    // beyond the 28 bits of a triple (needs windowLog > 27): the serial decoder decides
        *reinterpret_cast<uint2*>(out + 2 * n) = make_uint2(llen | (mlen << 18), ov | ((mlen >> 14) << 28));
        sum += mlen;
    }
    if (bs.pos > 0) return false;                                      // bits left over: corruption
    *mlsum = sum;
    return true;
}

__global__ __launch_bounds__(64)
void zst_entropy_kernel(const uint8_t* __restrict__ img, ZstBlock* bk, uint32_t r0, uint32_t r1, uint8_t* work, uint32_t round_cap)
{
    __shared__ ZstLds zs;
    const int lane = threadIdx.x;
    if (lane < 36) { zs.llb[lane] = kLLBase[lane]; zs.llx[lane] = kLLBits[lane]; }
    if (lane < 53) { zs.mlb[lane] = kMLBase[lane]; zs.mlx[lane] = kMLBits[lane]; }
    __syncthreads();
    const uint32_t i = r0 + blockIdx.x * 64u + uint32_t(lane);
    if (i >= r1) return;
    const ZstBlock e = bk[i];
    if (e.type != 2 || e.bad) return;
    const uint32_t slot = i - r0;
    ZState* const zl = reinterpret_cast<ZState*>(work + size_t(slot) * kZstState);
    uint8_t* const litarea = work + size_t(round_cap) * kZstState;
    uint32_t* const seqarea = reinterpret_cast<uint32_t*>(litarea + size_t(round_cap) * size_t(kBlockMax));
    const uint64_t lit0 = bk[r0].lit_pre, seq0 = bk[r0].seq_pre;
    const uint8_t* const bp = img + e.src;
    bool bad = false;
    // ---- Huffman literals: the table of this block, or of the block it refers to, built in this lane's slot
    if (e.ltype >= 2) {
        int huf_log = 0, my_used = 0;
        if (!e.def_huf) bad = true;
        else {
            const ZstBlock& dj = bk[e.def_huf - 1];
            const int used = read_huf_table(zl, img + dj.src + dj.lh, int(dj.lcsize), &huf_log);
            if (used < 0) bad = true;
            else if (e.ltype == 2) my_used = used;
        }
        if (!bad) {
            const uint16_t* const tab = zl->huf;
            const uint8_t* hp8 = bp + e.lh + my_used;
            const int hlen = int(e.lcsize) - my_used;
            uint8_t* const out = litarea + (e.lit_pre - lit0);
            int nstreams = 1, l1 = 0, l2 = 0, l3 = 0, seg = int(e.lsize);
            if (!e.one) {
                if (hlen < 10 || e.lsize < 6) bad = true;
                else {
                    l1 = hp8[0] | (hp8[1] << 8); l2 = hp8[2] | (hp8[3] << 8); l3 = hp8[4] | (hp8[5] << 8);
                    seg = (int(e.lsize) + 3) / 4; nstreams = 4;
                    if (hlen - 6 - l1 - l2 - l3 < 1 || 3 * seg > int(e.lsize)) bad = true;
                }
            } else if (hlen < 1) bad = true;
            for (int j = 0; j < nstreams && !bad; j++) {
                const int s_off = nstreams == 1 ? 0 : 6 + (j > 0 ? l1 : 0) + (j > 1 ? l2 : 0) + (j > 2 ? l3 : 0);
                const int s_len = nstreams == 1 ? hlen : (j == 0 ? l1 : (j == 1 ? l2 : (j == 2 ? l3 : hlen - 6 - l1 - l2 - l3)));
                const int o_off = nstreams == 1 ? 0 : seg * j, o_len = nstreams == 1 ? int(e.lsize) : ((j == 3) ? int(e.lsize) - 3 * seg : seg);
                BitsBack bs;
                if (!bs.init(hp8 + s_off, s_len)) { bad = true; break; }
                auto symbol = [&]() -> uint32_t {
                    const uint32_t idx = (bs.pos >= huf_log) ? bs.peek_at(bs.pos - huf_log, huf_log)
                                                             : (bs.peek_at(0, bs.pos > 0 ? bs.pos : 0) << (huf_log - (bs.pos > 0 ? bs.pos : 0)));
                    const uint32_t en = tab[idx];
                    bs.pos -= int(en >> 8);
                    return en & 0xff;
                };
                struct __attribute__((packed, aligned(1))) U4 { uint32_t v; };
                int k = 0;
                for (; k + 4 <= o_len; k += 4) {
                    uint32_t w4 = symbol(); w4 |= symbol() << 8; w4 |= symbol() << 16; w4 |= symbol() << 24;
                    reinterpret_cast<U4*>(out + o_off + k)->v = w4;
                }
                for (; k < o_len; k++) out[o_off + k] = uint8_t(symbol());
                if (bs.pos != 0) bad = true;                           // (the serial decoder has the end rules of both of the reference's decoders)
            }
        }
    }
    // ---- sequences
    uint64_t mlsum = 0;
    if (!bad && e.nseq > 0) {
        const uint64_t soff = e.seq_pre - seq0;
        if (soff + e.nseq > uint64_t(round_cap) * kZstSeqPer) bad = true;         // a round of blocks that decode to more than 128 KiB each
        else bad = !zst_sequences_lane(zl, &zs, img, bk, e, bp, seqarea + soff * 2, &mlsum);
    }
    if (!bad && uint64_t(e.lsize) + mlsum > kFrameMax) bad = true;
    if (bad) bk[i].bad = 1; else bk[i].out_size = uint32_t(uint64_t(e.lsize) + mlsum);
}

// ------------------------------------------------------------------------------------------------ sizes
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v)
{
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = uint32_t(__shfl_xor(int(uint32_t(v)), o)), hi = uint32_t(__shfl_xor(int(uint32_t(v >> 32)), o));
        v += (uint64_t(hi) << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(64)
void zst_sizes_kernel(const fourmc_zst_item* __restrict__ items, uint32_t n, ZstStream* st, ZstFrame* fr, const ZstBlock* bk, int has_dst)
{
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const int lane = threadIdx.x;
    const uint32_t f0 = st[i].frame0, nf = st[i].frames;
    uint64_t run = 0;
    uint32_t k = 0;
    for (; k < nf; k++) {
        const uint32_t b0 = fr[f0 + k].blk0, nb = fr[f0 + k].nblk;
        const uint64_t fcs = fr[f0 + k].fcs;
        uint64_t sum = 0; bool bad = false;
        for (uint32_t b = uint32_t(lane); b < nb; b += 64) { sum += bk[b0 + b].out_size; bad |= bk[b0 + b].bad != 0; }
        sum = wave_sum64(sum);
        if (__ballot(bad) || (fcs != ~0ull && fcs != sum) || sum > kFrameMax) break;
        if (lane == 0) { fr[f0 + k].out_off = run; fr[f0 + k].out_size = sum; }
        run += sum;
    }
    if (lane == 0) { st[i].total = run; st[i].n_ok = k; st[i].exec = (has_dst && run <= items[i].dst_cap) ? 1u : 0u; }
}

// ------------------------------------------------------------------------------------------------ execute
// Blocks [b_lo, b_hi) of one frame, in order, with the whole wave: step 2 of zstd_decode_frame_v2 reading the block table.  dst is
// the frame's first output byte, cap its size; positions count from there.  Returns 0 or kErr.
__device__ __forceinline__ int zst_exec_blocks(const uint8_t* img, const ZstBlock* bk, uint32_t b_lo, uint32_t b_hi, uint8_t* dst, const int cap,
                                               const uint8_t* litarea, const uint32_t* seqarea, uint64_t lit0, uint64_t seq0, uint8_t* own,
                                               int& op, uint32_t& rep0, uint32_t& rep1, uint32_t& rep2, int lane)
{
    uint32_t pv = 0; int p_base = 0, p_n = 0;
    for (uint32_t b = b_lo; b < b_hi; b++) {
        const int btype = bk[b].type;
        const uint32_t bsize = bk[b].size;
        const uint8_t* const bsrc = img + bk[b].src;
        if (btype == 0) {
            if (bsize > uint32_t(cap - op)) return kErr;
            wave_copy(dst + op, bsrc, int(bsize), lane);
            op += int(bsize);
            continue;
        }
        if (btype == 1) {
            if (bsize > uint32_t(cap - op)) return kErr;
            const uint8_t v = bsrc[0];
            for (uint32_t k = lane; k < bsize; k += 64) dst[op + k] = v;
            op += int(bsize);
            continue;
        }
        const uint32_t ltype = bk[b].ltype, lh = bk[b].lh;
        Lits lits; lits.pos = 0; lits.size = bk[b].lsize; lits.is_rle = ltype == 1; lits.rle = ltype == 1 ? bsrc[lh] : uint8_t(0);
        lits.p = ltype >= 2 ? litarea + (bk[b].lit_pre - lit0) : bsrc + lh;
        const int nsq = int(bk[b].nseq);
        const uint32_t* sq = seqarea + (bk[b].seq_pre - seq0) * 2;
        int n = 0;
        while (n < nsq) {
            const int take = min(64, nsq - n);
            uint32_t my_ll = 0, my_ml = 0, r_ov = 4;
            if (lane < take) {
                const uint32_t w0 = sq[2 * (n + lane)], w1 = sq[2 * (n + lane) + 1];
                my_ll = w0 & 0x3FFFF; my_ml = (w0 >> 18) | ((w1 >> 28) << 14); r_ov = w1 & 0x0FFFFFFF;
            }
            const uint32_t incl = scan_add(my_ll + my_ml);
            const unsigned long long over = __ballot(lane < take && incl > uint32_t(kOwnBytes));
            int cnt = over ? __builtin_ctzll(over) : take;
            const bool single = cnt == 0;                              // one sequence larger than a whole batch: executed alone below
            if (single) cnt = 1;
            if (lane >= cnt) { my_ll = 0; my_ml = 0; }
            const uint32_t T = uint32_t(__builtin_amdgcn_readlane(int(incl), cnt - 1));
            const uint32_t Lsum = uint32_t(__builtin_amdgcn_readlane(int(scan_add(my_ll)), 63));
            uint32_t my_off = r_ov - 3;                                // real offsets; repeat codes are patched below
            {
                const unsigned long long rmask = __ballot(lane < cnt && r_ov <= 3);
                int prev = -1;                                         // last position whose effect is folded into rep0..2
                auto advance = [&](int upto) {                         // fold the real offsets of positions (prev, upto) into the history
                    const int g = upto - 1 - prev;
                    if (g >= 3) { rep0 = uint32_t(__builtin_amdgcn_readlane(int(my_off), upto - 1)); rep1 = uint32_t(__builtin_amdgcn_readlane(int(my_off), upto - 2)); rep2 = uint32_t(__builtin_amdgcn_readlane(int(my_off), upto - 3)); }
                    else if (g == 2) { rep2 = rep0; rep0 = uint32_t(__builtin_amdgcn_readlane(int(my_off), upto - 1)); rep1 = uint32_t(__builtin_amdgcn_readlane(int(my_off), upto - 2)); }
                    else if (g == 1) { rep2 = rep1; rep1 = rep0; rep0 = uint32_t(__builtin_amdgcn_readlane(int(my_off), upto - 1)); }
                };
                for (unsigned long long todo = rmask; todo; todo &= todo - 1) {
                    const int k = __builtin_ctzll(todo);
                    advance(k);
                    const uint32_t ov = uint32_t(__builtin_amdgcn_readlane(int(r_ov), k));
                    const uint32_t idx = ov - 1 + (uint32_t(__builtin_amdgcn_readlane(int(my_ll), k)) == 0 ? 1u : 0u);
                    uint32_t offset;
                    if (idx == 0) offset = rep0;
                    else {
                        uint32_t t = idx == 1 ? rep1 : (idx == 2 ? rep2 : rep0 - 1);
                        t += !t;
                        if (idx != 1) rep2 = rep1;
                        rep1 = rep0; rep0 = offset = t;
                    }
                    if (lane == k) my_off = offset;
                    prev = k;
                }
                advance(cnt);
            }
            n += cnt;
            if (!single && Lsum <= lits.size - lits.pos && uint32_t(op) + T + 64 <= uint32_t(cap)) {
                const uint32_t sz = my_ll + my_ml;
                const uint32_t ostart = scan_add(sz) - sz, lstart = scan_add(my_ll) - my_ll;
                const bool badq = lane < cnt && my_off > uint32_t(op) + ostart + my_ll;
                if (__ballot(badq)) return kErr;
                for (uint32_t k = 4u * lane; k < T; k += 256) *reinterpret_cast<uint32_t*>(own + k) = 0;
                if (lane < cnt) own[ostart] = uint8_t(lane + 1);
                const uint8_t* const lbase = lits.is_rle ? dst : lits.p + lits.pos;
                uint32_t carry = 0;
                if (p_n == 0) p_base = op;
                for (uint32_t c0 = 0; c0 < T; c0 += 64) {
                    const uint32_t o = c0 + lane;
                    const bool live = o < T;
                    uint32_t m = live ? uint32_t(own[o]) : 0u;
                    m = max(scan_max(m), carry);
                    carry = uint32_t(__builtin_amdgcn_readlane(int(m), 63));
                    const int tl = (int(m) - 1) & 63;
                    const uint32_t os = __shfl(ostart, tl), lt = __shfl(my_ll, tl), offt = __shfl(my_off, tl), ls = __shfl(lstart, tl);
                    const uint32_t rel = o - os;
                    const bool is_lit = live && rel < lt;
                    const int sp = op + int(o) - int(offt);
                    const int cs = op + int(c0);
                    const bool is_match = live && !is_lit;
                    const bool from_mem = is_match && sp < cs - p_n;
                    const bool in_pend = is_match && sp >= cs - p_n && sp < cs;
                    const uint8_t* const addr = (is_lit && !lits.is_rle) ? lbase + ls + rel : dst + (from_mem ? sp : 0);
                    const uint32_t ld = *addr;
                    dst[p_base + lane] = uint8_t(pv);
                    const uint32_t fw = __shfl(pv, (sp - p_base) & 63);
                    uint32_t v = ld;
                    if (is_lit && lits.is_rle) v = lits.rle;
                    if (in_pend) v = fw;
                    bool done = !is_match || from_mem || in_pend;
                    int dep = sp - cs;
                    while (__ballot(!done)) {
                        const int d = dep & 63;
                        const uint32_t v2 = __shfl(v, d);
                        const int dn = __shfl(int(done), d);
                        const int dd = __shfl(dep, d);
                        if (!done) { if (dn) { v = v2; done = true; } else dep = dd; }
                    }
                    pv = v; p_base = cs; p_n = min(64, int(T - c0));
                }
                op += int(T); lits.pos += Lsum;
            } else {
                if (lane < p_n) dst[p_base + lane] = uint8_t(pv);
                p_n = 0;
                for (int k = 0; k < cnt; k++) {
                    const uint32_t llen = uint32_t(__builtin_amdgcn_readlane(int(my_ll), k)), mlen = uint32_t(__builtin_amdgcn_readlane(int(my_ml), k));
                    const uint32_t offset = uint32_t(__builtin_amdgcn_readlane(int(my_off), k));
                    if (llen > lits.size - lits.pos) return kErr;
                    if (uint64_t(llen) + mlen > uint64_t(cap - op)) return kErr;
                    copy_lits(dst + op, lits, llen, lane);
                    lits.pos += llen; op += int(llen);
                    if (offset > uint32_t(op)) return kErr;
                    copy_match(dst, op, int(offset), int(mlen), lane);
                    op += int(mlen);
                }
            }
        }
        if (lane < p_n) dst[p_base + lane] = uint8_t(pv);
        p_n = 0;
        {
            const uint32_t rest = lits.size - lits.pos;
            if (rest > uint32_t(cap - op)) return kErr;
            copy_lits(dst + op, lits, rest, lane);
            op += int(rest);
        }
    }
    return 0;
}

__global__ __launch_bounds__(64)
void zst_exec_kernel(const uint8_t* __restrict__ img, uint8_t* dst_base, const fourmc_zst_item* __restrict__ items, const ZstStream* st,
                     ZstFrame* fr, const ZstBlock* bk, uint32_t nf, uint32_t r0, uint32_t r1, const uint8_t* work, uint32_t round_cap)
{
    __shared__ uint8_t own[kOwnBytes];
    const uint32_t f = blockIdx.x;
    if (f >= nf) return;
    const int lane = threadIdx.x;
    const uint32_t s = fr[f].stream;
    if (!st[s].exec || f - st[s].frame0 >= st[s].n_ok || fr[f].result < 0) return;
    const uint32_t b0 = fr[f].blk0, b1 = b0 + fr[f].nblk;
    const uint32_t lo = uint32_t(__builtin_amdgcn_readfirstlane(int(max(b0, r0)))), hi = uint32_t(__builtin_amdgcn_readfirstlane(int(min(b1, r1))));
    if (lo >= hi) return;
    const uint8_t* const litarea = work + size_t(round_cap) * kZstState;
    const uint32_t* const seqarea = reinterpret_cast<const uint32_t*>(litarea + size_t(round_cap) * size_t(kBlockMax));
    uint8_t* const dst = dst_base + items[s].dst_off + fr[f].out_off;
    const int cap = __builtin_amdgcn_readfirstlane(int(fr[f].out_size));
    int op = __builtin_amdgcn_readfirstlane(fr[f].op);
    uint32_t rep0 = uint32_t(__builtin_amdgcn_readfirstlane(int(fr[f].rep[0]))), rep1 = uint32_t(__builtin_amdgcn_readfirstlane(int(fr[f].rep[1])));
    uint32_t rep2 = uint32_t(__builtin_amdgcn_readfirstlane(int(fr[f].rep[2])));
    int r = zst_exec_blocks(img, bk, lo, hi, dst, cap, litarea, seqarea, bk[r0].lit_pre, bk[r0].seq_pre, own, op, rep0, rep1, rep2, lane);
    if (r == 0 && hi == b1 && op != cap) r = kErr;
    if (lane == 0) {
        if (r < 0) fr[f].result = r;
        fr[f].op = op; fr[f].rep[0] = rep0; fr[f].rep[1] = rep1; fr[f].rep[2] = rep2;
    }
}

// ------------------------------------------------------------------------------------------------ checksum
__global__ __launch_bounds__(64)
void zst_checksum_kernel(const uint8_t* __restrict__ img, const uint8_t* dst_base, const fourmc_zst_item* __restrict__ items,
                         const ZstStream* st, ZstFrame* fr, uint32_t nf)
{
    const uint32_t f = blockIdx.x;
    if (f >= nf) return;
    const int lane = threadIdx.x;
    const uint32_t s = fr[f].stream;
    if (!fr[f].has_sum || !st[s].exec || f - st[s].frame0 >= st[s].n_ok || fr[f].result < 0) return;
    const uint32_t want = rd32(img + items[s].image_off + fr[f].end_off - 4);
    const uint64_t h = xxh64_wave(dst_base + items[s].dst_off + fr[f].out_off, fr[f].out_size, lane);
    if (uint32_t(h) != want && lane == 0) fr[f].result = kSumBad;
}

// ------------------------------------------------------------------------------------------------ serial hand-back
// d_list[k]: a stream whose frame n_ok the stages above declined.  The one-wave decoder takes that frame and everything behind it.
__global__ __launch_bounds__(64)
void zst_serial_kernel(const uint8_t* __restrict__ img, uint8_t* dst_base, const fourmc_zst_item* __restrict__ items, ZstStream* st,
                       const ZstFrame* fr, const uint32_t* d_list, uint32_t m, uint8_t* litbufs)
{
    __shared__ ZState zs;
    if (blockIdx.x >= m) return;
    const int lane = threadIdx.x;
    const uint32_t s = d_list[blockIdx.x];
    const ZstFrame& F = fr[st[s].frame0 + st[s].n_ok];
    const uint64_t src_len = items[s].image_bytes - F.src_off, cap = items[s].dst_cap - st[s].total;
    int r = kErr;
    if (src_len <= 0x7FFFFFFFull)
        r = zstd_decode_frames(img + items[s].image_off + F.src_off, int(src_len), dst_base + items[s].dst_off + st[s].total,
                               int(cap < kFrameMax ? cap : kFrameMax), litbufs + size_t(blockIdx.x) * (kBlockMax + 128), &zs, lane, true);
    if (lane == 0) { st[s].serial_r = r; st[s].serial_ran = 1; }
}

// ------------------------------------------------------------------------------------------------ status
__global__ __launch_bounds__(64)
void zst_status_kernel(const fourmc_zst_item* __restrict__ items, uint32_t n, const ZstStream* st, const ZstFrame* fr, int has_dst,
                       fourmc_zst_status* out)
{
    const uint32_t i = blockIdx.x * 64u + threadIdx.x;
    if (i >= n) return;
    const ZstStream s = st[i];
    const uint64_t len = items[i].image_bytes;
    fourmc_zst_status r = {};
    r.total_bytes = s.total; r.fail_offset = len; r.reason = FOURMC_ZST_OK;
    r.frames = s.frames; r.skippable = s.skips; r.blocks = s.blocks;
    const bool declined = s.n_ok < s.frames;
    const ZstFrame* const F = declined ? &fr[s.frame0 + s.n_ok] : nullptr;
    auto fail_at = [&](const ZstFrame* f, int code) {
        r.reason = FOURMC_ZST_FRAME; r.fail_offset = f->src_off; r.codec_result = code;
        r.frames = uint32_t(f - &fr[s.frame0]); r.skippable = f->skips_before; r.blocks = f->blk0 - s.block0;
    };
    if (declined) fail_at(F, kErr);
    else if (s.walk_bad) { r.reason = FOURMC_ZST_FRAME; r.fail_offset = s.fail_off; r.codec_result = kErr; }
    if (has_dst) {
        if (!s.exec) { r.reason = FOURMC_ZST_DST_SMALL; r.codec_result = 0; }
        else {
            const ZstFrame* fe = nullptr;
            for (uint32_t k = 0; k < s.n_ok; k++) if (fr[s.frame0 + k].result < 0) { fe = &fr[s.frame0 + k]; break; }
            if (fe) { fail_at(fe, fe->result); r.decoded_bytes = fe->out_off; }
            else {
                r.decoded_bytes = s.total;
                uint32_t blocks = declined ? F->blk0 - s.block0 : s.blocks;
                atomicAdd(&g_zst_counts[0], (unsigned long long)s.n_ok);
                atomicAdd(&g_zst_counts[2], (unsigned long long)blocks);
                if (declined && s.serial_ran) {
                    atomicAdd(&g_zst_counts[1], 1ull);
                    if (s.serial_r >= 0) {                             // the frame and what followed it were good after all
                        r.reason = FOURMC_ZST_OK; r.fail_offset = len; r.codec_result = 0;
                        r.frames = s.frames; r.skippable = s.skips; r.blocks = s.blocks;
                        r.decoded_bytes = r.total_bytes = s.total + uint64_t(s.serial_r);
                    } else r.codec_result = s.serial_r;
                }
            }
        }
    }
    out[i] = r;
}

size_t align256(size_t v) { return (v + 255) & ~size_t(255); }

} // namespace

extern "C" size_t fourmc_zst_per_block_bytes(void) { return kZstPerBlock; }

extern "C" int fourmc_zst_counts(unsigned long long* c3)
{
    unsigned long long z[3] = {0, 0, 0};
    if (hipMemcpyFromSymbol(c3, HIP_SYMBOL(g_zst_counts), sizeof z) != hipSuccess) return -1;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_zst_counts), z, sizeof z) != hipSuccess) return -1;
    return 0;
}

#define ZST_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { snprintf(err, err_cap, "%s: %s", #x, hipGetErrorString(e_)); return FOURMC_EHIP; } } while (0)

// The decode of n streams (the single call is its n = 1 case).  Workspaces, through `ws`: 0 - the items, the stream records and,
// sized after the first read-back, the frame table, the block table, the hand-back list and the statuses (a buffer that grows loses
// its contents, so items and records go up again); 1 - the tables, literal area and sequence area of one round; 2 - the literal
// buffers of the serial decoder.  Synchronizations: the walk's counts, the sizes, the statuses; the size query takes the first two.
extern "C" int fourmc_zst_run(const void* d_images, void* d_dst, fourmc_zst_item* items, uint32_t n, uint32_t round_blocks,
                              fourmc_zst_ws_fn ws, void* ws_ctx, char* err, size_t err_cap, hipStream_t s)
{
    const uint8_t* const img = static_cast<const uint8_t*>(d_images);
    uint8_t* const dst = static_cast<uint8_t*>(d_dst);
    const size_t o_st = align256(size_t(n) * sizeof(fourmc_zst_item)), o_fr = o_st + align256(size_t(n) * sizeof(ZstStream));
    void* w = nullptr;
    if (int r = ws(ws_ctx, 0, o_fr, &w)) return r;
    char* base = static_cast<char*>(w);
    ZST_TRY(hipMemcpyAsync(base, items, size_t(n) * sizeof(fourmc_zst_item), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(zst_walk_kernel, dim3(n), dim3(64), 0, s, img, reinterpret_cast<const fourmc_zst_item*>(base), n,
                       reinterpret_cast<ZstStream*>(base + o_st), static_cast<ZstFrame*>(nullptr), static_cast<ZstBlock*>(nullptr), 0);
    ZST_TRY(hipGetLastError());
    std::vector<ZstStream> st(n);
    ZST_TRY(hipMemcpyAsync(st.data(), base + o_st, size_t(n) * sizeof(ZstStream), hipMemcpyDeviceToHost, s));
    ZST_TRY(hipStreamSynchronize(s));                                  // 1: the counts
    uint64_t nf64 = 0, nb64 = 0;
    for (uint32_t i = 0; i < n; i++) {
        st[i].frame0 = uint32_t(nf64); st[i].block0 = uint32_t(nb64);
        nf64 += st[i].frames; nb64 += st[i].walked;
        if (nf64 > 0x7FFFFFFFull || nb64 > 0x7FFFFFFFull) { snprintf(err, err_cap, "zsts_decompress: more than 0x7FFFFFFF frames or blocks"); return FOURMC_EUNSUP; }
    }
    const uint32_t nf = uint32_t(nf64), nb = uint32_t(nb64);
    const size_t o_bk = o_fr + align256(size_t(nf) * sizeof(ZstFrame)), o_list = o_bk + align256(size_t(nb) * sizeof(ZstBlock));
    const size_t o_out = o_list + align256(size_t(n) * 4), o_end = o_out + align256(size_t(n) * sizeof(fourmc_zst_status));
    if (int r = ws(ws_ctx, 0, o_end, &w)) return r;
    base = static_cast<char*>(w);
    auto* d_items = reinterpret_cast<const fourmc_zst_item*>(base);
    auto* d_st = reinterpret_cast<ZstStream*>(base + o_st);
    auto* d_fr = reinterpret_cast<ZstFrame*>(base + o_fr);
    auto* d_bk = reinterpret_cast<ZstBlock*>(base + o_bk);
    auto* d_list = reinterpret_cast<uint32_t*>(base + o_list);
    auto* d_out = reinterpret_cast<fourmc_zst_status*>(base + o_out);
    ZST_TRY(hipMemcpyAsync(base, items, size_t(n) * sizeof(fourmc_zst_item), hipMemcpyHostToDevice, s));
    ZST_TRY(hipMemcpyAsync(d_st, st.data(), size_t(n) * sizeof(ZstStream), hipMemcpyHostToDevice, s));
    const uint32_t R = nb < round_blocks ? (nb ? nb : 1u) : round_blocks;
    uint8_t* work = nullptr;
    if (nb) {
        hipLaunchKernelGGL(zst_walk_kernel, dim3(n), dim3(64), 0, s, img, d_items, n, d_st, d_fr, d_bk, 1);
        hipLaunchKernelGGL(zst_headers_kernel, dim3((nb + 255) / 256), dim3(256), 0, s, img, d_bk, nb);
        hipLaunchKernelGGL(zst_scan_kernel, dim3(1), dim3(64), 0, s, d_bk, nb);
        ZST_TRY(hipGetLastError());
        void* w1 = nullptr;
        if (int r = ws(ws_ctx, 1, size_t(R) * kZstPerBlock + 256, &w1)) return r;
        work = static_cast<uint8_t*>(w1);
    }
    const bool one_round = nb <= R;
    auto entropy = [&](uint32_t r0) {
        const uint32_t r1 = nb - r0 < R ? nb : r0 + R;
        hipLaunchKernelGGL(zst_entropy_kernel, dim3((r1 - r0 + 63) / 64), dim3(64), 0, s, img, d_bk, r0, r1, work, R);
        return r1;
    };
    for (uint32_t r0 = 0; r0 < nb; r0 += R) entropy(r0);
    hipLaunchKernelGGL(zst_sizes_kernel, dim3(n), dim3(64), 0, s, d_items, n, d_st, d_fr, d_bk, dst ? 1 : 0);
    if (!dst) hipLaunchKernelGGL(zst_status_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_items, n, d_st, d_fr, 0, d_out);
    ZST_TRY(hipGetLastError());
    std::vector<fourmc_zst_status> back(n);
    if (!dst) ZST_TRY(hipMemcpyAsync(back.data(), d_out, size_t(n) * sizeof(fourmc_zst_status), hipMemcpyDeviceToHost, s));
    else ZST_TRY(hipMemcpyAsync(st.data(), d_st, size_t(n) * sizeof(ZstStream), hipMemcpyDeviceToHost, s));
    ZST_TRY(hipStreamSynchronize(s));                                  // 2: the sizes
    if (dst) {
        std::vector<uint32_t> list;
        bool any = false;
        for (uint32_t i = 0; i < n; i++) {
            if (!st[i].exec) continue;
            if (st[i].n_ok) any = true;
            if (st[i].n_ok < st[i].frames) list.push_back(i);
        }
        if (any && nf) {
            for (uint32_t r0 = 0; r0 < nb; r0 += R) {
                const uint32_t r1 = one_round ? nb : entropy(r0);      // one round: the triples and literals are still there
                hipLaunchKernelGGL(zst_exec_kernel, dim3(nf), dim3(64), 0, s, img, dst, d_items, d_st, d_fr, d_bk, nf, r0, r1, work, R);
            }
            hipLaunchKernelGGL(zst_checksum_kernel, dim3(nf), dim3(64), 0, s, img, dst, d_items, d_st, d_fr, nf);
            ZST_TRY(hipGetLastError());
        }
        if (!list.empty()) {
            void* w2 = nullptr;
            if (int r = ws(ws_ctx, 2, list.size() * size_t(kBlockMax + 128), &w2)) return r;
            ZST_TRY(hipMemcpyAsync(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(zst_serial_kernel, dim3(uint32_t(list.size())), dim3(64), 0, s, img, dst, d_items, d_st, d_fr, d_list,
                               uint32_t(list.size()), static_cast<uint8_t*>(w2));
        }
        hipLaunchKernelGGL(zst_status_kernel, dim3((n + 63) / 64), dim3(64), 0, s, d_items, n, d_st, d_fr, 1, d_out);
        ZST_TRY(hipGetLastError());
        ZST_TRY(hipMemcpyAsync(back.data(), d_out, size_t(n) * sizeof(fourmc_zst_status), hipMemcpyDeviceToHost, s));
        ZST_TRY(hipStreamSynchronize(s));                              // 3: the statuses
    }
    for (uint32_t i = 0; i < n; i++) items[i].status = back[i];
    return FOURMC_OK;
}
