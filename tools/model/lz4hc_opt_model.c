/*
 * tools/model/lz4hc_opt_model.c - executable model of the LZ4 HC level 9..12 encoder (4mc_amd/csrc/lz4hc_opt_encode.hip).
 * The serial parse is the kernel's own text (4mc_amd/csrc/lz4hc_opt_core.h, included here); the primitives below restate
 * what the wave does in parallel, lane by lane over 64 emulated lanes, where the decomposition could go wrong:
 *   - the batched insert: 64 positions per step, a position chains to the nearest earlier lane with its hash (lane distance),
 *     the first lane of a hash to the old head (delta clamped to 65535), the last lane of a hash becomes the head;
 *   - the chain-swap scan: deltas read 64 at a time, the step/accel recurrence (lz4hc.c:326-333) walked out of that chunk;
 *   - the price update: every lane computes its position from opt[cur] / opt[cur - ll] read before any lane writes, and
 *     last_match_pos is taken from the lane that holds ml == matchML.
 * The byte counts and emission are plain loops.  The CPU test compares this with the reference's LZ4_compress_HC.
 * Test / design aid only; not product.
 *   gcc -O2 -shared -fPIC -I4mc_amd/csrc -o /tmp/liblz4hc_opt_model.so tools/model/lz4hc_opt_model.c
 *
 * Mutants (tests/test_hc_opt_shapes_cpu.py): -DHO_MUTANT=n makes one primitive subtly wrong, so that the test can show that
 * the catalogue tests/hc_opt_shapes.py tells the difference.  1: the insert does not clamp a delta at 65535; 2: the first lane
 * of a hash becomes the head, not the last; 3: the swap scan never reloads its 64 deltas; 4: the swap scan drops matchChainPos;
 * 5: ho_opt_match returns the old last_match_pos when matchML > 64; 6: ho_count_back ignores maxn (it stops at the candidate's
 * own position alone).  0 or undefined: the model.
 */
#ifndef HO_MUTANT
#define HO_MUTANT 0
#endif
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define HO_FN static
#include "lz4hc_opt_core.h"

HO_FN uint32_t ho_ld32(const HO* c, uint32_t p) { uint32_t v; memcpy(&v, c->src + p, 4); return v; }
HO_FN uint32_t ho_ld16(const HO* c, uint32_t p) { uint16_t v; memcpy(&v, c->src + p, 2); return v; }
HO_FN uint32_t ho_chain(const HO* c, uint32_t idx) { return c->chain[idx & 0xFFFFu]; }
HO_FN uint32_t ho_head(const HO* c, uint32_t h) { return c->heads[h]; }

HO_FN void ho_insert(HO* c, uint32_t upto)
{
    while (c->ntu < upto) {
        uint32_t h[64], delta[64];
        int on[64], lane, l;
        for (lane = 0; lane < 64; lane++) {                 /* every lane reads before any lane writes */
            const uint32_t pos = c->ntu + (uint32_t)lane;
            on[lane] = pos < upto;
            if (!on[lane]) continue;
            h[lane] = ho_hash(ho_ld32(c, pos));
            for (l = lane - 1; l >= 0 && h[l] != h[lane]; l--) ;
            if (l >= 0) delta[lane] = (uint32_t)(lane - l);
            else { delta[lane] = pos + HO_IDX0 - c->heads[h[lane]]; if (delta[lane] > HO_MAXD && HO_MUTANT != 1) delta[lane] = HO_MAXD; }
        }
        for (lane = 0; lane < 64; lane++) {
            int later = 0;
            if (!on[lane]) continue;
            c->chain[(c->ntu + (uint32_t)lane) & 0xFFFFu] = (uint16_t)delta[lane];
            if (HO_MUTANT == 2) { for (l = lane - 1; l >= 0 && !later; l--) later = h[l] == h[lane]; }
            else for (l = lane + 1; l < 64 && !later; l++) later = on[l] && h[l] == h[lane];
            if (!later) c->heads[h[lane]] = c->ntu + (uint32_t)lane + HO_IDX0;
        }
        c->ntu = ho_min(upto, c->ntu + 64u);
    }
}

HO_FN uint32_t ho_count(const HO* c, uint32_t a, uint32_t b, uint32_t lim)
{ uint32_t n = 0; while (a + n < lim && c->src[a + n] == c->src[b + n]) n++; return n; }
HO_FN uint32_t ho_count_back(const HO* c, uint32_t a, uint32_t b, uint32_t maxn)
{ uint32_t n = 0; if (HO_MUTANT == 6) maxn = b; while (n < maxn && c->src[a - n - 1] == c->src[b - n - 1]) n++; return n; }
HO_FN uint32_t ho_run(const HO* c, uint32_t a, uint32_t byte, uint32_t lim)
{ uint32_t n = 0; while (a + n < lim && c->src[a + n] == byte) n++; return n; }
HO_FN uint32_t ho_run_back(const HO* c, uint32_t a, uint32_t byte)
{ uint32_t n = 0; while (n < a && c->src[a - n - 1] == byte) n++; return n; }

HO_FN uint32_t ho_swap_scan(const HO* c, uint32_t matchIndex, int end, uint32_t* mcp)
{
    uint32_t dist = 1, chunk[64];
    int pos = 0, step = 1, accel = 1 << 4, base = -64, lane;
    for (; pos < end; pos += step) {
        uint32_t cd;
        if (HO_MUTANT == 3 ? base < 0 : pos - base >= 64) {
            base = pos;
            for (lane = 0; lane < 64; lane++) chunk[lane] = c->chain[(matchIndex + (uint32_t)base + (uint32_t)lane) & 0xFFFFu];
        }
        cd = chunk[(pos - base) & 63];
        step = accel++ >> 4;
        if (cd > dist) { dist = cd; if (HO_MUTANT != 4) *mcp = (uint32_t)pos; accel = 1 << 4; }
    }
    return dist;
}

HO_FN HOpt ho_opt_get(const HO* c, int i) { return c->opt[i]; }
HO_FN void ho_opt_put(HO* c, int i, HOpt r) { c->opt[i] = r; }

HO_FN void ho_opt_first(HO* c, int llen, int matchML, int off)
{
    int p;
    for (p = 0; p <= matchML; p++) {
        HOpt r;
        if (p < HO_MINMATCH) { r.price = ho_lit_price(llen + p); r.off = 0; r.mlen = 1; r.litlen = llen + p; }
        else { r.price = ho_seq_price(llen, p); r.off = off; r.mlen = p; r.litlen = llen; }
        c->opt[p] = r;
    }
}

HO_FN int ho_opt_match(HO* c, int cur, int matchML, int off, int last)
{
    const HOpt base = c->opt[cur];
    const int before = (base.mlen == 1 && cur > base.litlen) ? c->opt[cur - base.litlen].price : 0;
    HOpt out[HO_OPT_NUM];
    int wr[HO_OPT_NUM], k, newlast = last;
    for (k = 1; k <= matchML; k++) {                         /* lane k-1 (mod 64): reads, decides */
        const int pos = cur + k;
        const HOpt old = c->opt[pos];
        wr[k] = 0;
        if (k < HO_MINMATCH) {
            const int price = base.price - ho_lit_price(base.litlen) + ho_lit_price(base.litlen + k);
            if (price < old.price) { out[k].price = price; out[k].off = 0; out[k].mlen = 1; out[k].litlen = base.litlen + k; wr[k] = 1; }
        } else {
            int ll, price;
            if (base.mlen == 1) { ll = base.litlen; price = before + ho_seq_price(ll, k); }
            else { ll = 0; price = base.price + ho_seq_price(0, k); }
            if (pos > last + HO_TRAIL || price <= old.price) {
                if (k == matchML && last < pos) newlast = pos;
                out[k].price = price; out[k].off = off; out[k].mlen = k; out[k].litlen = ll; wr[k] = 1;
            }
        }
    }
    for (k = 1; k <= matchML; k++) if (wr[k]) c->opt[cur + k] = out[k];     /* then every lane writes */
    return (HO_MUTANT == 5 && matchML > 64) ? last : newlast;
}

HO_FN void put_len(HO* c, uint32_t rest) { while (rest >= 255) { c->dst[c->op++] = 255; rest -= 255; } c->dst[c->op++] = (uint8_t)rest; }

HO_FN int ho_emit(HO* c, uint32_t* ipp, uint32_t* anchorp, int ml, uint32_t match)
{
    const uint32_t ip = *ipp, anchor = *anchorp, lit = ip - anchor, token = c->op;
    const uint32_t off = ip - match, mcode = (uint32_t)ml - HO_MINMATCH;
    uint32_t tok;
    if (c->limited && (int64_t)token + 1 + lit / 255 + lit + (2 + 1 + HO_LASTLIT) > c->cap) return 1;
    c->op = token + 1;
    if (lit >= 15) { tok = 0xF0; put_len(c, lit - 15); } else tok = lit << 4;
    memcpy(c->dst + c->op, c->src + anchor, lit); c->op += lit;
    c->dst[c->op++] = (uint8_t)off; c->dst[c->op++] = (uint8_t)(off >> 8);
    if (c->limited && (int64_t)c->op + mcode / 255 + (1 + HO_LASTLIT) > c->cap) return 1;
    if (mcode >= 15) { tok += 15; put_len(c, mcode - 15); } else tok += mcode;
    c->dst[token] = (uint8_t)tok;
    *ipp = ip + (uint32_t)ml; *anchorp = *ipp;
    return 0;
}

HO_FN int ho_last(HO* c, uint32_t anchor)
{
    const uint32_t run = c->n - anchor, add = (run + 255 - 15) / 255;
    if (c->limited && (int64_t)c->op + 1 + add + run > c->cap) return 0;
    if (run >= 15) { c->dst[c->op++] = 0xF0; put_len(c, run - 15); } else c->dst[c->op++] = (uint8_t)(run << 4);
    memcpy(c->dst + c->op, c->src + anchor, run);
    return (int)(c->op + run);
}

/* result = LZ4_compress_HC(src, dst, n, cap, level) for any level at or above 9 after lz4hc.c:840-841's mapping */
int lz4hc_opt_model_compress(const uint8_t* src, uint8_t* dst, int n, int cap, int level)
{
    HO c;
    int r;
    if (n < 0) return 0;
    if (level < 1) level = 9;
    if (level > 12) level = 12;
    if (level < 9) return -1;                                /* levels 1..8 are not this model's */
    memset(&c, 0, sizeof c);
    c.src = src; c.dst = dst; c.n = (uint32_t)n; c.cap = cap;
    c.limited = (int64_t)cap < (int64_t)n + n / 255 + 16;
    c.chain = (uint16_t*)malloc(65536 * sizeof(uint16_t));
    c.heads = (uint32_t*)calloc((size_t)1 << HO_HASHLOG, sizeof(uint32_t));
    c.opt = (HOpt*)calloc(HO_OPT_RECS, sizeof(HOpt));
    if (!c.chain || !c.heads || !c.opt) { free(c.chain); free(c.heads); free(c.opt); return -2; }
    memset(c.chain, 0xFF, 65536 * sizeof(uint16_t));
    r = ho_compress(&c, level);
    free(c.chain); free(c.heads); free(c.opt);
    return r;
}
