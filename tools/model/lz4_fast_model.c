/*
 * tools/model/lz4_fast_model.c - executable lane-level model of the exact LZ4 fast encoder (4mc_amd/csrc/lz4_encode.hip, K2)
 * and of its emitter (4mc_amd/csrc/lz4emit.h).  Plain C99.  It follows the KERNEL's control, not the reference's: every
 * wave-wide statement is a loop over 64 lanes, a ballot is a 64-bit mask, atomicMax / atomicMin on the table and the scoreboard
 * are done for real (their result does not depend on lane order), the scalar walk, the record round, the commit, the sparse
 * batch, sequence() and the drain are stated as the kernel states them.  The input ring moves no byte of the parse: its
 * bookkeeping (rend, reload, rotate, reset, ralign, the shifts of piece_store) is kept for the trace alone and every byte is
 * read from the source.  Test / design aid only; not product.
 *   gcc -O2 -std=c99 -shared -fPIC -o liblz4_fast_model.so tools/model/lz4_fast_model.c
 *   gcc -O1 -g -std=c99 -fsanitize=address,undefined -DLF_MAIN -Ioracle tools/model/lz4_fast_model.c oracle/lz4_port.c   (its own main)
 *
 * The trace (lf_trace: four tables of int32 rows, filled like orc_trace of oracle/oracle.h - a row is written whole or not at
 * all and n[] counts every word - and the counters K2_PROF counts, in the same places):
 *   LF_T_WIN  LF_WIN_WORDS  one row per dense window: sp0, k0, retest, LF_EXIT_*, 1 when the record limit ended the window loop too,
 *             inner iterations, record rounds, stop lane (64: none), capok, literals from before the window (-1: the anchor lies
 *             inside), then lo/hi pairs of m_hit, m_cond, m_dirty, m_slow, sat, second lanes, lanes refused by distance, lanes
 *             refused by check bits, then the set of LF_BK_* among hit lanes, the set of LF_FW_* among hit lanes, the largest
 *             number of lanes in one slot
 *   LF_T_SEQ  LF_SEQ_WORDS  one row per sequence, in order: window number (-1: sparse batch), lane, the position that hit, its
 *             candidate, literals, mcode, LF_HOW_*, 1 for a re-test hit
 *   LF_T_BATCH LF_BATCH_WORDS one row per sparse batch: sp, k0, rt, wide, cut lane (64: none), event lane (64: none), LF_EVK_*,
 *             1 when a lane had h == h2, cregs of the event lane, room, eq
 *   LF_T_EV   LF_EV_WORDS   event rows, unused words 0: LF_EV_* first, each described where it is written
 *
 * Mutants (tests/test_lz4_enc_shapes_cpu.py): -DLF_MUTANT=k takes ONE decision wrongly; the list stands in LF_MUTANTS of that
 * test with the same numbers.  0 or undefined: the model.
 */
#ifndef LF_MUTANT
#define LF_MUTANT 0
#endif
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* ---- constants of the kernel, restated --------------------------------------------------------------------------------------- */
#define K_HASHLOG   12                   /* lz4_encode.hip:49 */
#define K_SMALLLIM  (65536 + 11)         /* lz4_encode.hip:50 */
#define K_MAXDIST   65535u               /* lz4_encode.hip:51 */
#define K_MFLIMIT   12                   /* lz4_encode.hip:52 */
#define K_LASTLIT   5                    /* lz4_encode.hip:52 */
#define K_MINLEN    13                   /* lz4_encode.hip:52 */
#define K_SCORE     1024                 /* lz4_encode.hip:53 */
#define K_PIECE     1024u                /* lz4_encode.hip:57 */
#define K_PIECELOG  10                   /* lz4_encode.hip:57 */
#define K_RING      (2 * K_PIECE)        /* lz4_encode.hip:57 */
#define K_WINDOW_NEED 132                /* lz4_encode.hip:281  sp + 132 <= un */
#define K_K0_MAX    32                   /* lz4_encode.hip:281  k0 <= 32 */
#define K_CAPOK     (LF_MUTANT == 15 ? 256u : 320u)   /* lz4_encode.hip:439 */
#define K_RECLAST   0x80000000u          /* lz4emit.h:17 */
#define K_RECSLACK  128u                 /* lz4emit.h:19 */
#define K_BLOCKSIZE (4u << 20)           /* include/fourmc_gpu.h FOURMC_BLOCKSIZE */
#define K_WIDE      1024u                /* lz4_encode.hip:234  a + 1024 <= matchlimit && mcode >= 64 */
#define K_LONGLIT   64u                  /* lz4emit.h:96  lit > 64: the whole wave copies */

enum { LF_T_WIN = 0, LF_T_SEQ = 1, LF_T_BATCH = 2, LF_T_EV = 3 };
enum { LF_WIN_WORDS = 29, LF_SEQ_WORDS = 8, LF_BATCH_WORDS = 11, LF_EV_WORDS = 12 };
enum { LF_EXIT_NONE = 0, LF_EXIT_CROSS, LF_EXIT_DCUT, LF_EXIT_SCUT, LF_EXIT_LAST, LF_EXIT_FULL };
enum { LF_HOW_WALK = 0, LF_HOW_GENERAL, LF_HOW_SEQ_SLOW /* m_slow or a candidate below 4 */, LF_HOW_SEQ_CAPOK, LF_HOW_SEQ_CATCHUP /* 5: the catch-up goes on in memory */,
       LF_HOW_SEQ_RUN_RT, LF_HOW_SEQ_SECOND_VISITED, LF_HOW_SEQ_SECOND_ENTRY, LF_HOW_SEQ_SPARSE };
enum { LF_EVK_NONE = 0, LF_EVK_HIT, LF_EVK_TERM };
enum { LF_BK_0 = 0, LF_BK_1, LF_BK_2, LF_BK_3, LF_BK_4_C4, LF_BK_4_MORE };
enum { LF_FW_LT24 = 0, LF_FW_24_55, LF_FW_56 };
enum { LF_EV_SECOND = 1,    /* a second lane resolved: sp0, lane, predecessor lane, visited, hitA, hit, LF_PRED_*, 1 when it went back to the walk (gen) */
       LF_EV_RUN_RT,        /* sp0, lane, 0 miss / 1 hit / 2 refused because e < 2 */
       LF_EV_SEQUENCE,      /* ip, rt_hit, backward rounds (0: the loop did not run), bytes it added, LF_BSTOP_*, wide rounds, 16-byte piece
                               of the wide loop's mismatch (-1: none), narrow rounds, 1 when the match ended at matchlimit, return value, site of a return 2 (1, 2) */
       LF_EV_RING,          /* sp0, LF_RING_*, ralign, c_hi == rend, jump past rend, sh > 0 seen, sh < 0 seen, |sh| >= 16 seen */
       LF_EV_DRAIN,         /* records drained, 1 when a sequence() call wrote the last of them */
       LF_EV_TERM,          /* sp0, lane, d (1..6): a hit lane the term rule looked at with back == 5, 1 when it ended the chain */
       LF_EV_LAND,          /* sp0, landing lane of a chosen match (cur), 1 from sequence() */
       LF_EV_GENERAL5       /* sp0, lane: a first general step stopped by the catch-up limit 5 */ };
enum { LF_PRED_PROBE = 0, LF_PRED_OUTSIDE, LF_PRED_IN_MATCH, LF_PRED_REFILL, LF_PRED_XINT };
enum { LF_BSTOP_NONE = 0, LF_BSTOP_ANCHOR, LF_BSTOP_CAND, LF_BSTOP_BYTE };
enum { LF_RING_RELOAD = 0, LF_RING_ROTATE, LF_RING_RESET, LF_RING_KEPT };
enum { LF_C_NWIN = 0, LF_C_NSEQ, LF_C_NSLOW, LF_C_NONE, LF_C_CROSS, LF_C_DCUT, LF_C_SCUT, LF_C_NIT, LF_C_NREL, LF_C_NROT, LF_C_NRST, LF_C_COUNT };

typedef struct { int32_t* ev[4]; int cap[4]; int n[4]; int64_t cnt[LF_C_COUNT]; } lf_trace;
typedef struct { uint32_t x, y, z, w; } lf_rec;

typedef struct {
    const uint8_t* src; uint8_t* dst; uint32_t un; int n, cap, limited, u32tab, cbits, src_align;
    uint32_t cmask, tab32[1 << K_HASHLOG], score[K_SCORE], op, anchor, rc, reccap, lim, matchlimit, rend;
    lf_rec* rec; lf_trace* tr; int nwin, last_by_sequence, oob;
} LF;

static void lf_put(lf_trace* t, int table, const int32_t* row, int words)
{
    int i;
    if (!t) return;
    if (t->ev[table] && t->n[table] + words <= t->cap[table]) for (i = 0; i < words; i++) t->ev[table][t->n[table] + i] = row[i];
    t->n[table] += words;
}
static void lf_ev(lf_trace* t, int k, uint32_t a, int32_t b, int32_t c, int32_t d, int32_t e, int32_t f, int32_t g, int32_t h, int32_t i, int32_t j, int32_t l)
{ const int32_t row[LF_EV_WORDS] = {k, (int32_t)a, b, c, d, e, f, g, h, i, j, l}; lf_put(t, LF_T_EV, row, LF_EV_WORDS); }
#define CNT(c, k) do { if ((c)->tr) (c)->tr->cnt[k]++; } while (0)

static uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint64_t rd64(const uint8_t* p) { uint64_t v; memcpy(&v, p, 8); return v; }
static uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
static int imin(int a, int b) { return a < b ? a : b; }
static int ctz64(uint64_t v) { int k = 0; if (!v) return 64; while (!(v & 1)) { v >>= 1; k++; } return k; }
static int top64(uint64_t v) { int k = 63; while (!(v >> k)) k--; return k; }
static int pop64(uint64_t v) { int k = 0; for (; v; v &= v - 1) k++; return k; }
static uint64_t below_mask(int lane) { return ~(~0ull << lane); }                    /* lane 0..63 */
static int clz32(uint32_t v) { int k = 0; if (!v) return 32; while (!(v & 0x80000000u)) { v <<= 1; k++; } return k; }

static uint32_t hash_of(const LF* c, uint64_t v)                                       /* lz4_encode.hip:109-113 */
{
    if (c->u32tab) return (uint32_t)(((v << 24) * 889523592379ULL) >> (64 - K_HASHLOG));
    return ((uint32_t)v * 2654435761u) >> (32 - (K_HASHLOG + 1));
}
static uint32_t probe_offset(uint32_t K)                                               /* lz4_encode.hip:68-73 */
{
    if (K == 0) return 0;
    { const uint32_t T = K - 1, m = T >> 6, r = T & 63; return 1 + T + 32 * m * (m - 1) + m * r; }
}
static uint32_t chk_of(const LF* c, uint32_t w) { return (c->u32tab && c->cbits) ? (w * 2654435761u) >> (32 - c->cbits) : 0u; }
static uint32_t enc(const LF* c, uint32_t pos, uint32_t ck) { return c->u32tab ? (pos << c->cbits) | ck : pos; }
static uint32_t tab_get(const LF* c, uint32_t h) { return c->u32tab ? c->tab32[h] : (uint32_t)((const uint16_t*)c->tab32)[h]; }
static void tab_put(LF* c, uint32_t h, uint32_t pos, uint32_t ck) { if (c->u32tab) c->tab32[h] = enc(c, pos, ck); else ((uint16_t*)c->tab32)[h] = (uint16_t)pos; }
/* equal bytes of a[] and b[], at most `most` */
static uint32_t eq_fwd(const uint8_t* a, const uint8_t* b, uint32_t most) { uint32_t k = 0; while (k < most && a[k] == b[k]) k++; return k; }

/* ---- the emitter (lz4emit.h:81-109), one record after the other ---------------------------------------------------------------- */
static uint32_t put_len(uint8_t* d, uint32_t rest)                                     /* lz4emit.h:56-62 */
{
    const uint32_t n255 = rest / 255;
    memset(d, 255, n255);
    d[n255] = (uint8_t)(rest - n255 * 255);
    return n255 + 1;
}
static void emit_records(LF* c, uint32_t cnt, uint32_t tail)
{
    uint32_t i;
    for (i = 0; i < cnt; i++) {
        const lf_rec r = c->rec[i];
        const uint32_t nxt = i + 1 < cnt ? c->rec[i + 1].y : tail;
        const int last = (r.w & K_RECLAST) != 0;
        const uint32_t lit = r.z, mcode = last ? 0u : nxt - r.y - lit - 4;
        uint32_t p = r.x;
        {   /* the model's own check: a record whose bytes would leave [0, cap) is not written (a mutant's, or a bug's) */
            const uint64_t end = (uint64_t)p + 1 + (lit >= 15 ? (lit - 15) / 255 + 1 : 0) + lit + (last ? 0 : 2 + (mcode >= 15 ? (mcode - 15) / 255 + 1 : 0));
            if (end > (uint64_t)(c->cap > 0 ? c->cap : 1) || (uint64_t)r.y + lit > c->un) { c->oob = 1; continue; }
        }
        c->dst[p++] = (uint8_t)((umin(lit, 15u) << 4) | umin(mcode, 15u));
        if (lit >= 15) p += put_len(c->dst + p, lit - 15);
        memcpy(c->dst + p, c->src + r.y, lit);
        if (!last) {
            const uint32_t q = p + lit;
            c->dst[q] = (uint8_t)r.w; c->dst[q + 1] = (uint8_t)(r.w >> 8);
            if (mcode >= 15) put_len(c->dst + q + 2, mcode - 15);
        }
    }
}
static void drain_records(LF* c)                                                       /* lz4_encode.hip:117-122, :276 */
{
    lf_ev(c->tr, LF_EV_DRAIN, c->rc, c->last_by_sequence, 0, 0, 0, 0, 0, 0, 0, 0, 0);
    emit_records(c, c->rc, LF_MUTANT == 17 ? 0u : c->anchor);
    c->rc = 0;
}

/* ---- sequence() (lz4_encode.hip:201-265) ----------------------------------------------------------------------------------------- */
static int sequence(LF* c, uint32_t ip, uint32_t cand, int rt_hit, uint32_t back, int back_more, uint32_t fwd, int fwd_more, uint32_t* ip_out,
                    int win, int lane, int how)
{
    const uint8_t* src = c->src;
    const uint32_t ip_hit = ip, cand_hit = cand;
    uint32_t token_pos, lit = 0, off, mcode;
    int brounds = 0, bstop = LF_BSTOP_NONE, wrounds = 0, wpiece = -1, nrounds = 0, ret;
    uint32_t badd = 0;
    if (rt_hit) token_pos = c->op++;
    else {
        const uint32_t maxback = umin(ip - c->anchor, cand);
        uint32_t b = umin(back, maxback);
        if (back_more && maxback > back) {
            for (;;) {
                int t = 64, l;
                brounds++;
                for (l = 0; l < 64; l++) {                          /* ballot of the first lane that is not ok */
                    const uint32_t j = b + (uint32_t)l + 1;
                    const int ok = (j <= maxback) && src[ip - j] == src[cand - j];
                    if (!ok) { t = l; break; }
                }
                b += (uint32_t)t; badd += (uint32_t)t;
                if (t < 64) break;
            }
        }
        bstop = b == ip - c->anchor ? LF_BSTOP_ANCHOR : b == cand ? LF_BSTOP_CAND : LF_BSTOP_BYTE;
        ip -= b; cand -= b;
        fwd += b;
        lit = ip - c->anchor;
        token_pos = c->op++;
        if (c->limited && c->op + lit + (2 + 1 + K_LASTLIT) + lit / 255 > (uint32_t)c->cap) {
            lf_ev(c->tr, LF_EV_SEQUENCE, ip_hit, rt_hit, brounds, (int32_t)badd, bstop, 0, -1, 0, 0, 2, 1);
            return 2;
        }
        if (lit >= 15) c->op += (lit - 15) / 255 + 1;
        c->op += lit;
    }
    off = ip - cand;
    c->op += 2;
    mcode = fwd;
    if (fwd_more) {
        uint32_t a = ip + 4 + mcode, b = cand + 4 + mcode;
        for (;;) {
            if (a + K_WIDE <= c->matchlimit && (mcode >= 64 || LF_MUTANT == 16)) {
                const uint32_t eq = eq_fwd(src + a, src + b, K_WIDE);
                wrounds++;
                if (eq < K_WIDE) { mcode += eq; wpiece = (int)(eq / 16); break; }
                mcode += K_WIDE; a += K_WIDE; b += K_WIDE;
            } else {
                uint32_t t = 0;
                nrounds++;
                while (t < 64 && a + t < c->matchlimit && src[a + t] == src[b + t]) t++;
                if (t < 64) { mcode += t; break; }
                mcode += 64; a += 64; b += 64;
            }
        }
    }
    ip = ip + mcode + 4;
    if (c->limited && c->op + (1 + K_LASTLIT) + (mcode + 240) / 255 > (uint32_t)c->cap) {
        lf_ev(c->tr, LF_EV_SEQUENCE, ip_hit, rt_hit, brounds, (int32_t)badd, bstop, wrounds, wpiece, nrounds, ip == c->matchlimit, 2, 2);
        return 2;
    }
    if (mcode >= 15) c->op += (mcode - 15) / 255 + 1;
    c->rec[c->rc].x = token_pos; c->rec[c->rc].y = c->anchor; c->rec[c->rc].z = lit; c->rec[c->rc].w = off;
    c->rc++;
    c->last_by_sequence = 1;
    {   const int32_t row[LF_SEQ_WORDS] = {win, lane, (int32_t)ip_hit, (int32_t)cand_hit, (int32_t)lit, (int32_t)mcode, how, rt_hit};
        lf_put(c->tr, LF_T_SEQ, row, LF_SEQ_WORDS); }
    c->anchor = ip;
    *ip_out = ip;
    ret = ip >= c->lim ? 1 : 0;
    lf_ev(c->tr, LF_EV_SEQUENCE, ip_hit, rt_hit, brounds, (int32_t)badd, bstop, wrounds, wpiece, nrounds, ip == c->matchlimit, ret, 0);
    return ret;
}

/* ---- the ring's bookkeeping (lz4_encode.hip:174-189, :297-318) -------------------------------------------------------------------- */
static void piece_shifts(const LF* c, uint32_t k, uint32_t ralign, int* pos, int* neg, int* far_)
{
    int lane;
    for (lane = 0; lane < 64; lane++) {
        const int p = (int)(k * K_PIECE + 16u * (uint32_t)lane) - (int)ralign;
        const int q = imin(p > 0 ? p : 0, c->n - 16);
        const int sh = p - q;
        if (sh > 0) *pos = 1;
        if (sh < 0) *neg = 1;
        if (sh >= 16 || sh <= -16) *far_ = 1;
    }
}

/* ---- one block (lz4_encode.hip:124-745) -------------------------------------------------------------------------------------------- */
static int encode_block(LF* c)
{
    const uint8_t* src = c->src;
    const uint32_t un = c->un;
    uint32_t sp = 1, k0 = 0, rc_lim;
    int retest = 0, i;
    c->limited = c->cap < c->n + c->n / 255 + 16;
    c->op = 0; c->anchor = 0; c->rc = 0; c->rend = 0; c->nwin = 0; c->last_by_sequence = 0; c->oob = 0;
    memset(c->tab32, 0, sizeof c->tab32);
    for (i = 0; i < K_SCORE; i++) c->score[i] = 0xFFFFFFFFu;
    c->cbits = 0;
    if (c->u32tab) { c->cbits = clz32((uint32_t)(c->n - 1) | 1u) - 1; if (c->cbits < 0) c->cbits = 0; }
    c->cmask = (1u << c->cbits) - 1;
    if (c->n < K_MINLEN) goto last_literals;
    c->lim = un - K_MFLIMIT + 1;
    c->matchlimit = un - K_LASTLIT;
    tab_put(c, hash_of(c, rd64(src)), 0, chk_of(c, rd32(src)));          /* (n >= 13: eight bytes are there) */
    rc_lim = un / 4 > c->reccap - K_RECSLACK ? c->reccap - K_RECSLACK : 0xFFFFFFFFu;
    for (;;) {
        int status = 0;
        if (c->rc > rc_lim) drain_records(c);
        if (sp >= 4) while (sp + K_WINDOW_NEED <= un && k0 <= K_K0_MAX) {
            /* ---------------------------------------------------------------- dense window */
            const uint32_t sp0 = sp;
            uint32_t h[64], ck[64], ent[64], cnd[64], info[64], w4[64], fw[64], bk[64], nxt[64], nextE[64], fin[64], wpred[64], term_d[64];
            int pass[64], near[64], hit[64], slow[64], dirty[64], second[64], first[64], pred[64], hitA[64], sat[64];
            uint32_t h2 = 0xFFFFFFFFu, ck2 = 0;
            uint64_t m_cond = 0, m_hit = 0, m_dirty = 0, m_slow = 0, m_sat = 0, m_second = 0, m_nodist = 0, m_nochk = 0;
            uint64_t stop2, stop1, hd2, hd, stp, selw = 0, xint = 0, in1 = 0;
            int rounds = 0, cur = 0, anc, any = retest, fresh = 1, gen = 0, stoplane = 64, scut, lane, capok, inner = 0, exit_kind = LF_EXIT_NONE;
            int bkset = 0, fwset = 0, most_in_slot = 1;
            const int win = c->nwin++, k0_in = (int)k0, retest_in = retest;
            uint32_t before; int32_t before_word;
            if (c->u32tab) {
                const uint32_t ralign = (uint32_t)c->src_align & 15u;
                const uint32_t a0 = sp0 + ralign - 4;
                const uint32_t c_lo = a0 >> K_PIECELOG, c_hi = (a0 + 127) >> K_PIECELOG;
                int kind = LF_RING_KEPT, p = 0, ng = 0, fr = 0;
                if (c_hi >= c->rend) {
                    if (c->rend != 0 && c_hi == c->rend) { CNT(c, LF_C_NROT); kind = LF_RING_ROTATE; piece_shifts(c, c->rend, ralign, &p, &ng, &fr); c->rend++; }
                    else {
                        CNT(c, LF_C_NREL); kind = LF_RING_RELOAD;
                        piece_shifts(c, c_lo, ralign, &p, &ng, &fr); piece_shifts(c, c_lo + 1, ralign, &p, &ng, &fr);
                        lf_ev(c->tr, LF_EV_RING, sp0, kind, (int32_t)ralign, 0, c->rend != 0 && c_hi > c->rend, p, ng, fr, 0, 0, 0);
                        c->rend = c_lo + 2;
                        kind = -1;
                    }
                }
                if (kind == LF_RING_ROTATE) lf_ev(c->tr, LF_EV_RING, sp0, kind, (int32_t)ralign, 1, 0, p, ng, fr, 0, 0, 0);
            }
            CNT(c, LF_C_NWIN);
            for (lane = 0; lane < 64; lane++) {
                const uint32_t pos = sp0 + (uint32_t)lane;
                w4[lane] = rd32(src + pos);
                h[lane] = hash_of(c, rd64(src + pos));
                ck[lane] = chk_of(c, w4[lane]);
            }
            if (retest) { h2 = hash_of(c, rd64(src + sp0 - 2)); ck2 = chk_of(c, rd32(src + sp0 - 2)); tab_put(c, h2, sp0 - 2, ck2); }
            for (lane = 0; lane < 64; lane++) ent[lane] = tab_get(c, h[lane]);
            if (c->u32tab) {
                uint32_t tag[64];
                int anyloser = 0;
                for (lane = 0; lane < 64; lane++) { const uint32_t v = 0x80000000u | (uint32_t)(63 - lane); if (c->tab32[h[lane]] < v) c->tab32[h[lane]] = v; }
                for (lane = 0; lane < 64; lane++) tag[lane] = c->tab32[h[lane]];
                for (lane = 0; lane < 64; lane++) {
                    pred[lane] = 63 - (int)(tag[lane] & 63);
                    wpred[lane] = w4[pred[lane]];
                    first[lane] = pred[lane] == lane;
                    dirty[lane] = 0; second[lane] = 0;
                    if (!first[lane]) anyloser = 1;
                }
                if (anyloser) {
                    for (lane = 0; lane < 64; lane++) if (!first[lane]) { const uint32_t v = 0x80000040u | (uint32_t)(63 - lane); if (c->tab32[h[lane]] < v) c->tab32[h[lane]] = v; }
                    for (lane = 0; lane < 64; lane++) {
                        second[lane] = !first[lane] && 63 - (int)(c->tab32[h[lane]] & 63) == lane;
                        if (LF_MUTANT == 1) second[lane] = !first[lane];
                        dirty[lane] = !first[lane] && !second[lane];
                    }
                }
                for (lane = 0; lane < 64; lane++) if (first[lane]) c->tab32[h[lane]] = ent[lane];
            } else {
                for (lane = 0; lane < 64; lane++) { uint32_t* sc = &c->score[h[lane] & (K_SCORE - 1)]; if ((uint32_t)lane < *sc) *sc = (uint32_t)lane; }
                for (lane = 0; lane < 64; lane++) { dirty[lane] = c->score[h[lane] & (K_SCORE - 1)] != (uint32_t)lane; second[lane] = 0; pred[lane] = 0; wpred[lane] = 0; first[lane] = !dirty[lane]; }
                for (lane = 0; lane < 64; lane++) c->score[h[lane] & (K_SCORE - 1)] = 0xFFFFFFFFu;
            }
            for (lane = 0; lane < 64; lane++) {
                const uint32_t pos = sp0 + (uint32_t)lane;
                const uint32_t cc = c->u32tab ? ent[lane] >> c->cbits : ent[lane];
                int distok = 1, chkok = 1, l2, same = 1;
                cnd[lane] = cc;
                if (c->u32tab) {
                    distok = LF_MUTANT == 10 ? cc + K_MAXDIST > pos : cc + K_MAXDIST >= pos;
                    chkok = (cc == 0 && LF_MUTANT != 9) || (ent[lane] & c->cmask) == ck[lane];
                }
                pass[lane] = distok && chkok;
                if (!distok) m_nodist |= 1ull << lane; else if (!chkok) m_nochk |= 1ull << lane;
                near[lane] = pass[lane] && cc >= 4;
                hit[lane] = 0; slow[lane] = 0; fw[lane] = 0; bk[lane] = 0;
                if (near[lane]) {
                    hit[lane] = rd32(src + cc) == w4[lane];
                    { uint32_t b = 0; while (b < 4 && src[pos - 1 - b] == src[cc - 1 - b]) b++; bk[lane] = b; }
                    fw[lane] = eq_fwd(src + pos + 4, src + cc + 4, 24);
                }
                sat[lane] = hit[lane] && fw[lane] == 24;
                if (sat[lane] && LF_MUTANT != 12) fw[lane] = 24 + eq_fwd(src + pos + 28, src + cc + 28, 32);
                if (sat[lane]) m_sat |= 1ull << lane;
                if (!pass[lane]) info[lane] = (uint32_t)lane + 4;
                else if (cc >= 4) {
                    const int full = LF_MUTANT == 12 ? fw[lane] == 24 : fw[lane] == 56;
                    slow[lane] = full;
                    info[lane] = ((uint32_t)lane + 4 + fw[lane]) | ((bk[lane] == 4 && cc > 4 ? 5u : bk[lane]) << 8) | (bk[lane] << 12) | ((uint32_t)(bk[lane] == 4) << 15) | ((uint32_t)full << 16);
                } else {
                    hit[lane] = rd32(src + cc) == w4[lane];
                    slow[lane] = 1;
                    info[lane] = ((uint32_t)lane + 4) | (1u << 15) | (1u << 16);
                }
                hitA[lane] = second[lane] && wpred[lane] == w4[lane];
                if (second[lane]) m_second |= 1ull << lane;
                if (second[lane] && (hitA[lane] || hit[lane])) m_cond |= 1ull << lane;
                if (hit[lane]) m_hit |= 1ull << lane;
                if (dirty[lane]) m_dirty |= 1ull << lane;
                if (hit[lane] && slow[lane]) m_slow |= 1ull << lane;
                if (hit[lane] && c->tr) {
                    if (cc >= 4) bkset |= 1 << (bk[lane] < 4 ? (int)bk[lane] : cc == 4 ? LF_BK_4_C4 : LF_BK_4_MORE);
                    fwset |= 1 << (fw[lane] < 24 ? LF_FW_LT24 : fw[lane] < 56 ? LF_FW_24_55 : LF_FW_56);
                }
                if (c->tr) { for (l2 = 0; l2 < lane; l2++) same += h[l2] == h[lane]; if (same > most_in_slot) most_in_slot = same; }
            }
            m_hit &= ~m_cond;
            before = c->anchor < sp0 ? sp0 - c->anchor : 0u;
            before_word = c->anchor <= sp0 ? (int32_t)before : -1;
            capok = !c->limited || c->op + before + before / 255 + K_CAPOK <= (uint32_t)c->cap;
            stop2 = m_dirty | m_slow | m_cond | (capok ? 0ull : m_hit);
            stop1 = stop2;
            scut = (!retest && k0 > 1) ? (LF_MUTANT == 6 ? 66 : 65) - (int)k0 : 64;
            if (scut < 64) stop1 |= 1ull << scut;
            hd2 = m_hit | stop2;
            hd = m_hit | stop1; stp = stop1;
            anc = (int)(c->anchor - sp0);
            {   const uint64_t evs = m_hit | stop2;
                for (lane = 0; lane < 64; lane++) {
                    const uint32_t land = info[lane] & 255, la = land & 63;
                    const uint32_t d = (uint32_t)ctz64(evs >> lane), d2 = (uint32_t)ctz64(evs >> la);
                    const uint32_t E = (uint32_t)lane + d, E2 = la + d2;
                    const uint32_t infE = info[E & 63], infE2 = info[E2 & 63];
                    const uint32_t ds = (uint32_t)ctz64(stop2 >> lane), ds2 = (uint32_t)ctz64(stop2 >> la);
                    const uint32_t endE = 0x8000u | umin(E, 64u), endE2 = 0x8000u | umin(E2, 64u);
                    const uint32_t farlim = LF_MUTANT == 11 ? 4 : 5;
                    const int far_ = d >= farlim, far2 = d2 >= farlim, nothing = ds == d, nothing2 = ds2 == d2, out = land >= 64;
                    const uint32_t goE = (infE & 255) | (E << 8), goE2 = (infE2 & 255) | (E2 << 8);
                    const int term = nothing | ((((infE >> 8) & 7) == 5) & far_), term2 = nothing2 | ((((infE2 >> 8) & 7) == 5) & far2);
                    const uint32_t nl = term2 ? endE2 : goE2;
                    nxt[lane] = term ? endE : goE;
                    nextE[lane] = (out | term2) ? (uint32_t)lane : E2;
                    fin[lane] = out ? 0x4000u : nl;
                    term_d[lane] = (!out && !nothing2 && ((infE2 >> 8) & 7) == 5) ? d2 | ((uint32_t)term2 << 8) : 0u;   /* trace only */
                }
            }
            for (;;) {
                uint64_t sel = 0;
                int reason = -1, e = 0, how = LF_HOW_WALK, seqhow = LF_HOW_SEQ_SLOW;
                const int anc0 = anc;
                CNT(c, LF_C_NIT); inner++;
                if (gen || anc != cur || hd != hd2) {
                    const uint64_t ev = hd & (~0ull << cur);
                    gen = 0;
                    how = LF_HOW_GENERAL;
                    if (!ev) reason = 0;
                    else {
                        uint32_t inf;
                        e = ctz64(ev);
                        inf = info[e];
                        if ((stp >> e) & 1) reason = 1;
                        else if (imin((int)((inf >> 8) & 7), e - anc) == 5 && LF_MUTANT != 18) { reason = 1; lf_ev(c->tr, LF_EV_GENERAL5, sp0, e, 0, 0, 0, 0, 0, 0, 0, 0, 0); seqhow = LF_HOW_SEQ_CATCHUP; }
                        else {
                            sel = 1ull << e;
                            anc = cur = (int)(inf & 255);
                            hd = hd2; stp = stop2;
                            if (cur >= 64) reason = 2;
                        }
                    }
                }
                if (reason < 0) {
                    uint32_t t;
                    CNT(c, LF_C_NSEQ);
                    t = nxt[cur];
                    if (t & 0x8000u) { e = (int)(t & 127); reason = e == 64 ? 0 : 1; }
                    else {
                        uint32_t E = (t >> 8) & 63, f;
                        for (;;) {
                            uint32_t n1;
                            sel |= 1ull << E;
                            if (term_d[E]) lf_ev(c->tr, LF_EV_TERM, sp0, (int32_t)E, (int32_t)(term_d[E] & 255), (int32_t)(term_d[E] >> 8), 0, 0, 0, 0, 0, 0, 0);
                            n1 = nextE[E];
                            if (n1 == E) break;
                            E = n1;
                        }
                        f = fin[E];
                        cur = anc = (int)(info[E] & 255);
                        if (f & 0x4000u) reason = 2;
                        else { e = (int)(f & 127); reason = e == 64 ? 0 : 1; }
                    }
                }
                if (sel) {
                    /* the record round (lz4_encode.hip:529-547) */
                    uint32_t size[64], incl[64], myanc_pos[64], run = 0;
                    uint64_t in = 0;
                    for (lane = 0; lane < 64; lane++) {
                        const int mine = (int)((sel >> lane) & 1);
                        const uint64_t below = sel & below_mask(lane);
                        const int P = below ? top64(below) : 0;
                        const int endP = (int)(info[P] & 255);
                        const int myanc = below ? endP : anc0;
                        const uint32_t b = (uint32_t)imin((int)((info[lane] >> 8) & 7), lane - myanc);
                        const uint32_t lt = (uint32_t)(lane - myanc) - b, mc = (info[lane] & 255) - (uint32_t)lane - 4 + b;
                        myanc_pos[lane] = sp0 + (uint32_t)myanc;
                        size[lane] = mine ? 3 + lt + (lt >= 15 ? (lt - 15) / 255 + 1 : 0u) + (mc >= 15 ? 1u : 0u) : 0u;
                        run += size[lane]; incl[lane] = run;
                        if (mine) {
                            lf_rec* r = &c->rec[c->rc + (uint32_t)pop64(below)];
                            const int32_t row[LF_SEQ_WORDS] = {win, lane, (int32_t)(sp0 + (uint32_t)lane), (int32_t)cnd[lane], (int32_t)lt, (int32_t)mc, how,
                                                               (below || any) && lane == myanc};
                            r->x = c->op + incl[lane] - size[lane]; r->y = myanc_pos[lane]; r->z = lt; r->w = sp0 + (uint32_t)lane - cnd[lane];
                            lf_put(c->tr, LF_T_SEQ, row, LF_SEQ_WORDS);
                            lf_ev(c->tr, LF_EV_LAND, sp0, (int32_t)(info[lane] & 255), 0, 0, 0, 0, 0, 0, 0, 0, 0);
                        }
                        if (below && lane < endP && (lane != endP - 2 || LF_MUTANT == 4)) in |= 1ull << lane;
                    }
                    c->rc += (uint32_t)pop64(sel);
                    c->op += incl[63];
                    c->anchor = sp0 + (uint32_t)anc;
                    c->last_by_sequence = 0;
                    selw |= sel; any = 1; fresh = 0;
                    if (rounds++ == 0) in1 = in;
                }
                if (reason == 0) {
                    const int s = any ? anc + (LF_MUTANT == 20 ? 0 : 1) : -(int)k0;
                    CNT(c, LF_C_NONE);
                    k0 = (uint32_t)(64 - s); sp = sp0 + 64; retest = 0;
                    break;
                }
                if (reason == 2) {
                    const uint32_t ip = sp0 + (uint32_t)cur;
                    if (ip >= c->lim) { status = 1; break; }
                    sp = ip; k0 = 0; retest = 1;
                    CNT(c, LF_C_CROSS); exit_kind = LF_EXIT_CROSS;
                    break;
                }
                {
                    const int may_rt = ((m_dirty >> e) & 1) && any && e == anc;
                    int run_rt = may_rt && e >= 2 && (h[e >= 2 ? e - 2 : 0] == h[e] || LF_MUTANT == 3);
                    uint32_t s_cand, s_inf;
                    if (LF_MUTANT == 2) run_rt = 0;
                    if (may_rt && e < 2) lf_ev(c->tr, LF_EV_RUN_RT, sp0, e, 2, 0, 0, 0, 0, 0, 0, 0, 0);
                    if (!run_rt && (((m_dirty >> e) & 1) || (fresh && e == scut))) {
                        stoplane = e;
                        if ((m_dirty >> e) & 1) { CNT(c, LF_C_DCUT); exit_kind = LF_EXIT_DCUT; } else { CNT(c, LF_C_SCUT); exit_kind = LF_EXIT_SCUT; }
                        if (any && e == anc) { k0 = 0; retest = 1; }
                        else { k0 = (uint32_t)(e - (any ? anc + 1 : -(int)k0)); retest = 0; }
                        sp = sp0 + (uint32_t)e;
                        break;
                    }
                    s_cand = cnd[e]; s_inf = info[e];
                    if (seqhow != LF_HOW_SEQ_CATCHUP) seqhow = ((m_slow >> e) & 1) ? LF_HOW_SEQ_SLOW : !capok ? LF_HOW_SEQ_CAPOK : LF_HOW_SEQ_CATCHUP;
                    if (run_rt) {
                        if (w4[e - 2] != w4[e]) {
                            lf_ev(c->tr, LF_EV_RUN_RT, sp0, e, 0, 0, 0, 0, 0, 0, 0, 0, 0);
                            cur = e + 1;
                            if (cur < 64) continue;
                            k0 = (uint32_t)(64 - (anc + 1)); sp = sp0 + 64; retest = 0;
                            break;
                        }
                        lf_ev(c->tr, LF_EV_RUN_RT, sp0, e, 1, 0, 0, 0, 0, 0, 0, 0, 0);
                        s_cand = sp0 + (uint32_t)e - 2; s_inf = ((uint32_t)e + 4) | (1u << 15) | (1u << 16);
                        seqhow = LF_HOW_SEQ_RUN_RT;
                    } else if ((m_cond >> e) & 1) {
                        const int j = pred[e];
                        int inside_j, visited, use, place;
                        {   const uint64_t below = selw & below_mask(j);
                            const int P = below ? top64(below) : 0;
                            const int endP = (int)(info[P] & 255);
                            const int inm = below && j < endP && (j != endP - 2 || LF_MUTANT == 4);
                            const int inx = (int)((xint >> j) & 1) && LF_MUTANT != 7;
                            inside_j = inm || inx;
                            place = j >= anc ? LF_PRED_PROBE : inm ? LF_PRED_IN_MATCH : inx ? LF_PRED_XINT : (below && j == endP - 2) ? LF_PRED_REFILL : LF_PRED_OUTSIDE;
                        }
                        visited = j >= anc || !inside_j;
                        use = (visited || LF_MUTANT == 8) ? hitA[e] : hit[e];
                        if (!use) {
                            lf_ev(c->tr, LF_EV_SECOND, sp0, e, j, visited, hitA[e], hit[e], place, 0, 0, 0, 0);
                            cur = e + 1;
                            if (cur < 64) continue;
                            k0 = (uint32_t)(64 - (any ? anc + 1 : -(int)k0)); sp = sp0 + 64; retest = 0;
                            break;
                        }
                        if (visited) { s_cand = sp0 + (uint32_t)j; s_inf = ((uint32_t)e + 4) | (1u << 15) | (1u << 16); seqhow = LF_HOW_SEQ_SECOND_VISITED; }
                        else if (capok && !((m_slow >> e) & 1) && imin((int)((s_inf >> 8) & 7), e - anc) != 5) {
                            lf_ev(c->tr, LF_EV_SECOND, sp0, e, j, visited, hitA[e], hit[e], place, 1, 0, 0, 0);
                            stop2 &= ~(1ull << e); stp &= ~(1ull << e); gen = 1;
                            continue;
                        } else seqhow = LF_HOW_SEQ_SECOND_ENTRY;
                        lf_ev(c->tr, LF_EV_SECOND, sp0, e, j, visited, hitA[e], hit[e], place, 0, 0, 0, 0);
                    }
                    {
                        uint32_t ip = 0;
                        CNT(c, LF_C_NSLOW);
                        status = sequence(c, sp0 + (uint32_t)e, s_cand, any && e == anc, (s_inf >> 12) & 7, (int)((s_inf >> 15) & 1),
                                          (s_inf & 255) - (uint32_t)e - 4, (int)((s_inf >> 16) & 1), &ip, win, e, seqhow);
                        if (status) break;
                        any = 1; fresh = 0;
                        lf_ev(c->tr, LF_EV_LAND, sp0, (int32_t)(ip - sp0 > 255 ? 255 : ip - sp0), 1, 0, 0, 0, 0, 0, 0, 0, 0);
                        if (ip - sp0 >= 64) {
                            xint |= ~1ull << e;
                            sp = ip; k0 = 0; retest = 1;
                            exit_kind = LF_EXIT_CROSS;       /* (the kernel counts no window end here: K2_PROF's `cross` is reason 2 alone) */
                            break;
                        }
                        cur = anc = (int)(ip - sp0);
                        xint |= (~1ull << e) & ~(~0ull << cur) & ~(LF_MUTANT == 21 ? 0ull : 1ull << (cur - 2));
                        hd = hd2; stp = stop2;
                    }
                }
            }
            if (status) exit_kind = status == 1 ? LF_EXIT_LAST : LF_EXIT_FULL;
            if (!status) {
                /* commit (lz4_encode.hip:626-641) */
                uint64_t in = in1;
                if (rounds > 1 && LF_MUTANT != 22) {
                    in = 0;
                    for (lane = 0; lane < 64; lane++) {
                        const uint64_t below = selw & below_mask(lane);
                        const int P = below ? top64(below) : 0;
                        const int endP = (int)(info[P] & 255);
                        if (below && lane < endP && (lane != endP - 2 || LF_MUTANT == 4)) in |= 1ull << lane;
                    }
                }
                for (i = 0; i < 64; i++) {
                    const uint32_t pos = sp0 + (uint32_t)(LF_MUTANT == 5 ? 63 - i : i);
                    lane = LF_MUTANT == 5 ? 63 - i : i;
                    if (lane < stoplane && !(((in | xint) >> lane) & 1)) {
                        if (c->u32tab) { const uint32_t v = enc(c, pos, ck[lane]); if (LF_MUTANT == 5 || c->tab32[h[lane]] < v) c->tab32[h[lane]] = v; }
                        else ((uint16_t*)c->tab32)[h[lane]] = (uint16_t)pos;        /* the store is repeated until the latest position stands: lanes in rising order */
                    }
                }
            }
            {   const int32_t row[LF_WIN_WORDS] = {(int32_t)sp0, k0_in, retest_in, exit_kind, !status && c->rc > rc_lim, inner, rounds, stoplane, capok,
                    before_word,
                    (int32_t)m_hit, (int32_t)(m_hit >> 32), (int32_t)m_cond, (int32_t)(m_cond >> 32), (int32_t)m_dirty, (int32_t)(m_dirty >> 32),
                    (int32_t)m_slow, (int32_t)(m_slow >> 32), (int32_t)m_sat, (int32_t)(m_sat >> 32), (int32_t)m_second, (int32_t)(m_second >> 32),
                    (int32_t)m_nodist, (int32_t)(m_nodist >> 32), (int32_t)m_nochk, (int32_t)(m_nochk >> 32), bkset, fwset, most_in_slot};
                lf_put(c->tr, LF_T_WIN, row, LF_WIN_WORDS); }
            if (status) break;
            if (c->rc > rc_lim) break;
        }
        if (status == 2) return 0;
        if (status == 1) goto last_literals;
        if (c->rc > rc_lim) continue;
        /* -------------------------------------------------------------------- sparse batch (lz4_encode.hip:653-729) */
        {
            const int rt = retest, wide = sp >= 4;
            uint32_t pos[64], h[64], ck[64], cc[64], w4[64], h2 = 0xFFFFFFFFu, ck2 = 0;
            int in_range[64], pass[64], shared[64], hit[64], cregs[64], lane, cut, e, e_is_hit, same_h2 = 0;
            uint64_t m_cut = 0, m_term = 0, m_hit = 0, ev;
            if (c->u32tab && c->rend != 0) { for (i = 0; i < K_SCORE; i++) c->score[i] = 0xFFFFFFFFu; c->rend = 0; CNT(c, LF_C_NRST); lf_ev(c->tr, LF_EV_RING, sp, LF_RING_RESET, 0, 0, 0, 0, 0, 0, 0, 0, 0); }
            for (lane = 0; lane < 64; lane++) {
                uint32_t next, rp;
                if (k0 == 0) { pos[lane] = sp + (uint32_t)lane; next = pos[lane] + 1; }
                else { pos[lane] = sp + probe_offset(k0 + (uint32_t)lane) - probe_offset(k0); next = sp + probe_offset(k0 + (uint32_t)lane + 1) - probe_offset(k0); }
                in_range[lane] = next <= c->lim;
                rp = in_range[lane] ? pos[lane] : (wide ? 4u : 0u);
                w4[lane] = rd32(src + rp);
                h[lane] = hash_of(c, rd64(src + rp));
                ck[lane] = chk_of(c, w4[lane]);
            }
            if (rt) { h2 = hash_of(c, rd64(src + sp - 2)); ck2 = chk_of(c, rd32(src + sp - 2)); }
            for (lane = 0; lane < 64; lane++) {
                uint32_t entv = tab_get(c, h[lane]);
                if (h[lane] == h2) { same_h2 = 1; if (LF_MUTANT != 14) entv = enc(c, sp - 2, ck2); }
                cc[lane] = c->u32tab ? entv >> c->cbits : entv;
                pass[lane] = in_range[lane] && (!c->u32tab || ((LF_MUTANT == 10 ? cc[lane] + K_MAXDIST > pos[lane] : cc[lane] + K_MAXDIST >= pos[lane]) &&
                                                                  ((cc[lane] == 0 && LF_MUTANT != 9) || (entv & c->cmask) == ck[lane])));
            }
            for (lane = 0; lane < 64; lane++) { uint32_t* sc = &c->score[h[lane] & (K_SCORE - 1)]; if ((uint32_t)lane < *sc) *sc = (uint32_t)lane; }
            for (lane = 0; lane < 64; lane++) shared[lane] = c->score[h[lane] & (K_SCORE - 1)] != (uint32_t)lane;
            for (lane = 0; lane < 64; lane++) c->score[h[lane] & (K_SCORE - 1)] = 0xFFFFFFFFu;
            for (lane = 0; lane < 64; lane++) {
                cregs[lane] = pass[lane] && wide && cc[lane] >= 4;
                hit[lane] = pass[lane] && rd32(src + cc[lane]) == w4[lane];
                if (shared[lane] && LF_MUTANT != 19) m_cut |= 1ull << lane;
                if (!in_range[lane]) m_term |= 1ull << lane;
                if (hit[lane]) m_hit |= 1ull << lane;
            }
            cut = ctz64(m_cut);
            ev = (m_term | m_hit) & (cut >= 64 ? ~0ull : ((1ull << cut) - 1));
            e = ev ? ctz64(ev) : cut;
            e_is_hit = ev && ((m_hit >> e) & 1) && !((m_term >> e) & 1);
            if (rt) tab_put(c, h2, sp - 2, ck2);
            for (lane = 0; lane < 64; lane++) if (lane < e || (lane == e && (e_is_hit || (LF_MUTANT == 13 && ev)))) tab_put(c, h[lane], pos[lane], ck[lane]);
            {   int32_t row[LF_BATCH_WORDS] = {(int32_t)sp, (int32_t)k0, rt, wide, cut, ev ? e : 64, !ev ? LF_EVK_NONE : e_is_hit ? LF_EVK_HIT : LF_EVK_TERM, same_h2, 0, -1, -1};
                if (ev && e_is_hit && cregs[e]) { row[8] = 1; row[9] = (int32_t)(c->matchlimit - (pos[e] + 4)); row[10] = (int32_t)eq_fwd(src + pos[e] + 4, src + cc[e] + 4, 8); }
                lf_put(c->tr, LF_T_BATCH, row, LF_BATCH_WORDS); }
            if (ev) {
                uint32_t back = 0, fwd = 0, ipn = 0;
                int back_more = 1, fwd_more = 1, st;
                if (!e_is_hit) goto last_literals;
                if (cregs[e]) {
                    const uint32_t ip = pos[e], cd = cc[e], room = c->matchlimit - (ip + 4);
                    uint32_t eq;
                    while (back < 4 && src[ip - 1 - back] == src[cd - 1 - back]) back++;
                    back_more = back == 4;
                    eq = eq_fwd(src + ip + 4, src + cd + 4, 8);
                    fwd = umin(eq, room);
                    fwd_more = !((eq < 8) || (room <= 8));
                }
                st = sequence(c, pos[e], cc[e], rt && e == 0, back, back_more, fwd, fwd_more, &ipn, -1, e, LF_HOW_SEQ_SPARSE);
                if (st == 2) return 0;
                if (st == 1) goto last_literals;
                sp = ipn; k0 = 0; retest = 1;
                continue;
            }
            sp = sp + (k0 == 0 ? (uint32_t)e : probe_offset(k0 + (uint32_t)e) - probe_offset(k0));
            k0 = k0 + (uint32_t)e - (rt ? 1u : 0u);
            retest = 0;
        }
    }
last_literals:
    {
        const uint32_t run = (uint32_t)c->n - c->anchor;
        if (c->limited && c->op + run + 1 + (run + 255 - 15) / 255 > (uint32_t)c->cap) return 0;
        c->rec[c->rc].x = c->op; c->rec[c->rc].y = c->anchor; c->rec[c->rc].z = run; c->rec[c->rc].w = K_RECLAST;
        c->rc++;
        c->op += 1 + (run >= 15 ? (run - 15) / 255 + 1 : 0) + run;
    }
    return (int)c->op;
}

/* The kernel's result and bytes for one block in raw mode (lz4_encode.hip:752-779 with container_mode 0, then lz4_emit.hip:42).
 * `src_align` stands for the source address's low four bits, `reccap` for the record area (0: the default, FOURMC_BLOCKSIZE / 4 + 256);
 * `dst` needs max(cap, 1) bytes.  A block that does not fit returns 0; what a drain wrote before that stays in dst, as on the device. */
int lz4_fast_model_compress(const uint8_t* src, uint8_t* dst, int n, int cap, int src_align, uint32_t reccap, lf_trace* trace)
{
    LF* c;
    int r;
    if ((uint32_t)n > 0x7E000000u) return 0;
    if (n == 0) { if (cap < 16 && cap <= 0) return 0; dst[0] = 0; return 1; }
    c = (LF*)malloc(sizeof *c);
    if (!c) return -1;
    c->src = src; c->dst = dst; c->n = n; c->un = (uint32_t)n; c->cap = cap; c->src_align = src_align; c->tr = trace;
    c->u32tab = n >= K_SMALLLIM;
    c->reccap = reccap >= 2 * K_RECSLACK ? reccap : K_BLOCKSIZE / 4 + 2 * K_RECSLACK;       /* lz4_encode.hip:787-791 */
    c->rec = (lf_rec*)malloc(((size_t)c->reccap + 2 * K_RECSLACK) * sizeof(lf_rec));
    if (!c->rec) { free(c); return -1; }
    r = encode_block(c);
    if (r > 0) { if (c->rc > c->reccap) r = -2; else emit_records(c, c->rc, 0); }         /* (-2: the model's own check that an area never overflows) */
    if (c->oob) r = -3;                                                                     /* (-3: bytes outside the capacity) */
    free(c->rec); free(c);
    return r;
}

#ifdef LF_MAIN
/* Stand-alone check, for a sanitizer build: every line of the manifest names a file of input bytes, a capacity, a source alignment and
 * a record capacity; the model must give the port's result and bytes. */
#include <stdio.h>
#include "oracle.h"
int main(int argc, char** argv)
{
    FILE* m;
    char path[1024];
    int cap, align, reccap, bad = 0, runs = 0;
    if (argc != 2 || !(m = fopen(argv[1], "r"))) { fprintf(stderr, "usage: %s manifest\n", argv[0]); return 2; }
    while (fscanf(m, "%1023s %d %d %d", path, &cap, &align, &reccap) == 4) {
        FILE* f = fopen(path, "rb");
        long n;
        uint8_t *raw, *src, *a, *b;
        int ra, rb;
        if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
        fseek(f, 0, SEEK_END); n = ftell(f); fseek(f, 0, SEEK_SET);
        raw = (uint8_t*)malloc((size_t)n + 1);                    /* exactly n bytes behind the pointer: a read past the block is an error */
        src = raw;
        if (n && fread(src, 1, (size_t)n, f) != (size_t)n) return 2;
        fclose(f);
        a = (uint8_t*)calloc((size_t)(cap > 0 ? cap : 1), 1); b = (uint8_t*)calloc((size_t)(cap > 0 ? cap : 1), 1);
        ra = lz4_fast_model_compress(src, a, (int)n, cap, align, (uint32_t)reccap, NULL);
        rb = orc_lz4_compress_fast(src, b, (int)n, cap);
        if (ra != rb || (ra > 0 && memcmp(a, b, (size_t)ra))) { fprintf(stderr, "differs: %s cap %d align %d records %d: %d / %d\n", path, cap, align, reccap, ra, rb); bad++; }
        runs++;
        free(raw); free(a); free(b);
    }
    fclose(m);
    printf("%d runs, %d differ\n", runs, bad);
    return bad ? 1 : 0;
}
#endif
