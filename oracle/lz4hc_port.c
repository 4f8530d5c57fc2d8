/*
 * oracle/lz4hc_port.c — scalar restatement of LZ4_compress_HC at every level: the hash chain of levels 1..8
 * (4mc High = level 4, 4mc Ultra = level 8), the hash chain with pattern analysis of level 9 and the optimal
 * parser with pattern analysis and chain swap of levels 10..12 (the JNI compressBytesDirectHC(level) passes
 * any level; levels below 1 run as 9 and levels above 12 as 12, lz4hc.c:840-841).
 * TEST INFRASTRUCTURE, NOT PRODUCT (see oracle.h).
 *
 *   entry        LZ4_compress_HC            native/lz4/lz4hc.c:958-973 -> :939-949 -> :800-861
 *   parse        LZ4HC_compress_hashChain   native/lz4/lz4hc.c:553-788   (lazy 3-match arbitration)
 *   search       LZ4HC_InsertAndGetWiderMatch :239-447 with patternAnalysis = 0 (nbSearches <= 128,
 *                :565) and chainSwap = 0 (:461,:603,:648), no dictionary
 *   tables       LZ4HC_Insert :120-141, hash :82, table init :98-117 (indices start at 64 KiB)
 *   emit         LZ4HC_encodeSequence :467-548, last literals :735-762
 *   levels 9..12 LZ4HC_InsertAndGetWiderMatch :239-447 whole (pattern analysis :340-410, chain swap :317-338; no
 *                dictionary), LZ4HC_countPattern / _reverseCountPattern :176-224 for a one-byte pattern,
 *                prices :1276-1299, LZ4HC_FindLongerMatch :1307-1327, LZ4HC_compress_optimal :1330-1626
 *
 * Positions are plain offsets into the block; a table index is position + 65536 exactly as in the
 * reference (LZ4HC_init_internal), so an all-zero hash table means "no candidate".
 * Parity: pinned — byte-identical to oracle/_ref's LZ4_compress_HC at every level 1..8: on the edge
 * inputs at capacities bound / n-1 / n/3 (tests/test_oracle_golden.py), on every (input, capacity)
 * pair of the search-and-parse catalogue tests/hc_shapes.py (tests/test_hc_shapes_cpu.py), and, at
 * levels 4 and 8, to the per-block manifests of the reference CLI at `4mc -3` / `-4`
 * (tests/golden/corpus_manifest.json).  Levels 9..12: pinned on every (input, capacity) pair of tests/hc_opt_shapes.py, on
 * the inputs of tests/hc_opt_inputs.py and on corpus blocks (tests/test_hc_opt_shapes_cpu.py).
 *
 * orc_lz4hc_compress_ex additionally writes a trace of what the search and the parse did (oracle.h:
 * orc_trace); the catalogue's ledger is computed from it.  A NULL trace changes nothing.
 */
#include <stdlib.h>
#include <string.h>
#include "oracle.h"

#define HASH_LOG   15
#define MAXD       65536
#define MAX_DIST   65535
#define MINMATCH   4
#define MFLIMIT    12
#define LASTLIT    5
#define OPTIMAL_ML 18
#define IDX0       65536u                 /* index of position 0 */

typedef struct {
    uint32_t hash[1 << HASH_LOG];
    uint16_t chain[MAXD];
    uint32_t next_to_update;              /* index */
    const uint8_t* src;
} hc_t;

static uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
static uint16_t rd16(const uint8_t* p) { uint16_t v; memcpy(&v, p, 2); return v; }
static uint32_t hc_hash(const uint8_t* p) { return (rd32(p) * 2654435761u) >> (32 - HASH_LOG); }

static void hc_insert(hc_t* c, uint32_t ip /* position */)
{
    const uint32_t target = ip + IDX0;
    uint32_t idx = c->next_to_update;
    while (idx < target) {
        const uint32_t h = hc_hash(c->src + (idx - IDX0));
        uint32_t delta = idx - c->hash[h];
        if (delta > MAX_DIST) delta = MAX_DIST;
        c->chain[idx & 0xFFFF] = (uint16_t)delta;
        c->hash[h] = idx;
        idx++;
    }
    c->next_to_update = target;
}

static int count_fwd(const uint8_t* s, uint32_t a, uint32_t b, uint32_t lim)   /* a > b, stops at a == lim */
{
    const uint32_t a0 = a;
    while (a < lim && s[a] == s[b]) { a++; b++; }
    return (int)(a - a0);
}

/* best match for `ip`, allowed to start as early as `low` (lookback) and end by `high`; only
 * matches longer than `longest` count.  Returns the new longest; *mpos / *spos = match / start. */
static int hc_wider(hc_t* c, uint32_t ip, uint32_t low, uint32_t high, int longest,
                    uint32_t* mpos, uint32_t* spos, int attempts, orc_trace* t)
{
    const uint8_t* s = c->src;
    const int head_at = t ? t->n[ORC_TR_SEARCH] : 0, longest_in = longest;
    int walked = 0, win = -1;
    uint32_t last_delta = 0;
    int32_t w[ORC_TR_SEARCH_WORDS] = {0};
    const uint32_t ip_idx = ip + IDX0;
    const uint32_t lowest = (IDX0 + MAXD > ip_idx) ? IDX0 : ip_idx - MAX_DIST;
    const int lookback = (int)(ip - low);
    const uint32_t pattern = rd32(s + ip);
    uint32_t mi;
    hc_insert(c, ip);
    mi = c->hash[hc_hash(s + ip)];
    orc_tr_put(t, ORC_TR_SEARCH, w, ORC_TR_SEARCH_WORDS);                                   /* header: filled in at the end */
    while (mi >= lowest && attempts > 0) {
        const uint32_t m = mi - IDX0;
        int32_t cw[ORC_TR_CAND_WORDS] = {(int32_t)m, 0, 0, 0};
        attempts--;
        if (t && rd32(s + m) == pattern) {                               /* measured for the trace whatever the pre-filter says */
            int min = (int)low - (int)ip, b = 0;
            if (-(int)m > min) min = -(int)m;
            while (b > min && s[ip + b - 1] == s[m + b - 1]) b--;
            cw[1] = 1; cw[2] = count_fwd(s, ip + MINMATCH, m + MINMATCH, high); cw[3] = -b;
        }
        if (rd16(s + low + longest - 1) == rd16(s + m - lookback + longest - 1) && rd32(s + m) == pattern) {
            int back = 0, ml;
            if (lookback) {
                int min = (int)low - (int)ip;                      /* max(iMin - ip, mMin - match) */
                if (-(int)m > min) min = -(int)m;
                while (back > min && s[ip + back - 1] == s[m + back - 1]) back--;
            }
            ml = MINMATCH + count_fwd(s, ip + MINMATCH, m + MINMATCH, high) - back;
            if (ml > longest) { longest = ml; *mpos = m + back; *spos = ip + back; win = walked; }
        }
        orc_tr_put(t, ORC_TR_CAND, cw, ORC_TR_CAND_WORDS);
        walked++;
        last_delta = c->chain[mi & 0xFFFF];
        mi -= last_delta;
    }
    if (t && t->ev[ORC_TR_SEARCH] && head_at + ORC_TR_SEARCH_WORDS <= t->cap[ORC_TR_SEARCH]) {
        int32_t* h = t->ev[ORC_TR_SEARCH] + head_at;
        h[0] = t->n[ORC_TR_EMIT] / 3; h[1] = (int32_t)ip; h[2] = (int32_t)low; h[3] = longest_in; h[4] = walked;
        /* below `lowest`: an older position of this hash out of reach, or no position at all (empty bucket, or a delta that
         * was capped at insertion: 65535 steps back lies a word of another hash) */
        h[5] = mi >= lowest ? ORC_END_ATTEMPTS
             : (mi < IDX0 || (last_delta == MAX_DIST && hc_hash(s + (mi - IDX0)) != hc_hash(s + ip))) ? ORC_END_CHAIN : ORC_END_LOWEST;
        h[6] = win; h[7] = longest; h[8] = mi >= lowest ? (int32_t)(mi - IDX0) : -1;
    }
    return longest;
}

/* ---- levels 9..12 ---------------------------------------------------------------------------------------------------------- */
#define EV(t, ...) do { if (t) { const int32_t w_[ORC_HX_EV_WORDS] = {__VA_ARGS__}; orc_tr_put(t, ORC_TR_ARM, w_, ORC_HX_EV_WORDS); } } while (0)

/* an arm of the parse or a refusal: two words at levels 1..8, an event row at levels 9..12 (site: ORC_HX_SITE_*, -1 = levels 1..8) */
static void hc_arm(orc_trace* t, int site, int arm, uint32_t ip)
{
    if (site < 0) orc_tr_arm(t, arm, ip);
    else EV(t, arm, (int32_t)ip, site);
}

/* bytes equal to `b` from `a` on, short of `lim` (LZ4HC_countPattern for a pattern of one repeated byte) */
static uint32_t run_fwd(const uint8_t* s, uint32_t a, uint8_t b, uint32_t lim)
{
    const uint32_t a0 = a;
    while (a < lim && s[a] == b) a++;
    return a - a0;
}

/* bytes equal to `b` before `a`, down to position 0 (LZ4HC_reverseCountPattern, iLow = the block's start) */
static uint32_t run_back(const uint8_t* s, uint32_t a, uint8_t b)
{
    const uint32_t a0 = a;
    while (a > 0 && s[a - 1] == b) a--;
    return a0 - a;
}

/* LZ4HC_InsertAndGetWiderMatch with pattern analysis (`pa`) and chain swap (`swap`), as levels 9..12 call it.  The walk keeps an
 * index `mi` and, once a chain swap has chosen one, the offset `swap_at` inside the candidate whose chain it follows. */
static int hx_wider(hc_t* c, uint32_t ip, uint32_t low, uint32_t high, int longest, uint32_t* mpos, uint32_t* spos,
                    int attempts, int pa, int swap, orc_trace* t)
{
    const uint8_t* s = c->src;
    const int head_at = t ? t->n[ORC_TR_SEARCH] : 0, longest_in = longest;
    const int32_t ntu_in = (int32_t)(c->next_to_update - IDX0);
    const uint32_t ip_idx = ip + IDX0;
    const uint32_t lowest = (IDX0 + MAXD > ip_idx) ? IDX0 : ip_idx - MAX_DIST;
    const int lookback = (int)(ip - low);
    const uint32_t pattern = rd32(s + ip);
    const uint8_t pbyte = (uint8_t)pattern;
    int32_t w[ORC_HX_SEARCH_WORDS] = {0};
    int walked = 0, win = -1, broke = 0, by_pattern = 0;
    int rep = 0;                                   /* 0: not looked at yet, 1: not one repeated byte, 2: one repeated byte */
    uint32_t src_run = 0, swap_at = 0, mi;

    hc_insert(c, ip);
    mi = c->hash[hc_hash(s + ip)];
    orc_tr_put(t, ORC_TR_SEARCH, w, ORC_HX_SEARCH_WORDS);                 /* header: filled in at the end */
    while (mi >= lowest && attempts > 0) {
        const uint32_t m = mi - IDX0;
        const int probe = rd16(s + low + longest - 1) == rd16(s + m - lookback + longest - 1);
        const int eq4 = rd32(s + m) == pattern;
        int32_t cw[ORC_HX_CAND_WORDS] = {(int32_t)m, probe, eq4, 0, 0, -1, -1, ORC_HX_LEFT_CHAIN};
        int ml = 0;
        attempts--;
        if (eq4 && (t || probe)) {                 /* (measured for the trace whatever the probe says) */
            const int f = count_fwd(s, ip + MINMATCH, m + MINMATCH, high);
            int b = 0, room = lookback;
            if ((int)m < room) room = (int)m;      /* -max(iMin - ip, mMin - match) */
            while (b < room && s[ip - b - 1] == s[m - b - 1]) b++;
            cw[3] = f; cw[4] = b;
            cw[5] = ip + MINMATCH + f == high ? ORC_HX_STOP_LIMIT : ORC_HX_STOP_MISMATCH;
            cw[6] = b < room ? ORC_HX_STOP_MISMATCH : b == (int)m ? ORC_HX_STOP_CAND : ORC_HX_STOP_LIMIT;
            if (probe) {
                ml = MINMATCH + f + b;
                if (ml > longest) { longest = ml; *mpos = m - b; *spos = ip - b; win = walked; by_pattern = 0; }
            }
        }
        if (swap && ml == longest) {               /* as good as the best: is there a better chain inside this candidate? */
            if (mi + (uint32_t)longest <= ip_idx) {
                const int end = longest - MINMATCH + 1;
                uint32_t far = 1;
                int at, hop = 1, pace = 16, seen = 0, widest = 1, last_at = 0;
                for (at = 0; at < end; at += hop) {
                    const uint32_t d = c->chain[(mi + (uint32_t)at) & 0xFFFF];
                    seen++; last_at = at;
                    hop = pace++ >> 4;
                    if (hop > widest) widest = hop;
                    if (d > far) { far = d; swap_at = (uint32_t)at; pace = 16; }
                }
                EV(t, ORC_HX_EV_SWAP, (int32_t)ip, (int32_t)m, end, seen, widest, (int32_t)far, (int32_t)swap_at,
                   far <= 1 ? ORC_HX_SWAP_NONE : far > mi ? ORC_HX_SWAP_BREAK : ORC_HX_SWAP_JUMP, last_at);
                if (far > 1) {
                    if (far > mi) { cw[7] = ORC_HX_LEFT_BREAK; broke = 1; goto next; }
                    mi -= far; cw[7] = ORC_HX_LEFT_SWAP;
                    goto next;
                }
            } else EV(t, ORC_HX_EV_SWAP, (int32_t)ip, (int32_t)m, longest - MINMATCH + 1, 0, 0, 0, (int32_t)swap_at, ORC_HX_SWAP_OVERLAP, 0);
        }
        if (pa && c->chain[mi & 0xFFFF] == 1) {
            if (swap_at != 0) EV(t, ORC_HX_EV_PA, (int32_t)ip, (int32_t)m - 1, rep, (int32_t)src_run, 0, 0, 0, ORC_HX_PA_SWAPPED, (int32_t)swap_at);
            else {
                const uint32_t ci = mi - 1;        /* the position before: maybe more of one run */
                const int fresh = rep == 0;
                if (rep == 0) {
                    if (((pattern & 0xFFFF) == (pattern >> 16)) & ((pattern & 0xFF) == (pattern >> 24))) {
                        rep = 2;
                        src_run = run_fwd(s, ip + 4, pbyte, high) + 4;
                    } else rep = 1;
                }
                if (rep != 2) EV(t, ORC_HX_EV_PA, (int32_t)ip, (int32_t)m - 1, rep, 0, 0, 0, 0, ORC_HX_PA_NOT_PATTERN, fresh);
                else if (ci < lowest) EV(t, ORC_HX_EV_PA, (int32_t)ip, (int32_t)m - 1, rep, (int32_t)src_run, 0, 0, 0, ORC_HX_PA_BELOW_LOWEST, fresh);
                else if (rd32(s + (ci - IDX0)) != pattern) EV(t, ORC_HX_EV_PA, (int32_t)ip, (int32_t)m - 1, rep, (int32_t)src_run, 0, 0, 0, ORC_HX_PA_DIFFER, fresh);
                else {
                    const uint32_t cp = ci - IDX0;
                    const uint32_t fwd = run_fwd(s, cp + 4, pbyte, high) + 4;
                    const uint32_t back_all = run_back(s, cp, pbyte);
                    const uint32_t floor_i = ci - back_all > lowest ? ci - back_all : lowest;
                    const uint32_t back = ci - floor_i;                   /* not further than the lowest index in reach */
                    const uint32_t seg = back + fwd;
                    int arm, stop = 0;
                    if (seg >= src_run && fwd <= src_run) {               /* the whole source run fits: stand at its end */
                        mi = ci + fwd - src_run;
                        arm = ORC_HX_PA_TO_END;
                    } else {                                              /* else at the segment's start */
                        mi = ci - back;
                        arm = ORC_HX_PA_TO_START_LOOKBACK;
                        if (lookback == 0) {
                            const uint32_t best = seg < src_run ? seg : src_run;
                            arm = ORC_HX_PA_TO_START_NOT_LONGER;
                            if ((uint32_t)longest < best) {
                                if (ip_idx - mi > MAX_DIST) { arm = ORC_HX_PA_BREAK_DISTANCE; stop = 1; }
                                else { longest = (int)best; *mpos = mi - IDX0; *spos = ip; win = walked; by_pattern = 1; arm = ORC_HX_PA_TO_START_TAKEN; }
                            }
                            if (!stop) {
                                const uint32_t d = c->chain[mi & 0xFFFF];
                                if (d > mi) { arm = ORC_HX_PA_BREAK_DELTA; stop = 1; }
                                else mi -= d;
                            }
                        }
                    }
                    EV(t, ORC_HX_EV_PA, (int32_t)ip, (int32_t)cp, rep, (int32_t)src_run, (int32_t)fwd, (int32_t)back_all, (int32_t)back, arm, fresh,
                       (back != back_all) | (cp == back_all ? 2 : 0));
                    cw[7] = stop ? ORC_HX_LEFT_BREAK : ORC_HX_LEFT_PATTERN;
                    broke = stop;
                    goto next;
                }
            }
        }
        if (swap_at) cw[7] = ORC_HX_LEFT_CHAIN_SWAPPED;
        mi -= c->chain[(mi + swap_at) & 0xFFFF];
    next:
        orc_tr_put(t, ORC_TR_CAND, cw, ORC_HX_CAND_WORDS);
        walked++;
        if (broke) break;
    }
    if (t && t->ev[ORC_TR_SEARCH] && head_at + ORC_HX_SEARCH_WORDS <= t->cap[ORC_TR_SEARCH]) {
        int32_t* h = t->ev[ORC_TR_SEARCH] + head_at;
        h[0] = t->n[ORC_TR_EMIT] / 3; h[1] = (int32_t)ip; h[2] = (int32_t)low; h[3] = longest_in; h[4] = walked;
        h[5] = broke ? ORC_END_BREAK : mi >= lowest ? ORC_END_ATTEMPTS
             : (mi < IDX0 || hc_hash(s + (mi - IDX0)) != hc_hash(s + ip)) ? ORC_END_CHAIN : ORC_END_LOWEST;
        h[6] = win; h[7] = longest; h[8] = (!broke && mi >= lowest) ? (int32_t)(mi - IDX0) : -1;
        h[9] = ntu_in; h[10] = by_pattern; h[11] = (int32_t)swap_at;
    }
    return longest;
}

/* token + literals + offset + match length; returns 1 when `limited` and the output would overflow */
static int hc_emit(const uint8_t* src, uint32_t* ip, uint8_t** op, uint32_t* anchor, int ml, uint32_t match,
                   int limited, uint8_t* oend, orc_trace* t, int site)
{
    size_t len = *ip - *anchor;
    uint8_t* token = (*op)++;
    {   const int32_t w[3] = {(int32_t)len, ml, (int32_t)(*ip - match)}; orc_tr_put(t, ORC_TR_EMIT, w, 3); }
    if (limited && (*op + len / 255 + len + (2 + 1 + LASTLIT) > oend)) { hc_arm(t, site, ORC_REFUSE_LITERALS, *ip); return 1; }
    if (len >= 15) {
        size_t l = len - 15;
        *token = 0xF0;
        for (; l >= 255; l -= 255) *(*op)++ = 255;
        *(*op)++ = (uint8_t)l;
    } else *token = (uint8_t)(len << 4);
    memcpy(*op, src + *anchor, len); *op += len;
    (*op)[0] = (uint8_t)(*ip - match); (*op)[1] = (uint8_t)((*ip - match) >> 8); *op += 2;
    len = (size_t)ml - MINMATCH;
    if (limited && (*op + len / 255 + (1 + LASTLIT) > oend)) { hc_arm(t, site, ORC_REFUSE_MATCHLEN, *ip); return 1; }
    if (len >= 15) {
        *token += 15; len -= 15;
        for (; len >= 255; len -= 255) *(*op)++ = 255;
        *(*op)++ = (uint8_t)len;
    } else *token += (uint8_t)len;
    *ip += (uint32_t)ml;
    *anchor = *ip;
    return 0;
}

/* ---- the optimal parser of levels 10..12 (LZ4HC_compress_optimal) ------------------------------------------------------------- */
#define OPT_CELLS   4096
#define OPT_TAIL    3
typedef struct { int cost, off, len, lits; } cell_t;       /* len 1: a literal; lits: the literals in front of this cell's sequence */

static int lits_cost(int lits) { return lits >= 15 ? lits + 1 + (lits - 15) / 255 : lits; }
static int seq_cost(int lits, int len) { return 3 + lits_cost(lits) + (len >= 19 ? 1 + (len - 19) / 255 : 0); }

/* LZ4HC_FindLongerMatch: a match longer than `floor_len` at ip, or 0 */
static int hx_longer(hc_t* c, uint32_t ip, uint32_t high, int floor_len, int tries, int* off, orc_trace* t)
{
    uint32_t at = 0, from = ip;
    const int len = hx_wider(c, ip, ip, high, floor_len, &at, &from, tries, 1, 1, t);
    if (len <= floor_len) return 0;
    *off = (int)(ip - at);
    return len;
}

static void opt_tail(cell_t* cell, int last)
{
    int k;
    for (k = 1; k <= OPT_TAIL; k++) {
        cell[last + k].len = 1; cell[last + k].off = 0; cell[last + k].lits = k;
        cell[last + k].cost = cell[last].cost + lits_cost(k);
    }
}

/* returns 1 when the output overflows; *anchorp is where the last literals start */
static int hx_optimal(hc_t* c, int n, uint8_t** opp, uint8_t* oend, int limited, uint32_t* anchorp, int tries, int enough, int full, orc_trace* t)
{
    const uint8_t* src = c->src;
    cell_t* cell;
    uint32_t ip = 0, anchor = 0;
    int over = 0;
    if (n < MFLIMIT) return 0;
    if (enough >= OPT_CELLS) enough = OPT_CELLS - 1;
    cell = (cell_t*)malloc(sizeof(cell_t) * (OPT_CELLS + OPT_TAIL));
    {
        const uint32_t mflimit = (uint32_t)n - MFLIMIT, matchlimit = (uint32_t)n - LASTLIT;
        while (ip <= mflimit) {
            const int run = (int)(ip - anchor);
            int off0 = 0, last, cur, take_len, take_off, k, hops = 0, between = 0, matches = 0, lit_lo, lit_hi;
            const int len0 = hx_longer(c, ip, matchlimit, MINMATCH - 1, tries, &off0, t);
            if (!len0) { EV(t, ORC_HX_EV_OPT_NO_MATCH, (int32_t)ip); ip++; continue; }
            if (len0 > enough) {
                EV(t, ORC_HX_EV_OPT_FIRST_NOW, (int32_t)ip, len0, run);
                if (hc_emit(src, &ip, opp, &anchor, len0, ip - (uint32_t)off0, limited, oend, t, ORC_HX_SITE_FIRST)) { over = 1; break; }
                continue;
            }
            EV(t, ORC_HX_EV_OPT_FIRST, (int32_t)ip, len0, run, len0 == enough);
            lit_lo = run; lit_hi = run + MINMATCH - 1;
            for (k = 0; k < MINMATCH; k++) { cell[k].len = 1; cell[k].off = 0; cell[k].lits = run + k; cell[k].cost = lits_cost(run + k); }
            for (k = MINMATCH; k <= len0; k++) { cell[k].len = k; cell[k].off = off0; cell[k].lits = run; cell[k].cost = seq_cost(run, k); }
            last = len0;
            opt_tail(cell, last);
            take_len = 0; take_off = 0;
            for (cur = 1; cur < last; cur++) {
                const uint32_t at = ip + (uint32_t)cur;
                int off1 = 0, len1;
                if (at > mflimit) { EV(t, ORC_HX_EV_OPT_AT_MFLIMIT, (int32_t)ip, cur); break; }
                {
                    const int cheaper_next = cell[cur + 1].cost <= cell[cur].cost;
                    const int flat_after = cell[cur + MINMATCH].cost < cell[cur].cost + 3;
                    if (full ? (cheaper_next && flat_after) : cheaper_next) { EV(t, ORC_HX_EV_OPT_SKIP, (int32_t)ip, cur, cheaper_next, full ? flat_after : -1); continue; }
                    if (full && cheaper_next) EV(t, ORC_HX_EV_OPT_SEARCH_ANYWAY, (int32_t)ip, cur);
                }
                len1 = hx_longer(c, at, matchlimit, full ? MINMATCH - 1 : last - cur, tries, &off1, t);
                if (!len1) { EV(t, ORC_HX_EV_OPT_NO_LONGER, (int32_t)ip, cur); continue; }
                if (len1 > enough || len1 + cur >= OPT_CELLS) {
                    EV(t, len1 > enough ? ORC_HX_EV_OPT_INNER_NOW_ENOUGH : ORC_HX_EV_OPT_INNER_NOW_FULL, (int32_t)ip, cur, len1);
                    take_len = len1; take_off = off1; last = cur + 1;
                    break;
                }
                {   /* literals behind cur, then every length of the match at cur */
                    const int base_lits = cell[cur].lits, base_is_lit = cell[cur].len == 1;
                    const int last_in = last;
                    int beyond = 0, cheaper = 0, refused = 0, lit_better = 0;
                    for (k = 1; k < MINMATCH; k++) {
                        const int cost = cell[cur].cost - lits_cost(base_lits) + lits_cost(base_lits + k);
                        if (base_lits + k > lit_hi) lit_hi = base_lits + k;
                        if (cost < cell[cur + k].cost) {
                            cell[cur + k].len = 1; cell[cur + k].off = 0; cell[cur + k].lits = base_lits + k; cell[cur + k].cost = cost;
                            lit_better++;
                        }
                    }
                    if (base_lits < lit_lo) lit_lo = base_lits;
                    for (k = MINMATCH; k <= len1; k++) {
                        const int to = cur + k;
                        int cost, lits;
                        if (cell[cur].len == 1) { lits = cell[cur].lits; cost = (cur > lits ? cell[cur - lits].cost : 0) + seq_cost(lits, k); }
                        else { lits = 0; cost = cell[cur].cost + seq_cost(0, k); }
                        if (to > last + OPT_TAIL || cost <= cell[to].cost) {
                            if (to > last + OPT_TAIL) beyond++; else cheaper++;
                            if (k == len1 && last < to) last = to;
                            cell[to].len = k; cell[to].off = off1; cell[to].lits = lits; cell[to].cost = cost;
                        } else refused++;
                    }
                    EV(t, ORC_HX_EV_OPT_UPDATE, (int32_t)ip, cur, base_is_lit ? (cur > base_lits ? ORC_HX_BASE_LIT_INSIDE : ORC_HX_BASE_LIT_FROM_START) : ORC_HX_BASE_MATCH,
                       len1, last > last_in, beyond, cheaper, refused, lit_better);
                }
                opt_tail(cell, last);
            }
            if (!take_len) { take_len = cell[last].len; take_off = cell[last].off; cur = last - take_len; }
            {   /* walk back from the end, turning "how I got here" into "what to do from here" */
                int at = cur, len = take_len, off = take_off;
                for (;;) {
                    const int prev_len = cell[at].len, prev_off = cell[at].off;
                    cell[at].len = len; cell[at].off = off;
                    len = prev_len; off = prev_off;
                    hops++;
                    if (prev_len > at) break;
                    at -= prev_len;
                }
            }
            {
                const int starts_lit = cell[0].len == 1;
                for (k = 0; k < last; ) {
                    const int len = cell[k].len, off = cell[k].off;
                    if (len == 1) { if (matches) between = 1; ip++; k++; continue; }
                    k += len; matches++;
                    if (hc_emit(src, &ip, opp, &anchor, len, ip - (uint32_t)off, limited, oend, t, ORC_HX_SITE_SERIES)) { over = 1; break; }
                }
                EV(t, ORC_HX_EV_OPT_SERIES, (int32_t)ip, hops, between, starts_lit, last, matches, lit_lo, lit_hi);
                if (over) break;
            }
        }
    }
    free(cell);
    *anchorp = anchor;
    return over;
}

int orc_lz4hc_compress(const uint8_t* src, uint8_t* dst, int n, int cap, int level)
{ return orc_lz4hc_compress_ex(src, dst, n, cap, level, NULL); }

/* the arms of the parse are numbered in the order the statements below stand (oracle.h: ORC_ARM_*) */
int orc_lz4hc_compress_ex(const uint8_t* src, uint8_t* dst, int n, int cap, int level, orc_trace* t)
{
    static const int searches[10] = {2, 2, 2, 4, 8, 16, 32, 64, 128, 256};
    hc_t* c;
    int attempts, limited, result = 0;
    uint32_t ip = 0, anchor = 0;
    uint8_t* op = dst;
    uint8_t* const oend = dst + cap;
    int ml, ml2, ml3, ml0;
    uint32_t ref = 0, start2 = 0, ref2 = 0, start3 = 0, ref3 = 0, start0, ref0;

    int site;
#define FIND(c, ip, low, high, longest, mpos, spos, attempts, t) \
    (site < 0 ? hc_wider(c, ip, low, high, longest, mpos, spos, attempts, t) : hx_wider(c, ip, low, high, longest, mpos, spos, attempts, 1, 0, t))

    if (level < 1) level = 9;                           /* lz4hc.c:840-841 */
    if (level > 12) level = 12;
    site = level < 9 ? -1 : level == 9 ? ORC_HX_SITE_CHAIN : ORC_HX_SITE_SERIES;
    if ((unsigned)n > 0x7E000000u) return 0;
    attempts = searches[level < 9 ? level : 9];
    limited = cap < orc_lz4_compress_bound(n);
    c = (hc_t*)malloc(sizeof *c);
    memset(c->hash, 0, sizeof c->hash);
    memset(c->chain, 0xFF, sizeof c->chain);
    c->next_to_update = IDX0; c->src = src;

    if (level >= 10) {
        static const int nb[3] = {96, 512, 16384}, enough[3] = {64, 128, 4096};
        if (hx_optimal(c, n, &op, oend, limited, &anchor, nb[level - 10], enough[level - 10], level == 12, t)) goto overflow;
    } else if (n >= MFLIMIT + 1) {
        const uint32_t mflimit = (uint32_t)n - MFLIMIT, matchlimit = (uint32_t)n - LASTLIT;
        while (ip <= mflimit) {
            ml = FIND(c, ip, ip, matchlimit, MINMATCH - 1, &ref, &start0 /*unused*/, attempts, t);
            if (ml < MINMATCH) { ip++; continue; }
            start0 = ip; ref0 = ref; ml0 = ml;
        search2:
            if (ip + ml <= mflimit)
                ml2 = FIND(c, ip + ml - 2, ip, matchlimit, ml, &ref2, &start2, attempts, t);
            else { ml2 = ml; hc_arm(t, site, ORC_ARM_NO_SEARCH2, ip); }
            if (ml2 == ml) {                                            /* no better match: encode ML1 */
                hc_arm(t, site, ORC_ARM_ML1, ip);
                if (hc_emit(src, &ip, &op, &anchor, ml, ref, limited, oend, t, site)) goto overflow;
                continue;
            }
            if (start0 < ip && start2 < ip + ml0) { hc_arm(t, site, ORC_ARM_RESTORE0, ip); ip = start0; ref = ref0; ml = ml0; }
            if (start2 - ip < 3) {                                      /* first match too small: dropped */
                hc_arm(t, site, ORC_ARM_DROP1, ip);
                ml = ml2; ip = start2; ref = ref2;
                goto search2;
            }
        search3:
            if (start2 - ip < OPTIMAL_ML) {
                int new_ml = ml, correction;
                hc_arm(t, site, ORC_ARM_S3_NEAR, ip);
                if (new_ml > OPTIMAL_ML) { hc_arm(t, site, ORC_ARM_S3_CLAMP, ip); new_ml = OPTIMAL_ML; }
                if (ip + new_ml > start2 + ml2 - MINMATCH) { hc_arm(t, site, ORC_ARM_S3_TAIL, ip); new_ml = (int)(start2 - ip) + ml2 - MINMATCH; }
                correction = new_ml - (int)(start2 - ip);
                if (correction > 0) { hc_arm(t, site, ORC_ARM_S3_CORRECT, ip); start2 += correction; ref2 += correction; ml2 -= correction; }
            } else hc_arm(t, site, ORC_ARM_S3_FAR, ip);
            if (start2 + ml2 <= mflimit)
                ml3 = FIND(c, start2 + ml2 - 3, start2, matchlimit, ml2, &ref3, &start3, attempts, t);
            else { ml3 = ml2; hc_arm(t, site, ORC_ARM_NO_SEARCH3, ip); }
            if (ml3 == ml2) {                                           /* encode ML1 and ML2 */
                hc_arm(t, site, ORC_ARM_ML12, ip);
                if (start2 < ip + ml) { hc_arm(t, site, ORC_ARM_ML12_CUT, ip); ml = (int)(start2 - ip); }
                if (hc_emit(src, &ip, &op, &anchor, ml, ref, limited, oend, t, site)) goto overflow;
                ip = start2;
                if (hc_emit(src, &ip, &op, &anchor, ml2, ref2, limited, oend, t, site)) goto overflow;
                continue;
            }
            if (start3 < ip + ml + 3) {                                 /* not enough room for match 2 */
                if (start3 >= ip + ml) {                                /* Seq1 can go out now; Seq3 becomes Seq1 */
                    hc_arm(t, site, ORC_ARM_SEQ3_IS_1, ip);
                    if (start2 < ip + ml) {
                        const int correction = (int)(ip + ml - start2);
                        hc_arm(t, site, ORC_ARM_SEQ3_IS_1_CUT2, ip);
                        start2 += correction; ref2 += correction; ml2 -= correction;
                        if (ml2 < MINMATCH) { hc_arm(t, site, ORC_ARM_SEQ3_IS_1_2, ip); start2 = start3; ref2 = ref3; ml2 = ml3; }
                    }
                    if (hc_emit(src, &ip, &op, &anchor, ml, ref, limited, oend, t, site)) goto overflow;
                    ip = start3; ref = ref3; ml = ml3;
                    start0 = start2; ref0 = ref2; ml0 = ml2;
                    goto search2;
                }
                hc_arm(t, site, ORC_ARM_DROP2, ip);
                start2 = start3; ref2 = ref3; ml2 = ml3;
                goto search3;
            }
            /* three ascending matches: write the first */
            hc_arm(t, site, ORC_ARM_THREE, ip);
            if (start2 < ip + ml) {
                if (start2 - ip < OPTIMAL_ML) {
                    int correction;
                    hc_arm(t, site, ORC_ARM_THREE_NEAR, ip);
                    if (ml > OPTIMAL_ML) { hc_arm(t, site, ORC_ARM_THREE_CLAMP, ip); ml = OPTIMAL_ML; }
                    if (ip + ml > start2 + ml2 - MINMATCH) { hc_arm(t, site, ORC_ARM_THREE_TAIL, ip); ml = (int)(start2 - ip) + ml2 - MINMATCH; }
                    correction = ml - (int)(start2 - ip);
                    if (correction > 0) { hc_arm(t, site, ORC_ARM_THREE_CORRECT, ip); start2 += correction; ref2 += correction; ml2 -= correction; }
                } else { hc_arm(t, site, ORC_ARM_THREE_FAR, ip); ml = (int)(start2 - ip); }
            }
            if (hc_emit(src, &ip, &op, &anchor, ml, ref, limited, oend, t, site)) goto overflow;
            ip = start2; ref = ref2; ml = ml2;
            start2 = start3; ref2 = ref3; ml2 = ml3;
            goto search3;
        }
    }
    {   /* last literals (lz4hc.c:735-762) */
        const size_t run = (size_t)n - anchor, add = (run + 255 - 15) / 255;
        {   const int32_t w[3] = {(int32_t)run, 0, 0}; orc_tr_put(t, ORC_TR_EMIT, w, 3); }
        if (limited && op + 1 + add + run > oend) { hc_arm(t, site, ORC_REFUSE_LAST, anchor); goto overflow; }
        if (run >= 15) {
            size_t acc = run - 15;
            *op++ = 0xF0;
            for (; acc >= 255; acc -= 255) *op++ = 255;
            *op++ = (uint8_t)acc;
        } else *op++ = (uint8_t)(run << 4);
        memcpy(op, src + anchor, run); op += run;
        result = (int)(op - dst);
    }
overflow:
    free(c);
    return result;
}

int orc_codec_lz4hc4(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap)
{ (void)ctx; return orc_lz4hc_compress(src, dst, n, cap, 4); }
int orc_codec_lz4hc8(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap)
{ (void)ctx; return orc_lz4hc_compress(src, dst, n, cap, 8); }
