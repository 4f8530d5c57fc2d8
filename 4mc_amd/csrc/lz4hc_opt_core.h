/* 4mc_amd/csrc/lz4hc_opt_core.h - LZ4 HC levels 9..12 (LZ4_compress_HC, native/lz4/lz4hc.c of lz4 1.9.4): the serial part of
 * the parse, written once and compiled twice:
 *   - into the kernel lz4hc_opt_encode.hip, where one wavefront runs it with every lane holding the same values, and
 *   - into the CPU model tools/model/lz4hc_opt_model.c (gcc, C99), which the CPU test compares with the reference.
 *
 * Everything here is uniform control flow.  What the lanes do in parallel sits behind the primitives declared below; the includer
 * defines them (wave-wide in the kernel, as loops over 64 emulated lanes or plain loops in the model) after including this file.
 *
 * The state is the reference's for one LZ4_compress_HC call with a fresh stream: no dictionary, dictLimit == lowLimit, position p
 * has table index p + 65536 (LZ4HC_init_internal :100-116), hash heads start at 0 and chain deltas at 0xFFFF (:94-98), the chain
 * is a ring of 64 Ki u16 indexed (U16)idx (DELTANEXTU16 :84), and positions enter it lazily, up to each search's ip
 * (LZ4HC_Insert :120-141): the ring holds the reference's entries only because the insertion schedule is the reference's.
 * favorDecSpeed is 0 and the output limit is limitedOutput or notLimited (LZ4_compress_HC never asks for fillOutput).
 *
 * Includer defines HO_FN (function qualifiers) and, after the #include, every primitive prototyped below. */
#ifndef FOURMC_LZ4HC_OPT_CORE_H
#define FOURMC_LZ4HC_OPT_CORE_H

#define HO_MINMATCH   4
#define HO_MFLIMIT    12
#define HO_LASTLIT    5
#define HO_HASHLOG    15
#define HO_IDX0       65536u          /* table index of position 0 */
#define HO_MAXD       65535u          /* LZ4_DISTANCE_MAX */
#define HO_OPT_NUM    4096            /* LZ4_OPT_NUM */
#define HO_TRAIL      3               /* TRAILING_LITERALS */
#define HO_OPTIMAL_ML 18
#define HO_OPT_RECS   (HO_OPT_NUM + HO_TRAIL + 5)
#define HO_MAX_INPUT  0x7E000000u     /* LZ4_MAX_INPUT_SIZE */

/* one record of the optimal parser's price table (LZ4HC_optimal_t :1268-1273) */
typedef struct { int32_t price, off, mlen, litlen; } HOpt;

typedef struct {
    const uint8_t* src;
    uint8_t*       dst;
    uint32_t       n;
    int64_t        cap;       /* dst capacity; only read when `limited` */
    int            limited;   /* dstCapacity < LZ4_compressBound(n) (lz4hc.c:945) */
    uint16_t*      chain;     /* [65536] chain deltas (LDS in the kernel) */
    uint32_t*      heads;     /* [1 << HO_HASHLOG] hash heads */
    HOpt*          opt;       /* [HO_OPT_RECS] */
    uint32_t*      score;     /* kernel only: LDS scoreboard of the batched insert */
    uint32_t       ntu;       /* nextToUpdate, as a position */
    uint32_t       op;        /* bytes written */
    int            lane;      /* kernel only */
} HO;

/* ---- primitives (defined by the includer) ---------------------------------------------------------------------------------- */
HO_FN uint32_t ho_ld32(const HO* c, uint32_t p);
HO_FN uint32_t ho_ld16(const HO* c, uint32_t p);
HO_FN uint32_t ho_chain(const HO* c, uint32_t idx);                        /* DELTANEXTU16(chainTable, idx) */
HO_FN uint32_t ho_head(const HO* c, uint32_t h);                           /* HashTable[h] */
HO_FN void     ho_insert(HO* c, uint32_t upto);                            /* LZ4HC_Insert: positions [ntu, upto) */
HO_FN uint32_t ho_count(const HO* c, uint32_t a, uint32_t b, uint32_t lim);     /* LZ4_count(a, b, lim), b < a */
HO_FN uint32_t ho_count_back(const HO* c, uint32_t a, uint32_t b, uint32_t maxn);  /* -LZ4HC_countBack, at most maxn */
HO_FN uint32_t ho_run(const HO* c, uint32_t a, uint32_t byte, uint32_t lim);    /* bytes == byte in [a, lim) from a */
HO_FN uint32_t ho_run_back(const HO* c, uint32_t a, uint32_t byte);        /* bytes == byte going back from a (excl.) to 0 */
/* the chain-swap scan (:319-333): returns distanceToNextMatch, updates *mcp when a longer delta is found */
HO_FN uint32_t ho_swap_scan(const HO* c, uint32_t matchIndex, int end, uint32_t* mcp);
HO_FN HOpt     ho_opt_get(const HO* c, int i);
HO_FN void     ho_opt_put(HO* c, int i, HOpt r);                           /* uniform write: every lane writes the same record */
/* the optimal parser's table updates (lane-parallel in the kernel) */
HO_FN void     ho_opt_first(HO* c, int llen, int matchML, int off);        /* :1393-1416 */
HO_FN int      ho_opt_match(HO* c, int cur, int matchML, int off, int last);    /* :1465-1513, returns last_match_pos */
/* LZ4HC_encodeSequence (:467-548) at ip with anchor: 1 = would overflow; else ip/anchor advance */
HO_FN int      ho_emit(HO* c, uint32_t* ip, uint32_t* anchor, int ml, uint32_t match);
/* last literals (:734-764 / :1567-1600): result, 0 when they do not fit */
HO_FN int      ho_last(HO* c, uint32_t anchor);

/* ---- the algorithm ---------------------------------------------------------------------------------------------------------- */
HO_FN uint32_t ho_hash(uint32_t v) { return (v * 2654435761u) >> (32 - HO_HASHLOG); }
HO_FN uint32_t ho_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
HO_FN uint32_t ho_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

/* LZ4HC_literalsPrice :1276, LZ4HC_sequencePrice :1287 */
HO_FN int ho_lit_price(int litlen) { return litlen + (litlen >= 15 ? 1 + (litlen - 15) / 255 : 0); }
HO_FN int ho_seq_price(int litlen, int mlen) { return 3 + ho_lit_price(litlen) + (mlen >= 19 ? 1 + (mlen - 19) / 255 : 0); }

/* LZ4HC_InsertAndGetWiderMatch :239-447, no dictionary.  Positions, not pointers: *mpos / *spos are positions in src. */
HO_FN int ho_wider(HO* c, uint32_t ip, uint32_t ilow, uint32_t ihigh, int longest, uint32_t* mpos, uint32_t* spos,
                   int attempts, int pa, int chainswap)
{
    const uint32_t ipIndex = ip + HO_IDX0;
    const uint32_t lowest = (HO_IDX0 + HO_MAXD + 1 > ipIndex) ? HO_IDX0 : ipIndex - HO_MAXD;
    const uint32_t lookback = ip - ilow;
    const uint32_t pattern = ho_ld32(c, ip);
    uint32_t matchIndex, mcp = 0, srcLen = 0;
    int repeat = 0;                                             /* 0 untested, 1 not, 2 confirmed (:236) */
    ho_insert(c, ip);
    matchIndex = ho_head(c, ho_hash(pattern));
    while (matchIndex >= lowest && attempts > 0) {
        int ml = 0;
        const uint32_t m = matchIndex - HO_IDX0;
        attempts--;
        /* :288 - the 2-byte probe at `longest`; it decides whether a candidate of exactly `longest` counts for the chain swap */
        if (ho_ld16(c, ilow + (uint32_t)longest - 1) == ho_ld16(c, m + ((uint32_t)longest - 1 - lookback))) {
            if (ho_ld32(c, m) == pattern) {
                const uint32_t back = lookback ? ho_count_back(c, ip, m, ho_min(lookback, m)) : 0;
                ml = (int)(HO_MINMATCH + ho_count(c, ip + HO_MINMATCH, m + HO_MINMATCH, ihigh) + back);
                if (ml > longest) { longest = ml; *mpos = m - back; *spos = ip - back; }
            }
        }
        if (chainswap && ml == longest) {                       /* :317-338 */
            if (matchIndex + (uint32_t)longest <= ipIndex) {
                const uint32_t dist = ho_swap_scan(c, matchIndex, longest - HO_MINMATCH + 1, &mcp);
                if (dist > 1) {
                    if (dist > matchIndex) break;
                    matchIndex -= dist;
                    continue;
                }
            }
        }
        if (pa && mcp == 0 && ho_chain(c, matchIndex) == 1) {  /* :340-410 */
            const uint32_t mci = matchIndex - 1;
            if (repeat == 0) {
                /* (pattern & 0xFFFF) == (pattern >> 16) and low byte == high byte: one byte repeated */
                if (((pattern & 0xFFFF) == (pattern >> 16)) && ((pattern & 0xFF) == (pattern >> 24))) {
                    repeat = 2;
                    srcLen = ho_run(c, ip + 4, pattern & 0xFF, ihigh) + 4;       /* LZ4HC_countPattern :177 */
                } else repeat = 1;
            }
            /* LZ4HC_protectDictEnd (:231) holds for every index >= lowestMatchIndex >= dictLimit here */
            if (repeat == 2 && mci >= lowest) {
                const uint32_t mp = mci - HO_IDX0;
                if (ho_ld32(c, mp) == pattern) {
                    const uint32_t fwd = ho_run(c, mp + 4, pattern & 0xFF, ihigh) + 4;
                    uint32_t back = ho_run_back(c, mp, pattern & 0xFF);              /* LZ4HC_reverseCountPattern :210 */
                    back = mci - ho_max(mci - back, lowest);                          /* :373 */
                    if (back + fwd >= srcLen && fwd <= srcLen) {
                        matchIndex = mci + fwd - srcLen;                              /* :379 */
                    } else {
                        matchIndex = mci - back;                                      /* :388 */
                        if (lookback == 0) {
                            const uint32_t maxML = ho_min(back + fwd, srcLen);
                            if ((uint32_t)longest < maxML) {
                                if (ipIndex - matchIndex > HO_MAXD) break;
                                longest = (int)maxML;
                                *mpos = matchIndex - HO_IDX0; *spos = ip;
                            }
                            {
                                const uint32_t d = ho_chain(c, matchIndex);
                                if (d > matchIndex) break;
                                matchIndex -= d;
                            }
                        }
                    }
                    continue;
                }
            }
        }
        matchIndex -= ho_chain(c, matchIndex + mcp);           /* :413 */
    }
    return longest;
}

/* LZ4HC_compress_hashChain :553-788 at level 9 (256 attempts, pattern analysis on :565, no chain swap) */
HO_FN int ho_hash_chain(HO* c, int attempts)
{
    uint32_t ip = 0, anchor = 0;
    if (c->n >= HO_MFLIMIT + 1) {                                /* LZ4_minLength :589 */
        const uint32_t mflimit = c->n - HO_MFLIMIT, matchlimit = c->n - HO_LASTLIT;
        int ml, ml0, ml2 = 0, ml3 = 0;
        uint32_t ref = 0, start0, ref0, start2 = 0, ref2 = 0, start3 = 0, ref3 = 0, dummy = 0;
        while (ip <= mflimit) {
            ml = ho_wider(c, ip, ip, matchlimit, HO_MINMATCH - 1, &ref, &dummy, attempts, 1, 0);
            if (ml < HO_MINMATCH) { ip++; continue; }
            start0 = ip; ref0 = ref; ml0 = ml;
            for (;;) {                                           /* _Search2 */
                int search3 = 0;
                if (ip + (uint32_t)ml <= mflimit)
                    ml2 = ho_wider(c, ip + (uint32_t)ml - 2, ip, matchlimit, ml, &ref2, &start2, attempts, 1, 0);
                else ml2 = ml;
                if (ml2 == ml) {
                    if (ho_emit(c, &ip, &anchor, ml, ref)) return 0;
                    break;
                }
                if (start0 < ip && start2 < ip + (uint32_t)ml0) { ip = start0; ref = ref0; ml = ml0; }
                if (start2 - ip < 3) { ml = ml2; ip = start2; ref = ref2; continue; }
                for (;;) {                                       /* _Search3 */
                    if (start2 - ip < HO_OPTIMAL_ML) {
                        int new_ml = ml, correction;
                        if (new_ml > HO_OPTIMAL_ML) new_ml = HO_OPTIMAL_ML;
                        if (ip + (uint32_t)new_ml > start2 + (uint32_t)ml2 - HO_MINMATCH) new_ml = (int)(start2 - ip) + ml2 - HO_MINMATCH;
                        correction = new_ml - (int)(start2 - ip);
                        if (correction > 0) { start2 += (uint32_t)correction; ref2 += (uint32_t)correction; ml2 -= correction; }
                    }
                    if (start2 + (uint32_t)ml2 <= mflimit)
                        ml3 = ho_wider(c, start2 + (uint32_t)ml2 - 3, start2, matchlimit, ml2, &ref3, &start3, attempts, 1, 0);
                    else ml3 = ml2;
                    if (ml3 == ml2) {
                        if (start2 < ip + (uint32_t)ml) ml = (int)(start2 - ip);
                        if (ho_emit(c, &ip, &anchor, ml, ref)) return 0;
                        ip = start2;
                        if (ho_emit(c, &ip, &anchor, ml2, ref2)) return 0;
                        break;
                    }
                    if (start3 < ip + (uint32_t)ml + 3) {
                        if (start3 >= ip + (uint32_t)ml) {
                            if (start2 < ip + (uint32_t)ml) {
                                const int correction = (int)(ip + (uint32_t)ml - start2);
                                start2 += (uint32_t)correction; ref2 += (uint32_t)correction; ml2 -= correction;
                                if (ml2 < HO_MINMATCH) { start2 = start3; ref2 = ref3; ml2 = ml3; }
                            }
                            if (ho_emit(c, &ip, &anchor, ml, ref)) return 0;
                            ip = start3; ref = ref3; ml = ml3;
                            start0 = start2; ref0 = ref2; ml0 = ml2;
                            search3 = 2;                         /* back to _Search2 */
                            break;
                        }
                        start2 = start3; ref2 = ref3; ml2 = ml3;
                        continue;
                    }
                    if (start2 < ip + (uint32_t)ml) {
                        if (start2 - ip < HO_OPTIMAL_ML) {
                            int correction;
                            if (ml > HO_OPTIMAL_ML) ml = HO_OPTIMAL_ML;
                            if (ip + (uint32_t)ml > start2 + (uint32_t)ml2 - HO_MINMATCH) ml = (int)(start2 - ip) + ml2 - HO_MINMATCH;
                            correction = ml - (int)(start2 - ip);
                            if (correction > 0) { start2 += (uint32_t)correction; ref2 += (uint32_t)correction; ml2 -= correction; }
                        } else ml = (int)(start2 - ip);
                    }
                    if (ho_emit(c, &ip, &anchor, ml, ref)) return 0;
                    ip = start2; ref = ref2; ml = ml2;
                    start2 = start3; ref2 = ref3; ml2 = ml3;
                }
                if (search3 != 2) break;
            }
        }
    }
    return ho_last(c, anchor);
}

/* LZ4HC_FindLongerMatch :1308-1326: length (0: none longer than minLen) and offset */
HO_FN int ho_longer(HO* c, uint32_t ip, uint32_t ihigh, int minLen, int nbSearches, int* off)
{
    uint32_t mpos = 0, spos = ip;
    const int len = ho_wider(c, ip, ip, ihigh, minLen, &mpos, &spos, nbSearches, 1, 1);
    if (len <= minLen) return 0;
    *off = (int)(spos - mpos);
    return len;
}

/* the three literal records behind last_match_pos (:1418-1426, :1515-1522) */
HO_FN void ho_opt_trail(HO* c, int last)
{
    const int p0 = ho_opt_get(c, last).price;
    int a;
    for (a = 1; a <= HO_TRAIL; a++) {
        HOpt r; r.price = p0 + ho_lit_price(a); r.off = 0; r.mlen = 1; r.litlen = a;
        ho_opt_put(c, last + a, r);
    }
}

/* LZ4HC_compress_optimal :1330-1626 (levels 10..12) */
HO_FN int ho_optimal(HO* c, int nbSearches, int sufficient_len, int fullUpdate)
{
    uint32_t ip = 0, anchor = 0;
    if (sufficient_len >= HO_OPT_NUM) sufficient_len = HO_OPT_NUM - 1;     /* :1368 */
    if (c->n >= HO_MFLIMIT + 1) {            /* below, the loop has nothing to find: a 12-byte input only searches position 0 */
        const uint32_t mflimit = c->n - HO_MFLIMIT, matchlimit = c->n - HO_LASTLIT;
        while (ip <= mflimit) {
            const int llen = (int)(ip - anchor);
            int best_mlen, best_off, cur, last, first_off = 0, rpos;
            const int first = ho_longer(c, ip, matchlimit, HO_MINMATCH - 1, nbSearches, &first_off);
            if (first == 0) { ip++; continue; }
            if (first > sufficient_len) {                        /* immediate encoding :1379-1390 */
                if (ho_emit(c, &ip, &anchor, first, ip - (uint32_t)first_off)) return 0;
                continue;
            }
            ho_opt_first(c, llen, first, first_off);
            last = first;
            ho_opt_trail(c, last);
            best_mlen = 0; best_off = 0;
            for (cur = 1; cur < last; cur++) {                  /* :1429-1523 */
                int noff = 0, nlen;
                if (ip + (uint32_t)cur > mflimit) break;
                {
                    const int pc = ho_opt_get(c, cur).price, p1 = ho_opt_get(c, cur + 1).price;
                    if (fullUpdate) {
                        if (p1 <= pc && ho_opt_get(c, cur + HO_MINMATCH).price < pc + 3) continue;
                    } else if (p1 <= pc) continue;
                }
                nlen = ho_longer(c, ip + (uint32_t)cur, matchlimit, fullUpdate ? HO_MINMATCH - 1 : last - cur, nbSearches, &noff);
                if (!nlen) continue;
                if (nlen > sufficient_len || nlen + cur >= HO_OPT_NUM) {      /* immediate encoding :1455-1462 */
                    best_mlen = nlen; best_off = noff; last = cur + 1;
                    break;
                }
                last = ho_opt_match(c, cur, nlen, noff, last);
                ho_opt_trail(c, last);
            }
            if (best_mlen == 0) {                                /* :1526-1528 */
                const HOpt r = ho_opt_get(c, last);
                best_mlen = r.mlen; best_off = r.off; cur = last - best_mlen;
            }
            {   /* encode: reverse traversal :1534-1548 */
                int cand = cur, sel_ml = best_mlen, sel_off = best_off;
                for (;;) {
                    HOpt r = ho_opt_get(c, cand);
                    const int next_ml = r.mlen, next_off = r.off;
                    r.mlen = sel_ml; r.off = sel_off;
                    ho_opt_put(c, cand, r);
                    sel_ml = next_ml; sel_off = next_off;
                    if (next_ml > cand) break;
                    cand -= next_ml;
                }
            }
            rpos = 0;                                            /* :1551-1564 */
            while (rpos < last) {
                const HOpt r = ho_opt_get(c, rpos);
                if (r.mlen == 1) { ip++; rpos++; continue; }
                rpos += r.mlen;
                if (ho_emit(c, &ip, &anchor, r.mlen, ip - (uint32_t)r.off)) return 0;
            }
        }
    }
    return ho_last(c, anchor);
}

/* LZ4_compress_HC(src, dst, n, cap, level) for level 9..12 (the caller maps <= 0 to 9 and > 12 to 12, lz4hc.c:840-841) */
HO_FN int ho_compress(HO* c, int level)
{
    if (c->n > HO_MAX_INPUT) return 0;                           /* :837 */
    c->ntu = 0; c->op = 0;
    switch (level) {                                             /* clTable :817-831 */
        case 9:  return ho_hash_chain(c, 256);
        case 10: return ho_optimal(c, 96, 64, 0);
        case 11: return ho_optimal(c, 512, 128, 0);
        default: return ho_optimal(c, 16384, HO_OPT_NUM, 1);
    }
}

#endif
