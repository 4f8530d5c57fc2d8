/*
 * oracle/oracle.h — CPU restatement of the 4mc hot path.  TEST INFRASTRUCTURE, NOT PRODUCT.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library;
 * nothing under 4mc_amd/ links, imports or calls it.
 *
 * Every function restates, in plain scalar C written for this repository, the algorithm of the
 * reference function named beside it (paths relative to /root/reference).  Parity status:
 * PINNED — checked against (a) the reference's own compiled sources (oracle/_ref, built by
 * oracle/Makefile from the tree where it lies) on seeded and fuzzed inputs, and (b) the golden
 * vectors of SURVEY.md §8(c), committed under tests/golden/ with their generator.
 */
#ifndef ORACLE_H
#define ORACLE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORC_BLOCKSIZE   (4u * 1024u * 1024u)   /* native/4mc.c:116  FOURMC_BLOCKSIZE        */
#define ORC_MAGIC_4MC   0x344D4300u            /* native/4mc.c:111                           */
#define ORC_MAGIC_4MZ   0x344D5A00u            /* native/4mc.c:112                           */

/* XXH32 — native/lz4/xxhash.c:392-415 (round :276, finalize :291-345, avalanche :283). */
uint32_t orc_xxh32(const void* data, size_t len, uint32_t seed);

/* LZ4_compressBound — native/lz4/lz4.h:212 (LZ4_COMPRESSBOUND). */
int orc_lz4_compress_bound(int n);

/* LZ4_compress_default (acceleration 1, 64-bit little-endian build) —
 * native/lz4/lz4.c:1435 -> :1416 -> :1346-1367 -> :910-1302.
 * Returns bytes written, or 0 when the output does not fit `cap` (limitedOutput). */
int orc_lz4_compress_fast(const uint8_t* src, uint8_t* dst, int n, int cap);
/* The same call with an orc_trace (NULL: none, and nothing is computed for it; the rules of orc_trace below hold).  The trace
 * changes no byte.  Tables (int32 rows, positions are offsets into the input):
 *   ORC_TR_SEARCH  ORC_LF_SEARCH_WORDS, one row per search: its first position, probes made (the one that hit or ran past the
 *                  limit included), ORC_LF_END_HIT / ORC_LF_END_LIMIT (`fwd > mflimitPlusOne`), probes that read an empty slot (as position 0)
 *   ORC_TR_CAND    ORC_LF_HIT_WORDS, one row per hit that became a sequence: the position that hit, its candidate, 1 when the candidate
 *                  was an empty slot read as position 0, candidates of this search refused by distance and the last such distance,
 *                  bytes walked back and ORC_LF_STOP_* (what ended the walk), literals, mcode (match length - 4), 1 when the match
 *                  ended at matchlimit, 1 when the hit was the re-test behind a match (`_next_match` with no literals), 1 when that
 *                  re-test read the slot the ip-2 refill had just written
 *   ORC_TR_ARM     event rows of ORC_LF_EV_WORDS, unused words 0: ORC_REFUSE_LITERALS / _MATCHLEN / _LAST (the site of a refusal), position;
 *                  ORC_LF_EV_TABLE, 0, table kind (0: 16-bit, 1: 32-bit); ORC_LF_EV_DIST, position, distance, 1 when the refused
 *                  candidate holds the position's four bytes; ORC_LF_EV_RETEST, position, hit, 1 when the ip-2 refill wrote its slot
 *   ORC_TR_EMIT    ORC_LF_EMIT_WORDS: literals, match length (0: the last literals), offset */
enum { ORC_LF_SEARCH_WORDS = 4, ORC_LF_HIT_WORDS = 12, ORC_LF_EV_WORDS = 4, ORC_LF_EMIT_WORDS = 3 };
enum { ORC_LF_END_HIT = 0, ORC_LF_END_LIMIT = 1 };
enum { ORC_LF_STOP_ANCHOR = 0, ORC_LF_STOP_CAND0 = 1, ORC_LF_STOP_BYTE = 2, ORC_LF_STOP_NONE = 3 };
enum { ORC_LF_EV_TABLE = 64, ORC_LF_EV_DIST = 65, ORC_LF_EV_RETEST = 66 };

/* LZ4_compress_HC at any level (4mc uses 4 and 8; levels below 1 run as 9, levels above 12 as 12, native/lz4/lz4hc.c:840-841) -
 * :958-973 -> :553-788 (levels 1..9) / :1330-1626 (levels 10..12).  Returns bytes written, 0 when it does not fit `cap`. */
int orc_lz4hc_compress(const uint8_t* src, uint8_t* dst, int n, int cap, int level);

/* What a run of the HC or the Medium port did, as four tables of int32 rows.  A row is written whole or not at all; n[]
 * counts every word, also those that found no room, so a caller sizes a second run from a first one with ev[] = NULL.
 *   ORC_TR_SEARCH  HC, one row per search: sequences emitted before it, ip, low, longest on entry, candidates walked,
 *                  ORC_END_*, winner (its number in the walk, -1: none), longest on return, the candidate the walk would
 *                  have visited next (-1: none in reach).
 *                  Medium, one row per probe: sequences emitted before it, ip, step, tries, candidates walked, four-byte
 *                  matches among them, winner position (-1: none), match length, ORC_SHARE_* bits of the probe's three table
 *                  slots, the winner's number in the walk (-1: none), the candidate the walk would have visited next (-1)
 *   ORC_TR_CAND    HC, one row per candidate walked, in order: position, first four bytes equal (0/1), and for those the equal
 *                  bytes after the four and the equal bytes before (within the lookback the search allows)
 *   ORC_TR_ARM     arm (ORC_ARM_* / ORC_REFUSE_*), ip
 *   ORC_TR_EMIT    literal run, match length, offset (the final literals: match length 0) */
typedef struct { int32_t* ev[4]; int cap[4]; int n[4]; } orc_trace;
enum { ORC_TR_SEARCH = 0, ORC_TR_CAND = 1, ORC_TR_ARM = 2, ORC_TR_EMIT = 3 };
enum { ORC_TR_SEARCH_WORDS = 9, ORC_TR_CAND_WORDS = 4, ORC_TR_PROBE_WORDS = 11 };
static inline void orc_tr_put(orc_trace* t, int table, const int32_t* row, int words)
{
    int i;
    if (!t) return;
    if (t->ev[table] && t->n[table] + words <= t->cap[table]) for (i = 0; i < words; i++) t->ev[table][t->n[table] + i] = row[i];
    t->n[table] += words;
}
static inline void orc_tr_arm(orc_trace* t, int arm, int64_t ip) { const int32_t row[2] = {arm, (int32_t)ip}; orc_tr_put(t, ORC_TR_ARM, row, 2); }
enum { ORC_END_ATTEMPTS = 1, ORC_END_LOWEST = 2, ORC_END_CHAIN = 3 };     /* CHAIN: no older position of the hash exists */
enum {  /* the statements of LZ4HC_compress_hashChain's arbitration (lz4hc.c:592-732), in the order the port states them */
    ORC_ARM_NO_SEARCH2 = 1,     /* ip + ml > mflimit: no second search */
    ORC_ARM_ML1,                /* ml2 == ml: encode the first match */
    ORC_ARM_RESTORE0,           /* start0 < ip && start2 < ip + ml0: back to the earlier first match */
    ORC_ARM_DROP1,              /* start2 - ip < 3: the first match is dropped */
    ORC_ARM_S3_NEAR,            /* search3: start2 - ip < OPTIMAL_ML ... */
    ORC_ARM_S3_CLAMP,           /*   new_ml clamped to OPTIMAL_ML */
    ORC_ARM_S3_TAIL,            /*   new_ml cut so that match 2 keeps MINMATCH */
    ORC_ARM_S3_CORRECT,         /*   correction > 0: match 2 starts later */
    ORC_ARM_S3_FAR,             /* search3: start2 - ip >= OPTIMAL_ML */
    ORC_ARM_NO_SEARCH3,         /* start2 + ml2 > mflimit: no third search */
    ORC_ARM_ML12,               /* ml3 == ml2: encode matches 1 and 2 */
    ORC_ARM_ML12_CUT,           /*   match 1 cut at start2 */
    ORC_ARM_SEQ3_IS_1,          /* start3 in [ip+ml, ip+ml+3): match 1 goes out, match 3 becomes match 1 */
    ORC_ARM_SEQ3_IS_1_CUT2,     /*   match 2 cut at the end of match 1 */
    ORC_ARM_SEQ3_IS_1_2,        /*   ... and, shorter than MINMATCH, replaced by match 3 */
    ORC_ARM_DROP2,              /* start3 < ip + ml: match 2 is dropped */
    ORC_ARM_THREE,              /* three ascending matches: write the first */
    ORC_ARM_THREE_NEAR, ORC_ARM_THREE_CLAMP, ORC_ARM_THREE_TAIL, ORC_ARM_THREE_CORRECT, ORC_ARM_THREE_FAR,
    ORC_ARM_COUNT,
    ORC_REFUSE_LITERALS = 32,   /* limited output: token + literals + offset do not fit */
    ORC_REFUSE_MATCHLEN,        /*                 the match length bytes do not fit */
    ORC_REFUSE_LAST             /*                 the final literals do not fit */
};
enum { ORC_SHARE_NTU_PREV = 1, ORC_SHARE_NTU_IP = 2, ORC_SHARE_PREV_IP = 4,       /* two slots of one probe in one bucket ... */
       ORC_DIFF_NTU_PREV = 8, ORC_DIFF_NTU_IP = 16, ORC_DIFF_PREV_IP = 32 };      /* ... holding different words */
int orc_lz4hc_compress_ex(const uint8_t* src, uint8_t* dst, int n, int cap, int level, orc_trace* trace);
int orc_lz4_compress_fast_ex(const uint8_t* src, uint8_t* dst, int n, int cap, orc_trace* trace);   /* (described beside orc_lz4_compress_fast) */
/* The trace of HC levels 9..12 (any level below 1 or above 8 after the mapping) has rows of its own; the rules above hold.
 *   ORC_TR_SEARCH  one row per search, ORC_HX_SEARCH_WORDS: sequences emitted before it, ip, low, longest on entry, candidates
 *                  walked, ORC_END_* (ORC_END_BREAK: the walk left through a `break`), the winner's number in the walk (-1: none),
 *                  longest on return, the candidate the walk would have visited next (-1), nextToUpdate (a position) before the
 *                  insert, 1 when pattern analysis set the final length, matchChainPos on return
 *   ORC_TR_CAND    one row per candidate walked, ORC_HX_CAND_WORDS: position, the 2-byte probe at `longest` passed (0/1), four bytes
 *                  equal (0/1), and for those the equal bytes after the four and before (within the lookback and the candidate's
 *                  own position), what ended the forward count (ORC_HX_STOP_MISMATCH / _LIMIT = ihigh) and the backward count
 *                  (_MISMATCH / _LIMIT = the lookback / _CAND = the candidate's position), how the walk left it (ORC_HX_LEFT_*)
 *   ORC_TR_ARM     event rows of ORC_HX_EV_WORDS, unused words 0.  Word 0 below 40: ORC_ARM_* / ORC_REFUSE_*, ip, ORC_HX_SITE_*.
 *       ORC_HX_EV_SWAP   a chain-swap decision: ip, candidate, end, positions visited, largest step, the resulting distance,
 *                        matchChainPos after it, ORC_HX_SWAP_*, the last offset read (candidate + offset + 65536 is the ring index)
 *       ORC_HX_EV_PA     a candidate whose chain delta is 1: ip, the position before it, repeat state (1 not a pattern, 2 confirmed),
 *                        srcLen, forward run, backward run to position 0, backward run after the clamp at `lowest`, ORC_HX_PA_*,
 *                        1 when this event set the repeat state (ORC_HX_PA_SWAPPED: matchChainPos), bit 0: clamped by `lowest`,
 *                        bit 1: the run reached position 0
 *       ORC_HX_EV_OPT_*  the optimal parser: ip, then
 *           _NO_MATCH -;  _FIRST_NOW length, literals before;  _FIRST length, literals before, 1 when length == sufficient_len
 *           _AT_MFLIMIT cur;  _SKIP cur, p1 <= pc, the second condition of level 12 (-1: levels 10, 11);  _SEARCH_ANYWAY cur
 *           _NO_LONGER cur;  _INNER_NOW_ENOUGH / _INNER_NOW_FULL cur, length
 *           _UPDATE cur, ORC_HX_BASE_*, match length, last_match_pos rose, records written through `pos > last + 3`, through
 *                   `price <=`, refused, literal records improved
 *           _SERIES (ip behind it) hops of the reverse traversal, literal records between matches, first record a literal,
 *                   last_match_pos, matches, least and most literals priced
 *   ORC_TR_EMIT    as for levels 1..8 */
enum { ORC_HX_SEARCH_WORDS = 12, ORC_HX_CAND_WORDS = 8, ORC_HX_EV_WORDS = 12 };
enum { ORC_END_BREAK = 5 };
enum { ORC_HX_STOP_MISMATCH = 0, ORC_HX_STOP_LIMIT = 1, ORC_HX_STOP_CAND = 2 };
enum { ORC_HX_LEFT_CHAIN = 0, ORC_HX_LEFT_SWAP, ORC_HX_LEFT_PATTERN, ORC_HX_LEFT_BREAK,
       ORC_HX_LEFT_CHAIN_SWAPPED /* a chain step at a matchChainPos != 0 that an earlier candidate of this search set */ };
enum { ORC_HX_SITE_CHAIN = 0 /* level 9's loop */, ORC_HX_SITE_FIRST /* a first match encoded at once */, ORC_HX_SITE_SERIES /* the optimal parser's encode loop, and the last literals */ };
enum { ORC_HX_SWAP_OVERLAP = 0 /* candidate + longest > ip: no scan */, ORC_HX_SWAP_NONE /* distance <= 1 */, ORC_HX_SWAP_JUMP, ORC_HX_SWAP_BREAK /* distance > index */ };
enum { ORC_HX_PA_NOT_PATTERN = 0, ORC_HX_PA_BELOW_LOWEST, ORC_HX_PA_DIFFER /* four bytes differ */, ORC_HX_PA_TO_END /* lz4hc.c:379 */,
       ORC_HX_PA_TO_START_LOOKBACK /* :388, lookback != 0 */, ORC_HX_PA_TO_START_TAKEN, ORC_HX_PA_TO_START_NOT_LONGER,
       ORC_HX_PA_BREAK_DISTANCE /* :398 */, ORC_HX_PA_BREAK_DELTA /* :405 */, ORC_HX_PA_SWAPPED /* matchChainPos != 0: no analysis */ };
enum { ORC_HX_BASE_LIT_INSIDE = 0 /* cur > litlen */, ORC_HX_BASE_LIT_FROM_START /* cur <= litlen */, ORC_HX_BASE_MATCH };
enum { ORC_HX_EV_SWAP = 40, ORC_HX_EV_PA, ORC_HX_EV_OPT_NO_MATCH = 50, ORC_HX_EV_OPT_FIRST_NOW, ORC_HX_EV_OPT_FIRST, ORC_HX_EV_OPT_AT_MFLIMIT,
       ORC_HX_EV_OPT_SKIP, ORC_HX_EV_OPT_SEARCH_ANYWAY, ORC_HX_EV_OPT_NO_LONGER, ORC_HX_EV_OPT_INNER_NOW_ENOUGH, ORC_HX_EV_OPT_INNER_NOW_FULL,
       ORC_HX_EV_OPT_UPDATE, ORC_HX_EV_OPT_SERIES };
/* LZ4_compressMC (cap < 0) / LZ4_compressMC_limitedOutput — native/lz4/lz4mc.c:582-606. */
int orc_lz4mc_compress(const uint8_t* src, uint8_t* dst, int n, int cap);
int orc_lz4mc_compress_ex(const uint8_t* src, uint8_t* dst, int n, int cap, orc_trace* trace);

/* LZ4_decompress_safe — native/lz4/lz4.c:2345-2350 -> :1936-2339 (noDict, full block).
 * Returns decoded size (>=0) or a negative error. */
int orc_lz4_decompress_safe(const uint8_t* src, uint8_t* dst, int csize, int cap);
int orc_lz4_sequences(const uint8_t* src, int csize, int cap, uint32_t* tokpos, uint32_t* outpos, int maxseq, int* total);
int orc_lz4_sequences_ex(const uint8_t* src, int csize, int cap, uint32_t* tokpos, uint32_t* outpos, uint32_t* fields, int maxseq, int* total);

/* ---- container (native/4mc.c:220-386 writer, :560-707 reader; format spec 4mc-format-spec) */
typedef int (*orc_block_codec_fn)(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);

size_t  orc_container_bound(size_t n);
/* Writes header + blocks + end mark + footer.  `compress` is called once per <=4 MiB block with
 * cap = n-1 (native/4mc.c:301); a return <= 0 means "store raw" (native/4mc.c:318-329). */
int64_t orc_container_compress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap,
                               uint32_t magic, orc_block_codec_fn compress, void* ctx);
/* Reads ONE stream (header..footer).  Returns decoded bytes (>=0) and sets *consumed, or
 * -(exit code) as the reference CLI would exit (2 input / 4 content; native/4mc.c:135-161). */
int64_t orc_container_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap,
                                 uint32_t magic, orc_block_codec_fn decompress, void* ctx,
                                 size_t* consumed);

/* ZSTD_decompress for 4mz payloads (zstd_port.cpp) - native/zstd/decompress/zstd_decompress.c:1112.
 * Returns decoded bytes or < 0 where the reference reports an error. */
int64_t orc_zstd_decompress(const uint8_t* src, size_t csize, uint8_t* dst, size_t cap);
int     orc_codec_zstd_decode(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);

/* ZSTD_compress(dst, cap, src, n, level) for the 4mz encode path (zstd_enc_port.c) -
 * native/zstd/compress/zstd_compress.c:4806 as called by native/4mc.c:467.  Returns the frame size,
 * a negative ZSTD error number (-70 = dstSize_tooSmall), or ORC_ZSTD_UNSUPPORTED for a level outside
 * 1..12 (the port restates every row of clevels.h for those twelve: fast, dfast, greedy, lazy, lazy2,
 * btlazy2 and btopt).
 *
 * orc_zstd_compress_ex is the same call with an orc_trace (NULL: none, and nothing is computed for it).  The
 * rules of orc_trace hold: a row is written whole or not at all, n[] counts also what found no room.  Tables
 * (int32 rows; positions are offsets into the input):
 *   ORC_TR_EMIT    one row per stored sequence and one for the last literals of every inner block (match length 0,
 *                  off_base 0): inner block, start of the literals, literal length, off_base as stored (1..3: a
 *                  repeat offset, which with literal length 0 names the next one: 1 -> rep2, 2 -> rep3,
 *                  3 -> rep1 - 1), match length.  The rows of one block add up to its length.
 *   ORC_TR_BLOCK   (the slot of ORC_TR_CAND) one row per inner block, ORC_ZBLK_* names its words.
 *   ORC_TR_SEARCH  one row per search of the lazy family: ORC_ZSEARCH_HC / _ROW / _BT, ip, candidates compared,
 *                  ORC_END_* (why the walk ended), the winner's number in the walk (-1: none), its length.
 *                  btopt, one row per call of the match collector: ORC_ZSEARCH_OPT, ip, matches returned, 1 when the
 *                  longest is beyond sufficient_len, 1 when the 3-byte hash table gave one, the longest length.
 *   ORC_TR_ARM     ORC_ZARM_*, ip, a value (each arm says which). */
#define ORC_ZSTD_UNSUPPORTED (-1000)
enum { ORC_ZTR_SEARCH_WORDS = 6, ORC_ZTR_BLOCK_WORDS = 28, ORC_ZTR_ARM_WORDS = 3, ORC_ZTR_EMIT_WORDS = 5 };
enum { ORC_TR_BLOCK = ORC_TR_CAND };
enum { ORC_ZSEARCH_HC = 0, ORC_ZSEARCH_ROW = 1, ORC_ZSEARCH_BT = 2, ORC_ZSEARCH_OPT = 3 };
enum { ORC_END_INPUT = 4 };                 /* the match ran to the end of the input: the walk stops there */
enum {  /* words of a BLOCK row */
    ORC_ZBLK_NUMBER = 0, ORC_ZBLK_START, ORC_ZBLK_LEN, ORC_ZBLK_STRATEGY /* 1 fast .. 7 btopt */, ORC_ZBLK_NSEQ, ORC_ZBLK_NLIT,
    ORC_ZBLK_LIT_TYPE,      /* 0 raw, 1 rle, 2 Huffman with its table, 3 treeless; -1: no literals section was written */
    ORC_ZBLK_LIT_STREAMS,   /* 1 or 4 for a Huffman attempt, 0 where none was made */
    ORC_ZBLK_HUF_DROPPED,   /* ORC_ZHUF_* */
    ORC_ZBLK_LL_TYPE, ORC_ZBLK_LL_RULE, ORC_ZBLK_OF_TYPE, ORC_ZBLK_OF_RULE, ORC_ZBLK_ML_TYPE, ORC_ZBLK_ML_RULE,   /* 0 predefined, 1 rle, 2 fse, 3 repeat (-1: no sequences); ORC_ZSEL_* */
    ORC_ZBLK_OUTCOME,       /* ORC_ZOUT_* */
    ORC_ZBLK_REP_IN,        /* rep[0..2] on entry */
    ORC_ZBLK_REP_OUT = ORC_ZBLK_REP_IN + 3,   /* rep[0..2] on exit (the third moves in btopt alone) */
    ORC_ZBLK_PARAMS = ORC_ZBLK_REP_OUT + 3    /* the row of the level table that ran, after the clamps: windowLog, chainLog, hashLog, searchLog, minMatch, targetLength */
};
enum { ORC_ZHUF_KEPT = 0, ORC_ZHUF_TOO_SMALL /* below the 63 / 6 byte floor: no attempt */, ORC_ZHUF_NO_GAIN /* attempt not smaller than n - minGain, or refused by the histogram */,
       ORC_ZHUF_ONE_SYMBOL /* -> rle */ };
enum { ORC_ZSEL_ONE_SYMBOL = 1 /* rle, or predefined for at most two sequences */, ORC_ZSEL_REPEAT_SMALL /* fast .. greedy: a valid table and fewer than 1000 sequences */,
       ORC_ZSEL_PREDEF_FEW /* fast .. greedy: too few sequences or too flat for a table */, ORC_ZSEL_FSE_DEFAULT /* fast .. greedy: otherwise */,
       ORC_ZSEL_COST_PREDEF, ORC_ZSEL_COST_REPEAT, ORC_ZSEL_COST_FSE /* lazy and above: the cheapest of the three estimates */ };
enum { ORC_ZOUT_COMPRESSED = 0, ORC_ZOUT_RAW_NOT_SMALLER /* not below len - (len >> 6) - 2 */, ORC_ZOUT_RAW_TOO_SMALL /* dstSize_tooSmall with len <= the block's capacity */,
       ORC_ZOUT_RLE, ORC_ZOUT_RAW_SHORT /* fewer than 7 bytes: no attempt */, ORC_ZOUT_REFUSED /* the frame ends with an error here */ };
enum {  /* fast and dfast; value */
    ORC_ZARM_F_HIT_IP0 = 1,         /* hash hit at ip0; step */
    ORC_ZARM_F_HIT_IP1,             /* hash hit at ip1; step */
    ORC_ZARM_F_REP_IP2,             /* repeat offset 1 at ip2; step */
    ORC_ZARM_D_REP_IP1,             /* dfast: repeat offset 1 at ip + 1; step */
    ORC_ZARM_D_LONG,                /* dfast: the 8-byte table hit at ip; step */
    ORC_ZARM_D_SHORT,               /* dfast: the short table hit, the long table at ip + 1 did not; step */
    ORC_ZARM_D_SHORT_THEN_LONG,     /* dfast: the short table hit and the long table at ip + 1 took over; step */
    ORC_ZARM_STEP_UP,               /* the search step grew; the new step */
    ORC_ZARM_CATCHUP,               /* ip = the match's start after the backward walk; bytes walked back */
    ORC_ZARM_REP2_AFTER,            /* a repeat-offset-2 match right after a match; the iteration, from 1 */
    ORC_ZARM_REP_ZEROED,            /* block start: repeat offsets beyond the window put aside; 1 = rep1, 2 = rep2, 3 = both */
    ORC_ZARM_REP_RESTORED,          /* block end (ip = its end): put back; same bits */
    ORC_ZARM_START_NEAR_REP,        /* a block after the first: its first match starts less than max(rep1, rep2) + 4 past the block's start (the offsets as the block got them); that maximum */
    ORC_ZARM_END_BEHIND_ILIMIT,     /* a match ended behind ilimit: no table refill, no repeat loop; bytes left to the block's end */
    ORC_ZARM_OUT_OF_WINDOW,         /* every strategy but btlazy2 / btopt: a candidate holding ip's four bytes refused because it lies below the window; its distance */
    /* greedy, lazy, lazy2, btlazy2 */
    ORC_ZARM_L_REP_IP1 = 20,        /* repeat offset 1 at ip + 1 found (greedy: taken at once); its length */
    ORC_ZARM_L_SEARCH_WINS,         /* the search at ip beat it (or stood alone); its length */
    ORC_ZARM_L_D1_REP, ORC_ZARM_L_D1_SEARCH, ORC_ZARM_L_D2_REP, ORC_ZARM_L_D2_SEARCH,   /* an improvement at depth 1 / 2, by repeat offset / by search; its length */
    ORC_ZARM_L_CATCHUP,             /* as ORC_ZARM_CATCHUP */
    ORC_ZARM_L_REP_LOOP,            /* as ORC_ZARM_REP2_AFTER */
    ORC_ZARM_L_STEP_GROWN,          /* no match and the step to the next search is above 1; the step */
    ORC_ZARM_L_NTU_LIMIT,           /* block start, greedy and above (the fast finders keep no next_to_update): it lay more than 384 behind and moved up; the gap closed to (<= 192) */
    ORC_ZARM_BT_BATCH_FULL,         /* btlazy2: the stack of unsorted candidates reached nb_compares; that number */
    ORC_ZARM_ROW_WRAPS,             /* row finder: an insert moved a row's head from 0 onto its last entry and that entry was in use: the row's inserts have gone round; entries per row */
    ORC_ZARM_ROW_CACHE_AT_BLOCK,    /* row finder, a block after the first: the 8-entry hash cache is filled from next_to_update; 100000 + (block start - that position): above 100000 the cache starts with hashes of the previous block's last positions */
    /* btopt */
    ORC_ZARM_O_PREDEF = 40,         /* block start: predefined prices (at most 1024 bytes); the block's length */
    ORC_ZARM_O_STATS,               /* block start: first-block statistics; the block's length */
    ORC_ZARM_O_IMMEDIATE,           /* a match beyond sufficient_len taken at once; its length */
    ORC_ZARM_O_ARRAY_FULL,          /* cur + length reached the price array's end (4096); cur + length */
    ORC_ZARM_O_LL0_SHIFT,           /* a repeat-offset arrival with no literals before it: off_base names the next offset; off_base */
    ORC_ZARM_O_NOT_GREEDY           /* the series' first sequence is not the longest match found at its start; the length given up */
};
int64_t orc_zstd_compress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level);
int64_t orc_zstd_compress_ex(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level, orc_trace* trace);
int     orc_codec_zstd1(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);

/* ZSTD_initCStream(level) + ZSTD_compressStream + ZSTD_endStream for levels 1..4 (what ZstCodec writes, jniZStreamCompressor.c:86-137):
 * the frame without a content size, blocks of 128 KiB out of an input ring of window + 128 KiB bytes (zstd_compress.c:1591-1594,
 * :5517-5519), the window bookkeeping of ZSTD_window_update / ZSTD_window_enforceMaxDist (zstd_compress_internal.h:1177-1212,
 * :1086-1122), the ext-dict parsers (zstd_fast.c:684-935, zstd_double_fast.c:592-734) and the prefix-only parsers with
 * ZSTD_getLowestPrefixIndex's repeat-offset limit, and the block entropy stage of orc_zstd_compress.  The source is read at its
 * stream positions (both ring segments are contiguous there); every decision is taken on the reference's indices.
 * Returns the frame size, -70 when `cap` is too small (the reference never fails on output: give 2 n + 4096), ORC_ZSTD_UNSUPPORTED
 * for another level.  `trace` (NULL: none) never changes a byte; `mutate` (ORC_ZMUT_*, 0: none) takes ONE decision wrongly, for
 * the test that shows the catalogue of tests/zst_write_shapes.py tells each apart.
 * Tables (int32 rows, positions are stream offsets, indices are positions + 2):
 *   ORC_TR_BLOCK   ORC_ZSTR_BLOCK_WORDS, ORC_ZSB_* names the words
 *   ORC_TR_SEARCH  ORC_ZSTR_SEARCH_WORDS, one row per search of an ext-dict parser: block, first position, pairs (fast) or positions
 *                  (dfast) probed before the event, the step at the event, ORC_ZSARM_* of the event (0: the block ended), bytes from the
 *                  anchor to the event, the least number of probes between two probes of this search that fell into one table slot
 *                  (0: none within 63 probes), 1 when such a pair at most 15 probes apart also holds equal words, 1 when the two
 *                  positions of one pair fell into one slot (fast), the number of probes made when the step first grew inside the search (0: it did not)
 *   ORC_TR_ARM     ORC_ZSTR_SEQ_WORDS, one row per sequence: block, ORC_ZSARM_*, the match's start in the input (after the catch-up),
 *                  the candidate's index (a repeat-offset arm: the repeat index), segment the match starts in (0 ext, 1 prefix), 1 when
 *                  its forward count crosses the wrap point, catch-up length, ORC_ZSTOP_*, match length, bytes from the match's end to the
 *                  block's end, 1 when the candidate was entered by this same search, the turn of the behind-match loop (from 1).
 *                  A prefix-only block gives block, ORC_ZSARM_PFX_*, start, off_base, 1, 0, 0, 0, match length, 0, 0, 0.
 *   ORC_TR_EMIT    ORC_ZSTR_REP_WORDS, one row per repeat-offset test of an ext-dict parser that found equal bytes: block, site (0 the
 *                  search, 1 behind a match), the tested position, repeat index - prefixStartIndex, 1 accepted / 0 refused by the rule;
 *                  and one row per table entry at or up to 7 below the candidate bound that holds the probe's four bytes and is refused for
 *                  its index: block, site 2, the probing position, entry - dictStartIndex (0: dfast alone), 0 */
enum { ORC_ZSTR_SEARCH_WORDS = 10, ORC_ZSTR_BLOCK_WORDS = 20, ORC_ZSTR_SEQ_WORDS = 12, ORC_ZSTR_REP_WORDS = 5 };
enum { ORC_ZSB_NUMBER = 0, ORC_ZSB_START, ORC_ZSB_LEN, ORC_ZSB_MODE /* ORC_ZSMODE_* */, ORC_ZSB_DICT_IDX, ORC_ZSB_PFX_IDX,
       ORC_ZSB_REP_IN /* 2 words */, ORC_ZSB_REP_OUT = ORC_ZSB_REP_IN + 2 /* 2 words */, ORC_ZSB_ZEROED = ORC_ZSB_REP_OUT + 2 /* bit 0 rep1, bit 1 rep2 */,
       ORC_ZSB_RESTORED /* bit 0: rep1 <- saved1, bit 1: rep2 <- saved2, bit 2: rep2 <- saved1 */, ORC_ZSB_TYPE /* 0 raw, 1 rle, 2 compressed */,
       ORC_ZSB_NSEQ, ORC_ZSB_IN_CYCLE /* k mod m */, ORC_ZSB_CYCLE /* k / m */, ORC_ZSB_DEV_MAX, ORC_ZSB_REF_MAX /* prefix-only blocks */,
       ORC_ZSB_MAX_REP /* ext blocks of fast */, ORC_ZSB_LAST };
enum { ORC_ZSMODE_SHORT = 0 /* fewer than 7 bytes: not parsed */, ORC_ZSMODE_PREFIX, ORC_ZSMODE_PREFIX_CARRY /* an offset in (dev_max, ref_max] came in */,
       ORC_ZSMODE_EXT, ORC_ZSMODE_HANDOVER /* ext-dict mode, dictStartIndex == prefixStartIndex: the prefix-only parser's */, ORC_ZSMODE_HANDOVER_CARRY };
enum { ORC_ZSARM_REP = 1 /* fast: at ip2; dfast: at ip + 1 */, ORC_ZSARM_HIT_IP0, ORC_ZSARM_HIT_IP1, ORC_ZSARM_LONG, ORC_ZSARM_SHORT, ORC_ZSARM_SHORT_THEN_LONG,
       ORC_ZSARM_REP_LOOP /* behind a match */, ORC_ZSARM_PFX_REP, ORC_ZSARM_PFX_HIT };
enum { ORC_ZSTOP_NONE = 0 /* no catch-up is made (repeat-offset arms) */, ORC_ZSTOP_ANCHOR, ORC_ZSTOP_LOW_EQUAL /* the segment's low end, equal bytes in front */,
       ORC_ZSTOP_LOW, ORC_ZSTOP_MISMATCH };
enum { ORC_ZMUT_NONE = 0,
       ORC_ZMUT_CATCHUP_PFX,      /* the catch-up ignores the segment's low end, prefix source */
       ORC_ZMUT_CATCHUP_EXT,      /* ... ext source */
       ORC_ZMUT_FAST_REP_3,       /* fast search: (u32)(pfx - rep_idx) >= 3 */
       ORC_ZMUT_AFTER_REP_4,      /* behind a match: (u32)(pfx - 1 - rep_idx2) >= 4 */
       ORC_ZMUT_FAST_STRICT,      /* fast: candidate > dictStartIndex */
       ORC_ZMUT_DFAST_LOOSE,      /* dfast: candidate >= dictStartIndex */
       ORC_ZMUT_MAXREP_GT,        /* ext block start: offset > max_rep is dropped (not >=) */
       ORC_ZMUT_NO_RESTORE,       /* the saved repeat offsets are not put back */
       ORC_ZMUT_HANDOVER_EXT,     /* the hand-over block goes to the ext parser */
       ORC_ZMUT_DICT_FROM_START,  /* dictStartIndex from the block's start */
       ORC_ZMUT_CARRY_DROPPED,    /* a carried offset above dev_max is dropped */
       ORC_ZMUT_NO_UPGRADE,       /* dfast: no long match at ip + 1 */
       ORC_ZMUT_COUNT };
int64_t orc_zstd_stream_compress_ex(const uint8_t* src, size_t n, int level, uint8_t* dst, size_t cap, orc_trace* trace, int mutate);

/* codec adaptors with the orc_block_codec_fn shape (ctx unused) */
int orc_codec_lz4_fast(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);
int orc_codec_lz4_decode(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);
int orc_codec_lz4hc4(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);
int orc_codec_lz4hc8(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);

#ifdef __cplusplus
}
#endif
#endif
