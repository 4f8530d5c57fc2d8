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

/* LZ4_compress_HC, hash-chain levels 1..8 (4mc uses 4 and 8) - native/lz4/lz4hc.c:958-973 -> :553-788.
 * Returns bytes written, 0 when it does not fit `cap`, -2 for levels this port does not cover. */
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
 * a negative ZSTD error number (-70 = dstSize_tooSmall), or ORC_ZSTD_UNSUPPORTED for levels the
 * port does not restate (only level 1 / strategy "fast" so far). */
#define ORC_ZSTD_UNSUPPORTED (-1000)
int64_t orc_zstd_compress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, int level);
int     orc_codec_zstd1(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);

/* codec adaptors with the orc_block_codec_fn shape (ctx unused) */
int orc_codec_lz4_fast(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);
int orc_codec_lz4_decode(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);
int orc_codec_lz4hc4(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);
int orc_codec_lz4hc8(void* ctx, const uint8_t* src, int n, uint8_t* dst, int cap);

#ifdef __cplusplus
}
#endif
#endif
