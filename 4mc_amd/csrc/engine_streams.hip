// 4mc_amd/csrc/engine_streams.hip — Hadoop block streams (bstream.hip), the .4mc / .4mz images that share their write plan, and .zst streams read (zst.hip) and written (zstd_encode.hip).
#include "engine_int.h"

namespace {
// ---- .zst streams read.  Table entries per round: the setter's value, else FOURMC_ZST_ROUND_BLOCKS (read at every call), else
// what 4 GiB of round workspace hold
uint32_t g_zst_round = 0;
uint32_t zst_round()
{
    long long v = g_zst_round;
    if (!v) { const char* e = getenv("FOURMC_ZST_ROUND_BLOCKS"); v = e && *e ? atoll(e) : 0; }
    if (v < 1) v = (long long)((size_t(4) << 30) / fourmc_zst_per_block_bytes());
    return uint32_t(v > (1 << 24) ? (1 << 24) : v);
}
struct ZstLeases { WsLease tab{&g_img_ws}, round{&g_img_stage}, serial; hipStream_t s; };
int zst_ws(void* ctx, int which, size_t need, void** out)
{
    ZstLeases* l = static_cast<ZstLeases*>(ctx);
    return (which == 0 ? l->tab : which == 1 ? l->round : l->serial).get(l->s, need, out);
}
int zsts_run(const void* d_images, void* d_dst, fourmc_zst_item* items, uint32_t n, hipStream_t s)
{
    if (int r = ensure_device()) return r;
    ZstLeases l; l.s = s;
    return fourmc_zst_run(d_images, d_dst, items, n, zst_round(), zst_ws, &l, g_err, sizeof g_err, s);
}

// ---- .zst streams written
constexpr uint64_t kZstwMaxSource = 0xC0000000ull;
// The encode of n streams: the single call is its n = 1 case.  Workspace (g_img_ws): the items and the jobs (one upload), then the
// per-stream encoder areas (the stream's codec workspace).  One synchronization: the items come back with their status.
int zstw_run(const void* d_src, void* d_images, fourmc_zstw_item* items, uint32_t n, hipStream_t s)
{
    std::vector<fourmc_zstw_item> up(items, items + n);
    std::vector<fourmc_zstw_job> jobs[2];
    uint64_t work = 0;
    for (int fam = 1; fam <= 2; fam++)                       // the "fast" jobs first, the "dfast" jobs behind them
        for (uint32_t i = 0; i < n; i++) {
            fourmc_zstw_status st = {};
            const int strat = fourmc_zst_stream_strategy(items[i].level);
            if (!strat) st.reason = FOURMC_ZSTW_LEVEL;
            else if (items[i].src_bytes > kZstwMaxSource) st.reason = FOURMC_ZSTW_TOO_LONG;
            if (fam == 1) up[i].status = st;
            if (st.reason != FOURMC_ZSTW_OK || strat != fam) continue;
            fourmc_zstw_job j; j.item = i; j.level = items[i].level; j.work_off = work;
            work += align256(fourmc_zstd_enc_work_bytes(1, items[i].level));
            jobs[fam - 1].push_back(j);
        }
    const uint32_t nf = uint32_t(jobs[0].size()), nd = uint32_t(jobs[1].size());
    if (nf + nd) {
        if (int r = ensure_device()) return r;
        const size_t o_jobs = align256(size_t(n) * sizeof(fourmc_zstw_item)), head = o_jobs + align256(size_t(nf + nd) * sizeof(fourmc_zstw_job));
        std::vector<char> stage(head);
        memcpy(stage.data(), up.data(), size_t(n) * sizeof(fourmc_zstw_item));
        if (nf) memcpy(stage.data() + o_jobs, jobs[0].data(), size_t(nf) * sizeof(fourmc_zstw_job));
        if (nd) memcpy(stage.data() + o_jobs + size_t(nf) * sizeof(fourmc_zstw_job), jobs[1].data(), size_t(nd) * sizeof(fourmc_zstw_job));
        WsLease ws(&g_img_ws), cw; void* w = nullptr; void* d_work = nullptr;
        if (int r = ws.get(s, head, &w)) return r;
        if (int r = lease_codec_ws(cw, s, size_t(work), &d_work)) return r;
        char* base = static_cast<char*>(w);
        HIP_TRY(hipMemcpyAsync(base, stage.data(), head, hipMemcpyHostToDevice, s));
        HIP_TRY(fourmc_launch_zst_stream(d_src, d_images, reinterpret_cast<fourmc_zstw_item*>(base), reinterpret_cast<const fourmc_zstw_job*>(base + o_jobs),
                                         nf, nd, d_work, s));
        HIP_TRY(hipMemcpyAsync(up.data(), base, size_t(n) * sizeof(fourmc_zstw_item), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (uint32_t i = 0; i < n; i++) items[i].status = up[i].status;
    return FOURMC_OK;
}
} // namespace

int encode_raw_blocks(int codec, int level, const void* d_src, void* d_stage, fourmc_block* d_blk, uint32_t m, hipStream_t s)
{
    switch (codec) {
        case FOURMC_CODEC_LZ4_FAST: return fourmc_gpu_lz4_compress_fast(d_src, d_stage, d_blk, m, s);
        case FOURMC_CODEC_LZ4_MC:   return fourmc_gpu_lz4_compress_mc(d_src, d_stage, d_blk, m, s);
        case FOURMC_CODEC_LZ4_HC:   return fourmc_gpu_lz4_compress_hc(d_src, d_stage, d_blk, m, level, s);
        default:                    return fourmc_gpu_zstd_compress(d_src, d_stage, d_blk, m, level, s);
    }
}

extern "C" {

// ------------------------------------------------------------------------ Hadoop block streams (bstream.hip)
// The part files of Lz4Codec / ZstdCodec and their siblings: BlockCompressorStream's framing around raw LZ4 blocks / zstd frames
// (include/fourmc_gpu.h has the format, the reader rule and where they come from).
static int bs_family(int codec)                     // 0 the LZ4 codecs, 1 zstd, -1 no codec
{
    if (codec == FOURMC_CODEC_LZ4_FAST || codec == FOURMC_CODEC_LZ4_MC || codec == FOURMC_CODEC_LZ4_HC) return 0;
    return codec == FOURMC_CODEC_ZSTD ? 1 : -1;
}
static uint32_t bs_block_bound(int zstd, uint32_t n)
{ return zstd ? uint32_t(fourmc_ZSTD_compressBound(n)) : uint32_t(fourmc_LZ4_compressBound(int(n))); }
static int bs_bad_codec(const char* who, int codec)
{ snprintf(g_err, sizeof g_err, "%s: codec %d is none of FOURMC_CODEC_*", who, codec); return FOURMC_EINVAL; }

// MAX_INPUT_SIZE of BlockCompressorStream as the codecs construct it: the buffer less the overhead (Lz4Codec.java:102-103)
uint32_t fourmc_gpu_bstream_max_input(int codec)
{
    const int zstd = bs_family(codec);
    if (zstd < 0) return 0;
    return FOURMC_BLOCKSIZE - (bs_block_bound(zstd, FOURMC_BLOCKSIZE) - FOURMC_BLOCKSIZE);
}

uint64_t fourmc_gpu_bstream_bound(uint64_t src_bytes, int codec, uint32_t group_bytes)
{
    const int zstd = bs_family(codec);
    if (zstd < 0) return 0;
    const uint32_t M = fourmc_gpu_bstream_max_input(codec), G = group_bytes ? group_bytes : M;
    if (G > M) return 0;
    if (!src_bytes) return 4;
    const uint64_t full = src_bytes / G, per = 8ull + bs_block_bound(zstd, G);
    const uint32_t rest = uint32_t(src_bytes % G);
    if (full > (~0ull - 2 * per) / per) return ~0ull;
    return full * per + (rest ? 8ull + bs_block_bound(zstd, rest) : 0);
}

// Pieces of at most kBsPiece groups: descriptors, the raw codec call into the staging slots, the scan (its 64-bit carry lives on the
// device, in the summary) and the pack; one read-back of the length and the bad results at the end.
constexpr uint32_t kBsPiece = 512;                  // the file API's batch
int fourmc_gpu_bstream_compress(const void* d_src, uint64_t src_bytes, void* d_image, uint64_t image_cap, uint64_t* image_bytes,
                                int codec, int level, uint32_t group_bytes, void* stream)
{
    const int zstd = bs_family(codec);
    if (zstd < 0) return bs_bad_codec("bstream_compress", codec);
    if (!image_bytes || !d_image || (src_bytes && !d_src)) { snprintf(g_err, sizeof g_err, "bstream_compress: null pointer"); return FOURMC_EINVAL; }
    const uint32_t M = fourmc_gpu_bstream_max_input(codec), G = group_bytes ? group_bytes : M;
    if (G > M) { snprintf(g_err, sizeof g_err, "bstream_compress: group_bytes %u above the %u a chunk may hold", group_bytes, M); return FOURMC_EINVAL; }
    const uint64_t need = fourmc_gpu_bstream_bound(src_bytes, codec, group_bytes);
    if (image_cap < need) {
        snprintf(g_err, sizeof g_err, "bstream_compress: capacity %llu below the bound %llu", (unsigned long long)image_cap, (unsigned long long)need);
        return FOURMC_EINVAL;
    }
    if (zstd && !fourmc_zstd_enc_level_ok(level)) { snprintf(g_err, sizeof g_err, "ZSTD level %d not on the device (levels 1..12 are)", level); return FOURMC_EUNSUP; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!src_bytes) {                                // the stream nothing was written to: finish()'s rawlen of 0
        HIP_TRY(hipMemsetAsync(d_image, 0, 4, s));
        HIP_TRY(hipStreamSynchronize(s));
        *image_bytes = 4;
        return FOURMC_OK;
    }
    const uint64_t ng = src_bytes / G + (src_bytes % G ? 1 : 0);
    const uint32_t piece = uint32_t(ng < kBsPiece ? ng : kBsPiece);
    const uint32_t stride = uint32_t(align256(bs_block_bound(zstd, uint32_t(src_bytes < G ? src_bytes : G))));
    const size_t o_off = align256(sizeof(fourmc_bstream_enc_summary)), o_blk = o_off + align256(size_t(piece) * 8);
    const size_t o_stage = o_blk + align256(size_t(piece) * sizeof(fourmc_block));
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, o_stage + size_t(piece) * stride + kImagesStageSlack, &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_sum = reinterpret_cast<fourmc_bstream_enc_summary*>(base);
    auto* d_off = reinterpret_cast<uint64_t*>(base + o_off);
    auto* d_blk = reinterpret_cast<fourmc_block*>(base + o_blk);
    void* d_stage = base + o_stage;
    HIP_TRY(hipMemsetAsync(d_sum, 0, sizeof(fourmc_bstream_enc_summary), s));
    for (uint64_t g0 = 0; g0 < ng; g0 += piece) {
        const uint32_t m = uint32_t(ng - g0 < piece ? ng - g0 : piece);
        const uint64_t src0 = g0 * G, left = src_bytes - src0, span = uint64_t(m) * G;
        HIP_TRY(fourmc_launch_bstream_enc_desc(d_blk, src0, left < span ? left : span, G, stride, m, zstd, codec == FOURMC_CODEC_LZ4_MC, s));
        if (int r = encode_raw_blocks(codec, level, d_src, d_stage, d_blk, m, s)) return r;
        HIP_TRY(fourmc_launch_bstream_enc_pack(d_image, d_blk, d_off, m, zstd, d_stage, d_sum, s));
    }
    fourmc_bstream_enc_summary h;
    HIP_TRY(hipMemcpyAsync(&h, d_sum, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h.bad) { snprintf(g_err, sizeof g_err, "bstream_compress: %llu groups with a codec result outside [1, bound]", (unsigned long long)h.bad); return FOURMC_EINVAL; }
    *image_bytes = h.image_bytes;
    return FOURMC_OK;
}

// ---- block streams from write() sizes -------------------------------------------------------------------------------------------
// The most chunks and written groups any schedule over S bytes has (include/fourmc_gpu.h has the argument)
static uint64_t bsw_max_chunks(uint64_t S, uint32_t M) { const uint64_t r = S % (uint64_t(M) + 2); return 3 * (S / (uint64_t(M) + 2)) + (r < 2 ? r : 2); }
static uint64_t bsw_max_groups(uint64_t S, uint32_t M) { return 2 * (S / (uint64_t(M) + 1)) + (S % (uint64_t(M) + 1) ? 1 : 0); }

uint64_t fourmc_gpu_bstream_writes_bound(uint64_t src_bytes, int codec)
{
    const int zstd = bs_family(codec);
    if (zstd < 0) return 0;
    if (!src_bytes) return 4;
    const uint32_t M = fourmc_gpu_bstream_max_input(codec);
    const uint64_t C = bsw_max_chunks(src_bytes, M), G = bsw_max_groups(src_bytes, M);
    const uint64_t over = zstd ? src_bytes / 256 + 64 * C : src_bytes / 255 + 16 * C;
    if (src_bytes > (~0ull >> 1)) return ~0ull;
    return src_bytes + over + 4 * C + 4 * G + 4;
}

} // extern "C"

// ---- what bstreams_compress and images_compress_writes share: the argument pass, the plan and the rounds' common part --------------
namespace {
// Chunks per round: FOURMC_BSW_ROUND, read at every call (a test sets it between two calls)
uint32_t bsw_round()
{
    const char* e = getenv("FOURMC_BSW_ROUND");
    const long v = e && *e ? atol(e) : long(kBsPiece);
    return uint32_t(v < 1 ? 1 : v > (1 << 20) ? (1 << 20) : v);
}

// The checks of n > 0 items, in this order per item: null source, null write table, source, write sizes, region (the size query,
// d_images null, looks at no region); then the regions against each other.  Fills tile0[0 .. n]: the first 64-entry tile of every
// stream's write sizes.  Item: fourmc_bstream_enc_item or fourmc_image_wr_item, whose first nine fields lie at the same offsets.
template <class Item>
int bsw_args(const char* who, const void* d_src, uint64_t src_total, const uint32_t* d_writes, uint64_t writes_total, const void* d_images,
             uint64_t images_bytes, const Item* items, uint32_t n, std::vector<uint64_t>& tile0)
{
    std::vector<std::pair<uint64_t, uint64_t>> d;
    if (d_images) d.reserve(n);
    uint64_t tiles = 0;
    for (uint32_t i = 0; i < n; i++) {
        const Item& it = items[i];
        if (it.src_bytes && !d_src) { snprintf(g_err, sizeof g_err, "%s: null source", who); return FOURMC_EINVAL; }
        if (it.n_writes && !d_writes) { snprintf(g_err, sizeof g_err, "%s: null write table", who); return FOURMC_EINVAL; }
        if (span_outside(it.src_off, it.src_bytes, src_total)) return source_beyond(who, "stream", i, src_total);
        if (span_outside(it.writes_off, it.n_writes, writes_total)) return writes_beyond(who, i, writes_total);
        tile0[i] = tiles;
        tiles += it.n_writes / 64 + (it.n_writes % 64 ? 1 : 0);
        if (!d_images) continue;                          // the size query looks at no region
        if (span_outside(it.image_off, it.image_cap, images_bytes)) return region_beyond(who, "stream", i, images_bytes);
        if (it.image_cap) d.emplace_back(it.image_off, it.image_off + it.image_cap);
    }
    tile0[n] = tiles;
    return regions_overlap(who, "image regions", d);
}

// One call's state.  The caller sets the first line; bsw_plan() fills the second and third, bsw_round_open() the rest.
// g_img_ws: the planner's items, the first tile of every stream, the plans and the tile prefixes - what the plan computes and the
// rounds read.  g_img_stage, sized after the plan's read-back (so that sizing it cannot move the prefixes): the slices, the group
// table, the descriptors and side entries of one round, the caller's own arrays (d_own) and one round's staging.
struct BswCall {
    const void* d_src; const uint32_t* d_writes; uint32_t n, M; int zstd, codec, level; hipStream_t s;
    std::vector<fourmc_bsw_plan> plans; std::vector<fourmc_bsw_slice> slices; std::vector<uint64_t> worst; fourmc_bsw_slice at = {};
    WsLease ws{&g_img_ws}; fourmc_bstream_enc_item* d_items; uint64_t* d_tile0; fourmc_bsw_plan* d_plans; uint64_t* d_prefix;
    WsLease ws2{&g_img_stage}; uint64_t nc; uint32_t piece; fourmc_bsw_slice* d_slices; fourmc_bsw_group* d_grp; fourmc_block* d_blk;
    fourmc_bsw_side* d_side; char* d_own; char* d_stage;
};

// The plan of every stream, read back (the call's first synchronization), and each planned stream's share of the chunk numbers, the
// group table and the staging: c.slices, their totals in c.at.  `up`: the planner's items.  worst(plan, item): the stream's
// worst-case length, kept in c.worst; when the call writes, a smaller image_cap is the verdict FOURMC_BSW_CAP.  `noun`: what the
// family calls a chunk.
template <class Worst>
int bsw_plan(BswCall& c, const char* who, const char* noun, const fourmc_bstream_enc_item* up, const std::vector<uint64_t>& tile0, bool writes,
             Worst worst)
{
    const uint32_t n = c.n;
    hipStream_t s = c.s;
    const uint64_t ntiles = tile0[n];
    const size_t o_tile0 = align256(size_t(n) * sizeof(fourmc_bstream_enc_item)), o_plans = o_tile0 + align256((size_t(n) + 1) * 8);
    const size_t o_prefix = o_plans + align256(size_t(n) * sizeof(fourmc_bsw_plan));
    void* w = nullptr;
    if (int r = c.ws.get(s, o_prefix + size_t(ntiles) * 8, &w)) return r;
    char* base = static_cast<char*>(w);
    c.d_items = reinterpret_cast<fourmc_bstream_enc_item*>(base);
    c.d_tile0 = reinterpret_cast<uint64_t*>(base + o_tile0);
    c.d_plans = reinterpret_cast<fourmc_bsw_plan*>(base + o_plans);
    c.d_prefix = reinterpret_cast<uint64_t*>(base + o_prefix);
    HIP_TRY(hipMemcpyAsync(c.d_items, up, size_t(n) * sizeof(fourmc_bstream_enc_item), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(c.d_tile0, tile0.data(), (size_t(n) + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(fourmc_launch_bsw_sums(c.d_writes, c.d_items, c.d_tile0, n, ntiles, c.d_prefix, c.d_plans, s));
    HIP_TRY(fourmc_launch_bsw_chase(c.d_writes, c.d_items, c.d_tile0, c.d_prefix, n, c.M, c.zstd, c.d_plans, nullptr, nullptr, s));
    c.plans = std::vector<fourmc_bsw_plan>(n);
    HIP_TRY(hipMemcpyAsync(c.plans.data(), c.d_plans, size_t(n) * sizeof(fourmc_bsw_plan), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c.slices = std::vector<fourmc_bsw_slice>(size_t(n) + 1);
    c.worst = std::vector<uint64_t>(n);
    fourmc_bsw_slice& at = c.at;
    for (uint32_t i = 0; i < n; i++) {
        fourmc_bsw_plan& pl = c.plans[i];
        if (pl.reason == FOURMC_BSW_OK && (pl.groups > 0xFFFFFFFFull || pl.chunks > 0x7FFFFFFFull)) {
            snprintf(g_err, sizeof g_err, "%s: stream %u has %llu %s", who, i, (unsigned long long)pl.chunks, noun);
            return FOURMC_EUNSUP;
        }
        c.worst[i] = worst(pl, up[i]);
        if (writes && pl.reason == FOURMC_BSW_OK && up[i].image_cap < c.worst[i]) pl.reason = FOURMC_BSW_CAP;
        c.slices[i] = at;
        if (pl.reason != FOURMC_BSW_OK) continue;
        at.chunk0 += pl.chunks; at.stage0 += pl.stage;
        if (up[i].n_writes) at.group0 += pl.groups;
        if (at.chunk0 > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "%s: more than 0x7FFFFFFF %s", who, noun); return FOURMC_EUNSUP; }
    }
    c.slices[n] = at;
    return FOURMC_OK;
}

// The round size and the lease of g_img_stage; own(piece): the bytes of the caller's own arrays, which begin at c.d_own
template <class Own>
int bsw_round_open(BswCall& c, Own own)
{
    const uint32_t round = bsw_round();
    c.nc = c.at.chunk0;
    c.piece = uint32_t(c.nc < round ? c.nc : round);
    const uint64_t slot_m = align256(bs_block_bound(c.zstd, c.M));
    const uint64_t stage = c.at.stage0 < uint64_t(c.piece) * slot_m ? c.at.stage0 : uint64_t(c.piece) * slot_m;
    const size_t o_grp = align256((size_t(c.n) + 1) * sizeof(fourmc_bsw_slice)), o_blk = o_grp + align256(size_t(c.at.group0) * sizeof(fourmc_bsw_group));
    const size_t o_side = o_blk + align256(size_t(c.piece) * sizeof(fourmc_block)), o_own = o_side + align256(size_t(c.piece) * sizeof(fourmc_bsw_side));
    const size_t o_stage = o_own + own(c.piece);
    void* w = nullptr;
    if (int r = c.ws2.get(c.s, o_stage + size_t(stage) + kImagesStageSlack, &w)) return r;
    char* base = static_cast<char*>(w);
    c.d_slices = reinterpret_cast<fourmc_bsw_slice*>(base);
    c.d_grp = reinterpret_cast<fourmc_bsw_group*>(base + o_grp);
    c.d_blk = reinterpret_cast<fourmc_block*>(base + o_blk);
    c.d_side = reinterpret_cast<fourmc_bsw_side*>(base + o_side);
    c.d_own = base + o_own;
    c.d_stage = base + o_stage;
    return FOURMC_OK;
}

// Before the first round: the plans (with the _CAP verdicts) and the slices go up, the caller's two running arrays are cleared, and
// the group tables are written
int bsw_round_start(BswCall& c, void* d_zero0, size_t bytes0, void* d_zero1, size_t bytes1)
{
    HIP_TRY(hipMemcpyAsync(c.d_plans, c.plans.data(), size_t(c.n) * sizeof(fourmc_bsw_plan), hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipMemcpyAsync(c.d_slices, c.slices.data(), (size_t(c.n) + 1) * sizeof(fourmc_bsw_slice), hipMemcpyHostToDevice, c.s));
    HIP_TRY(hipMemsetAsync(d_zero0, 0, bytes0, c.s));
    HIP_TRY(hipMemsetAsync(d_zero1, 0, bytes1, c.s));
    if (c.at.group0) HIP_TRY(fourmc_launch_bsw_chase(c.d_writes, c.d_items, c.d_tile0, c.d_prefix, c.n, c.M, c.zstd, c.d_plans, c.d_slices, c.d_grp, c.s));
    return FOURMC_OK;
}

// The round that begins at chunk c0: its *m descriptors and side entries, and the raw codec launch into the staging
int bsw_round_encode(BswCall& c, uint64_t c0, uint32_t* m)
{
    *m = uint32_t(c.nc - c0 < c.piece ? c.nc - c0 : c.piece);
    HIP_TRY(fourmc_launch_bsw_desc(c.d_items, c.d_plans, c.d_slices, c.d_grp, c.n, c.M, c.zstd, c.codec == FOURMC_CODEC_LZ4_MC, c0, *m, c.d_blk, c.d_side, c.s));
    return encode_raw_blocks(c.codec, c.level, c.d_src, c.d_stage, c.d_blk, *m, c.s);
}
} // namespace

extern "C" {

// The host path above with M = the codec's chunk.  Its own arrays: one carry and one length per stream, the summary, and the
// offsets of one round.  Worst case: the plan's own.
int fourmc_gpu_bstreams_compress(const void* d_src, uint64_t src_total, const uint32_t* d_writes, uint64_t writes_total,
                                 void* d_images, uint64_t images_bytes, int codec, int level,
                                 fourmc_bstream_enc_item* items, uint32_t n, void* stream)
{
    const int zstd = bs_family(codec);
    if (zstd < 0) return bs_bad_codec("bstreams_compress", codec);
    if (n == 0) return FOURMC_OK;
    if (!items) { snprintf(g_err, sizeof g_err, "bstreams_compress: null items"); return FOURMC_EINVAL; }
    std::vector<uint64_t> tile0(size_t(n) + 1);
    if (int r = bsw_args("bstreams_compress", d_src, src_total, d_writes, writes_total, d_images, images_bytes, items, n, tile0)) return r;
    if (zstd && !fourmc_zstd_enc_level_ok(level)) { snprintf(g_err, sizeof g_err, "ZSTD level %d not on the device (levels 1..12 are)", level); return FOURMC_EUNSUP; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    BswCall c{d_src, d_writes, n, fourmc_gpu_bstream_max_input(codec), zstd, codec, level, s};
    if (int r = bsw_plan(c, "bstreams_compress", "chunks", items, tile0, d_images != nullptr,
                         [](const fourmc_bsw_plan& pl, const fourmc_bstream_enc_item&) { return pl.worst; })) return r;
    auto report = [&](const std::vector<uint64_t>* bytes) {
        for (uint32_t i = 0; i < n; i++) {
            const fourmc_bsw_plan& pl = c.plans[i];
            const bool planned = pl.reason == FOURMC_BSW_OK || pl.reason == FOURMC_BSW_CAP;
            items[i].reason = pl.reason;
            items[i].groups = planned ? uint32_t(pl.groups) : 0; items[i].chunks = planned ? uint32_t(pl.chunks) : 0;
            items[i].image_bytes = !planned ? 0 : bytes && pl.reason == FOURMC_BSW_OK ? (*bytes)[i] : pl.worst;
        }
    };
    if (!d_images) { report(nullptr); return FOURMC_OK; }
    const size_t o_bytes = align256(size_t(n) * 8), o_sum = o_bytes + align256(size_t(n) * 8), o_off = o_sum + align256(sizeof(fourmc_bstream_enc_summary));
    if (int r = bsw_round_open(c, [&](uint32_t piece) { return o_off + align256(size_t(piece) * 8); })) return r;
    auto* d_carry = reinterpret_cast<uint64_t*>(c.d_own);
    auto* d_bytes = reinterpret_cast<uint64_t*>(c.d_own + o_bytes);
    auto* d_sum = reinterpret_cast<fourmc_bstream_enc_summary*>(c.d_own + o_sum);
    auto* d_off = reinterpret_cast<uint64_t*>(c.d_own + o_off);
    if (int r = bsw_round_start(c, d_carry, size_t(n) * 8, d_sum, sizeof(fourmc_bstream_enc_summary))) return r;
    for (uint64_t c0 = 0; c0 < c.nc; c0 += c.piece) {
        uint32_t m;
        if (int r = bsw_round_encode(c, c0, &m)) return r;
        HIP_TRY(fourmc_launch_bsw_pack(d_images, c.d_items, c.d_blk, c.d_side, d_off, m, zstd, c.d_stage, d_carry, d_sum, s));
    }
    HIP_TRY(fourmc_launch_bsw_result(c.d_items, c.d_plans, d_carry, n, d_images, d_bytes, s));
    std::vector<uint64_t> bytes(n);
    fourmc_bstream_enc_summary h;
    HIP_TRY(hipMemcpyAsync(bytes.data(), d_bytes, size_t(n) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h, d_sum, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h.bad) { snprintf(g_err, sizeof g_err, "bstreams_compress: %llu chunks with a codec result outside [1, bound]", (unsigned long long)h.bad); return FOURMC_EINVAL; }
    report(&bytes);
    return FOURMC_OK;
}

// ---- .4mc / .4mz images from write() sizes --------------------------------------------------------------------------------------
// FourMcOutputStream's blocks are the chunks of the plan above with M = 4 MiB (include/fourmc_gpu.h has the rule and its lines)
uint64_t fourmc_gpu_image_writes_bound(uint64_t src_bytes)
{
    if (src_bytes > (~0ull >> 1)) return ~0ull;
    return 12 + 16 * bsw_max_chunks(src_bytes, FOURMC_BLOCKSIZE) + src_bytes + 32;
}

// The same host path with M = 4 MiB; the planner's items are the caller's in the planner's own item type.  Its own arrays: one
// running pair and one result per stream, the bad count, the offset of every block of the call (the footers' index) and the seal
// descriptors of one round.  Worst case: header, 12 + len per block, end mark, footer.
int fourmc_gpu_images_compress_writes(const void* d_src, uint64_t src_total, const uint32_t* d_writes, uint64_t writes_total,
                                      void* d_images, uint64_t images_bytes, uint32_t magic, int level,
                                      fourmc_image_wr_item* items, uint32_t n, void* stream)
{
    if (magic != FOURMC_MAGIC_4MC && magic != FOURMC_MAGIC_4MZ) { snprintf(g_err, sizeof g_err, "magic 0x%08x is neither 4mc nor 4mz", magic); return FOURMC_EINVAL; }
    if (n == 0) return FOURMC_OK;
    if (!items) { snprintf(g_err, sizeof g_err, "images_compress_writes: null items"); return FOURMC_EINVAL; }
    std::vector<uint64_t> tile0(size_t(n) + 1);
    if (int r = bsw_args("images_compress_writes", d_src, src_total, d_writes, writes_total, d_images, images_bytes, items, n, tile0)) return r;
    std::vector<fourmc_bstream_enc_item> bi(n);
    for (uint32_t i = 0; i < n; i++) {
        const fourmc_image_wr_item& it = items[i];
        fourmc_bstream_enc_item& b = bi[i];
        b = {};
        b.src_off = it.src_off; b.src_bytes = it.src_bytes; b.image_off = it.image_off; b.image_cap = it.image_cap;
        b.writes_off = it.writes_off; b.n_writes = it.n_writes; b.write_bytes = it.write_bytes;
    }
    int codec_level = 0;
    const int codec = fourmc_level_codec(magic, level, &codec_level);
    const int zstd = codec == FOURMC_CODEC_ZSTD;
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    BswCall c{d_src, d_writes, n, FOURMC_BLOCKSIZE, zstd, codec, codec_level, s};
    if (int r = bsw_plan(c, "images_compress_writes", "blocks", bi.data(), tile0, d_images != nullptr,
                         [](const fourmc_bsw_plan& pl, const fourmc_bstream_enc_item& it) { return 44 + 16 * pl.chunks + it.src_bytes; })) return r;
    auto report = [&](const std::vector<fourmc_imgw_result>* res) {
        for (uint32_t i = 0; i < n; i++) {
            const fourmc_bsw_plan& pl = c.plans[i];
            const bool planned = pl.reason == FOURMC_BSW_OK || pl.reason == FOURMC_BSW_CAP, written = res && pl.reason == FOURMC_BSW_OK;
            items[i].reason = pl.reason;
            items[i].blocks = planned ? pl.chunks : 0;
            items[i].stored_blocks = written ? (*res)[i].stored : 0;
            items[i].image_bytes = !planned ? 0 : written ? (*res)[i].image_bytes : c.worst[i];
        }
    };
    if (!d_images) { report(nullptr); return FOURMC_OK; }
    const size_t o_res = align256(size_t(n) * sizeof(fourmc_imgw_run)), o_bad = o_res + align256(size_t(n) * sizeof(fourmc_imgw_result));
    const size_t o_idx = o_bad + 256, o_seal = o_idx + align256(size_t(c.at.chunk0) * 8);
    if (int r = bsw_round_open(c, [&](uint32_t piece) { return o_seal + align256(size_t(piece) * sizeof(fourmc_block)); })) return r;
    auto* d_run = reinterpret_cast<fourmc_imgw_run*>(c.d_own);
    auto* d_res = reinterpret_cast<fourmc_imgw_result*>(c.d_own + o_res);
    auto* d_bad = reinterpret_cast<uint64_t*>(c.d_own + o_bad);
    auto* d_idx = reinterpret_cast<uint64_t*>(c.d_own + o_idx);
    auto* d_seal = reinterpret_cast<fourmc_block*>(c.d_own + o_seal);
    if (int r = bsw_round_start(c, d_run, size_t(n) * sizeof(fourmc_imgw_run), d_bad, 8)) return r;
    // the XXH32 and the pack read a stored block's bytes from d_src and a compressed one's from the staging through one base address:
    // the lower of the two, as the streaming writer's batches do
    const uintptr_t p_src = reinterpret_cast<uintptr_t>(d_src), p_stage = reinterpret_cast<uintptr_t>(c.d_stage);
    const uintptr_t lo = c.nc && p_src < p_stage ? p_src : p_stage;
    for (uint64_t c0 = 0; c0 < c.nc; c0 += c.piece) {
        uint32_t m;
        if (int r = bsw_round_encode(c, c0, &m)) return r;
        HIP_TRY(fourmc_launch_imgw_seal(c.d_blk, c.d_side, m, zstd, c.d_items, p_src - lo, p_stage - lo, d_seal, d_idx + c0, d_run, d_bad, s));
        HIP_TRY(fourmc_launch_xxh32(reinterpret_cast<const void*>(lo), d_seal, m, 0, FOURMC_HASH_DST_RESULT, s));
        HIP_TRY(fourmc_launch_pack_image(reinterpret_cast<const void*>(lo), d_images, d_seal, d_idx + c0, m, s));
    }
    HIP_TRY(fourmc_launch_imgw_tail(d_images, c.d_items, c.d_plans, c.d_slices, d_idx, d_run, n, magic, d_res, s));
    std::vector<fourmc_imgw_result> res(n);
    uint64_t bad = 0;
    HIP_TRY(hipMemcpyAsync(res.data(), d_res, size_t(n) * sizeof(fourmc_imgw_result), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (bad) { snprintf(g_err, sizeof g_err, "images_compress_writes: %llu blocks with a codec result outside [1, bound]", (unsigned long long)bad); return FOURMC_EINVAL; }
    report(&res);
    return FOURMC_OK;
}

// The decode of n streams: the single call is its n = 1 case.  Workspace (g_img_ws): the items, one summary, one first-descriptor
// number and one status per stream, then - sized after the first read-back - the descriptors and the side table of every stream.
// When that grows the buffer its contents are gone: the items and the summaries (the host has both) go up again.
static int bstreams_run(const void* d_images, void* d_dst, int zstd, fourmc_bstream_item* items, uint32_t n, hipStream_t s)
{
    if (int r = ensure_device()) return r;
    const uint32_t M = fourmc_gpu_bstream_max_input(zstd ? FOURMC_CODEC_ZSTD : FOURMC_CODEC_LZ4_FAST);
    const size_t o_ws = align256(size_t(n) * sizeof(fourmc_bstream_item)), o_first = o_ws + align256(size_t(n) * sizeof(fourmc_bstream_walk));
    const size_t o_st = o_first + align256(size_t(n) * 8), o_blk = o_st + align256(size_t(n) * sizeof(fourmc_bstream_status));
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, o_blk, &w)) return r;
    char* base = static_cast<char*>(w);
    HIP_TRY(hipMemcpyAsync(base, items, size_t(n) * sizeof(fourmc_bstream_item), hipMemcpyHostToDevice, s));
    HIP_TRY(fourmc_launch_bstream_walk(d_images, reinterpret_cast<fourmc_bstream_item*>(base), n, M,
                                       reinterpret_cast<fourmc_bstream_walk*>(base + o_ws), nullptr, nullptr, nullptr, s));
    std::vector<fourmc_bstream_walk> sums(n);
    HIP_TRY(hipMemcpyAsync(sums.data(), base + o_ws, size_t(n) * sizeof(fourmc_bstream_walk), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<fourmc_bstream_status> back(n);
    if (!d_dst) {                                    // the size query: the framing verdicts
        for (uint32_t i = 0; i < n; i++) {
            if (sums[i].chunks > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "bstreams_decompress: %llu chunks", (unsigned long long)sums[i].chunks); return FOURMC_EUNSUP; }
            fourmc_bstream_status st = {};
            st.total_bytes = sums[i].total; st.fail_offset = sums[i].fail_offset; st.groups = uint32_t(sums[i].groups);
            st.chunks = uint32_t(sums[i].chunks); st.reason = sums[i].reason;
            back[i] = st;
        }
        for (uint32_t i = 0; i < n; i++) items[i].status = back[i];
        return FOURMC_OK;
    }
    std::vector<uint64_t> first(n);
    uint64_t nb64 = 0;
    for (uint32_t i = 0; i < n; i++) {               // each stream's slice of the one descriptor table
        first[i] = nb64;
        if (sums[i].total <= items[i].dst_cap) nb64 += sums[i].chunks;
        if (nb64 > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "bstreams_decompress: more than 0x7FFFFFFF chunks"); return FOURMC_EUNSUP; }
    }
    const uint32_t nb = uint32_t(nb64);
    const size_t o_side = o_blk + align256(size_t(nb) * sizeof(fourmc_block));
    const size_t had = ws.cap();
    if (int r = ws.get(s, o_side + size_t(nb) * sizeof(fourmc_bstream_side), &w)) return r;
    base = static_cast<char*>(w);
    if (ws.cap() != had) {
        HIP_TRY(hipMemcpyAsync(base, items, size_t(n) * sizeof(fourmc_bstream_item), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(base + o_ws, sums.data(), size_t(n) * sizeof(fourmc_bstream_walk), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(base + o_first, first.data(), size_t(n) * 8, hipMemcpyHostToDevice, s));
    auto* d_items = reinterpret_cast<fourmc_bstream_item*>(base);
    auto* d_ws = reinterpret_cast<fourmc_bstream_walk*>(base + o_ws);
    auto* d_first = reinterpret_cast<uint64_t*>(base + o_first);
    auto* d_blk = reinterpret_cast<fourmc_block*>(base + o_blk);
    auto* d_side = reinterpret_cast<fourmc_bstream_side*>(base + o_side);
    if (nb) {
        HIP_TRY(fourmc_launch_bstream_walk(d_images, d_items, n, M, d_ws, d_first, d_blk, d_side, s));
        if (int r = zstd ? fourmc_gpu_zstd_decompress(d_images, d_dst, d_blk, nb, s) : fourmc_gpu_lz4_decompress(d_images, d_dst, d_blk, nb, s)) return r;
    }
    HIP_TRY(fourmc_launch_bstream_fold(d_items, n, d_ws, d_first, d_blk, d_side, reinterpret_cast<fourmc_bstream_status*>(base + o_st), s));
    HIP_TRY(hipMemcpyAsync(back.data(), base + o_st, size_t(n) * sizeof(fourmc_bstream_status), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; i++) items[i].status = back[i];
    return FOURMC_OK;
}

int fourmc_gpu_bstream_decompress(const void* d_image, uint64_t image_bytes, void* d_dst, uint64_t dst_cap, int codec,
                                  fourmc_bstream_status* status, void* stream)
{
    const int zstd = bs_family(codec);
    if (zstd < 0) return bs_bad_codec("bstream_decompress", codec);
    if (!status || (image_bytes && !d_image)) { snprintf(g_err, sizeof g_err, "bstream_decompress: null pointer"); return FOURMC_EINVAL; }
    fourmc_bstream_item it = {};
    it.image_bytes = image_bytes; it.dst_cap = d_dst ? dst_cap : 0;
    if (int r = bstreams_run(d_image, d_dst, zstd, &it, 1, static_cast<hipStream_t>(stream))) return r;
    *status = it.status;
    return FOURMC_OK;
}

int fourmc_gpu_bstreams_decompress(const void* d_images, uint64_t images_bytes, void* d_dst, uint64_t dst_bytes, int codec,
                                   fourmc_bstream_item* items, uint32_t n, void* stream)
{
    const int zstd = bs_family(codec);
    if (zstd < 0) return bs_bad_codec("bstreams_decompress", codec);
    if (n == 0) return FOURMC_OK;
    if (int r = decode_items_args("bstreams_decompress", "stream", "streams", d_images, images_bytes, d_dst, dst_bytes, items, n)) return r;
    return bstreams_run(d_images, d_dst, zstd, items, n, static_cast<hipStream_t>(stream));
}

const char* fourmc_gpu_bstream_reason_text(int reason)
{
    switch (reason) {
        case FOURMC_BS_OK:              return "";
        case FOURMC_BS_BAD_RAWLEN:      return "Block stream : group length beyond 2 GiB";
        case FOURMC_BS_CLEN_UNREADABLE: return "Block stream : cannot read next chunk length";
        case FOURMC_BS_BAD_CLEN:        return "Block stream : chunk length zero or beyond 4MB limit";
        case FOURMC_BS_DATA_UNREADABLE: return "Block stream : cannot read chunk data";
        case FOURMC_BS_CORRUPT:         return "Block stream : decoding failed, corrupted chunk";
        case FOURMC_BS_SHAPE:           return "Block stream : chunk shorter than the writer's shape allows";
        case FOURMC_BS_DST_SMALL:       return "Destination buffer too small";
        default:                        return "unknown";
    }
}

// ------------------------------------------------------------------------ .zst streams (zst.hip)
void fourmc_gpu_set_zst_round_blocks(uint32_t blocks) { g_zst_round = blocks; }
uint32_t fourmc_gpu_get_zst_round_blocks(void) { return zst_round(); }

int fourmc_gpu_zst_decompress(const void* d_image, uint64_t image_bytes, void* d_dst, uint64_t dst_cap, fourmc_zst_status* status, void* stream)
{
    if (!status || (image_bytes && !d_image)) { snprintf(g_err, sizeof g_err, "zst_decompress: null pointer"); return FOURMC_EINVAL; }
    fourmc_zst_item it = {};
    it.image_bytes = image_bytes; it.dst_cap = d_dst ? dst_cap : 0;
    if (int r = zsts_run(d_image, d_dst, &it, 1, static_cast<hipStream_t>(stream))) return r;
    *status = it.status;
    return FOURMC_OK;
}

int fourmc_gpu_zsts_decompress(const void* d_images, uint64_t images_bytes, void* d_dst, uint64_t dst_bytes, fourmc_zst_item* items,
                               uint32_t n, void* stream)
{
    if (n == 0) return FOURMC_OK;
    if (int r = decode_items_args("zsts_decompress", "stream", "streams", d_images, images_bytes, d_dst, dst_bytes, items, n)) return r;
    return zsts_run(d_images, d_dst, items, n, static_cast<hipStream_t>(stream));
}

const char* fourmc_gpu_zst_reason_text(int reason)
{
    switch (reason) {
        case FOURMC_ZST_OK:        return "";
        case FOURMC_ZST_FRAME:     return "zstd : frame decoding failed";
        case FOURMC_ZST_DST_SMALL: return "Destination buffer too small";
        default:                   return "unknown";
    }
}

void fourmc_gpu_zst_stats(unsigned long long* fast_frames, unsigned long long* serial_frames, unsigned long long* fast_blocks)
{
    unsigned long long c[3] = {0, 0, 0};
    if (ensure_device() == FOURMC_OK) (void)fourmc_zst_counts(c);
    if (fast_frames) *fast_frames = c[0];
    if (serial_frames) *serial_frames = c[1];
    if (fast_blocks) *fast_blocks = c[2];
}

// ------------------------------------------------------------------------ .zst streams written (zstd_encode.hip: zst_stream_*_kernel)
uint64_t fourmc_gpu_zst_bound(uint64_t src_bytes) { return 6 + src_bytes + 3 * (src_bytes / 131072 + 1); }
int fourmc_zst_codec_level(int configured) { return configured <= 0 || configured >= 23 ? 3 : configured; }

int fourmc_gpu_zsts_compress(const void* d_src, uint64_t src_total, void* d_images, uint64_t images_bytes, fourmc_zstw_item* items, uint32_t n, void* stream)
{
    if (n == 0) return FOURMC_OK;
    if (!items) { snprintf(g_err, sizeof g_err, "zsts_compress: null items"); return FOURMC_EINVAL; }
    {
        std::vector<std::pair<uint64_t, uint64_t>> d;
        d.reserve(n);
        for (uint32_t i = 0; i < n; i++) {
            const fourmc_zstw_item& it = items[i];
            const bool read = it.src_bytes <= kZstwMaxSource;            // (a source beyond the limit is refused unread: only its descriptor exists)
            if (read && it.src_bytes && !d_src) { snprintf(g_err, sizeof g_err, "zsts_compress: null source"); return FOURMC_EINVAL; }
            if (it.image_cap && !d_images) { snprintf(g_err, sizeof g_err, "zsts_compress: null images"); return FOURMC_EINVAL; }
            if (read && span_outside(it.src_off, it.src_bytes, src_total)) return source_beyond("zsts_compress", "stream", i, src_total);
            if (span_outside(it.image_off, it.image_cap, images_bytes)) return region_beyond("zsts_compress", "stream", i, images_bytes);
            if (it.image_cap) d.emplace_back(it.image_off, it.image_off + it.image_cap);
        }
        if (int r = regions_overlap("zsts_compress", "image regions", d)) return r;
    }
    return zstw_run(d_src, d_images, items, n, static_cast<hipStream_t>(stream));
}

int fourmc_gpu_zst_compress(const void* d_src, uint64_t src_bytes, void* d_image, uint64_t image_cap, int level, fourmc_zstw_status* status, void* stream)
{
    if (!status) { snprintf(g_err, sizeof g_err, "zst_compress: null status"); return FOURMC_EINVAL; }
    fourmc_zstw_item it = {};
    it.src_bytes = src_bytes; it.image_cap = image_cap; it.level = level;
    if (int r = fourmc_gpu_zsts_compress(d_src, src_bytes, d_image, image_cap, &it, 1, stream)) return r;
    *status = it.status;
    return FOURMC_OK;
}

const char* fourmc_gpu_zstw_reason_text(int reason)
{
    switch (reason) {
        case FOURMC_ZSTW_OK:        return "";
        case FOURMC_ZSTW_DST_SMALL: return "Destination buffer too small";
        case FOURMC_ZSTW_LEVEL:     return "zstd : level not written on the device (1 to 4 are)";
        case FOURMC_ZSTW_TOO_LONG:  return "zstd : source beyond 3 GiB";
        default:                    return "unknown";
    }
}

} // extern "C"
