// 4mc_amd/csrc/engine_text.hip — text lines written as the part files of a TextOutputFormat job (lines_pack.hip): the pack of lines in
// the readers' table layouts into data and write sizes, and the two writers, which are that pack into staging of their own followed by
// fourmc_gpu_images_compress_writes / fourmc_gpu_bstreams_compress as they are.
#include "engine_int.h"

namespace {
// what the three calls' items say about lines and places: `out_off, out_cap` is the packed region or the image region
struct LpIn { uint64_t line_off, n_lines, out_off, out_cap, writes_off; };

// The checks of the lines' description, then per item its lines and - unless this is the query - its region and its write slice;
// then the regions and the slices against each other.  `many`: what the output buffer holds; check_writes: lines_pack, whose write
// table is the caller's.
int lp_args(const char* who, const fourmc_lines_src* src, const void* items, const std::vector<LpIn>& in, bool query, uint64_t out_total,
            const char* many, bool check_writes, const uint32_t* d_writes, uint64_t writes_total)
{
    if (!src) { snprintf(g_err, sizeof g_err, "%s: null lines description", who); return FOURMC_EINVAL; }
    if (!items) { snprintf(g_err, sizeof g_err, "%s: null items", who); return FOURMC_EINVAL; }
    if (src->text_bytes && !src->d_text) { snprintf(g_err, sizeof g_err, "%s: null text", who); return FOURMC_EINVAL; }
    if (src->table_lines && !src->d_text_len) { snprintf(g_err, sizeof g_err, "%s: null text lengths", who); return FOURMC_EINVAL; }
    if (src->table_lines && !src->d_starts) {
        if (!src->row_bytes) { snprintf(g_err, sizeof g_err, "%s: neither line starts nor a row stride", who); return FOURMC_EINVAL; }
        if (src->table_lines > src->text_bytes / src->row_bytes) {
            snprintf(g_err, sizeof g_err, "%s: %llu rows of %u bytes lie beyond the %llu bytes of text", who, (unsigned long long)src->table_lines,
                     src->row_bytes, (unsigned long long)src->text_bytes);
            return FOURMC_EINVAL;
        }
    }
    const uint64_t lines_total = src->d_pick ? src->pick_total : src->table_lines;
    std::vector<std::pair<uint64_t, uint64_t>> d, w;
    for (uint32_t i = 0; i < in.size(); i++) {
        const LpIn& it = in[i];
        if (span_outside(it.line_off, it.n_lines, lines_total)) {
            snprintf(g_err, sizeof g_err, "%s: the lines of item %u lie beyond the %llu entries of the %s", who, i, (unsigned long long)lines_total,
                     src->d_pick ? "pick" : "tables");
            return FOURMC_EINVAL;
        }
        if (query) continue;                              // the size query looks at no region
        if (span_outside(it.out_off, it.out_cap, out_total)) {
            snprintf(g_err, sizeof g_err, "%s: the region of item %u lies beyond the %llu bytes of %s", who, i, (unsigned long long)out_total, many);
            return FOURMC_EINVAL;
        }
        if (it.out_cap) d.emplace_back(it.out_off, it.out_off + it.out_cap);
        if (!check_writes) continue;
        if (it.n_lines && !d_writes) { snprintf(g_err, sizeof g_err, "%s: null write table (item %u)", who, i); return FOURMC_EINVAL; }
        if (it.n_lines > (~0ull >> 1) || span_outside(it.writes_off, 2 * it.n_lines, writes_total)) return writes_beyond(who, i, writes_total);
        if (it.n_lines) w.emplace_back(it.writes_off, it.writes_off + 2 * it.n_lines);
    }
    if (int r = regions_overlap(who, check_writes ? "packed regions" : "image regions", d)) return r;
    return regions_overlap(who, "write slices", w);
}

// One call's tables (g_txt_ws): the items, what the measure leaves per item, the tile prefixes and the per-line offsets
struct LpRun {
    WsLease ws{&g_txt_ws};
    uint32_t n = 0; uint64_t ntiles = 0, lines = 0;
    fourmc_lp_item* d_items = nullptr; fourmc_lp_sum* d_sums = nullptr; uint64_t* d_prefix = nullptr; uint64_t* d_off = nullptr;
    std::vector<fourmc_lp_item> items; std::vector<fourmc_lp_sum> sums;
};

// The measure and its read-back (the call's first synchronization): r.sums[0 .. n], entry n the totals.  mode, base16: as
// fourmc_launch_lp_measure takes them.  The writers' slices of the write table follow one another (writes_off of `in` is not read).
int lp_measure(LpRun& r, const char* who, const fourmc_lines_src* src, const std::vector<LpIn>& in, int mode, uint32_t base16, hipStream_t s)
{
    const uint32_t n = r.n = uint32_t(in.size());
    r.items.assign(size_t(n) + 1, fourmc_lp_item{});
    uint64_t tiles = 0, offs = 0, lines = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (in[i].n_lines >> 38) { snprintf(g_err, sizeof g_err, "%s: item %u has %llu lines", who, i, (unsigned long long)in[i].n_lines); return FOURMC_EUNSUP; }
        fourmc_lp_item& d = r.items[i];
        d.line_off = in[i].line_off; d.n_lines = in[i].n_lines; d.packed_off = in[i].out_off; d.packed_cap = in[i].out_cap;
        d.writes_off = mode == 2 ? 2 * lines : in[i].writes_off;
        d.tile0 = tiles; d.off0 = offs;
        tiles += in[i].n_lines / 64 + (in[i].n_lines % 64 ? 1 : 0);
        offs += in[i].n_lines + 1; lines += in[i].n_lines;
    }
    r.items[n].tile0 = tiles; r.items[n].off0 = offs;
    r.ntiles = tiles; r.lines = lines;
    const size_t o_sums = align256((size_t(n) + 1) * sizeof(fourmc_lp_item)), o_prefix = o_sums + align256((size_t(n) + 1) * sizeof(fourmc_lp_sum));
    const size_t o_off = o_prefix + align256(size_t(tiles + n) * 8);
    void* w = nullptr;
    if (int rc = r.ws.get(s, o_off + size_t(offs) * 8, &w)) return rc;
    char* base = static_cast<char*>(w);
    r.d_items = reinterpret_cast<fourmc_lp_item*>(base);
    r.d_sums = reinterpret_cast<fourmc_lp_sum*>(base + o_sums);
    r.d_prefix = reinterpret_cast<uint64_t*>(base + o_prefix);
    r.d_off = reinterpret_cast<uint64_t*>(base + o_off);
    HIP_TRY(hipMemcpyAsync(r.d_items, r.items.data(), (size_t(n) + 1) * sizeof(fourmc_lp_item), hipMemcpyHostToDevice, s));
    HIP_TRY(fourmc_launch_lp_measure(src, r.d_items, n, tiles, mode, base16, r.d_prefix, r.d_off, r.d_sums, s));
    r.sums.assign(size_t(n) + 1, fourmc_lp_sum{});
    HIP_TRY(hipMemcpyAsync(r.sums.data(), r.d_sums, (size_t(n) + 1) * sizeof(fourmc_lp_sum), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (r.sums[n].chunk0 > 0x7FFFFFFFull) {
        snprintf(g_err, sizeof g_err, "%s: %llu bytes of text are more than 0x7FFFFFFF chunks", who, (unsigned long long)r.sums[n].bytes);
        return FOURMC_EUNSUP;
    }
    return FOURMC_OK;
}

// What the two writers ask of the call below them, and what it answers
struct LwRow { uint64_t src_off, src_bytes, image_off, image_cap, writes_off, n_writes; int32_t reason; uint64_t image_bytes, blocks, stored; };

// The writers: the checks (zstd: the one family that refuses levels), the measure, the pack into g_txt_stage, then
// below(d_src, src_total, d_writes, writes_total, rows) - one of the two calls from write() sizes, which lease their own workspaces -
// and the items' results
template <class Below>
int lines_write(const char* who, const fourmc_lines_src* src, void* d_images, uint64_t images_bytes, fourmc_lines_wr_item* items, uint32_t n,
                bool zstd, int level, hipStream_t s, Below below)
{
    std::vector<LpIn> in(items ? n : 0);
    for (uint32_t i = 0; i < in.size(); i++) in[i] = LpIn{items[i].line_off, items[i].n_lines, items[i].image_off, items[i].image_cap, 0};
    if (int rc = lp_args(who, src, items, in, d_images == nullptr, images_bytes, "images", false, nullptr, 0)) return rc;
    if (zstd && !fourmc_zstd_enc_level_ok(level)) { snprintf(g_err, sizeof g_err, "%s: ZSTD level %d not on the device (levels 1..12 are)", who, level); return FOURMC_EUNSUP; }
    if (int rc = ensure_device()) return rc;
    LpRun r;
    if (int rc = lp_measure(r, who, src, in, 2, 0, s)) return rc;
    const uint64_t total = r.sums[n].bytes;
    const size_t o_writes = align256(size_t(total)) + 256;
    WsLease stage(&g_txt_stage); void* w = nullptr;
    if (int rc = stage.get(s, o_writes + size_t(r.lines) * 8 + 256, &w)) return rc;      // (hipMalloc's alignment: the text starts on a 16-byte boundary, as the measure assumed)
    char* d_text = static_cast<char*>(w);
    uint32_t* d_writes = reinterpret_cast<uint32_t*>(d_text + o_writes);
    HIP_TRY(fourmc_launch_lp_copy(src, r.d_items, r.d_sums, n, r.ntiles, r.sums[n].chunk0, r.d_prefix, r.d_off, d_images ? d_text : nullptr, d_writes, s));
    std::vector<LwRow> rows(n, LwRow{});
    for (uint32_t i = 0; i < n; i++) {
        if (r.sums[i].reason != FOURMC_BSW_OK) continue;                                 // an item that owns nothing
        LwRow& row = rows[i];
        row.src_off = r.sums[i].packed_off; row.src_bytes = r.sums[i].bytes; row.image_off = items[i].image_off; row.image_cap = items[i].image_cap;
        row.writes_off = r.items[i].writes_off; row.n_writes = 2 * items[i].n_lines;
    }
    if (int rc = below(d_text, total, d_writes, 2 * r.lines, rows)) return rc;
    for (uint32_t i = 0; i < n; i++) {
        const bool packed = r.sums[i].reason == FOURMC_BSW_OK;
        items[i].reason = packed ? rows[i].reason : r.sums[i].reason; items[i].pad = 0;
        items[i].text_bytes = r.sums[i].bytes;
        items[i].image_bytes = packed ? rows[i].image_bytes : 0; items[i].blocks = packed ? rows[i].blocks : 0;
        items[i].stored_blocks = packed ? rows[i].stored : 0;
    }
    return FOURMC_OK;
}
} // namespace

extern "C" {

int fourmc_gpu_lines_pack(const fourmc_lines_src* src, void* d_packed, uint64_t packed_total, uint32_t* d_writes, uint64_t writes_total,
                          fourmc_lines_pack_item* items, uint32_t n, void* stream)
{
    if (n == 0) return FOURMC_OK;
    std::vector<LpIn> in(items ? n : 0);
    for (uint32_t i = 0; i < in.size(); i++) in[i] = LpIn{items[i].line_off, items[i].n_lines, items[i].packed_off, items[i].packed_cap, items[i].writes_off};
    if (int rc = lp_args("lines_pack", src, items, in, d_packed == nullptr, packed_total, "packed text", true, d_writes, writes_total)) return rc;
    if (int rc = ensure_device()) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    LpRun r;
    if (int rc = lp_measure(r, "lines_pack", src, in, d_packed ? 1 : 0, uint32_t(reinterpret_cast<uintptr_t>(d_packed) & 15), s)) return rc;
    if (d_packed) HIP_TRY(fourmc_launch_lp_copy(src, r.d_items, r.d_sums, n, r.ntiles, r.sums[n].chunk0, r.d_prefix, r.d_off, d_packed, d_writes, s));
    for (uint32_t i = 0; i < n; i++) { items[i].reason = r.sums[i].reason; items[i].pad = 0; items[i].packed_bytes = r.sums[i].bytes; }
    return FOURMC_OK;
}

int fourmc_gpu_images_write_lines(const fourmc_lines_src* src, void* d_images, uint64_t images_bytes, uint32_t magic, int level,
                                  fourmc_lines_wr_item* items, uint32_t n, void* stream)
{
    if (magic != FOURMC_MAGIC_4MC && magic != FOURMC_MAGIC_4MZ) { snprintf(g_err, sizeof g_err, "images_write_lines: magic 0x%08x is neither 4mc nor 4mz", magic); return FOURMC_EINVAL; }
    if (n == 0) return FOURMC_OK;
    return lines_write("images_write_lines", src, d_images, images_bytes, items, n, false, level, static_cast<hipStream_t>(stream),
                       [&](const void* d_src, uint64_t src_total, const uint32_t* d_writes, uint64_t writes_total, std::vector<LwRow>& rows) {
        std::vector<fourmc_image_wr_item> wi(rows.size());
        for (size_t i = 0; i < rows.size(); i++) {
            wi[i] = {};
            wi[i].src_off = rows[i].src_off; wi[i].src_bytes = rows[i].src_bytes; wi[i].image_off = rows[i].image_off; wi[i].image_cap = rows[i].image_cap;
            wi[i].writes_off = rows[i].writes_off; wi[i].n_writes = rows[i].n_writes;
        }
        if (int rc = fourmc_gpu_images_compress_writes(d_src, src_total, d_writes, writes_total, d_images, images_bytes, magic, level, wi.data(), n, stream)) return rc;
        for (size_t i = 0; i < rows.size(); i++) { rows[i].reason = wi[i].reason; rows[i].image_bytes = wi[i].image_bytes; rows[i].blocks = wi[i].blocks; rows[i].stored = wi[i].stored_blocks; }
        return int(FOURMC_OK);
    });
}

int fourmc_gpu_bstreams_write_lines(const fourmc_lines_src* src, void* d_images, uint64_t images_bytes, int codec, int level,
                                    fourmc_lines_wr_item* items, uint32_t n, void* stream)
{
    if (!fourmc_gpu_bstream_max_input(codec)) { snprintf(g_err, sizeof g_err, "bstreams_write_lines: codec %d is none of FOURMC_CODEC_*", codec); return FOURMC_EINVAL; }
    if (n == 0) return FOURMC_OK;
    return lines_write("bstreams_write_lines", src, d_images, images_bytes, items, n, codec == FOURMC_CODEC_ZSTD, level, static_cast<hipStream_t>(stream),
                       [&](const void* d_src, uint64_t src_total, const uint32_t* d_writes, uint64_t writes_total, std::vector<LwRow>& rows) {
        std::vector<fourmc_bstream_enc_item> wi(rows.size());
        for (size_t i = 0; i < rows.size(); i++) {
            wi[i] = {};
            wi[i].src_off = rows[i].src_off; wi[i].src_bytes = rows[i].src_bytes; wi[i].image_off = rows[i].image_off; wi[i].image_cap = rows[i].image_cap;
            wi[i].writes_off = rows[i].writes_off; wi[i].n_writes = rows[i].n_writes;
        }
        if (int rc = fourmc_gpu_bstreams_compress(d_src, src_total, d_writes, writes_total, d_images, images_bytes, codec, level, wi.data(), n, stream)) return rc;
        for (size_t i = 0; i < rows.size(); i++) { rows[i].reason = wi[i].reason; rows[i].image_bytes = wi[i].image_bytes; rows[i].blocks = wi[i].chunks; rows[i].stored = 0; }
        return int(FOURMC_OK);
    });
}

} // extern "C"
