// 4mc_amd/csrc/engine_lineat.hip — lines by number (lineat.hip): the line index of a device image, and reads of lines by their
// numbers that decode only the blocks those lines touch.
#include "engine_int.h"

namespace {
// rounds run, container decode calls made and blocks staged by image_read_lines_at (fourmc_gpu_image_lines_at_stats)
struct LineAtCounters { std::atomic<unsigned long long> rounds{0}, decodes{0}, staged{0}; };
LineAtCounters g_la;

// FOURMC_LINES_AT_GROUP: the most blocks staged at a time (a slot each); read at every call, like FOURMC_SPLIT_GROUP
uint32_t lines_at_group()
{
    const char* e = getenv("FOURMC_LINES_AT_GROUP");
    if (!e || !*e) return 256;
    const long v = strtol(e, nullptr, 10);
    return v < 1 ? 1u : v > 4096 ? 4096u : uint32_t(v);
}

constexpr uint64_t kSlot = uint64_t(FOURMC_BLOCKSIZE) + 64;
constexpr size_t kSlotTiles = FOURMC_BLOCKSIZE / FOURMC_RECORDS_TILE;
} // namespace

extern "C" {

// Read-backs: the index summary, the result.  Workspace (g_img_ws): the summary, the result, the entries, a group's descriptors,
// the per-block counts; staging (g_img_stage): a slot per block of a group.
int fourmc_gpu_image_line_index(const void* d_image, uint64_t image_bytes, fourmc_image_line_entry* d_index, uint64_t index_cap,
                                fourmc_image_line_info* info, void* stream)
{
    if (!info) { snprintf(g_err, sizeof g_err, "image_line_index: null info"); return FOURMC_EINVAL; }
    if (!d_image) { snprintf(g_err, sizeof g_err, "image_line_index: null image"); return FOURMC_EINVAL; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    memset(info, 0, sizeof *info);
    WsLease ws(&g_img_ws);
    fourmc_image_index_dev idx;
    if (int r = image_index_count(ws, s, d_image, image_bytes, &idx)) return r;
    const int64_t code = idx.info.nblocks < 0 ? idx.info.nblocks : idx.info.framing;
    if (code != 0) { info->result = code; return FOURMC_OK; }
    if (idx.info.nblocks > 0x7FFFFFFF) { snprintf(g_err, sizeof g_err, "image_line_index: %lld blocks", (long long)idx.info.nblocks); return FOURMC_EUNSUP; }
    const uint32_t nb = uint32_t(idx.info.nblocks), group = std::min(lines_at_group(), std::max(nb, 1u));
    const size_t o_sum = kIdxBytes, o_ent = o_sum + 256;
    const size_t o_desc = o_ent + align256(size_t(nb) * sizeof(fourmc_image_entry));
    const size_t o_blk = o_desc + align256(size_t(group) * sizeof(fourmc_block));
    void* w = nullptr;
    if (int r = ws.get(s, o_blk + size_t(nb) * sizeof(fourmc_lineat_blk), &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_idx = reinterpret_cast<fourmc_image_index_dev*>(base);
    auto* d_sum = reinterpret_cast<fourmc_lineat_sum*>(base + o_sum);
    auto* d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
    auto* d_desc = reinterpret_cast<fourmc_block*>(base + o_desc);
    auto* d_blk = reinterpret_cast<fourmc_lineat_blk*>(base + o_blk);
    HIP_TRY(fourmc_launch_image_index(d_image, image_bytes, d_idx, d_ent, nb, s));
    WsLease ws2(&g_img_stage);
    char* d_stage = nullptr;
    if (nb) {
        void* w2 = nullptr;
        if (int r = ws2.get(s, size_t(group) * kSlot, &w2)) return r;
        d_stage = static_cast<char*>(w2);
    }
    for (uint32_t b0 = 0; b0 < nb; b0 += group) {
        const uint32_t m = std::min(group, nb - b0);
        HIP_TRY(fourmc_launch_lineat_desc(d_ent, nullptr, b0, m, kSlot, d_desc, s));
        if (int r = fourmc_gpu_4mc_decode_blocks(d_image, d_stage, d_desc, m, image_codec(idx), s)) return r;
        HIP_TRY(fourmc_launch_lineat_block_count(d_stage, kSlot, d_ent, b0, d_desc, m, d_blk, s));
    }
    HIP_TRY(fourmc_launch_lineat_index_finish(d_ent, d_blk, nb, idx.info.total_bytes, d_index, index_cap, d_sum, s));
    fourmc_lineat_sum sum;
    HIP_TRY(hipMemcpyAsync(&sum, d_sum, sizeof sum, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    info->result = sum.result; info->lines = sum.lines; info->ends = sum.ends; info->total_bytes = sum.total; info->nblocks = nb;
    return FOURMC_OK;
}

// Read-backs: the index summary, the count of needed blocks, the count of rows written.  Workspace (g_img_ws): the summary, the
// counts, the entries, the block marks, the list of needed blocks, the requests, a round's descriptors and tile counts; staging
// (g_img_stage): a slot per block of a round.
int fourmc_gpu_image_read_lines_at(const void* d_image, uint64_t image_bytes, const fourmc_image_line_entry* d_index, uint64_t index_entries,
                                   const uint64_t* d_lines, uint32_t n, uint32_t max_line_len, void* d_rows, uint32_t row_bytes, uint8_t pad,
                                   uint32_t* d_text_len, int32_t* d_status, fourmc_image_lines_at* out, void* stream)
{
    if (!out) { snprintf(g_err, sizeof g_err, "image_read_lines_at: null result"); return FOURMC_EINVAL; }
    if (!d_image) { snprintf(g_err, sizeof g_err, "image_read_lines_at: null image"); return FOURMC_EINVAL; }
    if (!d_index) { snprintf(g_err, sizeof g_err, "image_read_lines_at: null index"); return FOURMC_EINVAL; }
    if (n && (!d_lines || !d_rows || !d_text_len || !d_status)) {
        snprintf(g_err, sizeof g_err, "image_read_lines_at: null d_lines, d_rows, d_text_len or d_status with %u requests", n);
        return FOURMC_EINVAL;
    }
    if (row_bytes == 0) { snprintf(g_err, sizeof g_err, "image_read_lines_at: row_bytes 0"); return FOURMC_EINVAL; }
    if (max_line_len > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "image_read_lines_at: max_line_len %u above 0x7FFFFFFF", max_line_len); return FOURMC_EINVAL; }
    // n and row_bytes are 32-bit here, so their product cannot pass 64 bits; the check stands for the day one of them widens
    if (uint64_t(n) > ~uint64_t(0) / row_bytes) { snprintf(g_err, sizeof g_err, "image_read_lines_at: %u rows of %u bytes", n, row_bytes); return FOURMC_EINVAL; }
    if (n == 0) { memset(out, 0, sizeof *out); return FOURMC_OK; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsLease ws(&g_img_ws);
    fourmc_image_index_dev idx;
    if (int r = image_index_count(ws, s, d_image, image_bytes, &idx)) return r;
    const int64_t code = idx.info.nblocks < 0 ? idx.info.nblocks : idx.info.framing;
    if (code != 0) {
        HIP_TRY(fourmc_launch_lineat_fill(d_status, d_text_len, n, int32_t(code), s));
        memset(out, 0, sizeof *out);
        out->result = code;
        return FOURMC_OK;
    }
    if (idx.info.nblocks > 0x7FFFFFFF) { snprintf(g_err, sizeof g_err, "image_read_lines_at: %lld blocks", (long long)idx.info.nblocks); return FOURMC_EUNSUP; }
    const uint32_t nb = uint32_t(idx.info.nblocks);
    if (index_entries != uint64_t(nb) + 1) {
        snprintf(g_err, sizeof g_err, "image_read_lines_at: an index of %llu entries for an image of %u blocks (blocks + 1 wanted)",
                 (unsigned long long)index_entries, nb);
        return FOURMC_EINVAL;
    }
    const uint32_t group = std::min(lines_at_group(), std::max(nb, 1u));
    const size_t o_cnt = kIdxBytes, o_ent = o_cnt + 256;
    const size_t o_flag = o_ent + align256(size_t(nb) * sizeof(fourmc_image_entry));
    const size_t o_list = o_flag + align256(size_t(nb) * sizeof(uint32_t));
    const size_t o_req = o_list + align256(size_t(nb) * sizeof(uint32_t));
    const size_t o_desc = o_req + align256(size_t(n) * sizeof(fourmc_lineat_req));
    const size_t o_tcnt = o_desc + align256(size_t(group) * sizeof(fourmc_block));
    void* w = nullptr;
    if (int r = ws.get(s, o_tcnt + size_t(group) * kSlotTiles * sizeof(uint32_t), &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_idx = reinterpret_cast<fourmc_image_index_dev*>(base);
    auto* d_cnt = reinterpret_cast<fourmc_lineat_counts*>(base + o_cnt);
    auto* d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
    auto* d_flag = reinterpret_cast<uint32_t*>(base + o_flag);
    auto* d_list = reinterpret_cast<uint32_t*>(base + o_list);
    auto* d_req = reinterpret_cast<fourmc_lineat_req*>(base + o_req);
    auto* d_desc = reinterpret_cast<fourmc_block*>(base + o_desc);
    auto* d_tcnt = reinterpret_cast<uint32_t*>(base + o_tcnt);
    const uint32_t L = std::min(row_bytes, max_line_len);
    HIP_TRY(fourmc_launch_image_index(d_image, image_bytes, d_idx, d_ent, nb, s));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(fourmc_lineat_counts), s));
    if (nb) HIP_TRY(hipMemsetAsync(d_flag, 0, size_t(nb) * sizeof(uint32_t), s));
    HIP_TRY(fourmc_launch_lineat_locate(d_ent, nb, idx.info.total_bytes, d_index, d_lines, n, L, d_req, d_flag, static_cast<uint8_t*>(d_rows),
                                        row_bytes, pad, d_text_len, d_status, s));
    HIP_TRY(fourmc_launch_lineat_compact(d_flag, nb, d_list, d_cnt, s));
    fourmc_lineat_counts cnt;
    HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t needed = std::min(cnt.needed, nb);
    WsLease ws2(&g_img_stage);
    char* d_stage = nullptr;
    if (needed) {
        void* w2 = nullptr;
        if (int r = ws2.get(s, size_t(std::min(group, needed)) * kSlot, &w2)) return r;
        d_stage = static_cast<char*>(w2);
    }
    uint64_t rounds = 0;
    for (uint32_t r0 = 0; r0 < needed; r0 += group) {
        const uint32_t m = std::min(group, needed - r0);
        rounds++; g_la.rounds++; g_la.decodes++; g_la.staged += m;
        HIP_TRY(fourmc_launch_lineat_desc(d_ent, d_list + r0, 0, m, kSlot, d_desc, s));
        if (int r = fourmc_gpu_4mc_decode_blocks(d_image, d_stage, d_desc, m, image_codec(idx), s)) return r;
        HIP_TRY(fourmc_launch_lineat_tiles(d_stage, kSlot, d_ent, d_list + r0, m, d_tcnt, s));
        HIP_TRY(fourmc_launch_lineat_resolve(d_stage, kSlot, d_ent, d_index, d_list + r0, d_desc, m, d_tcnt, d_req, n, max_line_len,
                                             static_cast<uint8_t*>(d_rows), row_bytes, pad, d_text_len, d_status, s));
    }
    HIP_TRY(fourmc_launch_lineat_served(d_status, n, d_cnt, s));
    HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->result = int64_t(cnt.served); out->served = cnt.served; out->blocks_staged = needed; out->rounds = rounds;
    return FOURMC_OK;
}

void fourmc_gpu_image_lines_at_stats(unsigned long long* rounds, unsigned long long* block_decodes, unsigned long long* blocks_staged)
{
    if (rounds) *rounds = g_la.rounds.load();
    if (block_decodes) *block_decodes = g_la.decodes.load();
    if (blocks_staged) *blocks_staged = g_la.staged.load();
}

} // extern "C"
