// 4mc_amd/csrc/engine_lines.hip — the records and lines of the splits of device images (records.hip): one split, many splits of one
// image, the splits of many images.
#include "engine_int.h"

namespace {
// The delimiter scan over d[0, len), count - finish - write; d_cnt holds fourmc_records_tiles(d, len) words.
int records_scan(const void* d, uint64_t len, uint8_t delim, uint64_t* d_cnt, const fourmc_block* d_desc, uint32_t ndesc,
                 int first_split, uint64_t ds, uint64_t body, uint64_t* d_starts, uint64_t starts_cap, fourmc_records_state* d_st,
                 hipStream_t s)
{
    const uint64_t ntiles = fourmc_records_tiles(d, len);
    if (ntiles > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "image_read_records: %llu bytes in one split", (unsigned long long)len); return FOURMC_EUNSUP; }
    HIP_TRY(fourmc_launch_records_count(d, len, delim, d_cnt, ntiles, s));
    HIP_TRY(fourmc_launch_records_finish(d, len, delim, d_cnt, ntiles, d_desc, ndesc, first_split, ds, body, d_starts, starts_cap, d_st, s));
    if (d_starts) HIP_TRY(fourmc_launch_records_write(d, len, delim, d_cnt, ntiles, d_st, d_starts, s));
    return FOURMC_OK;
}
// The line-end scan over d[0, len): the same passes by the line rule, and the text lengths behind them.
int lines_scan(const void* d, uint64_t len, uint32_t max_line_len, uint64_t* d_cnt, const fourmc_block* d_desc, uint32_t ndesc,
               int first_split, uint64_t ds, uint64_t body, uint64_t* d_starts, uint32_t* d_text_len, uint64_t lines_cap,
               fourmc_records_state* d_st, hipStream_t s)
{
    const uint64_t ntiles = fourmc_records_tiles(d, len);
    if (ntiles > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "image_read_lines: %llu bytes in one split", (unsigned long long)len); return FOURMC_EUNSUP; }
    HIP_TRY(fourmc_launch_lines_count(d, len, d_cnt, ntiles, s));
    HIP_TRY(fourmc_launch_lines_finish(d, len, d_cnt, ntiles, d_desc, ndesc, first_split, ds, body, d_starts, lines_cap, d_text_len, d_st, s));
    if (d_starts) HIP_TRY(fourmc_launch_lines_write(d, len, max_line_len, d_cnt, ntiles, d_st, d_starts, d_text_len, s));
    return FOURMC_OK;
}
// tile counts of any destination of `len` bytes (its address may add one chunk)
size_t records_cnt_bytes(uint64_t len) { return size_t((len + 16) / FOURMC_RECORDS_TILE + 2) * sizeof(uint64_t); }

// groups processed, tail rounds run and container decode calls made by the batch call (fourmc_gpu_image_lines_batch_stats), and
// the same with the index kernel's launches for the many-images call (fourmc_gpu_images_lines_stats)
struct LinesCounters { std::atomic<unsigned long long> groups{0}, rounds{0}, decodes{0}, index_launches{0}; };
LinesCounters g_lb, g_il;

// FOURMC_SPLIT_GROUP: the most splits of one group (a staging slot each); read at every call, like FOURMC_IMAGE_PARSE
static uint32_t split_group()
{
    const char* e = getenv("FOURMC_SPLIT_GROUP");
    if (!e || !*e) return 256;
    const long v = strtol(e, nullptr, 10);
    return v < 1 ? 1u : v > 4096 ? 4096u : uint32_t(v);
}

inline uint32_t item_image(const fourmc_image_split_item&) { return 0; }
inline uint32_t item_image(const fourmc_images_split_item& it) { return it.image; }

// what both line calls check of their buffers and regions, before a device is looked for
template <class Item>
int lines_args(const char* who, const void* d_image, const void* d_dst, uint64_t dst_bytes, const uint64_t* d_starts, const uint32_t* d_text_len,
               uint64_t table_entries, uint32_t max_line_len, const Item* items, uint32_t n)
{
    if (!items) { snprintf(g_err, sizeof g_err, "%s: null items", who); return FOURMC_EINVAL; }
    if (!d_image) { snprintf(g_err, sizeof g_err, "%s: null image", who); return FOURMC_EINVAL; }
    if (!d_dst) { snprintf(g_err, sizeof g_err, "%s: null destination", who); return FOURMC_EINVAL; }
    if (!d_starts != !d_text_len) { snprintf(g_err, sizeof g_err, "%s: d_starts and d_text_len go together (both NULL: count only)", who); return FOURMC_EINVAL; }
    if (max_line_len > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "%s: max_line_len %u above 0x7FFFFFFF", who, max_line_len); return FOURMC_EINVAL; }
    std::vector<std::pair<uint64_t, uint64_t>> d, t;
    d.reserve(n);
    if (d_starts) t.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        const Item& it = items[i];
        if (span_outside(it.dst_off, it.dst_cap, dst_bytes)) {
            snprintf(g_err, sizeof g_err, "%s: the output region of split %u lies beyond the %llu bytes of the destination", who, i,
                     (unsigned long long)dst_bytes);
            return FOURMC_EINVAL;
        }
        if (it.dst_cap) d.emplace_back(it.dst_off, it.dst_off + it.dst_cap);
        if (!d_starts) continue;                          // count only looks at no table
        if (span_outside(it.table_off, it.lines_cap, table_entries)) {
            snprintf(g_err, sizeof g_err, "%s: the table region of split %u lies beyond the %llu entries of the tables", who, i,
                     (unsigned long long)table_entries);
            return FOURMC_EINVAL;
        }
        if (it.lines_cap) t.emplace_back(it.table_off, it.table_off + it.lines_cap);
    }
    if (int r = regions_overlap(who, "output regions", d)) return r;
    return regions_overlap(who, "table regions", t);
}

// The images of a call in the workspace: the summaries, the image table, the entries of all images in one table.
inline size_t images_o_tab(uint32_t nimg) { return std::max(kIdxBytes, align256(size_t(nimg) * sizeof(fourmc_image_index_dev))); }
inline size_t images_o_ent(uint32_t nimg) { return images_o_tab(nimg) + align256(size_t(nimg) * sizeof(fourmc_images_tab)); }
inline int64_t index_code(const fourmc_image_index_dev& x) { return x.info.nblocks < 0 ? x.info.nblocks : x.info.framing; }

// what the many-images calls check of their images
int images_args(const char* who, uint64_t images_bytes, const fourmc_image_ref* images, uint32_t nimages)
{
    if (nimages && !images) { snprintf(g_err, sizeof g_err, "%s: null images", who); return FOURMC_EINVAL; }
    for (uint32_t k = 0; k < nimages; k++)
        if (span_outside(images[k].image_off, images[k].image_bytes, images_bytes)) {
            snprintf(g_err, sizeof g_err, "%s: image %u lies beyond the %llu bytes of the buffer", who, k, (unsigned long long)images_bytes);
            return FOURMC_EINVAL;
        }
    return FOURMC_OK;
}

// The summaries of all images, read back: the call's first synchronization.  tabs[k] comes back with image k's block count, and
// with its place in the entry table when named[k] says that somebody will look its entries up; *nent: the table's entries.
int images_index_count(const char* who, WsLease& ws, hipStream_t s, const void* d_images, const fourmc_image_ref* images, uint32_t nimages,
                       const std::vector<uint8_t>& named, std::vector<fourmc_images_tab>& tabs, std::vector<fourmc_image_index_dev>& sums,
                       uint64_t* nent)
{
    tabs.assign(nimages, fourmc_images_tab());
    sums.resize(nimages);
    for (uint32_t k = 0; k < nimages; k++) { tabs[k].image_off = images[k].image_off; tabs[k].image_bytes = images[k].image_bytes; }
    void* w = nullptr;
    if (int r = ws.get(s, images_o_ent(nimages), &w)) return r;
    auto* d_idx = static_cast<fourmc_image_index_dev*>(w);
    auto* d_tab = reinterpret_cast<fourmc_images_tab*>(static_cast<char*>(w) + images_o_tab(nimages));
    HIP_TRY(hipMemcpyAsync(d_tab, tabs.data(), size_t(nimages) * sizeof(fourmc_images_tab), hipMemcpyHostToDevice, s));
    HIP_TRY(fourmc_launch_images_index(d_images, d_tab, nimages, d_idx, nullptr, s));
    HIP_TRY(hipMemcpyAsync(sums.data(), d_idx, size_t(nimages) * sizeof(fourmc_image_index_dev), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t all = 0, ent = 0;
    for (uint32_t k = 0; k < nimages; k++) {
        if (index_code(sums[k]) != 0) continue;
        const uint64_t nb = uint64_t(sums[k].info.nblocks);
        all += nb;
        if (all > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "%s: more than 0x7FFFFFFF blocks in the images", who); return FOURMC_EUNSUP; }
        tabs[k].nblocks = uint32_t(nb);
        if (named[k]) { tabs[k].cap = uint32_t(nb); tabs[k].ent0 = ent; ent += nb; }
    }
    *nent = ent;
    return FOURMC_OK;
}

// The group walk of both line calls.  tabs / sums: the images and their summaries as read back (the one-image call passes a
// table of one image at offset 0), nent: the entries of the named images together.  The host walks the single call's steps for
// a group of splits at a time: the plans come back once, each tail round's verdicts once, the states once; everything between is
// one launch for the whole group, and one container decode per format the group's images have.  Workspace (g_img_ws): the
// summaries, the image table and the entries, then per group the requests, plans, jobs, tails and tail descriptors, and - sized
// after the rounds, when the spans are known - the spans, their two tables of firsts, the states, the body descriptors and the
// tile counts.  A buffer that grows there loses the entries: the index kernel runs again.  Staging (g_img_stage): one slot per
// split of the group that searches.  res[i]: item i's result, zeroed by the caller.
template <class Item>
int lines_groups(const char* who, LinesCounters& ctr, WsLease& ws, hipStream_t s, const void* d_images,
                 const std::vector<fourmc_images_tab>& tabs, const std::vector<fourmc_image_index_dev>& sums, uint64_t nent,
                 uint32_t max_line_len, void* d_dst, uint64_t* d_starts, uint32_t* d_text_len, const Item* items, uint32_t n,
                 fourmc_image_lines* res)
{
    const uint32_t nimg = uint32_t(tabs.size());
    auto total_of = [&](uint32_t im) { return index_code(sums[im]) != 0 ? uint64_t(0) : sums[im].info.total_bytes; };
    // the groups: at most FOURMC_SPLIT_GROUP splits, and no more tiles than one grid takes (by the bound the counts are sized by)
    const uint32_t most = split_group();
    std::vector<uint32_t> cut(1, 0);
    size_t cnt_most = 0;
    {
        uint64_t tiles = 0; uint32_t in = 0;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t t = records_cnt_bytes(std::min(items[i].dst_cap, total_of(item_image(items[i])))) / sizeof(uint64_t);
            if (in == most || (in && tiles + t > 0x7FFFFFFFull)) { cut.push_back(i); in = 0; tiles = 0; }
            in++; tiles += t;
            cnt_most = std::max(cnt_most, size_t(tiles) * sizeof(uint64_t));
        }
        cut.push_back(n);
    }
    uint32_t m_most = 0;
    for (size_t g = 1; g < cut.size(); g++) m_most = std::max(m_most, cut[g] - cut[g - 1]);
    // the layout: what is fixed for the call, then the group's first phase, then its second
    const size_t o_tab = images_o_tab(nimg), o_ent = images_o_ent(nimg);
    const size_t o_req = o_ent + align256(size_t(nent) * sizeof(fourmc_image_entry));
    const size_t o_plan = o_req + align256(size_t(m_most) * sizeof(fourmc_split_req));
    const size_t o_job = o_plan + align256(size_t(m_most) * sizeof(fourmc_records_plan));
    const size_t o_tail = o_job + align256(size_t(m_most) * sizeof(fourmc_tail_job));
    const size_t o_tdesc = o_tail + align256(size_t(m_most) * sizeof(fourmc_records_tail));
    const size_t o_span = o_tdesc + align256(size_t(m_most) * sizeof(fourmc_block));
    const size_t o_ft = o_span + align256(size_t(m_most) * sizeof(fourmc_lines_span));
    const size_t o_fd = o_ft + align256((size_t(m_most) + 1) * sizeof(uint64_t));
    const size_t o_st = o_fd + align256((size_t(m_most) + 1) * sizeof(uint32_t));
    const size_t o_cnt = o_st + align256(size_t(m_most) * sizeof(fourmc_records_state));
    auto o_bdesc = [&](uint64_t tiles) { return o_cnt + align256((size_t(tiles) + 1) * sizeof(uint64_t)); };
    void* w = nullptr;
    // the body descriptors of a partition of every image: a block each, and one more per split whose tail block ends with a CR
    if (int r = ws.get(s, o_bdesc(cnt_most / sizeof(uint64_t)) + (size_t(nent) + m_most) * sizeof(fourmc_block), &w)) return r;
    char* base = static_cast<char*>(w);
    // the image table with every image's place in the entry table, and the entries (the summaries again with them)
    auto index_all = [&]() -> int {
        ctr.index_launches++;
        auto* d_tab = reinterpret_cast<fourmc_images_tab*>(base + o_tab);
        HIP_TRY(hipMemcpyAsync(d_tab, tabs.data(), size_t(nimg) * sizeof(fourmc_images_tab), hipMemcpyHostToDevice, s));
        HIP_TRY(fourmc_launch_images_index(d_images, d_tab, nimg, reinterpret_cast<fourmc_image_index_dev*>(base),
                                           reinterpret_cast<fourmc_image_entry*>(base + o_ent), s));
        return FOURMC_OK;
    };
    if (int r = index_all()) return r;
    WsLease ws2(&g_img_stage);
    constexpr uint64_t kSlot = uint64_t(FOURMC_BLOCKSIZE) + 64;

    // b, bt and nb count the blocks of the split's own image, whose entries start at e0
    struct Search { bool live, searching, pending, zstd; uint32_t b, bt, slot, nb, e0; uint64_t hi, src_base; fourmc_records_tail tail; };
    auto run_group = [&](uint32_t g0, uint32_t m) -> int {
        ctr.groups++;
        auto* d_idx = reinterpret_cast<fourmc_image_index_dev*>(base);
        auto* d_tab = reinterpret_cast<fourmc_images_tab*>(base + o_tab);
        auto* d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
        auto* d_req = reinterpret_cast<fourmc_split_req*>(base + o_req);
        auto* d_plan = reinterpret_cast<fourmc_records_plan*>(base + o_plan);
        auto* d_job = reinterpret_cast<fourmc_tail_job*>(base + o_job);
        auto* d_tail = reinterpret_cast<fourmc_records_tail*>(base + o_tail);
        auto* d_tdesc = reinterpret_cast<fourmc_block*>(base + o_tdesc);
        std::vector<fourmc_split_req> req(m);
        for (uint32_t i = 0; i < m; i++) {
            req[i].split_start = items[g0 + i].split_start; req[i].split_end = items[g0 + i].split_end;
            req[i].image = item_image(items[g0 + i]); req[i].pad = 0;
        }
        std::vector<fourmc_records_plan> plan(m);
        HIP_TRY(hipMemcpyAsync(d_req, req.data(), size_t(m) * sizeof(fourmc_split_req), hipMemcpyHostToDevice, s));
        HIP_TRY(fourmc_launch_lines_batch_plan(d_ent, d_tab, d_idx, d_req, m, d_plan, s));
        HIP_TRY(hipMemcpyAsync(plan.data(), d_plan, size_t(m) * sizeof(fourmc_records_plan), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        // hi, split by split as the single call finds it; a round stages one block for every split that still searches
        std::vector<Search> q(m);
        uint32_t nslots = 0;
        for (uint32_t i = 0; i < m; i++) {
            Search& h = q[i];
            h = Search();
            const uint32_t im = req[i].image;
            if (const int64_t code = index_code(sums[im])) { res[g0 + i].result = code; continue; }      // the image cannot be indexed
            if (plan[i].code != 0) { res[g0 + i].result = plan[i].code; continue; }
            res[g0 + i].base = plan[i].ds;
            h.nb = tabs[im].nblocks; h.e0 = uint32_t(tabs[im].ent0); h.src_base = tabs[im].image_off; h.zstd = sums[im].info.is_zstd != 0;
            h.live = true; h.hi = plan[i].total; h.bt = h.nb; h.b = plan[i].b1;
            h.searching = plan[i].b1 < h.nb;
            if (h.searching) h.slot = nslots++;
        }
        char* d_stage = nullptr;
        if (nslots) {
            void* w2 = nullptr;
            if (int r = ws2.get(s, size_t(nslots) * kSlot, &w2)) return r;
            d_stage = static_cast<char*>(w2);
        }
        std::vector<fourmc_tail_job> jobs;
        std::vector<uint32_t> owner;
        std::vector<fourmc_records_tail> tails;
        for (;;) {
            jobs.clear(); owner.clear();
            uint32_t nj4 = 0;                                 // the .4mc jobs, which go first: one decode per format
            for (int z = 0; z < 2; z++) {
                for (uint32_t i = 0; i < m; i++)
                    if (q[i].searching && int(q[i].zstd) == z) {
                        fourmc_tail_job j; j.e = q[i].e0 + q[i].b; j.slot = q[i].slot; j.last_block = q[i].b + 1 == q[i].nb; j.pending = q[i].pending;
                        j.src_base = q[i].src_base;
                        jobs.push_back(j); owner.push_back(i);
                    }
                if (z == 0) nj4 = uint32_t(jobs.size());
            }
            if (jobs.empty()) break;
            const uint32_t nj = uint32_t(jobs.size());
            ctr.rounds++;
            tails.resize(nj);
            HIP_TRY(hipMemcpyAsync(d_job, jobs.data(), size_t(nj) * sizeof(fourmc_tail_job), hipMemcpyHostToDevice, s));
            HIP_TRY(fourmc_launch_lines_batch_tail_desc(d_ent, d_job, nj, kSlot, d_tdesc, s));
            if (nj4) {
                ctr.decodes++;
                if (int r = fourmc_gpu_4mc_decode_blocks(d_images, d_stage, d_tdesc, nj4, FOURMC_CODEC_LZ4_FAST, s)) return r;
            }
            if (nj > nj4) {
                ctr.decodes++;
                if (int r = fourmc_gpu_4mc_decode_blocks(d_images, d_stage, d_tdesc + nj4, nj - nj4, FOURMC_CODEC_ZSTD, s)) return r;
            }
            HIP_TRY(fourmc_launch_lines_batch_tail_find(d_stage, kSlot, d_tdesc, d_ent, d_job, nj, d_tail, s));
            HIP_TRY(hipMemcpyAsync(tails.data(), d_tail, size_t(nj) * sizeof(fourmc_records_tail), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (uint32_t j = 0; j < nj; j++) {
                Search& h = q[owner[j]];
                h.tail = tails[j];
                if (h.tail.code != 0) { res[g0 + owner[j]].result = h.tail.code; h.live = h.searching = false; continue; }
                if (h.tail.found == 1) { h.bt = h.b; h.hi = h.tail.hi; h.searching = false; continue; }
                if (h.tail.found == 2) { h.pending = true; h.hi = h.tail.hi; }
                if (++h.b == h.nb) h.searching = false;
            }
        }
        // the spans: the splits whose content fits, those of .4mc images first
        std::vector<fourmc_lines_span> spans;
        std::vector<uint64_t> first_tile;
        std::vector<uint32_t> first_desc, span_item;
        uint64_t tiles = 0, ndesc = 0, ndesc4 = 0, longest = 0, longest_copy = 0;
        for (int z = 0; z < 2; z++) {
            for (uint32_t i = 0; i < m; i++) {
                const Search& h = q[i];
                if (!h.live || int(h.zstd) != z) continue;
                const Item& it = items[g0 + i];
                const uint64_t len = h.hi - plan[i].ds;
                if (len > it.dst_cap) { res[g0 + i].result = -5; res[g0 + i].data_bytes = len; continue; }
                fourmc_lines_span sp;
                memset(&sp, 0, sizeof sp);
                sp.dst = static_cast<uint8_t*>(d_dst) + it.dst_off; sp.len = len;
                sp.tile0 = tiles; sp.ntiles = fourmc_records_tiles(sp.dst, len);
                sp.desc0 = uint32_t(ndesc); sp.ndesc = h.bt - plan[i].b0; sp.e0 = h.e0 + plan[i].b0; sp.src_base = h.src_base;
                sp.first_split = it.split_start == 0; sp.ds = plan[i].ds; sp.body = plan[i].de - plan[i].ds;
                if (d_starts) { sp.starts = d_starts + it.table_off; sp.tlen = d_text_len + it.table_off; sp.lines_cap = it.lines_cap; }
                if (h.bt < h.nb && h.hi > h.tail.data_off) {
                    sp.stage = reinterpret_cast<const uint8_t*>(d_stage) + uint64_t(h.slot) * kSlot;
                    sp.copy_off = h.tail.data_off - plan[i].ds; sp.copy_len = h.hi - h.tail.data_off;
                    longest_copy = std::max(longest_copy, sp.copy_len);
                }
                tiles += sp.ntiles; ndesc += sp.ndesc; longest = std::max(longest, len);
                if (tiles > 0x7FFFFFFFull || ndesc > 0x7FFFFFFFull) {
                    snprintf(g_err, sizeof g_err, "%s: %llu bytes or %llu blocks in one group", who, (unsigned long long)tiles * FOURMC_RECORDS_TILE,
                             (unsigned long long)ndesc);
                    return FOURMC_EUNSUP;
                }
                spans.push_back(sp); first_tile.push_back(sp.tile0); first_desc.push_back(sp.desc0); span_item.push_back(g0 + i);
            }
            if (z == 0) ndesc4 = ndesc;
        }
        if (spans.empty()) return FOURMC_OK;
        const uint32_t ns = uint32_t(spans.size());
        first_tile.push_back(tiles); first_desc.push_back(uint32_t(ndesc));
        const size_t had = ws.cap();
        void* wg = nullptr;
        if (int r = ws.get(s, o_bdesc(tiles) + size_t(ndesc) * sizeof(fourmc_block), &wg)) return r;
        base = static_cast<char*>(wg);
        d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
        if (ws.cap() != had)                                  // the buffer moved: the entries again
            if (int r = index_all()) return r;
        auto* d_span = reinterpret_cast<fourmc_lines_span*>(base + o_span);
        auto* d_ft = reinterpret_cast<uint64_t*>(base + o_ft);
        auto* d_fd = reinterpret_cast<uint32_t*>(base + o_fd);
        auto* d_st = reinterpret_cast<fourmc_records_state*>(base + o_st);
        auto* d_cnt = reinterpret_cast<uint64_t*>(base + o_cnt);
        auto* d_bdesc = reinterpret_cast<fourmc_block*>(base + o_bdesc(tiles));
        HIP_TRY(hipMemcpyAsync(d_span, spans.data(), size_t(ns) * sizeof(fourmc_lines_span), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_ft, first_tile.data(), (size_t(ns) + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(d_fd, first_desc.data(), (size_t(ns) + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (ndesc) {
            HIP_TRY(fourmc_launch_lines_batch_body_desc(d_ent, d_span, d_fd, ns, uint32_t(ndesc), d_dst, d_bdesc, s));
            if (ndesc4) {
                ctr.decodes++;
                if (int r = fourmc_gpu_4mc_decode_blocks(d_images, d_dst, d_bdesc, uint32_t(ndesc4), FOURMC_CODEC_LZ4_FAST, s)) return r;
            }
            if (ndesc > ndesc4) {
                ctr.decodes++;
                if (int r = fourmc_gpu_4mc_decode_blocks(d_images, d_dst, d_bdesc + ndesc4, uint32_t(ndesc - ndesc4), FOURMC_CODEC_ZSTD, s)) return r;
            }
        }
        HIP_TRY(fourmc_launch_lines_batch_copy(d_span, ns, longest_copy, s));
        HIP_TRY(fourmc_launch_lines_batch_count(d_span, d_ft, ns, d_cnt, tiles, s));
        HIP_TRY(fourmc_launch_lines_batch_finish(d_span, ns, d_cnt, d_bdesc, d_st, s));
        if (d_starts) HIP_TRY(fourmc_launch_lines_batch_write(d_span, d_ft, ns, d_cnt, tiles, longest, max_line_len, d_st, s));
        std::vector<fourmc_records_state> st(ns);
        HIP_TRY(hipMemcpyAsync(st.data(), d_st, size_t(ns) * sizeof(fourmc_records_state), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (uint32_t k = 0; k < ns; k++) memcpy(&res[span_item[k]], &st[k].r, sizeof(fourmc_image_lines));
        return FOURMC_OK;
    };
    for (size_t g = 1; g < cut.size(); g++)
        if (int r = run_group(cut[g - 1], cut[g] - cut[g - 1])) return r;
    return FOURMC_OK;
}
} // namespace

extern "C" {

// ------------------------------------------------------------------------ the line records of a split (records.hip)
// Read-backs: the summary; the plan (the split's blocks and decoded offsets); one per tail block staged in search of hi; the
// result.  Between the last two: the body's descriptors, ONE container decode straight into d_dst, the copy of the last tail
// block's prefix out of staging, and the scan.
int fourmc_gpu_image_read_records(const void* d_image, uint64_t image_bytes, uint64_t split_start, uint64_t split_end, uint8_t delim,
                                  void* d_dst, uint64_t dst_cap, uint64_t* d_starts, uint64_t starts_cap,
                                  fourmc_image_records* out, void* stream)
{
    if (!out) { snprintf(g_err, sizeof g_err, "image_read_records: null result"); return FOURMC_EINVAL; }
    if (!d_image) { snprintf(g_err, sizeof g_err, "image_read_records: null image"); return FOURMC_EINVAL; }
    if (!d_dst) { snprintf(g_err, sizeof g_err, "image_read_records: null destination"); return FOURMC_EINVAL; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    memset(out, 0, sizeof *out);
    WsLease ws(&g_img_ws);
    fourmc_image_index_dev idx;
    if (int r = image_index_count(ws, s, d_image, image_bytes, &idx)) return r;
    const int64_t code = idx.info.nblocks < 0 ? idx.info.nblocks : idx.info.framing;
    if (code != 0) { out->result = code; return FOURMC_OK; }
    const uint32_t n = uint32_t(idx.info.nblocks);
    const size_t o_plan = kIdxBytes, o_tail = o_plan + 256, o_st = o_tail + 256, o_ent = o_st + 256;
    const size_t o_desc = o_ent + align256(size_t(n) * sizeof(fourmc_image_entry));
    const size_t o_cnt = o_desc + align256((size_t(n) + 1) * sizeof(fourmc_block));
    void* w = nullptr;
    if (int r = ws.get(s, o_cnt + records_cnt_bytes(std::min(dst_cap, idx.info.total_bytes)), &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_idx = reinterpret_cast<fourmc_image_index_dev*>(base);
    auto* d_plan = reinterpret_cast<fourmc_records_plan*>(base + o_plan);
    auto* d_tail = reinterpret_cast<fourmc_records_tail*>(base + o_tail);
    auto* d_st = reinterpret_cast<fourmc_records_state*>(base + o_st);
    auto* d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
    auto* d_desc = reinterpret_cast<fourmc_block*>(base + o_desc);
    auto* d_cnt = reinterpret_cast<uint64_t*>(base + o_cnt);
    HIP_TRY(fourmc_launch_image_index(d_image, image_bytes, d_idx, d_ent, n, s));
    HIP_TRY(fourmc_launch_records_plan(d_ent, n, d_idx, split_start, split_end, d_plan, s));
    fourmc_records_plan plan;
    HIP_TRY(hipMemcpyAsync(&plan, d_plan, sizeof plan, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (plan.code != 0) { out->result = plan.code; return FOURMC_OK; }
    out->base = plan.ds;
    // hi: behind the first delimiter at or after de.  The blocks from b1 on go through the staging slot one at a time until one
    // shows a delimiter; bt is that block (n: the content ends first) and its prefix is still in the slot afterwards.
    uint64_t hi = plan.total;
    uint32_t bt = n;
    fourmc_records_tail tail = {};
    char* d_stage = nullptr;
    WsLease ws2(&g_img_stage);
    if (plan.b1 < n) {
        void* w2 = nullptr;
        if (int r = ws2.get(s, size_t(FOURMC_BLOCKSIZE) + 64, &w2)) return r;
        d_stage = static_cast<char*>(w2);
    }
    for (uint32_t b = plan.b1; b < n; b++) {
        HIP_TRY(fourmc_launch_records_desc(d_ent, b, 1, 0, 1, d_desc, s));
        if (int r = fourmc_gpu_4mc_decode_blocks(d_image, d_stage, d_desc, 1, image_codec(idx), s)) return r;
        HIP_TRY(fourmc_launch_records_tail_find(d_stage, d_desc, d_ent, b, delim, d_tail, s));
        HIP_TRY(hipMemcpyAsync(&tail, d_tail, sizeof tail, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (tail.code != 0) { out->result = tail.code; return FOURMC_OK; }
        if (tail.found) { bt = b; hi = tail.hi; break; }
    }
    const uint64_t len = hi - plan.ds;
    if (len > dst_cap) { out->result = -5; out->data_bytes = len; return FOURMC_OK; }
    const uint32_t count = bt - plan.b0;
    if (count) {
        HIP_TRY(fourmc_launch_records_desc(d_ent, plan.b0, count, plan.ds, 0, d_desc, s));
        if (int r = fourmc_gpu_4mc_decode_blocks(d_image, d_dst, d_desc, count, image_codec(idx), s)) return r;
    }
    if (bt < n && hi > tail.data_off)
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(d_dst) + (tail.data_off - plan.ds), d_stage, hi - tail.data_off, hipMemcpyDeviceToDevice, s));
    if (int r = records_scan(d_dst, len, delim, d_cnt, d_desc, count, split_start == 0, plan.ds, plan.de - plan.ds, d_starts, starts_cap, d_st, s)) return r;
    fourmc_records_state st;
    HIP_TRY(hipMemcpyAsync(&st, d_st, sizeof st, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = st.r;
    return FOURMC_OK;
}

// image_read_records with the line rule.  Read-backs: as there, and one more when a staged tail block ends with a CR: whether
// that CR ends the line is the next block's first byte, so that block is staged too.  The block with the CR then lies wholly
// inside [ds, hi) and is decoded with the body; of the block behind it at most the LF leaves the staging slot.
int fourmc_gpu_image_read_lines(const void* d_image, uint64_t image_bytes, uint64_t split_start, uint64_t split_end, uint32_t max_line_len,
                                void* d_dst, uint64_t dst_cap, uint64_t* d_starts, uint32_t* d_text_len, uint64_t lines_cap,
                                fourmc_image_lines* out, void* stream)
{
    if (!out) { snprintf(g_err, sizeof g_err, "image_read_lines: null result"); return FOURMC_EINVAL; }
    if (!d_image) { snprintf(g_err, sizeof g_err, "image_read_lines: null image"); return FOURMC_EINVAL; }
    if (!d_dst) { snprintf(g_err, sizeof g_err, "image_read_lines: null destination"); return FOURMC_EINVAL; }
    if (!d_starts != !d_text_len) { snprintf(g_err, sizeof g_err, "image_read_lines: d_starts and d_text_len go together (both NULL: count only)"); return FOURMC_EINVAL; }
    if (max_line_len > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "image_read_lines: max_line_len %u above 0x7FFFFFFF", max_line_len); return FOURMC_EINVAL; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    memset(out, 0, sizeof *out);
    WsLease ws(&g_img_ws);
    fourmc_image_index_dev idx;
    if (int r = image_index_count(ws, s, d_image, image_bytes, &idx)) return r;
    const int64_t code = idx.info.nblocks < 0 ? idx.info.nblocks : idx.info.framing;
    if (code != 0) { out->result = code; return FOURMC_OK; }
    const uint32_t n = uint32_t(idx.info.nblocks);
    const size_t o_plan = kIdxBytes, o_tail = o_plan + 256, o_st = o_tail + 256, o_ent = o_st + 256;
    const size_t o_desc = o_ent + align256(size_t(n) * sizeof(fourmc_image_entry));
    const size_t o_cnt = o_desc + align256((size_t(n) + 1) * sizeof(fourmc_block));
    void* w = nullptr;
    if (int r = ws.get(s, o_cnt + records_cnt_bytes(std::min(dst_cap, idx.info.total_bytes)), &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_idx = reinterpret_cast<fourmc_image_index_dev*>(base);
    auto* d_plan = reinterpret_cast<fourmc_records_plan*>(base + o_plan);
    auto* d_tail = reinterpret_cast<fourmc_records_tail*>(base + o_tail);
    auto* d_st = reinterpret_cast<fourmc_records_state*>(base + o_st);
    auto* d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
    auto* d_desc = reinterpret_cast<fourmc_block*>(base + o_desc);
    auto* d_cnt = reinterpret_cast<uint64_t*>(base + o_cnt);
    HIP_TRY(fourmc_launch_image_index(d_image, image_bytes, d_idx, d_ent, n, s));
    HIP_TRY(fourmc_launch_records_plan(d_ent, n, d_idx, split_start, split_end, d_plan, s));
    fourmc_records_plan plan;
    HIP_TRY(hipMemcpyAsync(&plan, d_plan, sizeof plan, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (plan.code != 0) { out->result = plan.code; return FOURMC_OK; }
    out->base = plan.ds;
    // hi: behind the first line end at or after de.  As in image_read_records the blocks from b1 on are staged one at a time; bt
    // is the first block the body decode leaves out (n: none), and [tail.data_off, hi) comes out of the slot.  `pending`: the
    // block staged last ended with a CR and is not the last one, hi so far is behind that CR.
    uint64_t hi = plan.total;
    uint32_t bt = n;
    bool pending = false;
    fourmc_records_tail tail = {};
    char* d_stage = nullptr;
    WsLease ws2(&g_img_stage);
    if (plan.b1 < n) {
        void* w2 = nullptr;
        if (int r = ws2.get(s, size_t(FOURMC_BLOCKSIZE) + 64, &w2)) return r;
        d_stage = static_cast<char*>(w2);
    }
    for (uint32_t b = plan.b1; b < n; b++) {
        HIP_TRY(fourmc_launch_records_desc(d_ent, b, 1, 0, 1, d_desc, s));
        if (int r = fourmc_gpu_4mc_decode_blocks(d_image, d_stage, d_desc, 1, image_codec(idx), s)) return r;
        HIP_TRY(fourmc_launch_lines_tail_find(d_stage, d_desc, d_ent, b, b + 1 == n, pending, d_tail, s));
        HIP_TRY(hipMemcpyAsync(&tail, d_tail, sizeof tail, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (tail.code != 0) { out->result = tail.code; return FOURMC_OK; }
        if (tail.found == 1) { bt = b; hi = tail.hi; break; }
        if (tail.found == 2) { pending = true; hi = tail.hi; }
    }
    const uint64_t len = hi - plan.ds;
    if (len > dst_cap) { out->result = -5; out->data_bytes = len; return FOURMC_OK; }
    const uint32_t count = bt - plan.b0;
    if (count) {
        HIP_TRY(fourmc_launch_records_desc(d_ent, plan.b0, count, plan.ds, 0, d_desc, s));
        if (int r = fourmc_gpu_4mc_decode_blocks(d_image, d_dst, d_desc, count, image_codec(idx), s)) return r;
    }
    if (bt < n && hi > tail.data_off)
        HIP_TRY(hipMemcpyAsync(static_cast<char*>(d_dst) + (tail.data_off - plan.ds), d_stage, hi - tail.data_off, hipMemcpyDeviceToDevice, s));
    if (int r = lines_scan(d_dst, len, max_line_len, d_cnt, d_desc, count, split_start == 0, plan.ds, plan.de - plan.ds, d_starts, d_text_len, lines_cap, d_st, s)) return r;
    fourmc_records_state st;
    HIP_TRY(hipMemcpyAsync(&st, d_st, sizeof st, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(out, &st.r, sizeof *out);
    return FOURMC_OK;
}

void fourmc_gpu_image_lines_batch_stats(unsigned long long* groups, unsigned long long* tail_rounds, unsigned long long* block_decodes)
{
    if (groups) *groups = g_lb.groups.load();
    if (tail_rounds) *tail_rounds = g_lb.rounds.load();
    if (block_decodes) *block_decodes = g_lb.decodes.load();
}
void fourmc_gpu_images_lines_stats(unsigned long long* groups, unsigned long long* tail_rounds, unsigned long long* block_decodes,
                                   unsigned long long* index_launches)
{
    if (groups) *groups = g_il.groups.load();
    if (tail_rounds) *tail_rounds = g_il.rounds.load();
    if (block_decodes) *block_decodes = g_il.decodes.load();
    if (index_launches) *index_launches = g_il.index_launches.load();
}

// image_read_lines for many splits: the group walk above over a table of one image.
int fourmc_gpu_image_read_lines_batch(const void* d_image, uint64_t image_bytes, uint32_t max_line_len, void* d_dst, uint64_t dst_bytes,
                                      uint64_t* d_starts, uint32_t* d_text_len, uint64_t table_entries,
                                      fourmc_image_split_item* items, uint32_t n, void* stream)
{
    if (n == 0) return FOURMC_OK;
    if (int r = lines_args("image_read_lines_batch", d_image, d_dst, dst_bytes, d_starts, d_text_len, table_entries, max_line_len, items, n)) return r;
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<fourmc_image_lines> res(n);                   // collected on the side: `items` changes only when the call succeeds
    memset(res.data(), 0, size_t(n) * sizeof(fourmc_image_lines));
    auto deliver = [&]() { for (uint32_t i = 0; i < n; i++) items[i].out = res[i]; return FOURMC_OK; };
    WsLease ws(&g_img_ws);
    std::vector<fourmc_image_index_dev> sums(1);
    if (int r = image_index_count(ws, s, d_image, image_bytes, &sums[0])) return r;
    const int64_t code = index_code(sums[0]);
    if (code != 0) { for (auto& o : res) o.result = code; return deliver(); }
    std::vector<fourmc_images_tab> tabs(1);
    memset(&tabs[0], 0, sizeof tabs[0]);
    tabs[0].image_bytes = image_bytes; tabs[0].nblocks = tabs[0].cap = uint32_t(sums[0].info.nblocks);
    if (int r = lines_groups("image_read_lines_batch", g_lb, ws, s, d_image, tabs, sums, tabs[0].nblocks, max_line_len, d_dst, d_starts,
                             d_text_len, items, n, res.data())) return r;
    return deliver();
}

// The same for the splits of many images: all summaries in one read-back, then the group walk over the table of all images.
int fourmc_gpu_images_read_lines(const void* d_images, uint64_t images_bytes, const fourmc_image_ref* images, uint32_t nimages,
                                 uint32_t max_line_len, void* d_dst, uint64_t dst_bytes, uint64_t* d_starts, uint32_t* d_text_len,
                                 uint64_t table_entries, fourmc_images_split_item* items, uint32_t n, void* stream)
{
    if (n == 0) return FOURMC_OK;
    if (int r = lines_args("images_read_lines", d_images, d_dst, dst_bytes, d_starts, d_text_len, table_entries, max_line_len, items, n)) return r;
    if (int r = images_args("images_read_lines", images_bytes, images, nimages)) return r;
    for (uint32_t i = 0; i < n; i++)
        if (items[i].image >= nimages) {
            snprintf(g_err, sizeof g_err, "images_read_lines: split %u names image %u of %u", i, items[i].image, nimages);
            return FOURMC_EINVAL;
        }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<fourmc_image_lines> res(n);                   // collected on the side: `items` changes only when the call succeeds
    memset(res.data(), 0, size_t(n) * sizeof(fourmc_image_lines));
    std::vector<uint8_t> named(nimages, 0);
    for (uint32_t i = 0; i < n; i++) named[items[i].image] = 1;
    WsLease ws(&g_img_ws);
    std::vector<fourmc_images_tab> tabs;
    std::vector<fourmc_image_index_dev> sums;
    uint64_t nent = 0;
    g_il.index_launches++;
    if (int r = images_index_count("images_read_lines", ws, s, d_images, images, nimages, named, tabs, sums, &nent)) return r;
    if (int r = lines_groups("images_read_lines", g_il, ws, s, d_images, tabs, sums, nent, max_line_len, d_dst, d_starts, d_text_len,
                             items, n, res.data())) return r;
    for (uint32_t i = 0; i < n; i++) items[i].out = res[i];
    return FOURMC_OK;
}

// Two read-backs: the summaries of all images, then the aligned slices.  The slices of an image that cannot be indexed or has no
// blocks are filled in here as fourmc_gpu_image_align_slices fills them; the align kernel leaves them alone.
int fourmc_gpu_images_align_slices(const void* d_images, uint64_t images_bytes, const fourmc_image_ref* images, uint32_t nimages,
                                   fourmc_images_slice* slices, uint32_t n, void* stream)
{
    if (n == 0) return FOURMC_OK;
    if (!slices) { snprintf(g_err, sizeof g_err, "images_align_slices: null slices"); return FOURMC_EINVAL; }
    if (!d_images) { snprintf(g_err, sizeof g_err, "images_align_slices: null image"); return FOURMC_EINVAL; }
    if (int r = images_args("images_align_slices", images_bytes, images, nimages)) return r;
    for (uint32_t i = 0; i < n; i++)
        if (slices[i].image >= nimages) {
            snprintf(g_err, sizeof g_err, "images_align_slices: slice %u names image %u of %u", i, slices[i].image, nimages);
            return FOURMC_EINVAL;
        }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    std::vector<uint8_t> named(nimages, 0);
    for (uint32_t i = 0; i < n; i++) named[slices[i].image] = 1;
    WsLease ws(&g_img_ws);
    std::vector<fourmc_images_tab> tabs;
    std::vector<fourmc_image_index_dev> sums;
    uint64_t nent = 0;
    if (int r = images_index_count("images_align_slices", ws, s, d_images, images, nimages, named, tabs, sums, &nent)) return r;
    const size_t o_tab = images_o_tab(nimages), o_ent = images_o_ent(nimages);
    const size_t o_sl = o_ent + align256(size_t(nent) * sizeof(fourmc_image_entry));
    void* w = nullptr;
    if (int r = ws.get(s, o_sl + size_t(n) * sizeof(fourmc_images_slice), &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_tab = reinterpret_cast<fourmc_images_tab*>(base + o_tab);
    auto* d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
    auto* d_sl = reinterpret_cast<fourmc_images_slice*>(base + o_sl);
    HIP_TRY(hipMemcpyAsync(d_tab, tabs.data(), size_t(nimages) * sizeof(fourmc_images_tab), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_sl, slices, size_t(n) * sizeof(fourmc_images_slice), hipMemcpyHostToDevice, s));
    HIP_TRY(fourmc_launch_images_index(d_images, d_tab, nimages, reinterpret_cast<fourmc_image_index_dev*>(base), d_ent, s));
    HIP_TRY(fourmc_launch_images_align(d_ent, d_tab, d_sl, n, s));
    std::vector<fourmc_images_slice> back(n);
    HIP_TRY(hipMemcpyAsync(back.data(), d_sl, size_t(n) * sizeof(fourmc_images_slice), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; i++) {
        fourmc_image_slice& q = back[i].s;
        const int64_t code = index_code(sums[back[i].image]);
        if (code != 0 || sums[back[i].image].info.nblocks == 0) {
            q.split_start = q.start; q.split_end = q.end; q.first_block = q.block_count = 0; q.result = code != 0 ? code : 1;
        }
        slices[i].s = q;
    }
    return FOURMC_OK;
}

#ifdef FOURMC_RESEARCH
int fourmc_gpu_debug_lines_scan(const void* d, uint64_t len, uint32_t max_line_len, uint64_t* d_starts, uint32_t* d_text_len,
                                uint64_t lines_cap, int64_t* lines, void* stream)
{
    if (!lines || (len && !d) || !d_starts != !d_text_len || max_line_len > 0x7FFFFFFFu) { snprintf(g_err, sizeof g_err, "debug_lines_scan: bad argument"); return FOURMC_EINVAL; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, 256 + records_cnt_bytes(len), &w)) return r;
    auto* d_st = static_cast<fourmc_records_state*>(w);
    if (int r = lines_scan(d, len, max_line_len, reinterpret_cast<uint64_t*>(static_cast<char*>(w) + 256), nullptr, 0, 1, 0, len, d_starts, d_text_len, lines_cap, d_st, s)) return r;
    fourmc_records_state st;
    HIP_TRY(hipMemcpyAsync(&st, d_st, sizeof st, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *lines = st.r.result;
    return FOURMC_OK;
}

int fourmc_gpu_debug_records_scan(const void* d, uint64_t len, uint8_t delim, uint64_t* d_starts, uint64_t starts_cap,
                                  int64_t* records, void* stream)
{
    if (!records || (len && !d)) { snprintf(g_err, sizeof g_err, "debug_records_scan: null pointer"); return FOURMC_EINVAL; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, 256 + records_cnt_bytes(len), &w)) return r;
    auto* d_st = static_cast<fourmc_records_state*>(w);
    if (int r = records_scan(d, len, delim, reinterpret_cast<uint64_t*>(static_cast<char*>(w) + 256), nullptr, 0, 1, 0, len, d_starts, starts_cap, d_st, s)) return r;
    fourmc_records_state st;
    HIP_TRY(hipMemcpyAsync(&st, d_st, sizeof st, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *records = st.r.result;
    return FOURMC_OK;
}
#endif

} // extern "C"
