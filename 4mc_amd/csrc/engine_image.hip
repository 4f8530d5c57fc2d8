// 4mc_amd/csrc/engine_image.hip — whole .4mc / .4mz file images in device memory (image.hip): one and many, the streaming writer and
// reader, and random access.
#include "engine_int.h"

// ------------------------------------------------------------------------ streaming image writer (image.hip)
// One device allocation per writer, made by begin and freed by finish / abort: the running state, the descriptors of one batch, the
// index (the absolute offset of every block header, then the running offset behind the last one), the carry slot and the staging.
// The carry slot sits in front of the staging, so a codec reading past the slot's end stays inside the allocation.
struct fourmc_image_writer {
    hipStream_t s;
    uint8_t* image;
    uint64_t cap;
    uint32_t magic;
    int codec, codec_level;
    uint32_t batch;                  // blocks per encode batch
    uint64_t max_blocks;             // the most blocks image_cap can hold (the index has one entry more)
    uint64_t total;                  // bytes appended so far
    uint32_t nblocks;                // blocks queued for encoding: the next one's number in the index
    uint32_t carry;                  // bytes of the incomplete block waiting in the carry slot
    int err;                         // the first failure: every later call returns it
    void* mem;
    fourmc_image_enc_summary* d_sum;
    fourmc_block* d_blk;
    uint64_t* d_idx;
    uint8_t* d_carry;
    uint8_t* d_stage;
};

// ------------------------------------------------------------------------ streaming image reader (image.hip)
// One device allocation per reader, made by begin and freed by finish / abort: the walk's state, the status, the descriptors and
// header offsets of one batch, the copy pieces of one walk and batch_blocks staging slots (64 bytes of slack behind the last one
// for the decoders' read-ahead).  A block cut by the end of a chunk waits in its own slot, so there is no separate carry slot.
struct fourmc_image_reader {
    hipStream_t s;
    uint8_t* dst;
    uint64_t cap;
    uint32_t magic;
    int codec;
    uint32_t batch;                  // blocks per decode batch
    uint64_t total;                  // bytes appended so far: N
    uint32_t pending;                // complete blocks waiting in the current batch
    bool final_;                     // the framing verdict is final: later appends only count
    int err;                         // the first failure: every later call returns it
    void* mem;
    fourmc_image_rd_state* d_st;
    fourmc_image_status* d_status;
    fourmc_block* d_desc;
    uint64_t* d_at;
    fourmc_image_piece* d_pc;
    uint8_t* d_stage;
};
namespace {

// One batch: the carry slot as block 0 when lead_len > 0, then m full blocks of src from src0; one container encode, the scan from
// the running offset, the pack at the offsets it wrote into the index.  A codec launch takes one source base and adds each block's
// 64-bit src_off to it, so the carry block shares the launch of the chunk's blocks: the base is the lower of the two addresses and
// both offsets count from there.  (Encoding the carry block alone costs a whole block's encode latency per append: see
// profiles/r09_image_writer.md.)
int writer_batch(fourmc_image_writer* w, const uint8_t* src, uint64_t src0, uint32_t m, uint32_t lead_len)
{
    hipStream_t s = w->s;
    const uint32_t lead = lead_len ? 1u : 0u;
    const uint8_t* base = !lead ? src : (!m || uintptr_t(w->d_carry) < uintptr_t(src)) ? w->d_carry : src;
    if (lead) HIP_TRY(fourmc_launch_image_wr_desc(w->d_blk, uint64_t(uintptr_t(w->d_carry) - uintptr_t(base)), 0, lead_len, 1, s));
    if (m) {
        HIP_TRY(fourmc_launch_image_wr_desc(w->d_blk + lead, uint64_t(uintptr_t(src) - uintptr_t(base)) + src0,
                                            uint64_t(lead) * FOURMC_BLOCKSIZE, uint64_t(m) * FOURMC_BLOCKSIZE, m, s));
    }
    if (int r = fourmc_gpu_4mc_encode_blocks(base, w->d_stage, w->d_blk, lead + m, w->codec, w->codec_level, s)) return r;
    HIP_TRY(fourmc_launch_image_wr_batch(w->image, w->d_blk, w->d_idx + w->nblocks, lead + m, w->d_stage, w->d_sum, s));
    w->nblocks += lead + m;
    return FOURMC_OK;
}

// The chunk after the capacity check: fill the carry slot; every complete block in batches; the rest into the carry slot.
int writer_append(fourmc_image_writer* w, const uint8_t* src, uint64_t bytes)
{
    hipStream_t s = w->s;
    uint64_t at = 0;
    uint32_t lead = 0;
    if (w->carry) {
        const uint64_t need = FOURMC_BLOCKSIZE - w->carry, take = bytes < need ? bytes : need;
        HIP_TRY(hipMemcpyAsync(w->d_carry + w->carry, src, take, hipMemcpyDeviceToDevice, s));
        at = take;
        if (take < need) { w->carry += uint32_t(take); return FOURMC_OK; }
        lead = FOURMC_BLOCKSIZE; w->carry = 0;
    }
    uint64_t full = (bytes - at) / FOURMC_BLOCKSIZE;
    while (lead || full) {
        const uint64_t room = w->batch - (lead ? 1u : 0u);
        const uint32_t m = uint32_t(full < room ? full : room);
        if (int r = writer_batch(w, src, at, m, lead)) return r;
        at += uint64_t(m) * FOURMC_BLOCKSIZE; full -= m; lead = 0;
    }
    if (at < bytes) {
        HIP_TRY(hipMemcpyAsync(w->d_carry, src + at, bytes - at, hipMemcpyDeviceToDevice, s));
        w->carry = uint32_t(bytes - at);
    }
    return FOURMC_OK;
}

// The carried tail as the last short block, the header / end mark / footer, one read-back of the running offset and the bad count.
int writer_finish(fourmc_image_writer* w, uint64_t* image_bytes)
{
    if (int r = ensure_device()) return r;
    hipStream_t s = w->s;
    if (w->carry) {
        if (int r = writer_batch(w, nullptr, 0, 0, w->carry)) return r;
        w->carry = 0;
    }
    HIP_TRY(fourmc_launch_image_wr_tail(w->image, w->d_idx, w->nblocks, w->magic, s));
    fourmc_image_enc_summary h;
    uint64_t end = 0;
    HIP_TRY(hipMemcpyAsync(&h, w->d_sum, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&end, w->d_idx + w->nblocks, sizeof end, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h.bad_blocks) { snprintf(g_err, sizeof g_err, "image_writer_finish: %u blocks with an encoder result outside [1, src_len]", h.bad_blocks); return FOURMC_EINVAL; }
    *image_bytes = end + 12 + 20 + 4ull * w->nblocks;
    return FOURMC_OK;
}

// Work may still be queued on the buffers unless the stream has just been synchronized.
void writer_free(fourmc_image_writer* w, bool synced)
{
    if (w->mem) {
        if (!synced) (void)hipStreamSynchronize(w->s);
        (void)hipFree(w->mem);
        (void)hipGetLastError();
    }
    delete w;
}

// the current batch: the container decode from staging (XXH32 check, then the codec), then the fold into the running verdict
int reader_decode(fourmc_image_reader* r)
{
    if (!r->pending) return FOURMC_OK;
    if (int e = fourmc_gpu_4mc_decode_blocks(r->d_stage, r->dst, r->d_desc, r->pending, r->codec, r->s)) return e;
    HIP_TRY(fourmc_launch_image_rd_fold(r->d_desc, r->d_at, r->pending, r->d_st, r->s));
    r->pending = 0;
    return FOURMC_OK;
}

// One walk per batch the chunk fills, each read back once: the gather of its pieces, and the decode when its batch is full.
int reader_append(fourmc_image_reader* r, const uint8_t* chunk, uint64_t bytes)
{
    uint64_t at = 0;
    for (;;) {
        HIP_TRY(fourmc_launch_image_rd_walk(chunk, bytes, at, r->d_st, r->magic, r->cap, r->batch, r->d_stage, r->d_desc, r->d_at,
                                            r->d_pc, r->s));
        struct { uint64_t cpos; uint32_t batch_n, npieces, max_piece, final_; } h;
        static_assert(sizeof h == 24 && offsetof(fourmc_image_rd_state, final_) == 20, "the read-back head of the walk's state");
        HIP_TRY(hipMemcpyAsync(&h, r->d_st, sizeof h, hipMemcpyDeviceToHost, r->s));
        HIP_TRY(hipStreamSynchronize(r->s));
        HIP_TRY(fourmc_launch_image_rd_gather(r->d_pc, h.npieces, h.max_piece, r->s));
        r->pending = h.batch_n;
        r->final_ = h.final_ != 0;
        if (r->pending == r->batch) { if (int e = reader_decode(r)) return e; }
        if (r->final_ || h.cpos >= bytes) return FOURMC_OK;
        at = h.cpos;
    }
}

int reader_finish(fourmc_image_reader* r, fourmc_image_status* status)
{
    if (int e = ensure_device()) return e;
    if (int e = reader_decode(r)) return e;
    HIP_TRY(fourmc_launch_image_rd_finish(r->d_st, r->total, r->cap, r->d_status, r->s));
    HIP_TRY(hipMemcpyAsync(status, r->d_status, sizeof *status, hipMemcpyDeviceToHost, r->s));
    HIP_TRY(hipStreamSynchronize(r->s));
    return FOURMC_OK;
}

void reader_free(fourmc_image_reader* r, bool synced)
{
    if (r->mem) {
        if (!synced) (void)hipStreamSynchronize(r->s);
        (void)hipFree(r->mem);
        (void)hipGetLastError();
    }
    delete r;
}

int image_args(const void* d_image, uint64_t image_bytes, const char* who)
{
    if (image_bytes && !d_image) { snprintf(g_err, sizeof g_err, "%s: null image", who); return FOURMC_EINVAL; }
    return FOURMC_OK;
}

} // namespace

// ---- what engine_int.h declares of this file
int image_index_count(WsLease& ws, hipStream_t s, const void* d_image, uint64_t image_bytes, fourmc_image_index_dev* out)
{
    void* w = nullptr;
    if (int r = ws.get(s, kIdxBytes, &w)) return r;
    auto* d_idx = static_cast<fourmc_image_index_dev*>(w);
    HIP_TRY(fourmc_launch_image_index(d_image, image_bytes, d_idx, nullptr, 0, s));
    HIP_TRY(hipMemcpyAsync(out, d_idx, sizeof *out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FOURMC_OK;
}
int image_codec(const fourmc_image_index_dev& idx) { return idx.info.is_zstd ? FOURMC_CODEC_ZSTD : FOURMC_CODEC_LZ4_FAST; }

extern "C" {

// ------------------------------------------------------------------------ whole file images (image.hip)
uint64_t fourmc_gpu_image_bound(uint64_t src_bytes)
{
    const uint64_t n = (src_bytes + FOURMC_BLOCKSIZE - 1) / FOURMC_BLOCKSIZE;
    return 12 + 12 * n + src_bytes + 12 + 20 + 4 * n;
}

// Descriptors from the size, the container encode (codec + XXH32, fourmc_gpu_4mc_encode_blocks) into 4 MiB staging slots, the
// scan into image offsets, the pack, the header / end mark / footer; one read-back of the image size.
int fourmc_gpu_image_compress(const void* d_src, uint64_t src_bytes, void* d_image, uint64_t image_cap,
                              uint64_t* image_bytes, uint32_t magic, int level, void* stream)
{
    if (int r = ensure_device()) return r;
    if (magic != FOURMC_MAGIC_4MC && magic != FOURMC_MAGIC_4MZ) { snprintf(g_err, sizeof g_err, "magic 0x%08x is neither 4mc nor 4mz", magic); return FOURMC_EINVAL; }
    if (!image_bytes || !d_image || (src_bytes && !d_src)) { snprintf(g_err, sizeof g_err, "image_compress: null pointer"); return FOURMC_EINVAL; }
    const uint64_t n64 = (src_bytes + FOURMC_BLOCKSIZE - 1) / FOURMC_BLOCKSIZE;
    if (n64 > 0x3FFFFFFFull) { snprintf(g_err, sizeof g_err, "image_compress: %llu blocks", (unsigned long long)n64); return FOURMC_EINVAL; }
    const uint32_t n = uint32_t(n64);
    if (image_cap < fourmc_gpu_image_bound(src_bytes)) {
        snprintf(g_err, sizeof g_err, "image capacity %llu below the bound %llu", (unsigned long long)image_cap,
                 (unsigned long long)fourmc_gpu_image_bound(src_bytes));
        return FOURMC_EINVAL;
    }
    int codec_level = 0;
    const int codec = fourmc_level_codec(magic, level, &codec_level);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t o_off = align256(sizeof(fourmc_image_enc_summary)), o_blk = o_off + align256((size_t(n) + 1) * 8);
    const size_t o_stage = o_blk + align256(size_t(n) * sizeof(fourmc_block));
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, o_stage + size_t(n) * FOURMC_BLOCKSIZE, &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_sum = reinterpret_cast<fourmc_image_enc_summary*>(base);
    auto* d_off = reinterpret_cast<uint64_t*>(base + o_off);
    auto* d_blk = reinterpret_cast<fourmc_block*>(base + o_blk);
    void* d_stage = base + o_stage;
    HIP_TRY(fourmc_launch_image_enc_desc(d_blk, src_bytes, n, s));
    if (n) { if (int r = fourmc_gpu_4mc_encode_blocks(d_src, d_stage, d_blk, n, codec, codec_level, s)) return r; }
    HIP_TRY(fourmc_launch_image_enc_frame(d_image, d_blk, d_off, n, magic, d_stage, d_sum, s));
    fourmc_image_enc_summary h;
    HIP_TRY(hipMemcpyAsync(&h, d_sum, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h.bad_blocks) { snprintf(g_err, sizeof g_err, "image_compress: %u blocks with an encoder result outside [1, src_len]", h.bad_blocks); return FOURMC_EINVAL; }
    *image_bytes = h.image_bytes;
    return FOURMC_OK;
}

// Many images with one call.  Every size is known on the host, so the argument loop lays out the tables: image i owns descriptors
// [first, first + nblocks) and a run of staging slots from stage_off, each block's slot its src_len rounded up to 256 bytes (only an
// image's last block is short, so the image's run is its src_bytes rounded up and block b's slot starts b * 4 MiB into it).
// Workspace (g_img_ws), one lease: the results, the plans, the end offsets, the dense offset table, the descriptors, the staging and
// kImagesStageSlack bytes behind it.  One upload (the plans), one container encode, one pack, one read-back (the results).
int fourmc_gpu_images_compress(const void* d_src, uint64_t src_total, void* d_images, uint64_t images_bytes,
                               uint32_t magic, int level, fourmc_image_enc_item* items, uint32_t n, void* stream)
{
    if (magic != FOURMC_MAGIC_4MC && magic != FOURMC_MAGIC_4MZ) { snprintf(g_err, sizeof g_err, "magic 0x%08x is neither 4mc nor 4mz", magic); return FOURMC_EINVAL; }
    if (n == 0) return FOURMC_OK;
    if (!items) { snprintf(g_err, sizeof g_err, "images_compress: null items"); return FOURMC_EINVAL; }
    if (!d_images) { snprintf(g_err, sizeof g_err, "images_compress: null images"); return FOURMC_EINVAL; }
    std::vector<fourmc_image_enc_plan> plans(n);
    uint64_t nb64 = 0, stage = 0;
    {
        std::vector<std::pair<uint64_t, uint64_t>> d(n);
        for (uint32_t i = 0; i < n; i++) {
            const fourmc_image_enc_item& it = items[i];
            if (it.src_bytes && !d_src) { snprintf(g_err, sizeof g_err, "images_compress: null source"); return FOURMC_EINVAL; }
            if (span_outside(it.src_off, it.src_bytes, src_total)) return source_beyond("images_compress", "image", i, src_total);
            const uint64_t k = it.src_bytes / FOURMC_BLOCKSIZE + (it.src_bytes % FOURMC_BLOCKSIZE ? 1 : 0);
            if (k > 0x3FFFFFFFull) { snprintf(g_err, sizeof g_err, "images_compress: image %u has %llu blocks", i, (unsigned long long)k); return FOURMC_EINVAL; }
            if (span_outside(it.image_off, it.image_cap, images_bytes)) return region_beyond("images_compress", "image", i, images_bytes);
            if (it.image_cap < fourmc_gpu_image_bound(it.src_bytes)) {
                snprintf(g_err, sizeof g_err, "images_compress: image %u: capacity %llu below the bound %llu", i, (unsigned long long)it.image_cap,
                         (unsigned long long)fourmc_gpu_image_bound(it.src_bytes));
                return FOURMC_EINVAL;
            }
            d[i] = { it.image_off, it.image_off + it.image_cap };
            fourmc_image_enc_plan& pl = plans[i];
            pl.src_off = it.src_off; pl.src_bytes = it.src_bytes; pl.image_off = it.image_off; pl.stage_off = stage;
            pl.first = uint32_t(nb64 > 0x7FFFFFFFull ? 0 : nb64); pl.nblocks = uint32_t(k);
            nb64 += k; stage += (it.src_bytes + 255) & ~uint64_t(255);
        }
        if (int r = regions_overlap("images_compress", "image regions", d)) return r;
    }
    if (nb64 > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "images_compress: %llu blocks", (unsigned long long)nb64); return FOURMC_EUNSUP; }
    if (int r = ensure_device()) return r;
    const uint32_t nb = uint32_t(nb64);
    int codec_level = 0;
    const int codec = fourmc_level_codec(magic, level, &codec_level);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t o_plan = align256(size_t(n) * sizeof(fourmc_image_enc_result)), o_end = o_plan + align256(size_t(n) * sizeof(fourmc_image_enc_plan));
    const size_t o_off = o_end + align256(size_t(n) * 8), o_blk = o_off + align256(size_t(nb) * 8);
    const size_t o_stage = o_blk + align256(size_t(nb) * sizeof(fourmc_block));
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, o_stage + size_t(stage) + kImagesStageSlack, &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_res = reinterpret_cast<fourmc_image_enc_result*>(base);
    auto* d_plans = reinterpret_cast<fourmc_image_enc_plan*>(base + o_plan);
    auto* d_end = reinterpret_cast<uint64_t*>(base + o_end);
    auto* d_off = reinterpret_cast<uint64_t*>(base + o_off);
    auto* d_blk = reinterpret_cast<fourmc_block*>(base + o_blk);
    void* d_stage = base + o_stage;
    HIP_TRY(hipMemcpyAsync(d_plans, plans.data(), size_t(n) * sizeof(fourmc_image_enc_plan), hipMemcpyHostToDevice, s));
    HIP_TRY(fourmc_launch_images_enc_desc(d_plans, n, d_blk, nb, s));
    if (nb) { if (int r = fourmc_gpu_4mc_encode_blocks(d_src, d_stage, d_blk, nb, codec, codec_level, s)) return r; }
    HIP_TRY(fourmc_launch_images_enc_frame(d_images, d_plans, n, d_blk, nb, d_off, d_end, magic, d_stage, d_res, s));
    std::vector<fourmc_image_enc_result> back(n);
    HIP_TRY(hipMemcpyAsync(back.data(), d_res, size_t(n) * sizeof(fourmc_image_enc_result), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t bad = 0;
    for (uint32_t i = 0; i < n; i++) bad += back[i].bad_blocks;
    if (bad) { snprintf(g_err, sizeof g_err, "images_compress: %llu blocks with an encoder result outside [1, src_len]", (unsigned long long)bad); return FOURMC_EINVAL; }
    for (uint32_t i = 0; i < n; i++) items[i].image_bytes = back[i].image_bytes;
    return FOURMC_OK;
}

int fourmc_gpu_image_writer_begin(fourmc_image_writer** out, void* d_image, uint64_t image_cap, uint32_t magic, int level,
                                  uint32_t batch_blocks, void* stream)
{
    if (!out) { snprintf(g_err, sizeof g_err, "image_writer_begin: null writer"); return FOURMC_EINVAL; }
    *out = nullptr;
    if (magic != FOURMC_MAGIC_4MC && magic != FOURMC_MAGIC_4MZ) { snprintf(g_err, sizeof g_err, "magic 0x%08x is neither 4mc nor 4mz", magic); return FOURMC_EINVAL; }
    if (!d_image) { snprintf(g_err, sizeof g_err, "image_writer_begin: null image"); return FOURMC_EINVAL; }
    if (image_cap < fourmc_gpu_image_bound(0)) {
        snprintf(g_err, sizeof g_err, "image capacity %llu below the bound %llu of an empty input", (unsigned long long)image_cap,
                 (unsigned long long)fourmc_gpu_image_bound(0));
        return FOURMC_EINVAL;
    }
    if (int r = ensure_device()) return r;
    // n blocks need at least bound((n-1) * 4 MiB + 1) = 45 + 16 n + (n-1) * 4 MiB bytes of image
    uint64_t max_blocks = (image_cap - 45 + FOURMC_BLOCKSIZE) / (FOURMC_BLOCKSIZE + 16);
    if (max_blocks > 0x3FFFFFFFull) max_blocks = 0x3FFFFFFFull;
    uint64_t batch = batch_blocks ? batch_blocks : 512;
    if (batch > max_blocks) batch = max_blocks ? max_blocks : 1;
    const size_t o_blk = align256(sizeof(fourmc_image_enc_summary)), o_idx = o_blk + align256(size_t(batch) * sizeof(fourmc_block));
    const size_t o_carry = o_idx + align256((size_t(max_blocks) + 1) * 8), o_stage = o_carry + FOURMC_BLOCKSIZE;
    const size_t bytes = o_stage + size_t(batch) * FOURMC_BLOCKSIZE;
    auto* w = new fourmc_image_writer();
    w->s = static_cast<hipStream_t>(stream);
    w->image = static_cast<uint8_t*>(d_image); w->cap = image_cap; w->magic = magic;
    w->codec = fourmc_level_codec(magic, level, &w->codec_level);
    w->batch = uint32_t(batch); w->max_blocks = max_blocks;
    const hipError_t me = hipMalloc(&w->mem, bytes);
    if (me != hipSuccess) {
        (void)hipGetLastError(); w->mem = nullptr;
        delete w;
        if (me == hipErrorOutOfMemory) { snprintf(g_err, sizeof g_err, "hipMalloc(%zu bytes of image writer): out of memory", bytes); return FOURMC_ENOMEM; }
        return fail_hip(me, "hipMalloc(image writer)");
    }
    char* base = static_cast<char*>(w->mem);
    w->d_sum = reinterpret_cast<fourmc_image_enc_summary*>(base);
    w->d_blk = reinterpret_cast<fourmc_block*>(base + o_blk);
    w->d_idx = reinterpret_cast<uint64_t*>(base + o_idx);
    w->d_carry = reinterpret_cast<uint8_t*>(base + o_carry);
    w->d_stage = reinterpret_cast<uint8_t*>(base + o_stage);
    // no bad result yet; the running offset starts behind the 12-byte file header
    hipError_t e = hipMemsetAsync(w->d_sum, 0, sizeof(fourmc_image_enc_summary), w->s);
    if (e == hipSuccess) e = hipMemsetAsync(w->d_idx, 0, 8, w->s);
    if (e == hipSuccess) e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w->d_idx), 12, 1, w->s);
    if (e != hipSuccess) { const int r = fail_hip(e, "image_writer_begin: state"); writer_free(w, false); return r; }
    *out = w;
    return FOURMC_OK;
}

int fourmc_gpu_image_writer_append(fourmc_image_writer* w, const void* d_src, uint64_t bytes)
{
    if (!w) { snprintf(g_err, sizeof g_err, "image_writer_append: null writer"); return FOURMC_EINVAL; }
    if (w->err) { snprintf(g_err, sizeof g_err, "image_writer_append: the writer failed earlier (%d)", w->err); return w->err; }
    if (bytes && !d_src) { snprintf(g_err, sizeof g_err, "image_writer_append: null source"); return w->err = FOURMC_EINVAL; }
    // the capacity refusal: the host knows the total exactly; nothing is queued and the writer stays usable
    const uint64_t total = w->total + bytes;
    if (total < w->total || (total + FOURMC_BLOCKSIZE - 1) / FOURMC_BLOCKSIZE > w->max_blocks || fourmc_gpu_image_bound(total) > w->cap) {
        snprintf(g_err, sizeof g_err, "image_writer_append: %llu bytes after %llu would pass the image capacity %llu",
                 (unsigned long long)bytes, (unsigned long long)w->total, (unsigned long long)w->cap);
        return FOURMC_EINVAL;
    }
    if (!bytes) return FOURMC_OK;
    int r = ensure_device();
    if (!r) r = writer_append(w, static_cast<const uint8_t*>(d_src), bytes);
    if (r) return w->err = r;
    w->total = total;
    return FOURMC_OK;
}

int fourmc_gpu_image_writer_finish(fourmc_image_writer* w, uint64_t* image_bytes)
{
    if (!w) { snprintf(g_err, sizeof g_err, "image_writer_finish: null writer"); return FOURMC_EINVAL; }
    int r = w->err;
    if (r) snprintf(g_err, sizeof g_err, "image_writer_finish: the writer failed earlier (%d)", r);
    else if (!image_bytes) { snprintf(g_err, sizeof g_err, "image_writer_finish: null image_bytes"); r = FOURMC_EINVAL; }
    else r = writer_finish(w, image_bytes);
    writer_free(w, r == FOURMC_OK);
    return r;
}

void fourmc_gpu_image_writer_abort(fourmc_image_writer* w)
{
    if (w) writer_free(w, false);
}

int fourmc_gpu_image_reader_begin(fourmc_image_reader** out, void* d_dst, uint64_t dst_cap, uint32_t magic, uint32_t batch_blocks,
                                  void* stream)
{
    if (!out) { snprintf(g_err, sizeof g_err, "image_reader_begin: null reader"); return FOURMC_EINVAL; }
    *out = nullptr;
    if (magic != FOURMC_MAGIC_4MC && magic != FOURMC_MAGIC_4MZ) { snprintf(g_err, sizeof g_err, "magic 0x%08x is neither 4mc nor 4mz", magic); return FOURMC_EINVAL; }
    if (!d_dst) { snprintf(g_err, sizeof g_err, "image_reader_begin: null destination"); return FOURMC_EINVAL; }
    if (int r = ensure_device()) return r;
    const uint32_t batch = batch_blocks ? batch_blocks : 512;
    const size_t o_status = align256(sizeof(fourmc_image_rd_state)), o_desc = o_status + align256(sizeof(fourmc_image_status));
    const size_t o_at = o_desc + align256(size_t(batch) * sizeof(fourmc_block)), o_pc = o_at + align256(size_t(batch) * 8);
    const size_t o_stage = o_pc + align256((size_t(batch) + 1) * sizeof(fourmc_image_piece));
    const size_t bytes = o_stage + size_t(batch) * FOURMC_BLOCKSIZE + 256;
    auto* r = new fourmc_image_reader();
    r->s = static_cast<hipStream_t>(stream);
    r->dst = static_cast<uint8_t*>(d_dst); r->cap = dst_cap; r->magic = magic;
    r->codec = magic == FOURMC_MAGIC_4MZ ? FOURMC_CODEC_ZSTD : FOURMC_CODEC_LZ4_FAST;
    r->batch = batch;
    const hipError_t me = hipMalloc(&r->mem, bytes);
    if (me != hipSuccess) {
        (void)hipGetLastError(); r->mem = nullptr;
        delete r;
        if (me == hipErrorOutOfMemory) { snprintf(g_err, sizeof g_err, "hipMalloc(%zu bytes of image reader): out of memory", bytes); return FOURMC_ENOMEM; }
        return fail_hip(me, "hipMalloc(image reader)");
    }
    char* base = static_cast<char*>(r->mem);
    r->d_st = reinterpret_cast<fourmc_image_rd_state*>(base);
    r->d_status = reinterpret_cast<fourmc_image_status*>(base + o_status);
    r->d_desc = reinterpret_cast<fourmc_block*>(base + o_desc);
    r->d_at = reinterpret_cast<uint64_t*>(base + o_at);
    r->d_pc = reinterpret_cast<fourmc_image_piece*>(base + o_pc);
    r->d_stage = reinterpret_cast<uint8_t*>(base + o_stage);
    // the walk starts at the file header of the first stream, nothing counted
    const hipError_t e = hipMemsetAsync(r->d_st, 0, sizeof(fourmc_image_rd_state), r->s);
    if (e != hipSuccess) { const int rr = fail_hip(e, "image_reader_begin: state"); reader_free(r, false); return rr; }
    *out = r;
    return FOURMC_OK;
}

int fourmc_gpu_image_reader_append(fourmc_image_reader* r, const void* d_chunk, uint64_t bytes)
{
    if (!r) { snprintf(g_err, sizeof g_err, "image_reader_append: null reader"); return FOURMC_EINVAL; }
    if (r->err) { snprintf(g_err, sizeof g_err, "image_reader_append: the reader failed earlier (%d)", r->err); return r->err; }
    if (bytes && !d_chunk) { snprintf(g_err, sizeof g_err, "image_reader_append: null chunk"); return FOURMC_EINVAL; }
    if (r->total + bytes < r->total) { snprintf(g_err, sizeof g_err, "image_reader_append: image length overflows"); return FOURMC_EINVAL; }
    if (bytes && !r->final_) {                       // once the verdict is final, appends only count toward N
        int e = ensure_device();
        if (!e) e = reader_append(r, static_cast<const uint8_t*>(d_chunk), bytes);
        if (e) return r->err = e;
    }
    r->total += bytes;
    return FOURMC_OK;
}

int fourmc_gpu_image_reader_finish(fourmc_image_reader* r, fourmc_image_status* status)
{
    if (!r) { snprintf(g_err, sizeof g_err, "image_reader_finish: null reader"); return FOURMC_EINVAL; }
    int e = r->err;
    if (e) snprintf(g_err, sizeof g_err, "image_reader_finish: the reader failed earlier (%d)", e);
    else if (!status) { snprintf(g_err, sizeof g_err, "image_reader_finish: null status"); e = FOURMC_EINVAL; }
    else e = reader_finish(r, status);
    reader_free(r, e == FOURMC_OK);
    return e;
}

void fourmc_gpu_image_reader_abort(fourmc_image_reader* r)
{
    if (r) reader_free(r, false);
}

const char* fourmc_gpu_image_reason_text(int reason)
{
    switch (reason) {                       // fourmc_file.c: decode_stream, the writer thread (wjob_main)
        case FOURMC_IMG_OK:                    return "";
        case FOURMC_IMG_MAGIC_UNREADABLE:      return "Unrecognized header : Magic Number unreadable";
        case FOURMC_IMG_NOT_4MC:               return "Unrecognized header : not a 4mc file";
        case FOURMC_IMG_HEADER_UNREADABLE:     return "Unreadable header";
        case FOURMC_IMG_VERSION:               return "Wrong version number";
        case FOURMC_IMG_HEADER_CHECKSUM:       return "Wrong header checksum";
        case FOURMC_IMG_BLOCK_SIZE_UNREADABLE: return "Read error : cannot read next block size";
        case FOURMC_IMG_CSIZE_BEYOND:          return "Read error: block size beyond 4MB limit";
        case FOURMC_IMG_DATA_UNREADABLE:       return "Read error : cannot read data block";
        case FOURMC_IMG_USIZE_BEYOND:          return "Read error: uncompressed block size beyond 4MB limit";
        case FOURMC_IMG_BLOCK_CHECKSUM:        return "Error : invalid block checksum detected";
        case FOURMC_IMG_CORRUPT:               return "Decoding Failed ! Corrupted input detected !";
        case FOURMC_IMG_FOOTER_UNREADABLE:     return "Unreadable footer";
        case FOURMC_IMG_FOOTER_SHORT:          return "Read error : cannot read footer";
        case FOURMC_IMG_FOOTER_CHECKSUM:       return "Error : invalid footer checksum detected";
        case FOURMC_IMG_FOOTER_VERSION:        return "Read error : unsupported footer version";
        case FOURMC_IMG_DST_SMALL:             return "Destination buffer too small";
        default:                               return "unknown";
    }
}

// images parsed so far by the fast path and by the walk (fourmc_gpu_image_parse_stats)
static std::atomic<unsigned long long> g_img_fast{0}, g_img_walk{0};
void fourmc_gpu_image_parse_stats(unsigned long long* fast, unsigned long long* walk)
{
    if (fast) *fast = g_img_fast.load();
    if (walk) *walk = g_img_walk.load();
}

// FOURMC_IMAGE_PARSE=walk: every image takes the file-order walk (test knob; the results are the same).  Read at every call, so
// that one process can run an image under both parsers.
static bool image_walk_forced()
{
    const char* e = getenv("FOURMC_IMAGE_PARSE");
    return e && !strcmp(e, "walk");
}

// Parse (fast path, else the walk) into a summary read back once; descriptors for exactly that many blocks; the container decode
// (XXH32 verify + codec, fourmc_gpu_4mc_decode_blocks); the reduction into the status, read back.
int fourmc_gpu_image_decompress(const void* d_image, uint64_t image_bytes, void* d_dst, uint64_t dst_cap,
                                uint32_t magic, fourmc_image_status* status, void* stream)
{
    if (int r = ensure_device()) return r;
    if (magic != FOURMC_MAGIC_4MC && magic != FOURMC_MAGIC_4MZ) { snprintf(g_err, sizeof g_err, "magic 0x%08x is neither 4mc nor 4mz", magic); return FOURMC_EINVAL; }
    if (!status || (image_bytes && !d_image)) { snprintf(g_err, sizeof g_err, "image_decompress: null pointer"); return FOURMC_EINVAL; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t o_st = align256(sizeof(fourmc_image_parse)), o_blk = o_st + align256(sizeof(fourmc_image_status));
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, o_blk, &w)) return r;
    auto* d_ps = static_cast<fourmc_image_parse*>(w);
    HIP_TRY(hipMemsetAsync(d_ps, 0, sizeof(fourmc_image_parse), s));
    const bool walk_only = image_walk_forced();
    HIP_TRY(fourmc_launch_image_parse(d_image, image_bytes, magic, !walk_only, 1, d_ps, nullptr, s));
    fourmc_image_parse ps;
    HIP_TRY(hipMemcpyAsync(&ps, d_ps, sizeof ps, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    (ps.fast ? g_img_fast : g_img_walk)++;
    memset(status, 0, sizeof *status);
    status->total_bytes = ps.total; status->streams = ps.streams;
    if (ps.nblocks > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "image_decompress: %llu blocks", (unsigned long long)ps.nblocks); return FOURMC_EUNSUP; }
    const uint32_t n = uint32_t(ps.nblocks);
    if (!d_dst) {                                                        // size query: the framing verdict
        status->blocks = n; status->reason = ps.reason; status->exit_code = fourmc_image_exit_code(ps.reason); status->fail_offset = ps.fail_offset;
        return FOURMC_OK;
    }
    if (ps.total > dst_cap) {
        status->reason = FOURMC_IMG_DST_SMALL; status->exit_code = fourmc_image_exit_code(FOURMC_IMG_DST_SMALL); status->fail_offset = 0;
        return FOURMC_OK;
    }
    if (int r = ws.get(s, o_blk + size_t(n) * sizeof(fourmc_block), &w)) return r;   // may move the buffer: the summary goes up again
    char* base = static_cast<char*>(w);
    d_ps = reinterpret_cast<fourmc_image_parse*>(base);
    auto* d_st = reinterpret_cast<fourmc_image_status*>(base + o_st);
    auto* d_blk = reinterpret_cast<fourmc_block*>(base + o_blk);
    HIP_TRY(hipMemcpyAsync(d_ps, &ps, sizeof ps, hipMemcpyHostToDevice, s));
    if (n) {
        HIP_TRY(fourmc_launch_image_parse(d_image, image_bytes, magic, ps.fast, !ps.fast, d_ps, d_blk, s));
        if (int r = fourmc_gpu_4mc_decode_blocks(d_image, d_dst, d_blk, n, magic == FOURMC_MAGIC_4MZ ? FOURMC_CODEC_ZSTD : FOURMC_CODEC_LZ4_FAST, s)) return r;
    }
    HIP_TRY(fourmc_launch_image_reduce(d_blk, n, d_ps, d_st, s));
    HIP_TRY(hipMemcpyAsync(status, d_st, sizeof *status, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FOURMC_OK;
}

// Many images with one call.  Workspace (g_img_ws): the summary, the items, one parse and one first-descriptor number per image,
// the statuses, then - sized after the first read-back - the descriptors of every image.  When that grows the buffer its contents
// are gone: the items go up again and the count parse and the plan run again before the fill.
int fourmc_gpu_images_decompress(const void* d_images, uint64_t images_bytes, void* d_dst, uint64_t dst_bytes,
                                 uint32_t magic, fourmc_image_item* items, uint32_t n, void* stream)
{
    if (magic != FOURMC_MAGIC_4MC && magic != FOURMC_MAGIC_4MZ) { snprintf(g_err, sizeof g_err, "magic 0x%08x is neither 4mc nor 4mz", magic); return FOURMC_EINVAL; }
    if (n == 0) return FOURMC_OK;
    if (int r = decode_items_args("images_decompress", "image", "images", d_images, images_bytes, d_dst, dst_bytes, items, n)) return r;
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool query = !d_dst;
    const size_t o_items = align256(sizeof(fourmc_images_summary)), o_ps = o_items + align256(size_t(n) * sizeof(fourmc_image_item));
    const size_t o_first = o_ps + align256(size_t(n) * sizeof(fourmc_image_parse)), o_st = o_first + align256(size_t(n) * 8);
    const size_t o_blk = o_st + align256(size_t(n) * sizeof(fourmc_image_status));
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, o_blk, &w)) return r;
    char* base = static_cast<char*>(w);
    const bool try_fast = !image_walk_forced();
    // the items, the count parse and the plan; again after the buffer has grown
    auto count_and_plan = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(base + o_items, items, size_t(n) * sizeof(fourmc_image_item), hipMemcpyHostToDevice, s));
        HIP_TRY(fourmc_launch_images_parse(d_images, reinterpret_cast<fourmc_image_item*>(base + o_items), n, magic, try_fast,
                                           reinterpret_cast<fourmc_image_parse*>(base + o_ps), nullptr, nullptr, s));
        HIP_TRY(fourmc_launch_images_plan(reinterpret_cast<fourmc_image_item*>(base + o_items), n, reinterpret_cast<fourmc_image_parse*>(base + o_ps),
                                          query, reinterpret_cast<uint64_t*>(base + o_first), reinterpret_cast<fourmc_images_summary*>(base),
                                          reinterpret_cast<fourmc_image_status*>(base + o_st), s));
        return FOURMC_OK;
    };
    if (int r = count_and_plan()) return r;
    fourmc_images_summary sum;
    std::vector<fourmc_image_status> back(n);
    HIP_TRY(hipMemcpyAsync(&sum, base, sizeof sum, hipMemcpyDeviceToHost, s));
    if (query) HIP_TRY(hipMemcpyAsync(back.data(), base + o_st, size_t(n) * sizeof(fourmc_image_status), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    g_img_fast += sum.fast; g_img_walk += sum.walk;
    if (sum.nblocks > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "images_decompress: %llu blocks", (unsigned long long)sum.nblocks); return FOURMC_EUNSUP; }
    if (!query) {
        const uint32_t nb = uint32_t(sum.nblocks);
        const size_t had = ws.cap();
        if (int r = ws.get(s, o_blk + size_t(nb) * sizeof(fourmc_block), &w)) return r;
        base = static_cast<char*>(w);
        if (ws.cap() != had) if (int r = count_and_plan()) return r;
        auto* d_items = reinterpret_cast<fourmc_image_item*>(base + o_items);
        auto* d_ps = reinterpret_cast<fourmc_image_parse*>(base + o_ps);
        auto* d_first = reinterpret_cast<uint64_t*>(base + o_first);
        auto* d_blk = reinterpret_cast<fourmc_block*>(base + o_blk);
        if (nb) {
            HIP_TRY(fourmc_launch_images_parse(d_images, d_items, n, magic, try_fast, d_ps, d_first, d_blk, s));
            if (int r = fourmc_gpu_4mc_decode_blocks(d_images, d_dst, d_blk, nb, magic == FOURMC_MAGIC_4MZ ? FOURMC_CODEC_ZSTD : FOURMC_CODEC_LZ4_FAST, s)) return r;
        }
        HIP_TRY(fourmc_launch_images_reduce(d_items, n, d_ps, d_first, d_blk, reinterpret_cast<fourmc_image_status*>(base + o_st), s));
        HIP_TRY(hipMemcpyAsync(back.data(), base + o_st, size_t(n) * sizeof(fourmc_image_status), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (uint32_t i = 0; i < n; i++) items[i].status = back[i];
    return FOURMC_OK;
}

// ------------------------------------------------------------------------ random access into images (image.hip)
// Workspace of the three calls (g_img_ws): the index summary, then - sized after its read-back - the entries and what the call
// needs besides.  A buffer that grows loses its contents: everything after the first read-back is recomputed on the device.

// One wave reads the footer and every block header; one read-back.
int fourmc_gpu_image_index(const void* d_image, uint64_t image_bytes, fourmc_image_entry* d_entries, uint64_t entries_cap,
                           fourmc_image_index_info* info, void* stream)
{
    if (!info) { snprintf(g_err, sizeof g_err, "image_index: null info"); return FOURMC_EINVAL; }
    if (int r = image_args(d_image, image_bytes, "image_index")) return r;
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, kIdxBytes, &w)) return r;
    auto* d_idx = static_cast<fourmc_image_index_dev*>(w);
    HIP_TRY(fourmc_launch_image_index(d_image, image_bytes, d_idx, d_entries, d_entries ? entries_cap : 0, s));
    fourmc_image_index_dev h;
    HIP_TRY(hipMemcpyAsync(&h, d_idx, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *info = h.info;
    return FOURMC_OK;
}

// The summary (first read-back) gives n; the entries, the range's checks and descriptors, ONE container decode straight into d_dst,
// the reduction; the result (second read-back).
int fourmc_gpu_image_decode_blocks(const void* d_image, uint64_t image_bytes, uint32_t first, uint32_t count,
                                   void* d_dst, uint64_t dst_cap, int64_t* result, void* stream)
{
    if (!result) { snprintf(g_err, sizeof g_err, "image_decode_blocks: null result"); return FOURMC_EINVAL; }
    if (int r = image_args(d_image, image_bytes, "image_decode_blocks")) return r;
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsLease ws(&g_img_ws);
    fourmc_image_index_dev idx;
    if (int r = image_index_count(ws, s, d_image, image_bytes, &idx)) return r;
    const int64_t n = idx.info.nblocks;
    if (n < 0) { *result = n; return FOURMC_OK; }                          // fourmc_file_decode_blocks' order
    if (uint64_t(first) + count > uint64_t(n)) { *result = -3; return FOURMC_OK; }
    if (count == 0) { *result = 0; return FOURMC_OK; }
    const size_t o_span = kIdxBytes, o_res = o_span + 256, o_ent = o_res + 256;
    const size_t o_desc = o_ent + align256(size_t(n) * sizeof(fourmc_image_entry));
    void* w = nullptr;
    if (int r = ws.get(s, o_desc + size_t(count) * sizeof(fourmc_block), &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_idx = reinterpret_cast<fourmc_image_index_dev*>(base);
    auto* d_span = reinterpret_cast<fourmc_image_span*>(base + o_span);
    auto* d_res = reinterpret_cast<int64_t*>(base + o_res);
    auto* d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
    auto* d_desc = reinterpret_cast<fourmc_block*>(base + o_desc);
    HIP_TRY(fourmc_launch_image_index(d_image, image_bytes, d_idx, d_ent, uint64_t(n), s));
    HIP_TRY(fourmc_launch_image_span(d_ent, d_idx, image_bytes, first, count, dst_cap, d_span, d_desc, s));
    if (int r = fourmc_gpu_4mc_decode_blocks(d_image, d_dst, d_desc, count, image_codec(idx), s)) return r;
    HIP_TRY(fourmc_launch_image_span_reduce(d_desc, count, d_span, d_res, s));
    HIP_TRY(hipMemcpyAsync(result, d_res, sizeof *result, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FOURMC_OK;
}

// Three read-backs: the summary (n, framing, total), the plan's counts (direct descriptors, staging slots, longest piece), the
// results.  Between the last two: descriptors, ONE container decode over direct and staged blocks together (relative to the lower
// of d_dst and the staging, so that every offset is positive), the copies out of staging, the per-range reduction.
int fourmc_gpu_image_read(const void* d_image, uint64_t image_bytes, fourmc_image_range* ranges, uint32_t nranges,
                          void* d_dst, uint64_t dst_cap, void* stream)
{
    if (nranges && !ranges) { snprintf(g_err, sizeof g_err, "image_read: null ranges"); return FOURMC_EINVAL; }
    if (int r = image_args(d_image, image_bytes, "image_read")) return r;
    if (nranges > (1u << 30)) { snprintf(g_err, sizeof g_err, "image_read: %u ranges", nranges); return FOURMC_EINVAL; }
    {   // destinations may not overlap (empty ranges have none)
        std::vector<std::pair<uint64_t, uint64_t>> d;
        d.reserve(nranges);
        for (uint32_t i = 0; i < nranges; i++)
            if (ranges[i].length) d.emplace_back(ranges[i].dst_off, ranges[i].dst_off + std::min(ranges[i].length, ~uint64_t(0) - ranges[i].dst_off));
        if (int r = regions_overlap("image_read", "destinations", d)) return r;
        if (!d.empty() && !d_dst) { snprintf(g_err, sizeof g_err, "image_read: null destination"); return FOURMC_EINVAL; }
    }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsLease ws(&g_img_ws);
    fourmc_image_index_dev idx;
    if (int r = image_index_count(ws, s, d_image, image_bytes, &idx)) return r;
    const int64_t code = idx.info.nblocks < 0 ? idx.info.nblocks : idx.info.framing;
    if (code != 0) { for (uint32_t i = 0; i < nranges; i++) ranges[i].result = code; return FOURMC_OK; }
    if (!nranges) return FOURMC_OK;
    const uint32_t n = uint32_t(idx.info.nblocks);
    const size_t o_plan = kIdxBytes, o_ent = o_plan + 256;
    const size_t o_rng = o_ent + align256(size_t(n) * sizeof(fourmc_image_entry));
    const size_t o_rp = o_rng + align256(size_t(nranges) * sizeof(fourmc_image_range));
    const size_t o_flag = o_rp + align256(size_t(nranges) * sizeof(fourmc_image_rplan));
    void* w = nullptr;
    if (int r = ws.get(s, o_flag + size_t(n) * 4 + 4, &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_idx = reinterpret_cast<fourmc_image_index_dev*>(base);
    auto* d_plan = reinterpret_cast<fourmc_image_plan*>(base + o_plan);
    auto* d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
    auto* d_rng = reinterpret_cast<fourmc_image_range*>(base + o_rng);
    auto* d_rp = reinterpret_cast<fourmc_image_rplan*>(base + o_rp);
    auto* d_flag = reinterpret_cast<uint32_t*>(base + o_flag);
    HIP_TRY(hipMemsetAsync(d_plan, 0, sizeof(fourmc_image_plan), s));
    HIP_TRY(hipMemsetAsync(d_flag, 0, size_t(n) * 4 + 4, s));
    HIP_TRY(hipMemcpyAsync(d_rng, ranges, size_t(nranges) * sizeof(fourmc_image_range), hipMemcpyHostToDevice, s));
    HIP_TRY(fourmc_launch_image_index(d_image, image_bytes, d_idx, d_ent, n, s));
    HIP_TRY(fourmc_launch_image_plan(d_ent, n, d_idx, d_rng, nranges, dst_cap, d_rp, d_flag, d_plan, s));
    fourmc_image_plan plan;
    HIP_TRY(hipMemcpyAsync(&plan, d_plan, sizeof plan, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t ndesc = plan.ndirect + plan.nstaged;
    if (ndesc > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "image_read: %llu blocks to decode", (unsigned long long)ndesc); return FOURMC_EUNSUP; }
    WsLease ws2(&g_img_stage); void* w2 = nullptr;
    const size_t o_stage = align256(size_t(ndesc) * sizeof(fourmc_block));
    if (int r = ws2.get(s, o_stage + size_t(plan.nstaged) * FOURMC_BLOCKSIZE, &w2)) return r;
    auto* d_desc = static_cast<fourmc_block*>(w2);
    char* d_stage = static_cast<char*>(w2) + o_stage;
    if (ndesc) {
        const uintptr_t pd = reinterpret_cast<uintptr_t>(d_dst), ps = reinterpret_cast<uintptr_t>(d_stage), lo = std::min(pd, ps);
        HIP_TRY(fourmc_launch_image_read_desc(d_ent, n, d_rng, nranges, d_rp, d_flag, plan.nstaged, plan.ndirect, pd - lo, ps - lo, d_desc, s));
        if (int r = fourmc_gpu_4mc_decode_blocks(d_image, reinterpret_cast<void*>(lo), d_desc, uint32_t(ndesc), image_codec(idx), s)) return r;
        HIP_TRY(fourmc_launch_image_read_copy(d_ent, d_rng, nranges, d_rp, d_flag, d_stage, d_dst, plan.max_piece, s));
        HIP_TRY(fourmc_launch_image_read_reduce(d_ent, d_rng, nranges, d_rp, d_flag, d_desc, plan.ndirect, s));
    }
    std::vector<fourmc_image_range> back(nranges);
    HIP_TRY(hipMemcpyAsync(back.data(), d_rng, size_t(nranges) * sizeof(fourmc_image_range), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < nranges; i++) ranges[i].result = back[i].result;
    return FOURMC_OK;
}

// The splits of a record reader (records.hip; the reads themselves are in engine_lines.hip).
// Two read-backs: the summary, then the aligned slices.  An image without blocks leaves every slice as it came (getSplits'
// "leave the default split for empty block index").
int fourmc_gpu_image_align_slices(const void* d_image, uint64_t image_bytes, fourmc_image_slice* slices, uint32_t nslices, void* stream)
{
    if (nslices && !slices) { snprintf(g_err, sizeof g_err, "image_align_slices: null slices"); return FOURMC_EINVAL; }
    if (!d_image) { snprintf(g_err, sizeof g_err, "image_align_slices: null image"); return FOURMC_EINVAL; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsLease ws(&g_img_ws);
    fourmc_image_index_dev idx;
    if (int r = image_index_count(ws, s, d_image, image_bytes, &idx)) return r;
    const int64_t code = idx.info.nblocks < 0 ? idx.info.nblocks : idx.info.framing;
    if (code != 0 || idx.info.nblocks == 0) {
        for (uint32_t i = 0; i < nslices; i++) {
            slices[i].split_start = slices[i].start; slices[i].split_end = slices[i].end;
            slices[i].first_block = slices[i].block_count = 0;
            slices[i].result = code != 0 ? code : 1;
        }
        return FOURMC_OK;
    }
    if (!nslices) return FOURMC_OK;
    const uint32_t n = uint32_t(idx.info.nblocks);
    const size_t o_ent = kIdxBytes, o_sl = o_ent + align256(size_t(n) * sizeof(fourmc_image_entry));
    void* w = nullptr;
    if (int r = ws.get(s, o_sl + size_t(nslices) * sizeof(fourmc_image_slice), &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_idx = reinterpret_cast<fourmc_image_index_dev*>(base);
    auto* d_ent = reinterpret_cast<fourmc_image_entry*>(base + o_ent);
    auto* d_sl = reinterpret_cast<fourmc_image_slice*>(base + o_sl);
    HIP_TRY(hipMemcpyAsync(d_sl, slices, size_t(nslices) * sizeof(fourmc_image_slice), hipMemcpyHostToDevice, s));
    HIP_TRY(fourmc_launch_image_index(d_image, image_bytes, d_idx, d_ent, n, s));
    HIP_TRY(fourmc_launch_image_align(d_ent, n, image_bytes, d_sl, nslices, s));
    std::vector<fourmc_image_slice> back(nslices);
    HIP_TRY(hipMemcpyAsync(back.data(), d_sl, size_t(nslices) * sizeof(fourmc_image_slice), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(slices, back.data(), size_t(nslices) * sizeof(fourmc_image_slice));
    return FOURMC_OK;
}

} // extern "C"
