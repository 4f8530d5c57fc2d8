// 4mc_amd/csrc/engine.hip — host side of the C ABI in include/fourmc_gpu.h: device selection, the state every call family shares
// (engine_int.h) and the block codecs.  The other families: engine_image.hip, engine_lines.hip, engine_streams.hip, engine_host.hip.
//
// There is NO CPU codec behind these calls: without a usable gfx950 device every entry point
// fails with FOURMC_ENODEV (the product must fail loudly rather than fall back).
#include "engine_int.h"

namespace {

char g_arch[128] = "";
std::mutex g_wsmu;                      // guards the three registries of StreamWs
StreamWs* g_ws_last = nullptr;          // for fourmc_gpu_debug_read_workspace

// The LZ4 decode workspace.  Path, piece size and bytes are resolved once (fourmc_lz4_decode_plan) and handed to the launcher; when
// the device cannot give the workspace the pieces halve FOR THIS CALL (the launch is then cut into more of them) until they are
// below 64 blocks: there an automatic choice ends at the exact walker, which needs none, and an explicit tile / seg choice fails
// with FOURMC_ENOMEM.
int lease_lz4_decode(WsLease& ws, hipStream_t s, uint32_t n, void** work, fourmc_lz4_plan* plan)
{
    fourmc_lz4_plan prev; prev.path = -1; prev.batch = 0; prev.work_bytes = 0; prev.ok = 0;
    int r = FOURMC_ENOMEM;
    for (uint32_t shrink = 0;; shrink++) {
        *plan = fourmc_lz4_decode_plan(n, shrink);
        if (!plan->ok) { snprintf(g_err, sizeof g_err, "LZ4 decode workspace cannot be allocated"); return FOURMC_ENOMEM; }
        if (plan->work_bytes == 0) { *work = nullptr; return FOURMC_OK; }
        // An unchanged plan cannot succeed where the last one failed.  On the tile / seg paths (11..16) it only means the halved
        // batch is still above n: the halving goes on until the plan changes or ends (path 2 or !ok).  Any other path has no batch
        // to shrink (the research paths 1 / 3) and stops here (this loop spun forever; r6: it stopped on the first turn).
        const bool same = shrink && plan->path == prev.path && plan->batch == prev.batch && plan->work_bytes == prev.work_bytes;
        if (same && (plan->path < 11 || plan->path > 16)) return r;
        prev = *plan;
        if (same) continue;
        r = lease_codec_ws(ws, s, plan->work_bytes, work);
        if (r == FOURMC_OK) return r;
        // only "out of memory" is answered with smaller pieces: any other device error is the caller's to see
        if (r != FOURMC_ENOMEM) return r;
    }
}

// A launch whose workspace grows with its blocks.  When the device cannot give the memory for all of them at once the launch is cut
// into pieces, halved until the allocation succeeds: the blocks are independent, so the results are the same and only the chip is
// filled less well (a 512-block batch of level-12 tables is 25 GiB; nothing retried with a smaller batch).
// `cap`: the most blocks a piece may have (0: no limit).  The lease honours FOURMC_WS_FAIL_ABOVE (lease_codec_ws).
template <class Bytes, class Launch>
int in_pieces(hipStream_t s, uint32_t n, uint32_t cap, Bytes bytes, Launch launch)
{
    uint32_t piece = cap && cap < n ? cap : n;
    WsLease ws; void* work = nullptr;
    for (;;) {
        const int r = lease_codec_ws(ws, s, bytes(piece), &work);
        if (r == FOURMC_OK) break;
        if (r != FOURMC_ENOMEM || piece <= 1) return r;
        piece = (piece + 1) / 2;
    }
    for (uint32_t b0 = 0; b0 < n; b0 += piece)
        if (int r = launch(b0, n - b0 < piece ? n - b0 : piece, work)) return r;
    return FOURMC_OK;
}

} // namespace

// ---- what engine_int.h declares
__thread char g_err[512] = "";
std::mutex g_mu;
std::atomic<int> g_device{-1};

int fail_hip(hipError_t e, const char* what)
{
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return FOURMC_EHIP;
}

// The HIP current device belongs to the THREAD: the file API runs engine calls on helper threads, which would otherwise
// work on device 0 whatever fourmc_gpu_init / FOURMC_DEVICE selected.  Every entry point passes through here.
int ensure_device()
{
    int d = g_device.load(std::memory_order_acquire);
    if (d < 0) { if (int r = fourmc_gpu_init(-1)) return r; d = g_device.load(std::memory_order_acquire); }
    // (the embedding application may have changed this thread's current device between two calls: ask, do not remember)
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != d) HIP_TRY(hipSetDevice(d));
    return FOURMC_OK;
}

std::map<hipStream_t, StreamWs*> g_ws;
std::map<hipStream_t, StreamWs*> g_img_ws;
std::map<hipStream_t, StreamWs*> g_img_stage;
std::map<hipStream_t, StreamWs*> g_txt_ws;
std::map<hipStream_t, StreamWs*> g_txt_stage;

int WsLease::get(hipStream_t s, size_t need, void** out)
{
    if (!w_) {
        {
            std::lock_guard<std::mutex> lk(g_wsmu);
            auto it = reg_->find(s);
            if (it == reg_->end()) it = reg_->emplace(s, new StreamWs()).first;
            w_ = it->second;
            if (reg_ == &g_ws) g_ws_last = w_;
        }
        w_->mu.lock();          // entries are never removed; the registry lock is not held while waiting here
    }
    if (need > w_->cap) {
        if (w_->p) { HIP_TRY(hipStreamSynchronize(s)); HIP_TRY(hipFree(w_->p)); w_->p = nullptr; w_->cap = 0; }
        const size_t want = need + need / 16 + 4096;
        const hipError_t me = hipMalloc(&w_->p, want);
        if (me == hipErrorOutOfMemory) {          // the one failure a caller may answer with smaller pieces
            (void)hipGetLastError(); w_->p = nullptr;
            snprintf(g_err, sizeof g_err, "hipMalloc(%zu bytes of workspace): out of memory", want);
            return FOURMC_ENOMEM;
        }
        HIP_TRY(me);
        w_->cap = want;
    }
    *out = w_->p;
    return FOURMC_OK;
}

// A codec's per-block workspace, leased on its stream.  FOURMC_WS_FAIL_ABOVE=N (test aid, read once per process) makes every such
// lease of more than N bytes fail the way hipMalloc does when the device is out of memory, so that the answers to it - the pieces
// of in_pieces, the smaller batches and the exact walker of lease_lz4_decode - run on any device.  (The image calls' descriptor and
// staging leases are not codec workspaces and are never refused.)
int lease_codec_ws(WsLease& ws, hipStream_t s, size_t need, void** work)
{
    static const size_t fail_above = [] { const char* e = getenv("FOURMC_WS_FAIL_ABOVE"); return e ? size_t(strtoull(e, nullptr, 10)) : size_t(0); }();
    if (fail_above && need > fail_above) {
        snprintf(g_err, sizeof g_err, "workspace of %zu bytes refused (FOURMC_WS_FAIL_ABOVE)", need);
        return FOURMC_ENOMEM;
    }
    return ws.get(s, need, work);
}

int regions_overlap(const char* who, const char* what, std::vector<std::pair<uint64_t, uint64_t>>& r)
{
    std::sort(r.begin(), r.end());
    for (size_t i = 1; i < r.size(); i++)
        if (r[i].first < r[i - 1].second) {
            snprintf(g_err, sizeof g_err, "%s: %s overlap at %llu", who, what, (unsigned long long)r[i].first);
            return FOURMC_EINVAL;
        }
    return FOURMC_OK;
}

extern "C" {

// Gives the device back every workspace the engine keeps per stream (a 64 GiB decode leaves 92 GB behind on its stream; they are kept
// because the next call of the same size reuses them).  Each stream is synchronized before its buffer goes; a lease in flight on
// another thread is waited for.  Returns FOURMC_OK or a device error.
int fourmc_gpu_release_workspaces(void)
{
    std::vector<std::pair<hipStream_t, StreamWs*>> all;
    { std::lock_guard<std::mutex> lk(g_wsmu); for (auto& kv : g_ws) all.push_back(kv); for (auto& kv : g_img_ws) all.push_back(kv);
      for (auto& kv : g_img_stage) all.push_back(kv); for (auto& kv : g_txt_ws) all.push_back(kv); for (auto& kv : g_txt_stage) all.push_back(kv); }
    for (auto& kv : all) {
        std::lock_guard<std::mutex> lk(kv.second->mu);
        if (kv.second->p) {
            HIP_TRY(hipStreamSynchronize(kv.first)); HIP_TRY(hipFree(kv.second->p));
            kv.second->p = nullptr; kv.second->cap = 0;
        }
    }
    return FOURMC_OK;
}

const char* fourmc_gpu_last_error(void) { return g_err; }
const char* fourmc_gpu_arch(void) { return g_arch; }

int fourmc_gpu_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { fail_hip(e, "hipGetDeviceCount"); return FOURMC_ENODEV; }
    return n;
}

int fourmc_gpu_init(int device)
{
    std::lock_guard<std::mutex> lk(g_mu);
    int n = fourmc_gpu_device_count();
    if (n <= 0) {
        if (n == 0) snprintf(g_err, sizeof g_err, "no HIP device visible (4mc GPU engine has no CPU fallback)");
        return FOURMC_ENODEV;
    }
    if (device < 0) {
        // honour an already-selected device (one process per GPU: LOCAL_RANK / hipSetDevice upstream)
        const char* env = getenv("FOURMC_DEVICE");
        if (env) device = atoi(env);
        else if (hipGetDevice(&device) != hipSuccess) device = 0;
    }
    if (device >= n) { snprintf(g_err, sizeof g_err, "device %d out of range (%d visible)", device, n); return FOURMC_EINVAL; }
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    snprintf(g_arch, sizeof g_arch, "%s", prop.gcnArchName);
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        snprintf(g_err, sizeof g_err, "device %d is %s; this build carries gfx950 code only", device, prop.gcnArchName);
        return FOURMC_ENODEV;
    }
    g_device.store(device, std::memory_order_release);
    return FOURMC_OK;
}

// ------------------------------------------------------------------------ device-resident API
int fourmc_gpu_lz4_decompress(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n, void* stream)
{
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    WsLease ws; void* work = nullptr;
    fourmc_lz4_plan plan;
    if (int r = lease_lz4_decode(ws, s, n, &work, &plan)) return r;
    HIP_TRY(fourmc_launch_lz4_decode(d_src, d_dst, d_blocks, n, 0, &plan, work, s));
    return FOURMC_OK;
}

// LZ4 fast encoder of the launches: 0 the reference parse, byte for byte (default); 1 the ratio-tolerance encoder
// (lz4_par_encode.hip: valid LZ4 blocks, not the reference's bytes).  FOURMC_LZ4_ENCODE = exact | parallel.
static std::atomic<int> g_lz4_encode_mode{-1};
void fourmc_gpu_set_lz4_encode_mode(int mode) { g_lz4_encode_mode.store(mode == 1 ? 1 : 0, std::memory_order_release); }
int fourmc_gpu_get_lz4_encode_mode(void)
{
    int m = g_lz4_encode_mode.load(std::memory_order_acquire);
    if (m < 0) {
        const char* e = getenv("FOURMC_LZ4_ENCODE");
        m = (e && (!strcmp(e, "parallel") || !strcmp(e, "par") || !strcmp(e, "1"))) ? 1 : 0;
        g_lz4_encode_mode.store(m, std::memory_order_release);
    }
    return m;
}

static int lz4_fast_encode(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n, int container_mode, hipStream_t s)
{
    if (fourmc_gpu_get_lz4_encode_mode() == 1) {
        // pieces bound the workspace (4 MiB per block)
        return in_pieces(s, n, 4096, fourmc_lz4_par_work_bytes, [&](uint32_t b0, uint32_t m, void* work) -> int {
            HIP_TRY(fourmc_launch_lz4_encode_par(d_src, d_dst, d_blocks + b0, m, container_mode, work, s)); return FOURMC_OK; });
    }
    // the reference's parse writes sequence records (16 bytes each, a 4 MiB block's area is 16 MiB), the emit kernel the bytes; the
    // headline's blocks stay ONE parse launch (every piece costs a whole per-block chain), pieces only when the records do not fit
    return in_pieces(s, n, 0, fourmc_lz4_fast_work_bytes, [&](uint32_t b0, uint32_t m, void* work) -> int {
        HIP_TRY(fourmc_launch_lz4_encode_fast(d_src, d_dst, d_blocks + b0, m, container_mode, work, s)); return FOURMC_OK; });
}

int fourmc_gpu_lz4_compress_fast(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n, void* stream)
{
    if (int r = ensure_device()) return r;
    return lz4_fast_encode(d_src, d_dst, d_blocks, n, 0, static_cast<hipStream_t>(stream));
}

// LZ4 HC at any level, as LZ4_compress_HC takes it: <= 0 is the default 9 and above 12 is 12 (lz4hc.c:840-841); 1..8 run the
// hash-chain kernel (lz4hc_encode.hip), 9..12 the one with pattern analysis, chain swap and the optimal parser (lz4hc_opt_encode.hip)
static int lz4hc_encode(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n, int level, int container_mode, hipStream_t s)
{
    if (level < 1) level = 9;
    if (level > 12) level = 12;
    if (level <= 8)
        return in_pieces(s, n, 0, fourmc_lz4hc_work_bytes, [&](uint32_t b0, uint32_t m, void* work) -> int {
            HIP_TRY(fourmc_launch_lz4hc_encode(d_src, d_dst, d_blocks + b0, m, work, level, container_mode, s)); return FOURMC_OK; });
    return in_pieces(s, n, 0, fourmc_lz4hc_opt_work_bytes, [&](uint32_t b0, uint32_t m, void* work) -> int {
        HIP_TRY(fourmc_launch_lz4hc_opt_encode(d_src, d_dst, d_blocks + b0, m, work, level, container_mode, s)); return FOURMC_OK; });
}

int fourmc_gpu_lz4_compress_hc(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n, int level, void* stream)
{
    if (int r = ensure_device()) return r;
    return lz4hc_encode(d_src, d_dst, d_blocks, n, level, 0, static_cast<hipStream_t>(stream));
}

int fourmc_gpu_lz4_compress_mc(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n, void* stream)
{
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return in_pieces(s, n, 0, fourmc_lz4hc_work_bytes, [&](uint32_t b0, uint32_t m, void* work) -> int {      // same layout as HC
        HIP_TRY(fourmc_launch_lz4mc_encode(d_src, d_dst, d_blocks + b0, m, work, 0, s)); return FOURMC_OK; });
}

#ifdef FOURMC_RESEARCH      /* debug / profiling exports: the research side build only (make research), never the product's ABI */
/* profiling aid: copies `bytes` of the shared per-block workspace at `offset` to the host (phase cycle counters
 * the zstd kernels leave behind their literal buffers) */
int fourmc_gpu_debug_read_workspace(void* host, size_t offset, size_t bytes)
{
    if (int r = ensure_device()) return r;
    HIP_TRY(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(g_wsmu);                 // the workspace of the stream that was served last
    if (!g_ws_last || !g_ws_last->p || offset + bytes > g_ws_last->cap) { snprintf(g_err, sizeof g_err, "workspace range out of bounds"); return FOURMC_EINVAL; }
    HIP_TRY(hipMemcpy(host, static_cast<char*>(g_ws_last->p) + offset, bytes, hipMemcpyDeviceToHost));
    return FOURMC_OK;
}

/* test aid: run ONLY the parser of the block-parallel LZ4 decoder and copy the first `bytes` of block 0's workspace slot
 * (header, window descriptors, token positions: lz4par.h) to the host */
int fourmc_gpu_debug_lz4_parse(const void* d_src, const void* d_dst, fourmc_block* d_blocks, uint32_t n, int container_mode,
                               void* host, size_t bytes, size_t* layout)
{
    if (int r = ensure_device()) return r;
    if (layout) { layout[0] = fourmc_lz4_parse_work_bytes(1); layout[1] = 64; layout[2] = fourmc_lz4_decode_tok_offset(); }
    if (n == 0) return FOURMC_OK;
    WsLease ws; void* work = nullptr;
    if (int r = ws.get(nullptr, fourmc_lz4_parse_work_bytes(n), &work)) return r;
    HIP_TRY(fourmc_launch_lz4_parse(d_src, d_dst, d_blocks, n, container_mode, work, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    const size_t have = fourmc_lz4_parse_work_bytes(n);
    if (host && bytes) HIP_TRY(hipMemcpy(host, work, bytes < have ? bytes : have, hipMemcpyDeviceToHost));
    return FOURMC_OK;
}

#endif

int fourmc_gpu_zstd_decompress(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n, void* stream)
{
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return in_pieces(s, n, 0, fourmc_zstd_scratch_bytes, [&](uint32_t b0, uint32_t m, void* scratch) -> int {
        HIP_TRY(fourmc_launch_zstd_decode(d_src, d_dst, d_blocks + b0, m, scratch, 0, s)); return FOURMC_OK; });
}

// zstd levels on the device: 1..12 (fast, dfast, greedy, lazy, lazy2 and - for the short last block of a file - btlazy2 / btopt: every
// strategy clevels.h names for them); 4mz itself uses 1, 3, 6, 12.  Levels 13 and above (btlazy2 on full blocks, btultra) and levels
// below 1 are refused rather than answered with bytes the reference would not emit
static int zstd_level_ok(const fourmc_block*, uint32_t, int level, hipStream_t)
{
    if (fourmc_zstd_enc_level_ok(level)) return FOURMC_OK;
    snprintf(g_err, sizeof g_err, "ZSTD level %d not on the device (levels 1..12 are)", level);
    return FOURMC_EUNSUP;
}

static int zstd_enc_serial() { const char* e = getenv("FOURMC_ZSTD_SERIAL"); return e && *e == '1'; }

int fourmc_gpu_zstd_compress(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n, int level, void* stream)
{
    if (int r = ensure_device()) return r;
    if (int r = zstd_level_ok(d_blocks, n, level, static_cast<hipStream_t>(stream))) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return in_pieces(s, n, 0, [&](uint32_t m) { return fourmc_zstd_enc_work_bytes(m, level); }, [&](uint32_t b0, uint32_t m, void* work) -> int {
        HIP_TRY(fourmc_launch_zstd_encode(d_src, d_dst, d_blocks + b0, m, work, 0, level, zstd_enc_serial(), s)); return FOURMC_OK; });
}

int fourmc_gpu_xxh32(const void* d_src, fourmc_block* d_blocks, uint32_t n, uint32_t seed, void* stream)
{
    if (int r = ensure_device()) return r;
    HIP_TRY(fourmc_launch_xxh32(d_src, d_blocks, n, seed, FOURMC_HASH_SRC, static_cast<hipStream_t>(stream)));
    return FOURMC_OK;
}

int fourmc_gpu_4mc_encode_blocks(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                 int codec, int level, void* stream)
{
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (codec == FOURMC_CODEC_LZ4_HC) {
        if (int r = lz4hc_encode(d_src, d_dst, d_blocks, n, level, 1, s)) return r;
        HIP_TRY(fourmc_launch_xxh32(d_dst, d_blocks, n, 0, FOURMC_HASH_DST_RESULT, s));
        return FOURMC_OK;
    }
    if (codec == FOURMC_CODEC_LZ4_MC) {
        if (int r = in_pieces(s, n, 0, fourmc_lz4hc_work_bytes, [&](uint32_t b0, uint32_t m, void* work) -> int {
                HIP_TRY(fourmc_launch_lz4mc_encode(d_src, d_dst, d_blocks + b0, m, work, 1, s)); return FOURMC_OK; })) return r;
        HIP_TRY(fourmc_launch_xxh32(d_dst, d_blocks, n, 0, FOURMC_HASH_DST_RESULT, s));
        return FOURMC_OK;
    }
    if (codec == FOURMC_CODEC_ZSTD) {
        if (int r = zstd_level_ok(d_blocks, n, level, s)) return r;
        if (int r = in_pieces(s, n, 0, [&](uint32_t m) { return fourmc_zstd_enc_work_bytes(m, level); }, [&](uint32_t b0, uint32_t m, void* work) -> int {
                HIP_TRY(fourmc_launch_zstd_encode(d_src, d_dst, d_blocks + b0, m, work, 1, level, zstd_enc_serial(), s)); return FOURMC_OK; })) return r;
        HIP_TRY(fourmc_launch_xxh32(d_dst, d_blocks, n, 0, FOURMC_HASH_DST_RESULT, s));
        return FOURMC_OK;
    }
    if (codec != FOURMC_CODEC_LZ4_FAST) {
        snprintf(g_err, sizeof g_err, "codec %d not implemented on the device yet", codec);
        return FOURMC_EUNSUP;
    }
    if (int r = lz4_fast_encode(d_src, d_dst, d_blocks, n, 1, s)) return r;
    HIP_TRY(fourmc_launch_xxh32(d_dst, d_blocks, n, 0, FOURMC_HASH_DST_RESULT, s));
    return FOURMC_OK;
}

int fourmc_gpu_4mc_decode_blocks(const void* d_src, void* d_dst, fourmc_block* d_blocks, uint32_t n,
                                 int codec, void* stream)
{
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (codec == FOURMC_CODEC_ZSTD) {              // .4mz: every level decodes with the same kernel
        HIP_TRY(fourmc_launch_xxh32(d_src, d_blocks, n, 0, FOURMC_VERIFY_SRC, s));
        return in_pieces(s, n, 0, fourmc_zstd_scratch_bytes, [&](uint32_t b0, uint32_t m, void* scratch) -> int {
            HIP_TRY(fourmc_launch_zstd_decode(d_src, d_dst, d_blocks + b0, m, scratch, 1, s)); return FOURMC_OK; });
    }
    if (codec != FOURMC_CODEC_LZ4_FAST && codec != FOURMC_CODEC_LZ4_MC && codec != FOURMC_CODEC_LZ4_HC) {
        snprintf(g_err, sizeof g_err, "codec %d not implemented on the device yet", codec);
        return FOURMC_EUNSUP;
    }
    WsLease ws; void* work = nullptr;
    fourmc_lz4_plan plan;
    if (int r = lease_lz4_decode(ws, s, n, &work, &plan)) return r;
    HIP_TRY(fourmc_launch_xxh32(d_src, d_blocks, n, 0, FOURMC_VERIFY_SRC, s));
    HIP_TRY(fourmc_launch_lz4_decode(d_src, d_dst, d_blocks, n, 1, &plan, work, s));
    return FOURMC_OK;
}

int fourmc_gpu_4mc_pack_image(const void* d_staging, void* d_image, const fourmc_block* d_blocks,
                              const uint64_t* d_image_off, uint32_t n, void* stream)
{
    if (int r = ensure_device()) return r;
    HIP_TRY(fourmc_launch_pack_image(d_staging, d_image, d_blocks, d_image_off, n, static_cast<hipStream_t>(stream)));
    return FOURMC_OK;
}

} // extern "C"
