// 4mc_amd/csrc/engine.hip — host side of the C ABI in include/fourmc_gpu.h: device selection,
// batched launches, and the host-buffer staging used by the CLI / JNI entry points.
//
// There is NO CPU codec behind these calls: without a usable gfx950 device every entry point
// fails with FOURMC_ENODEV (the product must fail loudly rather than fall back).
#include <hip/hip_runtime.h>
#include <mutex>
#include <condition_variable>
#include <vector>
#include <algorithm>
#include <map>
#include <atomic>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fourmc_gpu.h"
#include "kernels.h"
#include "codec_level.h"

namespace {

thread_local char g_err[512] = "";
std::mutex g_mu;                 // guards device selection and the host-staging arena
std::atomic<int> g_device{-1};
char g_arch[128] = "";

int fail_hip(hipError_t e, const char* what)
{
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return FOURMC_EHIP;
}
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail_hip(e_, #x); } while (0)

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

// Host-staging arena: device buffers reused across host-buffer calls (grown on demand).
struct Arena {
    void* d_src = nullptr; size_t src_cap = 0;
    void* d_dst = nullptr; size_t dst_cap = 0;
    fourmc_block* d_blk = nullptr; size_t blk_cap = 0;
    hipStream_t stream = nullptr;
    int device = -1;
};
// Shard 0 serves every host-buffer call; with FOURMC_GPUS=N > 1 a batch of blocks is cut into N contiguous block ranges,
// one arena (device buffers + stream) per range, placed round robin on the visible devices starting at the selected one.
// N may exceed the number of devices: the surplus shards share devices (that is how the sharding is exercised on a
// one-GPU box).  One process, several devices: the per-range results come back to host memory, so the "gather of the
// per-rank block index" of the multi-process layout (bench.py, container.py: RCCL all_gather) is a plain array here.
constexpr int kMaxShards = 16;
Arena g_arenas[kMaxShards];
Arena& g_arena = g_arenas[0];

int host_shards()
{
    static int n = [] { const char* e = getenv("FOURMC_GPUS"); int v = e ? atoi(e) : 1; return v < 1 ? 1 : v > kMaxShards ? kMaxShards : v; }();
    return n;
}

// Device workspaces (per-block scratch of the kernels: LZ4 decode records, LZ4 HC/MC tables, zstd literals / sequence
// areas / encoder tables).  ONE GROWABLE BUFFER PER STREAM: launches on a stream are ordered, so consecutive calls on the
// same stream can share a buffer, while calls on different streams (the JNI queue's own stream next to a device-API
// caller's, two device-API callers) never see each other's scratch.  A lease keeps the stream's entry locked from the
// moment the pointer is handed out until the caller's launches are enqueued; growing synchronizes THAT stream before the
// old buffer is freed, so no launch can still be using it.
struct StreamWs { std::mutex mu; void* p = nullptr; size_t cap = 0; };
std::mutex g_wsmu;
std::map<hipStream_t, StreamWs*> g_ws;
StreamWs* g_ws_last = nullptr;          // for fourmc_gpu_debug_read_workspace

// The image calls (image.hip) keep their descriptors, offsets and staging slots in a second registry of the same kind: they hold
// that lease while the codec launches they make lease the stream's workspace.
std::map<hipStream_t, StreamWs*> g_img_ws;
// image_read's descriptors and staging slots: a third registry, so that sizing them after the plan's read-back cannot move the
// index and the plan that the second one holds
std::map<hipStream_t, StreamWs*> g_img_stage;

class WsLease {
    StreamWs* w_ = nullptr;
    std::map<hipStream_t, StreamWs*>* reg_ = &g_ws;
public:
    WsLease() {}
    explicit WsLease(std::map<hipStream_t, StreamWs*>* reg) : reg_(reg) {}
    WsLease(const WsLease&) = delete;
    ~WsLease() { if (w_) w_->mu.unlock(); }
    size_t cap() const { return w_ ? w_->cap : 0; }          // changes exactly when get() had to grow the buffer
    int get(hipStream_t s, size_t need, void** out)
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
};

} // namespace (the export below is part of the boundary)
// Gives the device back every workspace the engine keeps per stream (a 64 GiB decode leaves 92 GB behind on its stream; they are kept
// because the next call of the same size reuses them).  Each stream is synchronized before its buffer goes; a lease in flight on
// another thread is waited for.  Returns FOURMC_OK or a device error.
extern "C" int fourmc_gpu_release_workspaces(void)
{
    std::vector<std::pair<hipStream_t, StreamWs*>> all;
    { std::lock_guard<std::mutex> lk(g_wsmu); for (auto& kv : g_ws) all.push_back(kv); for (auto& kv : g_img_ws) all.push_back(kv);
      for (auto& kv : g_img_stage) all.push_back(kv); }
    for (auto& kv : all) {
        std::lock_guard<std::mutex> lk(kv.second->mu);
        if (kv.second->p) {
            HIP_TRY(hipStreamSynchronize(kv.first)); HIP_TRY(hipFree(kv.second->p));
            kv.second->p = nullptr; kv.second->cap = 0;
        }
    }
    return FOURMC_OK;
}
namespace {

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

int arena_reserve(Arena& g_arena, size_t src_bytes, size_t dst_bytes, size_t nblk)
{
    if (!g_arena.stream) HIP_TRY(hipStreamCreateWithFlags(&g_arena.stream, hipStreamNonBlocking));
    auto grow = [](void** p, size_t* cap, size_t need) -> hipError_t {
        if (need <= *cap) return hipSuccess;
        if (*p) { hipError_t e = hipFree(*p); if (e != hipSuccess) return e; *p = nullptr; *cap = 0; }
        size_t want = need + need / 4 + 4096;
        hipError_t e = hipMalloc(p, want);
        if (e == hipSuccess) *cap = want;
        return e;
    };
    HIP_TRY(grow(&g_arena.d_src, &g_arena.src_cap, src_bytes + 64));
    HIP_TRY(grow(&g_arena.d_dst, &g_arena.dst_cap, dst_bytes + 64));
    HIP_TRY(grow(reinterpret_cast<void**>(&g_arena.d_blk), &g_arena.blk_cap, nblk * sizeof(fourmc_block)));
    return FOURMC_OK;
}

} // namespace

extern "C" {

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

// ------------------------------------------------------------------------ whole file images (image.hip)
uint64_t fourmc_gpu_image_bound(uint64_t src_bytes)
{
    const uint64_t n = (src_bytes + FOURMC_BLOCKSIZE - 1) / FOURMC_BLOCKSIZE;
    return 12 + 12 * n + src_bytes + 12 + 20 + 4 * n;
}

static size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

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
constexpr size_t kImagesStageSlack = 4096;
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
            if (it.src_off > src_total || it.src_bytes > src_total - it.src_off) {
                snprintf(g_err, sizeof g_err, "images_compress: the source of image %u lies beyond the %llu bytes of sources", i, (unsigned long long)src_total);
                return FOURMC_EINVAL;
            }
            const uint64_t k = it.src_bytes / FOURMC_BLOCKSIZE + (it.src_bytes % FOURMC_BLOCKSIZE ? 1 : 0);
            if (k > 0x3FFFFFFFull) { snprintf(g_err, sizeof g_err, "images_compress: image %u has %llu blocks", i, (unsigned long long)k); return FOURMC_EINVAL; }
            if (it.image_off > images_bytes || it.image_cap > images_bytes - it.image_off) {
                snprintf(g_err, sizeof g_err, "images_compress: the region of image %u lies beyond the %llu bytes of images", i, (unsigned long long)images_bytes);
                return FOURMC_EINVAL;
            }
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
        std::sort(d.begin(), d.end());
        for (size_t i = 1; i < d.size(); i++)
            if (d[i].first < d[i - 1].second) {
                snprintf(g_err, sizeof g_err, "images_compress: image regions overlap at %llu", (unsigned long long)d[i].first);
                return FOURMC_EINVAL;
            }
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

// ------------------------------------------------------------------------ streaming image writer (image.hip)
// One device allocation per writer, made by begin and freed by finish / abort: the running state, the descriptors of one batch, the
// index (the absolute offset of every block header, then the running offset behind the last one), the carry slot and the staging.
// The carry slot sits in front of the staging, so a codec reading past the slot's end stays inside the allocation.
}   // extern "C"
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

} // namespace
extern "C" {

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

// ------------------------------------------------------------------------ streaming image reader (image.hip)
// One device allocation per reader, made by begin and freed by finish / abort: the walk's state, the status, the descriptors and
// header offsets of one batch, the copy pieces of one walk and batch_blocks staging slots (64 bytes of slack behind the last one
// for the decoders' read-ahead).  A block cut by the end of a chunk waits in its own slot, so there is no separate carry slot.
}   // extern "C"
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

} // namespace
extern "C" {

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
    if (!items) { snprintf(g_err, sizeof g_err, "images_decompress: null items"); return FOURMC_EINVAL; }
    {
        std::vector<std::pair<uint64_t, uint64_t>> d;
        if (d_dst) d.reserve(n);
        for (uint32_t i = 0; i < n; i++) {
            const fourmc_image_item& it = items[i];
            if (it.image_bytes && !d_images) { snprintf(g_err, sizeof g_err, "images_decompress: null images"); return FOURMC_EINVAL; }
            if (it.image_off > images_bytes || it.image_bytes > images_bytes - it.image_off) {
                snprintf(g_err, sizeof g_err, "images_decompress: image %u lies beyond the %llu bytes of images", i, (unsigned long long)images_bytes);
                return FOURMC_EINVAL;
            }
            if (!d_dst) continue;                             // the size query looks at no destination
            if (it.dst_off > dst_bytes || it.dst_cap > dst_bytes - it.dst_off) {
                snprintf(g_err, sizeof g_err, "images_decompress: the output region of image %u lies beyond the %llu bytes of the destination", i,
                         (unsigned long long)dst_bytes);
                return FOURMC_EINVAL;
            }
            if (it.dst_cap) d.emplace_back(it.dst_off, it.dst_off + it.dst_cap);
        }
        std::sort(d.begin(), d.end());
        for (size_t i = 1; i < d.size(); i++)
            if (d[i].first < d[i - 1].second) {
                snprintf(g_err, sizeof g_err, "images_decompress: output regions overlap at %llu", (unsigned long long)d[i].first);
                return FOURMC_EINVAL;
            }
    }
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
        int r;
        switch (codec) {
            case FOURMC_CODEC_LZ4_FAST: r = fourmc_gpu_lz4_compress_fast(d_src, d_stage, d_blk, m, s); break;
            case FOURMC_CODEC_LZ4_MC:   r = fourmc_gpu_lz4_compress_mc(d_src, d_stage, d_blk, m, s); break;
            case FOURMC_CODEC_LZ4_HC:   r = fourmc_gpu_lz4_compress_hc(d_src, d_stage, d_blk, m, level, s); break;
            default:                    r = fourmc_gpu_zstd_compress(d_src, d_stage, d_blk, m, level, s); break;
        }
        if (r) return r;
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

// Chunks per round: FOURMC_BSW_ROUND, read at every call (a test sets it between two calls)
static uint32_t bsw_round()
{
    const char* e = getenv("FOURMC_BSW_ROUND");
    const long v = e && *e ? atol(e) : long(kBsPiece);
    return uint32_t(v < 1 ? 1 : v > (1 << 20) ? (1 << 20) : v);
}

// Workspaces.  g_img_ws: the items, the first tile of every stream, the plans and the tile prefixes - what the plan computes and the
// rounds read.  g_img_stage, sized after the plan's read-back (so that sizing it cannot move the prefixes): the slices, one carry and
// one length per stream, the summary, the group table, and the descriptors, side entries, offsets and staging of one round.
int fourmc_gpu_bstreams_compress(const void* d_src, uint64_t src_total, const uint32_t* d_writes, uint64_t writes_total,
                                 void* d_images, uint64_t images_bytes, int codec, int level,
                                 fourmc_bstream_enc_item* items, uint32_t n, void* stream)
{
    const int zstd = bs_family(codec);
    if (zstd < 0) return bs_bad_codec("bstreams_compress", codec);
    if (n == 0) return FOURMC_OK;
    if (!items) { snprintf(g_err, sizeof g_err, "bstreams_compress: null items"); return FOURMC_EINVAL; }
    std::vector<uint64_t> tile0(size_t(n) + 1);
    {
        std::vector<std::pair<uint64_t, uint64_t>> d;
        if (d_images) d.reserve(n);
        uint64_t tiles = 0;
        for (uint32_t i = 0; i < n; i++) {
            const fourmc_bstream_enc_item& it = items[i];
            if (it.src_bytes && !d_src) { snprintf(g_err, sizeof g_err, "bstreams_compress: null source"); return FOURMC_EINVAL; }
            if (it.n_writes && !d_writes) { snprintf(g_err, sizeof g_err, "bstreams_compress: null write table"); return FOURMC_EINVAL; }
            if (it.src_off > src_total || it.src_bytes > src_total - it.src_off) {
                snprintf(g_err, sizeof g_err, "bstreams_compress: the source of stream %u lies beyond the %llu bytes of sources", i, (unsigned long long)src_total);
                return FOURMC_EINVAL;
            }
            if (it.writes_off > writes_total || it.n_writes > writes_total - it.writes_off) {
                snprintf(g_err, sizeof g_err, "bstreams_compress: the write sizes of stream %u lie beyond the %llu entries of the table", i, (unsigned long long)writes_total);
                return FOURMC_EINVAL;
            }
            tile0[i] = tiles;
            tiles += it.n_writes / 64 + (it.n_writes % 64 ? 1 : 0);
            if (!d_images) continue;                          // the size query looks at no region
            if (it.image_off > images_bytes || it.image_cap > images_bytes - it.image_off) {
                snprintf(g_err, sizeof g_err, "bstreams_compress: the region of stream %u lies beyond the %llu bytes of images", i, (unsigned long long)images_bytes);
                return FOURMC_EINVAL;
            }
            if (it.image_cap) d.emplace_back(it.image_off, it.image_off + it.image_cap);
        }
        tile0[n] = tiles;
        std::sort(d.begin(), d.end());
        for (size_t i = 1; i < d.size(); i++)
            if (d[i].first < d[i - 1].second) {
                snprintf(g_err, sizeof g_err, "bstreams_compress: image regions overlap at %llu", (unsigned long long)d[i].first);
                return FOURMC_EINVAL;
            }
    }
    if (zstd && !fourmc_zstd_enc_level_ok(level)) { snprintf(g_err, sizeof g_err, "ZSTD level %d not on the device (levels 1..12 are)", level); return FOURMC_EUNSUP; }
    if (int r = ensure_device()) return r;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint32_t M = fourmc_gpu_bstream_max_input(codec);
    const uint64_t ntiles = tile0[n];
    const size_t o_tile0 = align256(size_t(n) * sizeof(fourmc_bstream_enc_item)), o_plans = o_tile0 + align256((size_t(n) + 1) * 8);
    const size_t o_prefix = o_plans + align256(size_t(n) * sizeof(fourmc_bsw_plan));
    WsLease ws(&g_img_ws); void* w = nullptr;
    if (int r = ws.get(s, o_prefix + size_t(ntiles) * 8, &w)) return r;
    char* base = static_cast<char*>(w);
    auto* d_items = reinterpret_cast<fourmc_bstream_enc_item*>(base);
    auto* d_tile0 = reinterpret_cast<uint64_t*>(base + o_tile0);
    auto* d_plans = reinterpret_cast<fourmc_bsw_plan*>(base + o_plans);
    auto* d_prefix = reinterpret_cast<uint64_t*>(base + o_prefix);
    HIP_TRY(hipMemcpyAsync(d_items, items, size_t(n) * sizeof(fourmc_bstream_enc_item), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_tile0, tile0.data(), (size_t(n) + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(fourmc_launch_bsw_sums(d_writes, d_items, d_tile0, n, ntiles, d_prefix, d_plans, s));
    HIP_TRY(fourmc_launch_bsw_chase(d_writes, d_items, d_tile0, d_prefix, n, M, zstd, d_plans, nullptr, nullptr, s));
    std::vector<fourmc_bsw_plan> plans(n);
    HIP_TRY(hipMemcpyAsync(plans.data(), d_plans, size_t(n) * sizeof(fourmc_bsw_plan), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<fourmc_bsw_slice> slices(size_t(n) + 1);
    fourmc_bsw_slice at = {};
    for (uint32_t i = 0; i < n; i++) {                   // each encoded stream's share of the chunk numbers, the group table and the staging
        fourmc_bsw_plan& pl = plans[i];
        if (pl.reason == FOURMC_BSW_OK && (pl.groups > 0xFFFFFFFFull || pl.chunks > 0x7FFFFFFFull)) {
            snprintf(g_err, sizeof g_err, "bstreams_compress: stream %u has %llu chunks", i, (unsigned long long)pl.chunks);
            return FOURMC_EUNSUP;
        }
        if (d_images && pl.reason == FOURMC_BSW_OK && items[i].image_cap < pl.worst) pl.reason = FOURMC_BSW_CAP;
        slices[i] = at;
        if (pl.reason != FOURMC_BSW_OK) continue;
        at.chunk0 += pl.chunks; at.stage0 += pl.stage;
        if (items[i].n_writes) at.group0 += pl.groups;
        if (at.chunk0 > 0x7FFFFFFFull) { snprintf(g_err, sizeof g_err, "bstreams_compress: more than 0x7FFFFFFF chunks"); return FOURMC_EUNSUP; }
    }
    slices[n] = at;
    auto report = [&](const std::vector<uint64_t>* bytes) {
        for (uint32_t i = 0; i < n; i++) {
            const fourmc_bsw_plan& pl = plans[i];
            const bool planned = pl.reason == FOURMC_BSW_OK || pl.reason == FOURMC_BSW_CAP;
            items[i].reason = pl.reason;
            items[i].groups = planned ? uint32_t(pl.groups) : 0; items[i].chunks = planned ? uint32_t(pl.chunks) : 0;
            items[i].image_bytes = !planned ? 0 : bytes && pl.reason == FOURMC_BSW_OK ? (*bytes)[i] : pl.worst;
        }
    };
    if (!d_images) { report(nullptr); return FOURMC_OK; }
    const uint32_t round = bsw_round();
    const uint64_t nc = at.chunk0;
    const uint32_t piece = uint32_t(nc < round ? nc : round);
    const uint64_t slot_m = align256(bs_block_bound(zstd, M));
    const uint64_t stage = at.stage0 < uint64_t(piece) * slot_m ? at.stage0 : uint64_t(piece) * slot_m;
    const size_t o_carry = align256((size_t(n) + 1) * sizeof(fourmc_bsw_slice)), o_bytes = o_carry + align256(size_t(n) * 8);
    const size_t o_sum = o_bytes + align256(size_t(n) * 8), o_grp = o_sum + align256(sizeof(fourmc_bstream_enc_summary));
    const size_t o_blk = o_grp + align256(size_t(at.group0) * sizeof(fourmc_bsw_group)), o_side = o_blk + align256(size_t(piece) * sizeof(fourmc_block));
    const size_t o_off = o_side + align256(size_t(piece) * sizeof(fourmc_bsw_side)), o_stage = o_off + align256(size_t(piece) * 8);
    WsLease ws2(&g_img_stage); void* w2 = nullptr;
    if (int r = ws2.get(s, o_stage + size_t(stage) + kImagesStageSlack, &w2)) return r;
    char* b2 = static_cast<char*>(w2);
    auto* d_slices = reinterpret_cast<fourmc_bsw_slice*>(b2);
    auto* d_carry = reinterpret_cast<uint64_t*>(b2 + o_carry);
    auto* d_bytes = reinterpret_cast<uint64_t*>(b2 + o_bytes);
    auto* d_sum = reinterpret_cast<fourmc_bstream_enc_summary*>(b2 + o_sum);
    auto* d_grp = reinterpret_cast<fourmc_bsw_group*>(b2 + o_grp);
    auto* d_blk = reinterpret_cast<fourmc_block*>(b2 + o_blk);
    auto* d_side = reinterpret_cast<fourmc_bsw_side*>(b2 + o_side);
    auto* d_off = reinterpret_cast<uint64_t*>(b2 + o_off);
    void* d_stage = b2 + o_stage;
    HIP_TRY(hipMemcpyAsync(d_plans, plans.data(), size_t(n) * sizeof(fourmc_bsw_plan), hipMemcpyHostToDevice, s));      // with the _CAP verdicts
    HIP_TRY(hipMemcpyAsync(d_slices, slices.data(), (size_t(n) + 1) * sizeof(fourmc_bsw_slice), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(d_carry, 0, size_t(n) * 8, s));
    HIP_TRY(hipMemsetAsync(d_sum, 0, sizeof(fourmc_bstream_enc_summary), s));
    if (at.group0) HIP_TRY(fourmc_launch_bsw_chase(d_writes, d_items, d_tile0, d_prefix, n, M, zstd, d_plans, d_slices, d_grp, s));
    for (uint64_t c0 = 0; c0 < nc; c0 += piece) {
        const uint32_t m = uint32_t(nc - c0 < piece ? nc - c0 : piece);
        HIP_TRY(fourmc_launch_bsw_desc(d_items, d_plans, d_slices, d_grp, n, M, zstd, codec == FOURMC_CODEC_LZ4_MC, c0, m, d_blk, d_side, s));
        int r;
        switch (codec) {
            case FOURMC_CODEC_LZ4_FAST: r = fourmc_gpu_lz4_compress_fast(d_src, d_stage, d_blk, m, s); break;
            case FOURMC_CODEC_LZ4_MC:   r = fourmc_gpu_lz4_compress_mc(d_src, d_stage, d_blk, m, s); break;
            case FOURMC_CODEC_LZ4_HC:   r = fourmc_gpu_lz4_compress_hc(d_src, d_stage, d_blk, m, level, s); break;
            default:                    r = fourmc_gpu_zstd_compress(d_src, d_stage, d_blk, m, level, s); break;
        }
        if (r) return r;
        HIP_TRY(fourmc_launch_bsw_pack(d_images, d_items, d_blk, d_side, d_off, m, zstd, d_stage, d_carry, d_sum, s));
    }
    HIP_TRY(fourmc_launch_bsw_result(d_items, d_plans, d_carry, n, d_images, d_bytes, s));
    std::vector<uint64_t> bytes(n);
    fourmc_bstream_enc_summary h;
    HIP_TRY(hipMemcpyAsync(bytes.data(), d_bytes, size_t(n) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h, d_sum, sizeof h, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h.bad) { snprintf(g_err, sizeof g_err, "bstreams_compress: %llu chunks with a codec result outside [1, bound]", (unsigned long long)h.bad); return FOURMC_EINVAL; }
    report(&bytes);
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
    if (!items) { snprintf(g_err, sizeof g_err, "bstreams_decompress: null items"); return FOURMC_EINVAL; }
    {
        std::vector<std::pair<uint64_t, uint64_t>> d;
        if (d_dst) d.reserve(n);
        for (uint32_t i = 0; i < n; i++) {
            const fourmc_bstream_item& it = items[i];
            if (it.image_bytes && !d_images) { snprintf(g_err, sizeof g_err, "bstreams_decompress: null images"); return FOURMC_EINVAL; }
            if (it.image_off > images_bytes || it.image_bytes > images_bytes - it.image_off) {
                snprintf(g_err, sizeof g_err, "bstreams_decompress: stream %u lies beyond the %llu bytes of streams", i, (unsigned long long)images_bytes);
                return FOURMC_EINVAL;
            }
            if (!d_dst) continue;                             // the size query looks at no destination
            if (it.dst_off > dst_bytes || it.dst_cap > dst_bytes - it.dst_off) {
                snprintf(g_err, sizeof g_err, "bstreams_decompress: the output region of stream %u lies beyond the %llu bytes of the destination", i,
                         (unsigned long long)dst_bytes);
                return FOURMC_EINVAL;
            }
            if (it.dst_cap) d.emplace_back(it.dst_off, it.dst_off + it.dst_cap);
        }
        std::sort(d.begin(), d.end());
        for (size_t i = 1; i < d.size(); i++)
            if (d[i].first < d[i - 1].second) {
                snprintf(g_err, sizeof g_err, "bstreams_decompress: output regions overlap at %llu", (unsigned long long)d[i].first);
                return FOURMC_EINVAL;
            }
    }
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
namespace {
// Table entries per round: the setter's value, else FOURMC_ZST_ROUND_BLOCKS (read at every call), else what 4 GiB of round
// workspace hold
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
}

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
    if (!items) { snprintf(g_err, sizeof g_err, "zsts_decompress: null items"); return FOURMC_EINVAL; }
    {
        std::vector<std::pair<uint64_t, uint64_t>> d;
        if (d_dst) d.reserve(n);
        for (uint32_t i = 0; i < n; i++) {
            const fourmc_zst_item& it = items[i];
            if (it.image_bytes && !d_images) { snprintf(g_err, sizeof g_err, "zsts_decompress: null images"); return FOURMC_EINVAL; }
            if (it.image_off > images_bytes || it.image_bytes > images_bytes - it.image_off) {
                snprintf(g_err, sizeof g_err, "zsts_decompress: stream %u lies beyond the %llu bytes of streams", i, (unsigned long long)images_bytes);
                return FOURMC_EINVAL;
            }
            if (!d_dst) continue;                             // the size query looks at no destination
            if (it.dst_off > dst_bytes || it.dst_cap > dst_bytes - it.dst_off) {
                snprintf(g_err, sizeof g_err, "zsts_decompress: the output region of stream %u lies beyond the %llu bytes of the destination", i,
                         (unsigned long long)dst_bytes);
                return FOURMC_EINVAL;
            }
            if (it.dst_cap) d.emplace_back(it.dst_off, it.dst_off + it.dst_cap);
        }
        std::sort(d.begin(), d.end());
        for (size_t i = 1; i < d.size(); i++)
            if (d[i].first < d[i - 1].second) {
                snprintf(g_err, sizeof g_err, "zsts_decompress: output regions overlap at %llu", (unsigned long long)d[i].first);
                return FOURMC_EINVAL;
            }
    }
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

namespace {
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
}

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
            if (read && (it.src_off > src_total || it.src_bytes > src_total - it.src_off)) {
                snprintf(g_err, sizeof g_err, "zsts_compress: the source of stream %u lies beyond the %llu bytes of sources", i, (unsigned long long)src_total);
                return FOURMC_EINVAL;
            }
            if (it.image_off > images_bytes || it.image_cap > images_bytes - it.image_off) {
                snprintf(g_err, sizeof g_err, "zsts_compress: the region of stream %u lies beyond the %llu bytes of images", i, (unsigned long long)images_bytes);
                return FOURMC_EINVAL;
            }
            if (it.image_cap) d.emplace_back(it.image_off, it.image_off + it.image_cap);
        }
        std::sort(d.begin(), d.end());
        for (size_t i = 1; i < d.size(); i++)
            if (d[i].first < d[i - 1].second) {
                snprintf(g_err, sizeof g_err, "zsts_compress: image regions overlap at %llu", (unsigned long long)d[i].first);
                return FOURMC_EINVAL;
            }
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

// ------------------------------------------------------------------------ random access into images (image.hip)
// Workspace of the three calls (g_img_ws): the index summary, then - sized after its read-back - the entries and what the call
// needs besides.  A buffer that grows loses its contents: everything after the first read-back is recomputed on the device.
namespace {
constexpr size_t kIdxBytes = 256;           // fourmc_image_index_dev
int image_args(const void* d_image, uint64_t image_bytes, const char* who)
{
    if (image_bytes && !d_image) { snprintf(g_err, sizeof g_err, "%s: null image", who); return FOURMC_EINVAL; }
    return FOURMC_OK;
}
// the summary, read back (the call's first synchronization)
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
} // namespace

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
        std::sort(d.begin(), d.end());
        for (size_t i = 1; i < d.size(); i++)
            if (d[i].first < d[i - 1].second) {
                snprintf(g_err, sizeof g_err, "image_read: destinations overlap at %llu", (unsigned long long)d[i].first);
                return FOURMC_EINVAL;
            }
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

// ------------------------------------------------------------------------ the line records of a split (records.hip)
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
} // namespace

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

// groups processed, tail rounds run and container decode calls made by the batch call (fourmc_gpu_image_lines_batch_stats), and
// the same with the index kernel's launches for the many-images call (fourmc_gpu_images_lines_stats)
namespace {
struct LinesCounters { std::atomic<unsigned long long> groups{0}, rounds{0}, decodes{0}, index_launches{0}; };
LinesCounters g_lb, g_il;
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

// FOURMC_SPLIT_GROUP: the most splits of one group (a staging slot each); read at every call, like FOURMC_IMAGE_PARSE
static uint32_t split_group()
{
    const char* e = getenv("FOURMC_SPLIT_GROUP");
    if (!e || !*e) return 256;
    const long v = strtol(e, nullptr, 10);
    return v < 1 ? 1u : v > 4096 ? 4096u : uint32_t(v);
}

extern "C++" {                                                // templates below
namespace {
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
        if (it.dst_off > dst_bytes || it.dst_cap > dst_bytes - it.dst_off) {
            snprintf(g_err, sizeof g_err, "%s: the output region of split %u lies beyond the %llu bytes of the destination", who, i,
                     (unsigned long long)dst_bytes);
            return FOURMC_EINVAL;
        }
        if (it.dst_cap) d.emplace_back(it.dst_off, it.dst_off + it.dst_cap);
        if (!d_starts) continue;                          // count only looks at no table
        if (it.table_off > table_entries || it.lines_cap > table_entries - it.table_off) {
            snprintf(g_err, sizeof g_err, "%s: the table region of split %u lies beyond the %llu entries of the tables", who, i,
                     (unsigned long long)table_entries);
            return FOURMC_EINVAL;
        }
        if (it.lines_cap) t.emplace_back(it.table_off, it.table_off + it.lines_cap);
    }
    std::sort(d.begin(), d.end());
    for (size_t i = 1; i < d.size(); i++)
        if (d[i].first < d[i - 1].second) {
            snprintf(g_err, sizeof g_err, "%s: output regions overlap at %llu", who, (unsigned long long)d[i].first);
            return FOURMC_EINVAL;
        }
    std::sort(t.begin(), t.end());
    for (size_t i = 1; i < t.size(); i++)
        if (t[i].first < t[i - 1].second) {
            snprintf(g_err, sizeof g_err, "%s: table regions overlap at %llu", who, (unsigned long long)t[i].first);
            return FOURMC_EINVAL;
        }
    return FOURMC_OK;
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
        if (images[k].image_off > images_bytes || images[k].image_bytes > images_bytes - images[k].image_off) {
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
} // extern "C++"

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

// ------------------------------------------------------------------------ host-buffer API
int fourmc_LZ4_compressBound(int n) { return (unsigned)n > 0x7E000000u ? 0 : n + n / 255 + 16; }

// d_src / d_dst: the bases the descriptors' offsets are relative to (they may point below an arena's allocation when only
// a slice of the host buffers was staged)
static int launch_host_op(int op, int codec, int level, const void* d_src, void* d_dst, fourmc_block* d_blk, uint32_t n, hipStream_t s)
{
    switch (op) {
        case 0: return fourmc_gpu_4mc_encode_blocks(d_src, d_dst, d_blk, n, codec, level, s);
        case 1: return fourmc_gpu_4mc_decode_blocks(d_src, d_dst, d_blk, n, codec, s);
        case 2: return fourmc_gpu_lz4_compress_fast(d_src, d_dst, d_blk, n, s);
        case 3: return fourmc_gpu_lz4_decompress(d_src, d_dst, d_blk, n, s);
        case 5: return fourmc_gpu_zstd_decompress(d_src, d_dst, d_blk, n, s);
        case 8: return fourmc_gpu_zstd_compress(d_src, d_dst, d_blk, n, level, s);
        case 7: return fourmc_gpu_lz4_compress_mc(d_src, d_dst, d_blk, n, s);
        case 6: return fourmc_gpu_lz4_compress_hc(d_src, d_dst, d_blk, n, level, s);
        default: return fourmc_gpu_xxh32(d_src, d_blk, n, (uint32_t)level, s);
    }
}

// FOURMC_GPUS > 1: contiguous block ranges, one per shard, all in flight together (native/4mc.c:280-333 is the serial
// loop this replaces; the ranges are independent, nothing crosses between devices)
static int host_roundtrip_sharded(const void* src, void* dst, fourmc_block* blocks, uint32_t n, int op, int codec, int level, int shards)
{
    int ndev = fourmc_gpu_device_count();
    if (ndev <= 0) return FOURMC_ENODEV;
    const int dev0 = g_device.load(std::memory_order_acquire);
    const uint32_t per = (n + uint32_t(shards) - 1) / uint32_t(shards);
    struct Range { uint32_t lo, hi; uint64_t smin, smax, dmin, dmax; };
    std::vector<Range> rg;
    for (int k = 0; k < shards; k++) {
        Range r; r.lo = std::min(n, uint32_t(k) * per); r.hi = std::min(n, r.lo + per);
        if (r.lo >= r.hi) break;
        r.smin = r.dmin = ~0ull; r.smax = r.dmax = 0;
        for (uint32_t b = r.lo; b < r.hi; b++) {
            r.smin = std::min<uint64_t>(r.smin, blocks[b].src_off); r.smax = std::max<uint64_t>(r.smax, blocks[b].src_off + blocks[b].src_len);
            r.dmin = std::min<uint64_t>(r.dmin, blocks[b].dst_off); r.dmax = std::max<uint64_t>(r.dmax, blocks[b].dst_off + blocks[b].dst_cap);
        }
        rg.push_back(r);
    }
    int rc = FOURMC_OK;
    for (size_t k = 0; k < rg.size() && rc == FOURMC_OK; k++) {                      // stage + launch every range
        Arena& a = g_arenas[k]; const Range& r = rg[k];
        a.device = (dev0 + int(k)) % ndev;
        // no return from inside this loop: earlier ranges are in flight against the caller's buffers and have to be waited for
        // below, and the thread's device has to be put back
        auto step = [&](hipError_t e, const char* what) { if (e != hipSuccess && rc == FOURMC_OK) rc = fail_hip(e, what); return rc == FOURMC_OK; };
        if (!step(hipSetDevice(a.device), "hipSetDevice")) break;
        if ((rc = arena_reserve(a, size_t(r.smax - r.smin), size_t(r.dmax - r.dmin), r.hi - r.lo))) break;
        if (!step(hipMemcpyAsync(a.d_src, static_cast<const char*>(src) + r.smin, size_t(r.smax - r.smin), hipMemcpyHostToDevice, a.stream), "hipMemcpyAsync")) break;
        if (!step(hipMemcpyAsync(a.d_blk, blocks + r.lo, (r.hi - r.lo) * sizeof(fourmc_block), hipMemcpyHostToDevice, a.stream), "hipMemcpyAsync")) break;
        rc = launch_host_op(op, codec, level, static_cast<char*>(a.d_src) - r.smin, static_cast<char*>(a.d_dst) - r.dmin, a.d_blk, r.hi - r.lo, a.stream);
        if (rc) break;
        if (!step(hipMemcpyAsync(blocks + r.lo, a.d_blk, (r.hi - r.lo) * sizeof(fourmc_block), hipMemcpyDeviceToHost, a.stream), "hipMemcpyAsync")) break;
    }
    for (size_t k = 0; k < rg.size(); k++) {                                          // results, then what each block produced
        Arena& a = g_arenas[k]; const Range& r = rg[k];
        if (!a.stream) continue;
        (void)hipSetDevice(a.device);
        hipError_t e = hipStreamSynchronize(a.stream);
        if (e != hipSuccess && rc == FOURMC_OK) rc = fail_hip(e, "hipStreamSynchronize");
        if (rc != FOURMC_OK || op == 4) continue;
        for (uint32_t b = r.lo; b < r.hi; b++)
            if (blocks[b].result > 0) {
                e = hipMemcpyAsync(static_cast<char*>(dst) + blocks[b].dst_off, static_cast<char*>(a.d_dst) + (blocks[b].dst_off - r.dmin),
                                   (size_t)blocks[b].result, hipMemcpyDeviceToHost, a.stream);
                if (e != hipSuccess && rc == FOURMC_OK) rc = fail_hip(e, "hipMemcpyAsync");
            }
    }
    for (size_t k = 0; k < rg.size(); k++) {
        Arena& a = g_arenas[k];
        if (!a.stream) continue;
        (void)hipSetDevice(a.device);
        hipError_t e = hipStreamSynchronize(a.stream);
        if (e != hipSuccess && rc == FOURMC_OK) rc = fail_hip(e, "hipStreamSynchronize");
    }
    (void)hipSetDevice(dev0);
    return rc;
}

static int host_roundtrip_many(const void* src, size_t src_bytes, void* dst, size_t dst_bytes,
                               fourmc_block* blocks, uint32_t n, int op, int codec, int level)
{
    if (int r = ensure_device()) return r;
    std::lock_guard<std::mutex> lk(g_mu);
    if (host_shards() > 1 && n > 1) return host_roundtrip_sharded(src, dst, blocks, n, op, codec, level, host_shards());
    if (int r = arena_reserve(g_arena, src_bytes, dst_bytes, n)) return r;
    hipStream_t s = g_arena.stream;
    HIP_TRY(hipMemcpyAsync(g_arena.d_src, src, src_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(g_arena.d_blk, blocks, n * sizeof(fourmc_block), hipMemcpyHostToDevice, s));
    if (int r = launch_host_op(op, codec, level, g_arena.d_src, g_arena.d_dst, g_arena.d_blk, n, s)) return r;
    HIP_TRY(hipMemcpyAsync(blocks, g_arena.d_blk, n * sizeof(fourmc_block), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (op != 4) {
        // copy back only what each block produced
        for (uint32_t b = 0; b < n; b++) {
            if (blocks[b].result > 0)
                HIP_TRY(hipMemcpyAsync(static_cast<char*>(dst) + blocks[b].dst_off,
                                       static_cast<char*>(g_arena.d_dst) + blocks[b].dst_off,
                                       (size_t)blocks[b].result, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FOURMC_OK;
}

// ---- one-block calls (the JNI methods, the LZ4_* / ZSTD_* twins).  One call is one block and returns synchronously, so
// a lone caller cannot be batched - but Hadoop runs many compressor objects on many threads.  Calls that arrive while a
// launch is in flight queue up; the caller that finds nobody serving becomes the server and takes everything queued for
// the same operation into ONE staging copy and ONE launch.  No timer: a lone caller pays nothing, concurrency batches itself.
struct OneReq {
    const void* src; size_t src_bytes; void* dst; size_t dst_bytes; fourmc_block* blk;
    int op, codec, level, rc; bool done; OneReq* next;
    char err[256];                      // fourmc_gpu_last_error() of the launch that served the request
};
static std::mutex g_qmu;
static std::condition_variable g_qcv;
static OneReq* g_qhead = nullptr; static OneReq* g_qtail = nullptr;
static bool g_qserving = false;
static unsigned long long g_one_calls = 0, g_one_launches = 0;

static int serve_group(std::vector<OneReq*>& g)
{
    if (int r = ensure_device()) return r;
    std::lock_guard<std::mutex> lk(g_mu);
    const uint32_t n = (uint32_t)g.size();
    std::vector<fourmc_block> blocks(n);
    size_t so = 0, dof = 0;
    for (uint32_t i = 0; i < n; i++) {
        blocks[i] = *g[i]->blk;
        blocks[i].src_off = so; blocks[i].dst_off = dof;
        so += (g[i]->src_bytes + 63) & ~size_t(63); dof += (g[i]->dst_bytes + 63) & ~size_t(63);
    }
    if (int r = arena_reserve(g_arena, so, dof, n)) return r;
    hipStream_t s = g_arena.stream;
    for (uint32_t i = 0; i < n; i++)
        if (g[i]->src_bytes) HIP_TRY(hipMemcpyAsync(static_cast<char*>(g_arena.d_src) + blocks[i].src_off, g[i]->src, g[i]->src_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(g_arena.d_blk, blocks.data(), n * sizeof(fourmc_block), hipMemcpyHostToDevice, s));
    if (int r = launch_host_op(g[0]->op, g[0]->codec, g[0]->level, g_arena.d_src, g_arena.d_dst, g_arena.d_blk, n, s)) return r;
    HIP_TRY(hipMemcpyAsync(blocks.data(), g_arena.d_blk, n * sizeof(fourmc_block), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (uint32_t i = 0; i < n; i++) {
        g[i]->blk->result = blocks[i].result; g[i]->blk->xxh32 = blocks[i].xxh32;
        if (g[i]->op != 4 && blocks[i].result > 0)
            HIP_TRY(hipMemcpyAsync(g[i]->dst, static_cast<char*>(g_arena.d_dst) + blocks[i].dst_off, (size_t)blocks[i].result, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return FOURMC_OK;
}

static int host_one(const void* src, size_t src_bytes, void* dst, size_t dst_bytes, fourmc_block* blk, int op, int codec, int level)
{
    OneReq me = {src, src_bytes, dst, dst_bytes, blk, op, codec, level, FOURMC_OK, false, nullptr, {0}};
    std::unique_lock<std::mutex> lk(g_qmu);
    g_one_calls++;
    if (g_qtail) g_qtail->next = &me; else g_qhead = &me;
    g_qtail = &me;
    // Whoever finds nobody serving serves ONE group (the oldest request's kind) and hands the role on: a caller never
    // keeps serving other threads' requests after its own has been answered.
    for (;;) {
        if (me.done) { if (me.rc) snprintf(g_err, sizeof g_err, "%s", me.err); return me.rc; }
        if (g_qserving) { g_qcv.wait(lk, [&] { return me.done || !g_qserving; }); continue; }
        g_qserving = true;
        {
        // everything queued for the same operation as the oldest request, in arrival order
        std::vector<OneReq*> grp;
        OneReq* keep_head = nullptr; OneReq* keep_tail = nullptr;
        const OneReq* first = g_qhead;
        for (OneReq* r = g_qhead; r; ) {
            OneReq* nx = r->next; r->next = nullptr;
            if (r->op == first->op && r->codec == first->codec && r->level == first->level && grp.size() < 4096) grp.push_back(r);
            else { if (keep_tail) keep_tail->next = r; else keep_head = r; keep_tail = r; }
            r = nx;
        }
        g_qhead = keep_head; g_qtail = keep_tail;
        g_one_launches++;
        lk.unlock();
        const int rc = serve_group(grp);
        char err[256]; snprintf(err, sizeof err, "%s", g_err);
        lk.lock();
        for (OneReq* r : grp) { r->rc = rc; if (rc) memcpy(r->err, err, sizeof err); r->done = true; }
        }
        g_qserving = false;
        g_qcv.notify_all();
    }
}

static int host_roundtrip(const void* src, size_t src_bytes, void* dst, size_t dst_bytes,
                          fourmc_block* blocks, uint32_t n, int op, int codec, int level)
{
    if (n == 1 && op >= 2) return host_one(src, src_bytes, dst, dst_bytes, blocks, op, codec, level);
    return host_roundtrip_many(src, src_bytes, dst, dst_bytes, blocks, n, op, codec, level);
}

void fourmc_gpu_one_block_stats(unsigned long long* calls, unsigned long long* launches)
{
    std::lock_guard<std::mutex> lk(g_qmu);
    if (calls) *calls = g_one_calls;
    if (launches) *launches = g_one_launches;
}
#ifdef FOURMC_RESEARCH
void fourmc_debug_one_block_counters(unsigned long long* calls, unsigned long long* launches) { fourmc_gpu_one_block_stats(calls, launches); }
#endif

/* page-locked host buffers for the file API's staging (H2D / D2H at PCIe rate instead of the pageable path's bounce copies);
 * NULL when no device is usable or the allocation fails - the caller then falls back to malloc() */
void* fourmc_host_alloc(size_t bytes)
{
    if (ensure_device() != FOURMC_OK) return nullptr;
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void fourmc_host_free(void* p) { if (p) (void)hipHostFree(p); }

int fourmc_host_4mc_encode(const void* src, size_t src_bytes, void* dst, size_t dst_bytes,
                           fourmc_block* blocks, uint32_t n, int codec, int level)
{ return host_roundtrip(src, src_bytes, dst, dst_bytes, blocks, n, 0, codec, level); }

int fourmc_host_4mc_decode(const void* src, size_t src_bytes, void* dst, size_t dst_bytes,
                           fourmc_block* blocks, uint32_t n, int codec)
{ return host_roundtrip(src, src_bytes, dst, dst_bytes, blocks, n, 1, codec, 0); }

// Encode `n` blocks and hand back the finished piece of the .4mc / .4mz file: "12-byte header + payload" per block, back
// to back (native/4mc.c:309-315), laid down in HBM by pack.hip and copied to `image` in ONE transfer - `image` may be the
// file itself (a shared mapping): nothing passes through a staging buffer or stdio.  image_off[b] = where block b's header
// sits in the piece (the footer index is built from these), *image_bytes = its length.
int fourmc_host_4mc_encode_image(const void* src, size_t src_bytes, fourmc_block* blocks, uint32_t n, int codec, int level,
                                 void* image, size_t image_cap, uint64_t* image_off, size_t* image_bytes)
{
    if (int r = ensure_device()) return r;
    if (n == 0) { *image_bytes = 0; return FOURMC_OK; }
    std::lock_guard<std::mutex> lk(g_mu);
    static void* d_img = nullptr; static size_t img_cap = 0; static int img_dev = -1;          // guarded by g_mu, like the arena; keyed by the device
    static uint64_t* d_ioff = nullptr; static size_t ioff_cap = 0; static int ioff_dev = -1;
    size_t dst_bytes = 0;
    for (uint32_t b = 0; b < n; b++) dst_bytes = std::max<size_t>(dst_bytes, blocks[b].dst_off + blocks[b].dst_cap);
    if (int r = arena_reserve(g_arena, src_bytes, dst_bytes, n)) return r;
    hipStream_t s = g_arena.stream;
    // every exit behind the first asynchronous copy waits for the stream: the copies read and write the CALLER's memory (the
    // descriptor array, the mapped files), and the next user of the arena must not meet them still in flight
    int rc = FOURMC_OK; uint64_t pos = 0;
    auto step = [&](hipError_t e, const char* what) { if (rc == FOURMC_OK && e != hipSuccess) rc = fail_hip(e, what); return rc == FOURMC_OK; };
    do {
        if (!step(hipMemcpyAsync(g_arena.d_src, src, src_bytes, hipMemcpyHostToDevice, s), "H2D source")) break;
        if (!step(hipMemcpyAsync(g_arena.d_blk, blocks, n * sizeof(fourmc_block), hipMemcpyHostToDevice, s), "H2D descriptors")) break;
        if (int r = launch_host_op(0, codec, level, g_arena.d_src, g_arena.d_dst, g_arena.d_blk, n, s)) { rc = r; break; }
        if (!step(hipMemcpyAsync(blocks, g_arena.d_blk, n * sizeof(fourmc_block), hipMemcpyDeviceToHost, s), "D2H descriptors")) break;
        if (!step(hipStreamSynchronize(s), "hipStreamSynchronize")) break;
        for (uint32_t b = 0; b < n && rc == FOURMC_OK; b++) {
            if (blocks[b].result <= 0 || uint32_t(blocks[b].result) > blocks[b].src_len) { snprintf(g_err, sizeof g_err, "block %u: encoder returned %d", b, blocks[b].result); rc = FOURMC_EINVAL; break; }
            image_off[b] = pos; pos += 12ull + uint32_t(blocks[b].result);
        }
        if (rc != FOURMC_OK) break;
        if (pos > image_cap) { snprintf(g_err, sizeof g_err, "image capacity %zu below %llu", image_cap, (unsigned long long)pos); rc = FOURMC_EINVAL; break; }
        if (pos > img_cap || img_dev != g_device.load()) {
            if (d_img) step(hipFree(d_img), "hipFree"); d_img = nullptr; img_cap = 0;
            if (!step(hipMalloc(&d_img, pos + pos / 8 + 4096), "hipMalloc image")) break;
            img_cap = pos + pos / 8 + 4096; img_dev = g_device.load();
        }
        if (n > ioff_cap || ioff_dev != g_device.load()) {
            if (d_ioff) step(hipFree(d_ioff), "hipFree"); d_ioff = nullptr; ioff_cap = 0;
            if (!step(hipMalloc(&d_ioff, (size_t(n) + 64) * 8), "hipMalloc offsets")) break;
            ioff_cap = size_t(n) + 64; ioff_dev = g_device.load();
        }
        if (!step(hipMemcpyAsync(d_ioff, image_off, size_t(n) * 8, hipMemcpyHostToDevice, s), "H2D offsets")) break;
        if (!step(fourmc_launch_pack_image(g_arena.d_dst, d_img, g_arena.d_blk, d_ioff, n, s), "pack")) break;
        if (!step(hipMemcpyAsync(image, d_img, pos, hipMemcpyDeviceToHost, s), "D2H image")) break;
    } while (0);
    { const hipError_t e = hipStreamSynchronize(s); if (rc == FOURMC_OK && e != hipSuccess) rc = fail_hip(e, "hipStreamSynchronize"); }
    if (rc != FOURMC_OK) return rc;
    *image_bytes = pos;
    return FOURMC_OK;
}

int fourmc_LZ4_compress_default(const char* src, char* dst, int srcSize, int dstCapacity)
{
    if (srcSize < 0 || dstCapacity < 0) return 0;
    fourmc_block b; memset(&b, 0, sizeof b);
    b.src_len = (uint32_t)srcSize; b.dst_cap = (uint32_t)dstCapacity;
    size_t dst_bytes = (size_t)dstCapacity;
    int r = host_roundtrip(src, (size_t)srcSize, dst, dst_bytes, &b, 1, 2, FOURMC_CODEC_LZ4_FAST, 0);
    if (r) { fprintf(stderr, "4mc-gpu: %s\n", g_err); return 0; }
    return b.result;
}

static int host_mc(const char* src, char* dst, int srcSize, uint32_t cap_field, size_t dst_bytes)
{
    if (srcSize < 0) return 0;
    fourmc_block b; memset(&b, 0, sizeof b);
    b.src_len = (uint32_t)srcSize; b.dst_cap = cap_field;
    int r = host_roundtrip(src, (size_t)srcSize, dst, dst_bytes, &b, 1, 7, FOURMC_CODEC_LZ4_MC, 0);
    if (r) { fprintf(stderr, "4mc-gpu: %s\n", g_err); return 0; }
    return b.result;
}

/* LZ4_compressMC writes without an output limit: dst must hold LZ4_compressBound(srcSize) (lz4mc.h) */
int fourmc_LZ4_compressMC(const char* src, char* dst, int srcSize)
{ return host_mc(src, dst, srcSize, 0xFFFFFFFFu, (size_t)fourmc_LZ4_compressBound(srcSize)); }

int fourmc_LZ4_compressMC_limitedOutput(const char* src, char* dst, int srcSize, int maxOutputSize)
{ return maxOutputSize < 0 ? 0 : host_mc(src, dst, srcSize, (uint32_t)maxOutputSize, (size_t)maxOutputSize); }

int fourmc_LZ4_compress_HC(const char* src, char* dst, int srcSize, int dstCapacity, int compressionLevel)
{
    if (srcSize < 0 || dstCapacity < 0) return 0;
    fourmc_block b; memset(&b, 0, sizeof b);
    b.src_len = (uint32_t)srcSize; b.dst_cap = (uint32_t)dstCapacity;
    int r = host_roundtrip(src, (size_t)srcSize, dst, (size_t)dstCapacity, &b, 1, 6, FOURMC_CODEC_LZ4_HC, compressionLevel);
    if (r) { fprintf(stderr, "4mc-gpu: %s\n", g_err); return 0; }
    return b.result;
}

int fourmc_LZ4_decompress_safe(const char* src, char* dst, int compressedSize, int dstCapacity)
{
    if (compressedSize < 0 || dstCapacity < 0) return -1;
    fourmc_block b; memset(&b, 0, sizeof b);
    b.src_len = (uint32_t)compressedSize; b.dst_cap = (uint32_t)dstCapacity;
    int r = host_roundtrip(src, (size_t)compressedSize, dst, (size_t)dstCapacity, &b, 1, 3, FOURMC_CODEC_LZ4_FAST, 0);
    if (r) { fprintf(stderr, "4mc-gpu: %s\n", g_err); return -1; }
    return b.result;
}

size_t fourmc_ZSTD_decompress(void* dst, size_t dstCapacity, const void* src, size_t compressedSize)
{
    const size_t kCorrupt = (size_t)-20;           /* ZSTD_error_corruption_detected: ZSTD_isError() is true */
    if (compressedSize > 0x7FFFFFFFu || dstCapacity > 0x7FFFFFFFu) return (size_t)-72;   /* srcSize_wrong */
    fourmc_block b; memset(&b, 0, sizeof b);
    b.src_len = (uint32_t)compressedSize; b.dst_cap = (uint32_t)dstCapacity;
    int r = host_roundtrip(src, compressedSize, dst, dstCapacity, &b, 1, 5, FOURMC_CODEC_ZSTD, 0);
    if (r) { fprintf(stderr, "4mc-gpu: %s\n", g_err); return (size_t)-1; }
    return b.result < 0 ? kCorrupt : (size_t)b.result;
}

size_t fourmc_ZSTD_compressBound(size_t n)
{ return n + (n >> 8) + (n < (128u << 10) ? ((128u << 10) - n) >> 11 : 0); }

size_t fourmc_ZSTD_compress(void* dst, size_t dstCapacity, const void* src, size_t srcSize, int compressionLevel)
{
    if (srcSize > 0x7FFFFFFFu) return (size_t)-72;                           /* srcSize_wrong */
    if (dstCapacity > 0x7FFFFFFFu) dstCapacity = 0x7FFFFFFFu;                /* Java passes 1 GiB (jniZstdCompressor.c:93) */
    const size_t bound = fourmc_ZSTD_compressBound(srcSize);
    const size_t cap = dstCapacity < bound ? dstCapacity : bound;            /* the frame never exceeds the bound */
    fourmc_block b; memset(&b, 0, sizeof b);
    b.src_len = (uint32_t)srcSize; b.dst_cap = (uint32_t)cap;
    int r = host_roundtrip(src, srcSize, dst, cap, &b, 1, 8, FOURMC_CODEC_ZSTD, compressionLevel);
    if (r) { fprintf(stderr, "4mc-gpu: %s\n", g_err); return (size_t)-1; }
    return b.result < 0 ? (size_t)(ptrdiff_t)b.result : (size_t)b.result;  /* -(error number), ZSTD_isError() is true */
}

} // extern "C"
