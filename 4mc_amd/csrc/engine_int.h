// 4mc_amd/csrc/engine_int.h — what the engine_*.hip files share: the host side of the C ABI is one file per call family, and this
// header is the only way state passes between them.  Declarations only (the definitions are in engine.hip unless a line says
// otherwise); none of it is part of the library's dynamic symbol table.
#ifndef FOURMC_ENGINE_INT_H
#define FOURMC_ENGINE_INT_H
#include <hip/hip_runtime.h>
#include <mutex>
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

#pragma GCC visibility push(hidden)

// fourmc_gpu_last_error().  __thread, not thread_local: across translation units a thread_local is reached through an init wrapper
// whose weak, hidden reference does not resolve to null in a shared library, and the first use from another file crashes.
extern __thread char g_err[512];
extern std::mutex g_mu;                       // guards device selection and the host-staging arena
extern std::atomic<int> g_device;
int fail_hip(hipError_t e, const char* what);
#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail_hip(e_, #x); } while (0)
int ensure_device();                          // every entry point passes through here

inline size_t align256(size_t x) { return (x + 255) & ~size_t(255); }

// Device workspaces (per-block scratch of the kernels: LZ4 decode records, LZ4 HC/MC tables, zstd literals / sequence
// areas / encoder tables).  ONE GROWABLE BUFFER PER STREAM: launches on a stream are ordered, so consecutive calls on the
// same stream can share a buffer, while calls on different streams (the JNI queue's own stream next to a device-API
// caller's, two device-API callers) never see each other's scratch.  A lease keeps the stream's entry locked from the
// moment the pointer is handed out until the caller's launches are enqueued; growing synchronizes THAT stream before the
// old buffer is freed, so no launch can still be using it.
struct StreamWs { std::mutex mu; void* p = nullptr; size_t cap = 0; };
extern std::map<hipStream_t, StreamWs*> g_ws;
// The image calls (image.hip) keep their descriptors, offsets and staging slots in a second registry of the same kind: they hold
// that lease while the codec launches they make lease the stream's workspace.
extern std::map<hipStream_t, StreamWs*> g_img_ws;
// image_read's descriptors and staging slots: a third registry, so that sizing them after the plan's read-back cannot move the
// index and the plan that the second one holds
extern std::map<hipStream_t, StreamWs*> g_img_stage;
// The line writers (engine_text.hip) call the write planner's host path, which leases and may grow both of those: their own tables
// (items, tile prefixes, per-line offsets) and their staging (the packed text and its write table) live in two registries of their own
extern std::map<hipStream_t, StreamWs*> g_txt_ws;
extern std::map<hipStream_t, StreamWs*> g_txt_stage;

class WsLease {
    StreamWs* w_ = nullptr;
    std::map<hipStream_t, StreamWs*>* reg_ = &g_ws;
public:
    WsLease() {}
    explicit WsLease(std::map<hipStream_t, StreamWs*>* reg) : reg_(reg) {}
    WsLease(const WsLease&) = delete;
    ~WsLease() { if (w_) w_->mu.unlock(); }
    size_t cap() const { return w_ ? w_->cap : 0; }          // changes exactly when get() had to grow the buffer
    int get(hipStream_t s, size_t need, void** out);
};
int lease_codec_ws(WsLease& ws, hipStream_t s, size_t need, void** work);      // honours FOURMC_WS_FAIL_ABOVE

// ---- the region checks of the many-item calls: all of them run before a device is looked for
// [off, off + len) does not lie inside [0, total): the comparison that cannot overflow
inline bool span_outside(uint64_t off, uint64_t len, uint64_t total) { return off > total || len > total - off; }
// sorts the [first, second) regions and compares neighbours: FOURMC_OK, or FOURMC_EINVAL with "<who>: <what> overlap at <first>"
int regions_overlap(const char* who, const char* what, std::vector<std::pair<uint64_t, uint64_t>>& r);

// What images_decompress, bstreams_decompress and zsts_decompress check of their n > 0 items: every stream inside the buffer, and -
// unless the call is a size query, which looks at no destination - every output region inside the destination and no two
// non-empty ones overlapping.  `one` / `many`: "image" / "images", "stream" / "streams".
template <class Item>
int decode_items_args(const char* who, const char* one, const char* many, const void* d_images, uint64_t images_bytes, const void* d_dst,
                      uint64_t dst_bytes, const Item* items, uint32_t n)
{
    if (!items) { snprintf(g_err, sizeof g_err, "%s: null items", who); return FOURMC_EINVAL; }
    std::vector<std::pair<uint64_t, uint64_t>> d;
    if (d_dst) d.reserve(n);
    for (uint32_t i = 0; i < n; i++) {
        const Item& it = items[i];
        if (it.image_bytes && !d_images) { snprintf(g_err, sizeof g_err, "%s: null images", who); return FOURMC_EINVAL; }
        if (span_outside(it.image_off, it.image_bytes, images_bytes)) {
            snprintf(g_err, sizeof g_err, "%s: %s %u lies beyond the %llu bytes of %s", who, one, i, (unsigned long long)images_bytes, many);
            return FOURMC_EINVAL;
        }
        if (!d_dst) continue;                             // the size query looks at no destination
        if (span_outside(it.dst_off, it.dst_cap, dst_bytes)) {
            snprintf(g_err, sizeof g_err, "%s: the output region of %s %u lies beyond the %llu bytes of the destination", who, one, i,
                     (unsigned long long)dst_bytes);
            return FOURMC_EINVAL;
        }
        if (it.dst_cap) d.emplace_back(it.dst_off, it.dst_off + it.dst_cap);
    }
    return regions_overlap(who, "output regions", d);
}

// The encode side (images_compress, bstreams_compress, images_compress_writes, zsts_compress) keeps its loops - each checks other
// things between these - and shares the words: FOURMC_EINVAL with the message of a source, a write table slice or an image region
// that span_outside() found outside its buffer.  `one`: "image" / "stream".
inline int source_beyond(const char* who, const char* one, uint32_t i, uint64_t src_total)
{
    snprintf(g_err, sizeof g_err, "%s: the source of %s %u lies beyond the %llu bytes of sources", who, one, i, (unsigned long long)src_total);
    return FOURMC_EINVAL;
}
inline int writes_beyond(const char* who, uint32_t i, uint64_t writes_total)
{
    snprintf(g_err, sizeof g_err, "%s: the write sizes of stream %u lie beyond the %llu entries of the table", who, i, (unsigned long long)writes_total);
    return FOURMC_EINVAL;
}
inline int region_beyond(const char* who, const char* one, uint32_t i, uint64_t images_bytes)
{
    snprintf(g_err, sizeof g_err, "%s: the region of %s %u lies beyond the %llu bytes of images", who, one, i, (unsigned long long)images_bytes);
    return FOURMC_EINVAL;
}

// ---- engine_streams.hip
// the raw codec launch of m described blocks, by FOURMC_CODEC_* selector (`level`: the codec's own; the two LZ4 codecs without one ignore it)
int encode_raw_blocks(int codec, int level, const void* d_src, void* d_stage, fourmc_block* d_blk, uint32_t m, hipStream_t s);

// ---- engine_image.hip, for engine_lines.hip and engine_streams.hip
constexpr size_t kImagesStageSlack = 4096;  // bytes behind the staging of the many-image and block-stream encodes
constexpr size_t kIdxBytes = 256;           // fourmc_image_index_dev
// the summary, read back (the call's first synchronization)
int image_index_count(WsLease& ws, hipStream_t s, const void* d_image, uint64_t image_bytes, fourmc_image_index_dev* out);
int image_codec(const fourmc_image_index_dev& idx);

#pragma GCC visibility pop
#endif
