// 4mc_amd/csrc/lz4_emit.hip — the byte emitter of the exact LZ4 fast encoder: turns the sequence records K2
// (lz4_encode.hip) left in the workspace into the LZ4 payloads, after the parse and outside its dependency chain.
//
// Every record carries its output position and its literals' source position (lz4emit.h), so the records of a launch
// are independent of one another: kEmitGroups workgroups per block, each wavefront takes 64 records at a time, one
// per lane.  A block stored raw (container mode, the encode did not fit) is copied by the same workgroups, each a
// slice.  Exactly `result` bytes are written per block, nothing past them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fourmc_gpu.h"
#include "kernels.h"
#include "lz4emit.h"

namespace {

constexpr uint32_t kEmitGroups = 8;     // workgroups per block
constexpr int      kEmitThreads = 256;  // four wavefronts

__global__ __launch_bounds__(kEmitThreads)
void lz4_emit_kernel(const uint8_t* __restrict__ src_base, uint8_t* __restrict__ dst_base, const fourmc_block* blocks,
                     uint32_t nblocks, const uint8_t* __restrict__ work, uint32_t reccap)
{
    const uint32_t b = blockIdx.x / kEmitGroups, g = blockIdx.x % kEmitGroups;
    if (b >= nblocks) return;
    const uint32_t cnt = reinterpret_cast<const uint32_t*>(work)[b];
    if (cnt == 0) return;
    const fourmc_block blk = uniform_block(blocks[b]);
    const uint8_t* src = src_base + blk.src_off;
    uint8_t* dst = dst_base + blk.dst_off;
    if (cnt == kRecRawCopy) {                                           // native/4mc.c:318-324: the input as it is
        const uint32_t n = blk.src_len;
        const uint32_t slice = ((n + kEmitGroups - 1) / kEmitGroups + 15) & ~15u;
        const uint32_t lo = min(n, g * slice), hi = min(n, lo + slice);
        copy_group<kEmitThreads>(dst + lo, src + lo, hi - lo, int(threadIdx.x));
        return;
    }
    const uint4* rec = reinterpret_cast<const uint4*>(work + lz4rec_count_bytes(nblocks) + size_t(b) * lz4rec_area_bytes(reccap));
    const uint32_t wave = threadIdx.x / 64;
    const int lane = int(threadIdx.x % 64);
    constexpr uint32_t kWaves = kEmitThreads / 64;
    for (uint32_t t = g * kWaves + wave; size_t(t) * 64 < cnt; t += kEmitGroups * kWaves)
        emit_records(rec, t * 64, cnt, 0, src, dst, lane);
}

} // namespace

extern "C" hipError_t fourmc_launch_lz4_emit(const void* d_src, void* d_dst, const fourmc_block* d_blocks, uint32_t n,
                                             const void* d_work, uint32_t reccap, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(lz4_emit_kernel, dim3(n * kEmitGroups), dim3(kEmitThreads), 0, stream,
                       static_cast<const uint8_t*>(d_src), static_cast<uint8_t*>(d_dst), d_blocks, n,
                       static_cast<const uint8_t*>(d_work), reccap);
    return hipGetLastError();
}
