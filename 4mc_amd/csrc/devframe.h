// 4mc_amd/csrc/devframe.h - what the framing kernels share (image.hip, bstream.hip): big-endian u32 fields at any byte offset and
// the wave64 prefix sum their scans are built on.
#ifndef FOURMC_DEVFRAME_H
#define FOURMC_DEVFRAME_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__device__ __forceinline__ uint32_t be32(const uint8_t* p)
{ return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | uint32_t(p[3]); }
__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v)
{ p[0] = uint8_t(v >> 24); p[1] = uint8_t(v >> 16); p[2] = uint8_t(v >> 8); p[3] = uint8_t(v); }

// wave64 inclusive prefix sum: 4 row_shr steps scan each row of 16 lanes, row_bcast15 / row_bcast31 carry the row totals
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t dpp0(uint32_t v)
{ return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), CTRL, ROWMASK, 0xf, false)); }
__device__ __forceinline__ uint32_t scan_add(uint32_t v)
{
    v += dpp0<0x111, 0xf>(v); v += dpp0<0x112, 0xf>(v); v += dpp0<0x114, 0xf>(v); v += dpp0<0x118, 0xf>(v);
    v += dpp0<0x142, 0xa>(v);
    v += dpp0<0x143, 0xc>(v);
    return v;
}
__device__ __forceinline__ uint32_t wave_total(uint32_t incl) { return uint32_t(__builtin_amdgcn_readlane(int(incl), 63)); }

} // namespace
#endif
