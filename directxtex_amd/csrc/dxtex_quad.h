// Four consecutive texels of a row through 16-byte accesses: the formats whose texel is a whole number of dwords, and the register image
// of a quad that load_texel / store_texel decode and encode with every index a compile-time constant. Shared by the Convert kernels
// (scanline.hip) and the diagnostics (diag.hip).
#pragma once
#include "dxtex_device.h"

namespace dxtex
{
// every format whose texel is a whole number of dwords (the quad kernels' domain), with the bytes of a quad
#define DXTEX_QUAD_FORMATS(X) \
    X(FMT_R32G32B32A32_FLOAT, 64) X(FMT_R32G32B32A32_UINT, 64) X(FMT_R32G32B32A32_SINT, 64) X(FMT_R32G32B32_FLOAT, 48) X(FMT_R32G32B32_UINT, 48) \
    X(FMT_R32G32B32_SINT, 48) X(FMT_R16G16B16A16_FLOAT, 32) X(FMT_R16G16B16A16_UNORM, 32) X(FMT_R16G16B16A16_UINT, 32) X(FMT_R16G16B16A16_SNORM, 32) \
    X(FMT_R16G16B16A16_SINT, 32) X(FMT_R32G32_FLOAT, 32) X(FMT_R32G32_UINT, 32) X(FMT_R32G32_SINT, 32) X(FMT_Y416, 32) \
    X(FMT_R10G10B10A2_UNORM, 16) X(FMT_R10G10B10A2_UINT, 16) X(FMT_R11G11B10_FLOAT, 16) X(FMT_R8G8B8A8_UNORM, 16) X(FMT_R8G8B8A8_UNORM_SRGB, 16) \
    X(FMT_R8G8B8A8_UINT, 16) X(FMT_R8G8B8A8_SNORM, 16) X(FMT_R8G8B8A8_SINT, 16) X(FMT_R16G16_FLOAT, 16) X(FMT_R16G16_UNORM, 16) \
    X(FMT_R16G16_UINT, 16) X(FMT_R16G16_SNORM, 16) X(FMT_R16G16_SINT, 16) X(FMT_R32_FLOAT, 16) X(FMT_R32_UINT, 16) \
    X(FMT_R32_SINT, 16) X(FMT_R9G9B9E5_SHAREDEXP, 16) X(FMT_B8G8R8A8_UNORM, 16) X(FMT_B8G8R8X8_UNORM, 16) X(FMT_R10G10B10_XR_BIAS_A2_UNORM, 16) \
    X(FMT_B8G8R8A8_UNORM_SRGB, 16) X(FMT_B8G8R8X8_UNORM_SRGB, 16) X(FMT_AYUV, 16) X(FMT_Y410, 16) X(FMT_D32_FLOAT_S8X24_UINT, 32) \
    X(FMT_D32_FLOAT, 16) X(FMT_D24_UNORM_S8_UINT, 16) X(FMT_R10G10B10_7E3_A2_FLOAT, 16) X(FMT_R10G10B10_6E4_A2_FLOAT, 16) \
    X(FMT_R10G10B10_SNORM_A2_UNORM, 16)

// the bytes of a quad of `format`, 0 for a format outside the list
__host__ __device__ inline uint32_t quad_bytes(int format)
{
    switch (format)
    {
#define DXTEX_QCASE(F, QB) case F: return QB;
        DXTEX_QUAD_FORMATS(DXTEX_QCASE)
#undef DXTEX_QCASE
    default: return 0u;
    }
}

template<int W>
__device__ __forceinline__ void load_quad(uint32_t (&q)[W], const uint8_t* p, uint32_t bytes)
{
    const uint4* v = reinterpret_cast<const uint4*>(p);
    { const uint4 a = v[0]; q[0] = a.x; q[1] = a.y; q[2] = a.z; q[3] = a.w; }
    if constexpr (W >= 8) if (bytes >= 32u) { const uint4 a = v[1]; q[4] = a.x; q[5] = a.y; q[6] = a.z; q[7] = a.w; }
    if constexpr (W >= 12) if (bytes >= 48u) { const uint4 a = v[2]; q[8] = a.x; q[9] = a.y; q[10] = a.z; q[11] = a.w; }
    if constexpr (W >= 16) if (bytes >= 64u) { const uint4 a = v[3]; q[12] = a.x; q[13] = a.y; q[14] = a.z; q[15] = a.w; }
}

template<int W>
__device__ __forceinline__ void store_quad(uint8_t* p, const uint32_t (&q)[W], uint32_t bytes)
{
    uint4* v = reinterpret_cast<uint4*>(p);
    v[0] = make_uint4(q[0], q[1], q[2], q[3]);
    if constexpr (W >= 8) if (bytes >= 32u) v[1] = make_uint4(q[4], q[5], q[6], q[7]);
    if constexpr (W >= 12) if (bytes >= 48u) v[2] = make_uint4(q[8], q[9], q[10], q[11]);
    if constexpr (W >= 16) if (bytes >= 64u) v[3] = make_uint4(q[12], q[13], q[14], q[15]);
}
} // namespace dxtex
