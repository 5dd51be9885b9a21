// ComputeNormalMap's per-texel arithmetic (DirectXTexNormalMaps.cpp:21-47, :77-240), shared by the GPU kernel (scanline.hip,
// nmap_kernel) and the host check (tests/cpp/nmap_check.cpp), so everything here is __host__ __device__. Compiled with
// -ffp-contract=off -fno-fast-math: every product and sum below rounds on its own, in the reference's order.
//
//   height   = the selected channel of LoadScanline's float4 (no sRGB decode); luminance = (r * 0.2125 + g * 0.7154) + b * 0.0721
//   dzx      = (((tL - tR) + (mL - mR)) + (bL - bR)) * amplitude / 6      t / m / b = the rows above / at / below, L / C / R the columns
//   dzy      = (((tL - bL) + (tC - bC)) + (tR - bR)) * amplitude / 6
//   normal   = XMVector3Normalize(XMVector3Cross((-1, 0, dzx), (0, -1, dzy))), both in their SSE2 shape
//   alpha    = 1, or the occlusion term of CNMAP_COMPUTE_OCCLUSION
//   row      = UNORM destination: normal * (+-0.5) + 0.5 (mul, then add); other: normal, or 0 - normal under CNMAP_INVERT_SIGN
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dxtex
{
// CNMAP_FLAGS (DirectXTex.h)
enum : uint32_t
{
    NMAP_CHANNEL_MASK = 0xF, NMAP_CHANNEL_RED = 1, NMAP_CHANNEL_GREEN = 2, NMAP_CHANNEL_BLUE = 3, NMAP_CHANNEL_ALPHA = 4,
    NMAP_CHANNEL_LUMINANCE = 5, NMAP_MIRROR_U = 0x1000, NMAP_MIRROR_V = 0x2000, NMAP_INVERT_SIGN = 0x4000, NMAP_COMPUTE_OCCLUSION = 0x8000,
};

struct NmapOut { float x, y, z, w; };

__host__ __device__ inline uint32_t nmap_bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
__host__ __device__ inline float nmap_float(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }

// EvaluateColor: channel 0 and RED read x. The luminance products are formed lane-wise (XMVectorMultiply), then summed x + y + z.
__host__ __device__ inline float nmap_height(float r, float g, float b, float a, uint32_t flags)
{
    switch (flags & NMAP_CHANNEL_MASK)
    {
    case NMAP_CHANNEL_GREEN: return g;
    case NMAP_CHANNEL_BLUE: return b;
    case NMAP_CHANNEL_ALPHA: return a;
    case NMAP_CHANNEL_LUMINANCE:
    {
        const float lr = r * 0.2125f, lg = g * 0.7154f, lb = b * 0.0721f;
        return (lr + lg) + lb;
    }
    default: return r;
    }
}

// The neighbour index of EvaluateRow / the row loads: i in [-1, n]; wrap by default, repeat the edge (the reference's "mirror") when
// clamp is set.
__host__ __device__ inline uint32_t nmap_edge(int64_t i, uint32_t n, bool clamp)
{
    if (i < 0) return clamp ? 0u : n - 1u;
    if (i >= int64_t(n)) return clamp ? n - 1u : 0u;
    return uint32_t(i);
}

// One output texel from the 3 x 3 heights h[row][column] (row 0 = above, column 0 = left): the float4 ComputeNMap hands to StoreScanline.
__host__ __device__ inline NmapOut nmap_texel(const float (&h)[3][3], uint32_t flags, float amplitude, bool unorm)
{
    float tot = ((h[0][0] - h[0][2]) + (h[1][0] - h[1][2])) + (h[2][0] - h[2][2]);
    const float dzx = tot * amplitude / 6.f;
    tot = ((h[0][0] - h[2][0]) + (h[0][1] - h[2][1])) + (h[0][2] - h[2][2]);
    const float dzy = tot * amplitude / 6.f;

    // XMVector3Cross(V1 = (-1, 0, dzx), V2 = (0, -1, dzy)): (y1 z2, z1 x2, x1 y2) - (z1 y2, x1 z2, y1 x2), as products and differences
    const float zero = 0.0f, neg1 = -1.0f;
    const float cx = zero * dzy - dzx * neg1;
    const float cy = dzx * zero - neg1 * dzy;
    const float cz = neg1 * neg1 - zero * zero;

    // XMVector3Normalize, SSE2: len2 = (x^2 + y^2) + z^2, divide by sqrt(len2); a zero length gives 0 (a NaN length passes through),
    // an infinite len2 gives the QNaN pattern
    const float len2 = (cx * cx + cy * cy) + cz * cz;
    const float len = sqrtf(len2);
    float nx, ny, nz;
    if (len2 == nmap_float(0x7F800000u)) nx = ny = nz = nmap_float(0x7FC00000u);
    else if (len == 0.0f) nx = ny = nz = 0.0f;
    else { nx = cx / len; ny = cy / len; nz = cz / len; }

    float alpha = 1.f;
    if (flags & NMAP_COMPUTE_OCCLUSION)
    {
        float delta = 0.f;
        const float c = h[1][1];
        float t;
        t = h[0][0] - c; if (t > 0.f) delta += t;
        t = h[0][1] - c; if (t > 0.f) delta += t;
        t = h[0][2] - c; if (t > 0.f) delta += t;
        t = h[1][0] - c; if (t > 0.f) delta += t;
        t = h[1][2] - c; if (t > 0.f) delta += t;
        t = h[2][0] - c; if (t > 0.f) delta += t;
        t = h[2][1] - c; if (t > 0.f) delta += t;
        t = h[2][2] - c; if (t > 0.f) delta += t;
        delta = delta * (0.125f * amplitude);
        if (delta > 0.f)
        {
            const float r = sqrtf(1.f + delta * delta);
            alpha = (r - delta) / r;
        }
    }

    NmapOut o;
    if (unorm)
    {
        const float s = (flags & NMAP_INVERT_SIGN) ? -0.5f : 0.5f;
        o.x = s * nx + 0.5f; o.y = s * ny + 0.5f; o.z = s * nz + 0.5f;
    }
    else if (flags & NMAP_INVERT_SIGN) { o.x = zero - nx; o.y = zero - ny; o.z = zero - nz; }
    else { o.x = nx; o.y = ny; o.z = nz; }
    o.w = alpha;
    return o;
}
} // namespace dxtex
