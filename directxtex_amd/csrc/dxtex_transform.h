// texconv's per-texel TransformImage lambdas (Texconv/texconv.cpp): swizzle (:2645-2694), tone map (:2966-3044), colour key
// (:3134-3191), invert Y (:3193-3240) and reconstruct Z (:3242-3301). Shared by the GPU kernel (scanline.hip, transform_kernel) and the
// host check (tests/cpp/transform_check.cpp), so everything here is __host__ __device__. Compiled with -ffp-contract=off
// -fno-fast-math: every product and sum below rounds on its own, in the SSE2 order of the DirectXMath calls.
//
//   swizzle        out[k] = in[s[k]]; 0 where zero[k], then 1 where one[k] (XMVectorSwizzle + two XMVectorSelect)
//   tone map       v = (r * 0.3 + g * 0.59) + b * 0.11 (XMVector3Dot), m = maxps(v, m) from +0 over every image, M = m * m;
//                  rgb = c * ((1 + c / M) / (1 + c)), alpha kept
//   colour key     key = XMLoadColor(0x00RRGGBB) = channel * fl(1/255), alpha 0; d = c - key, match when maxps(0 - d, d) <= 0.2f for r, g
//                  and b (XMVector3NearEqual): (0, 0, 0, 0), else alpha = 1
//   invert Y       g = 1 - g
//   reconstruct Z  UNORM: x2 = c * 2 + (-1), z = sqrt(1 - (x2.x^2 + x2.y^2)) * 0.5 + 0.5; else z = sqrt(1 - (x^2 + y^2))
//
// NaN results follow the x86 instructions the reference runs: an operation on a NaN returns the first NaN operand made quiet, and one
// that makes a NaN from numbers (0 / 0, inf / inf, sqrt of a negative) returns the x86 default NaN, 0xFFC00000. Every channel an op does
// not write is moved, never computed, so its bits (NaN payloads, -0) survive.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dxtex
{
// dxtex_transform.op (include/dxtex_amd.h)
enum : uint32_t { XFORM_SWIZZLE = 0, XFORM_TONEMAP = 1, XFORM_COLOR_KEY = 2, XFORM_INVERT_Y = 3, XFORM_RECONSTRUCT_Z = 4 };

// what the kernel needs of a dxtex_transform, resolved on the host
struct XformArgs
{
    uint32_t swz[4];        // source channel of each output channel
    uint32_t zero, one;     // bit k: output channel k is forced to 0 / 1
    float key[3];           // the colour key as XMLoadColor loads it
    int unorm;              // reconstruct Z: FormatDataType(format) == FORMAT_TYPE_UNORM
};

__host__ __device__ inline uint32_t xf_bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
__host__ __device__ inline float xf_float(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }
__host__ __device__ inline bool xf_nan(float f) { return (xf_bits(f) & 0x7FFFFFFFu) > 0x7F800000u; }
__host__ __device__ inline float xf_quiet(float f) { return xf_float(xf_bits(f) | 0x00400000u); }
constexpr uint32_t kXfDefaultNaN = 0xFFC00000u;       // the x86 "real indefinite"

// the x86 NaN of a result computed from inputs a (then b): the first NaN input made quiet, else the default NaN where r is a NaN
__host__ __device__ inline float xf_nan_of(float r, float a, float b)
{
    if (xf_nan(a)) return xf_quiet(a);
    if (xf_nan(b)) return xf_quiet(b);
    return xf_nan(r) ? xf_float(kXfDefaultNaN) : r;
}

__host__ __device__ inline void xf_swizzle(float (&c)[4], const XformArgs& a)
{
    const float in[4] = { c[0], c[1], c[2], c[3] };
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        const uint32_t s = a.swz[k];
        float v = s == 0 ? in[0] : s == 1 ? in[1] : s == 2 ? in[2] : in[3];
        if (a.zero & (1u << k)) v = 0.0f;
        if (a.one & (1u << k)) v = 1.0f;
        c[k] = v;
    }
}

// XMVector3Dot(c, (0.3, 0.59, 0.11, 0)) in the shim's order, and the bits it adds to the running maximum: maxps(v, m) keeps m for a NaN
// v and m never falls below +0, so max(m, v) over non-negative floats = max of these bits read as unsigned integers
__host__ __device__ inline float xf_luminance(float r, float g, float b) { return (r * 0.3f + g * 0.59f) + b * 0.11f; }
__host__ __device__ inline uint32_t xf_lum_bits(float r, float g, float b)
{
    const float v = xf_luminance(r, g, b);
    return v > 0.0f ? xf_bits(v) : 0u;
}

// maxLum = XMVectorMultiply(maxLum, maxLum); value * ((1 + value / M) / (1 + value)) on r, g, b
__host__ __device__ inline float xf_tonemap1(float v, float M)
{
    const float scale = (1.0f + v / M) / (1.0f + v);
    return xf_nan_of(v * scale, v, M);
}
__host__ __device__ inline void xf_tonemap(float (&c)[4], float M)
{
    c[0] = xf_tonemap1(c[0], M); c[1] = xf_tonemap1(c[1], M); c[2] = xf_tonemap1(c[2], M);
}

// XMLoadColor of colorKey & 0xFFFFFF: (channel << shift) * (1 / (255 * 2^shift)) = channel * fl(1/255) exactly
__host__ __device__ inline void xf_color_key_value(uint32_t key, float (&k)[3])
{
    const float s = 1.0f / 255.0f;
    k[0] = float((key >> 16) & 0xFFu) * s; k[1] = float((key >> 8) & 0xFFu) * s; k[2] = float(key & 0xFFu) * s;
}
// XMVector3NearEqual: maxps(0 - d, d) <= eps per lane; maxps(a, b) = a > b ? a : b (b when either is NaN), so a NaN never matches
__host__ __device__ inline bool xf_near(float v, float key)
{
    const float d = v - key, n = 0.0f - d;
    const float m = n > d ? n : d;
    return m <= 0.2f;
}
__host__ __device__ inline void xf_color_key(float (&c)[4], const XformArgs& a)
{
    if (xf_near(c[0], a.key[0]) && xf_near(c[1], a.key[1]) && xf_near(c[2], a.key[2])) { c[0] = c[1] = c[2] = c[3] = 0.0f; return; }
    c[3] = 1.0f;
}

__host__ __device__ inline void xf_invert_y(float (&c)[4]) { c[1] = xf_nan_of(1.0f - c[1], c[1], 0.0f); }

// XMVectorMultiplyAdd (SSE2: multiply, then add), XMVector2Dot (x * x + y * y), XMVectorSqrt (sqrtps: correctly rounded)
__host__ __device__ inline void xf_reconstruct_z(float (&c)[4], int unorm)
{
    const float x = c[0], y = c[1];
    float z;
    if (unorm)
    {
        const float x2 = x * 2.0f + -1.0f, y2 = y * 2.0f + -1.0f;
        z = sqrtf(1.0f - (x2 * x2 + y2 * y2)) * 0.5f + 0.5f;
    }
    else z = sqrtf(1.0f - (x * x + y * y));
    c[2] = xf_nan_of(z, x, y);
}

template<uint32_t OP>
__host__ __device__ inline void xf_apply(float (&c)[4], const XformArgs& a, float M)
{
    if constexpr (OP == XFORM_SWIZZLE) xf_swizzle(c, a);
    else if constexpr (OP == XFORM_TONEMAP) xf_tonemap(c, M);
    else if constexpr (OP == XFORM_COLOR_KEY) xf_color_key(c, a);
    else if constexpr (OP == XFORM_INVERT_Y) xf_invert_y(c);
    else xf_reconstruct_z(c, a.unorm);
}
} // namespace dxtex
