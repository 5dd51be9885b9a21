// texdiag's per-texel and per-block rules (Texdiag/texdiag.cpp): Analyze's luminance and extrema (:698-787), AnalyzeBC's block
// classification (:906-1226), Difference's lambda (:1285-1309), and the per-texel part of ComputeMSE_ with every CMSE_FLAGS bit
// (DirectXTexMisc.cpp:27-176). Shared by the GPU kernels (diag.hip) and the host check (tests/cpp/diag_check.cpp), so everything here
// is __host__ __device__. Compiled with -ffp-contract=off -fno-fast-math: every product and sum rounds on its own, in the SSE2 order of
// the DirectXMath calls.
//
//   luminance    max(+0, (r * 0.3 + g * 0.59) + b * 0.11) (XMVector3Dot under XMVectorMax from zero); a NaN value takes no part
//   extrema      minimum and maximum over the values that are not NaN, starting from +FLT_MAX / -FLT_MAX as the reference does. The
//                reference's minps / maxps keep whichever operand comes second for a NaN and for +0 against -0, so its result depends
//                on texel order; here a NaN is skipped and -0 orders below +0, which no order of evaluation changes. Values travel as
//                monotone unsigned keys (dg_key) so that workgroups can combine them with integer atomics.
//   BC bins      BC1 rgb[0] <= rgb[1] -> 1 else 0; BC3 / BC4 / BC5 endpoint0 > endpoint1 -> 0 else 1 (BC5 green: 2 / 3; SNORM compares
//                signed); BC6H the 2-bit then 5-bit prefix -> 1..14, reserved -> 0; BC7 lowest set bit of byte 0 -> 0..7, none -> 8
//   difference   d = |a - b| on r, g, b (XMVectorAbs: maxps(0 - v, v)), alpha 1; the colour where diffColor != 0 and all three d >= t
//   mse          v^2.2 on r, g, b (powf, correctly rounded; alpha's exponent is 1), then v * 2 - 1 on all four, per image; the ignored channels are zero
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

namespace dxtex
{
// CMSE_FLAGS (DirectXTex.h:1022-1038)
enum : uint32_t
{
    DG_CMSE_IMAGE1_SRGB = 0x1, DG_CMSE_IMAGE2_SRGB = 0x2,
    DG_CMSE_IGNORE_RED = 0x10, DG_CMSE_IGNORE_GREEN = 0x20, DG_CMSE_IGNORE_BLUE = 0x40, DG_CMSE_IGNORE_ALPHA = 0x80,
    DG_CMSE_IMAGE1_X2_BIAS = 0x100, DG_CMSE_IMAGE2_X2_BIAS = 0x200,
};

__host__ __device__ inline uint32_t dg_bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
__host__ __device__ inline float dg_float(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }
__host__ __device__ inline bool dg_nan(float f) { return (dg_bits(f) & 0x7FFFFFFFu) > 0x7F800000u; }
__host__ __device__ inline bool dg_finite(float f) { return (dg_bits(f) & 0x7F800000u) != 0x7F800000u; }

// A float that is not NaN as an unsigned key of the same order (-inf < ... < -0 < +0 < ... < +inf). Keys lie in
// [0x007FFFFF, 0xFF800000]: 0 is below every key, which makes it the identity of a running maximum.
__host__ __device__ inline uint32_t dg_key(float f) { const uint32_t b = dg_bits(f); return (b & 0x80000000u) ? ~b : (b | 0x80000000u); }
__host__ __device__ inline float dg_unkey(uint32_t k) { return dg_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }
constexpr uint32_t kDgFltMaxBits = 0x7F7FFFFFu;

// the running maximum / the complement of the running minimum that an accumulator cell holds (0 = nothing seen) -> the reference's
// result, which starts from -FLT_MAX / +FLT_MAX
__host__ __device__ inline float dg_max_of(uint32_t maxKey)
{
    const uint32_t floor = dg_key(dg_float(kDgFltMaxBits | 0x80000000u));
    return dg_unkey(maxKey > floor ? maxKey : floor);
}
__host__ __device__ inline float dg_min_of(uint32_t minKeyInv)
{
    const uint32_t ceil = dg_key(dg_float(kDgFltMaxBits));
    const uint32_t k = ~minKeyInv;
    return dg_unkey((minKeyInv != 0u && k < ceil) ? k : ceil);
}

// XMVector3Dot(v, (0.3, 0.59, 0.11)) and the bits it contributes to the maximum: +0 unless the value is above zero (a NaN is not)
__host__ __device__ inline float dg_luminance(float r, float g, float b) { return (r * 0.3f + g * 0.59f) + b * 0.11f; }
__host__ __device__ inline uint32_t dg_lum_bits(float r, float g, float b)
{
    const float v = dg_luminance(r, g, b);
    return v > 0.0f ? dg_bits(v) : 0u;
}

// ---- AnalyzeBC ---------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline int dg_bc6h_bin(uint32_t byte0)
{
    switch (byte0 & 0x03u)
    {
    case 0x00: return 1;
    case 0x01: return 2;
    default: break;
    }
    switch (byte0 & 0x1Fu)
    {
    case 0x02: return 3;
    case 0x06: return 4;
    case 0x0A: return 5;
    case 0x0E: return 6;
    case 0x12: return 7;
    case 0x16: return 8;
    case 0x1A: return 9;
    case 0x1E: return 10;
    case 0x03: return 11;
    case 0x07: return 12;
    case 0x0B: return 13;
    case 0x0F: return 14;
    default: return 0;       // 10011, 10111, 11011, 11111: reserved
    }
}
__host__ __device__ inline int dg_bc7_bin(uint32_t byte0)
{
    for (int m = 0; m < 8; ++m)
        if (byte0 & (1u << m)) return m;
    return 8;
}

// bytes of a block of BC format `format` (0: not a BC format this classifier knows)
__host__ __device__ inline uint32_t dg_bc_block_bytes(int format)
{
    switch (format)
    {
    case 71: case 72: case 80: case 81: return 8u;
    case 74: case 75: case 77: case 78: case 83: case 84: case 95: case 96: case 98: case 99: return 16u;
    default: return 0u;
    }
}

// the bins (0..14) one block adds to; -1 = none. Reads at most bytes 0..3 and 8..9 of the block.
__host__ __device__ inline void dg_bc_bins(int format, const uint8_t* block, int& bin0, int& bin1)
{
    bin0 = bin1 = -1;
    switch (format)
    {
    case 71: case 72:        // BC1: the two 565 colours as little-endian words
    {
        const uint32_t c0 = uint32_t(block[0]) | (uint32_t(block[1]) << 8), c1 = uint32_t(block[2]) | (uint32_t(block[3]) << 8);
        bin0 = (c0 <= c1) ? 1 : 0;
        break;
    }
    case 77: case 78: case 80: bin0 = (block[0] > block[1]) ? 0 : 1; break;                     // BC3 alpha, BC4 UNORM
    case 81: bin0 = (int8_t(block[0]) > int8_t(block[1])) ? 0 : 1; break;                       // BC4 SNORM
    case 83: bin0 = (block[0] > block[1]) ? 0 : 1; bin1 = (block[8] > block[9]) ? 2 : 3; break;
    case 84: bin0 = (int8_t(block[0]) > int8_t(block[1])) ? 0 : 1; bin1 = (int8_t(block[8]) > int8_t(block[9])) ? 2 : 3; break;
    case 95: case 96: bin0 = dg_bc6h_bin(block[0]); break;
    case 98: case 99: bin0 = dg_bc7_bin(block[0]); break;
    default: break;          // BC2 has a single kind of block
    }
}

// ---- Difference --------------------------------------------------------------------------------------------------------------------
// XMLoadColor(0x00RRGGBB) with alpha from g_XMIdentityR3: channel * fl(1/255)
__host__ __device__ inline void dg_diff_color(uint32_t diffColor, float (&c)[4])
{
    const float s = 1.0f / 255.0f;
    c[0] = float((diffColor >> 16) & 0xFFu) * s; c[1] = float((diffColor >> 8) & 0xFFu) * s; c[2] = float(diffColor & 0xFFu) * s; c[3] = 1.0f;
}
// XMVectorAbs, SSE2: maxps(0 - v, v) = (0 - v) > v ? (0 - v) : v
__host__ __device__ inline float dg_abs(float v) { const float n = 0.0f - v; return n > v ? n : v; }
// a = image 1's texel (in / out), b = image 2's; color = dg_diff_color(diffColor)
__host__ __device__ inline void dg_difference(float (&a)[4], const float (&b)[4], uint32_t diffColor, const float (&color)[4], float threshold)
{
    const float d0 = dg_abs(a[0] - b[0]), d1 = dg_abs(a[1] - b[1]), d2 = dg_abs(a[2] - b[2]);
    if (diffColor && d0 >= threshold && d1 >= threshold && d2 >= threshold) { a[0] = color[0]; a[1] = color[1]; a[2] = color[2]; a[3] = color[3]; }
    else { a[0] = d0; a[1] = d1; a[2] = d2; a[3] = 1.0f; }
}

// ---- ComputeMSE --------------------------------------------------------------------------------------------------------------------
// XMVectorPow(v, g_Gamma22) per component: scalar powf(v, 2.2f) in DirectXMath's SSE2 build. pow() in double precision rounded once to fp32
// is the correctly rounded powf (dxtex_device.h, pow_rn), the same on the host and on the device.
__host__ __device__ inline float dg_gamma22(float v) { return float(pow(double(v), double(2.2f))); }
// one image's texel before the subtraction: srgb = CMSE_IMAGEn_SRGB, bias = CMSE_IMAGEn_X2_BIAS
__host__ __device__ inline void dg_mse_prepare(float (&c)[4], bool srgb, bool bias)
{
    if (srgb) { c[0] = dg_gamma22(c[0]); c[1] = dg_gamma22(c[1]); c[2] = dg_gamma22(c[2]); }
    if (bias) { c[0] = c[0] * 2.0f + -1.0f; c[1] = c[1] * 2.0f + -1.0f; c[2] = c[2] * 2.0f + -1.0f; c[3] = c[3] * 2.0f + -1.0f; }
}
// the flags an image's format implies (:47-91), for image 1; shift left by one for image 2's sRGB bit
__host__ __device__ inline uint32_t dg_mse_format_flags(int format, bool second)
{
    const uint32_t srgb = second ? DG_CMSE_IMAGE2_SRGB : DG_CMSE_IMAGE1_SRGB;
    switch (format)
    {
    case 88: return DG_CMSE_IGNORE_ALPHA;                    // B8G8R8X8_UNORM
    case 93: return srgb | DG_CMSE_IGNORE_ALPHA;             // B8G8R8X8_UNORM_SRGB
    case 29: case 72: case 75: case 78: case 91: case 99: return srgb;
    default: return 0u;
    }
}
} // namespace dxtex
