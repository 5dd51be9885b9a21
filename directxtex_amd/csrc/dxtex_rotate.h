// texconv's HDR colour rotation (Texconv/texconv.cpp:2696-2964): the eight TransformImage lambdas that move r, g and b between the Rec.709,
// Rec.2020 and Display-P3 primaries and into / out of HDR10 (Rec.2020 with the SMPTE ST.2084 curve, scaled by a paper-white level in
// nits). Shared by the GPU kernel (rotate_color.hip) and the host check (tests/cpp/rotate_check.cpp), so everything here is
// __host__ __device__. Compiled with -ffp-contract=off -fno-fast-math: every product and sum below rounds on its own.
//
//   XMVector3Transform(v, M)   DirectXMath's SSE2 path (no FMA), per output channel k:
//                              t = z * M[2][k]; t = t + M[3][k]; t = y * M[1][k] + t; t = x * M[0][k] + t
//                              M[3][k] is +0 in all five matrices; the addition stays because it turns -0 into +0
//   to HDR10                   n = transform(v); n = (n * nits) / 10000; LinearToST2084 on x, y, z          (:2744-2775, :2848-2879)
//   from HDR10                 ST2084ToLinear on x, y, z; l = (l * 10000) / nits; transform(l, 2020 -> 709) (:2796-2827)
//   LinearToST2084(v)          p = powf(|v|, 0.1593017578); powf((0.8359375 + 18.8515625 * p) / (1 + 18.6875 * p), 78.84375)   (:1145-1149)
//   ST2084ToLinear(v)          p = powf(|v|, 1 / 78.84375); n = std::max(p - 0.8359375, 0): a NaN n stays;
//                              powf(n / (18.8515625 - 18.6875 * p), 1 / 0.1593017578)                       (:1151-1155)
//
// powf is the correctly rounded one, the project's rule for the sRGB curves (dxtex_device.h, pow_rn; dxtex_diag.h, dg_gamma22): pow() in
// double precision rounded once to fp32, the same on the host and on the device. Alpha is never computed: the caller moves it.
//
// Non-finite values: an infinite result follows from the fixed order of the operations above. Where the arithmetic gives a NaN (a NaN
// input, inf - inf, a negative base of the second pow once |v| is above about 1.99) the channel is a NaN; its payload is not specified,
// since the reference's own depends on how its compiler ordered the operands of addps.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace dxtex
{
// texconv's ROTATE_* (texconv.cpp:181-188) = DXTEX_ROTATE_* (include/dxtex_amd.h)
enum : uint32_t
{
    ROTATE_709_TO_HDR10 = 1, ROTATE_HDR10_TO_709 = 2, ROTATE_709_TO_2020 = 3, ROTATE_2020_TO_709 = 4,
    ROTATE_P3D65_TO_HDR10 = 5, ROTATE_P3D65_TO_2020 = 6, ROTATE_709_TO_P3D65 = 7, ROTATE_P3D65_TO_709 = 8,
};
// the transfer curve an operation applies: after the matrix (to HDR10) or before it (from HDR10)
enum : int { ROTATE_CURVE_NONE = 0, ROTATE_CURVE_TO_ST2084 = 1, ROTATE_CURVE_FROM_ST2084 = 2 };

// what the kernel needs of an operation: rows 0-2 of its matrix (row 3 is (0, 0, 0, 1)) and the paper-white level
struct RotateArgs
{
    float m[3][3];
    float nits;
};

// the five matrices of texconv.cpp:1101-1143
struct RotateMatrix { float m[3][3]; };
constexpr RotateMatrix kRotate709to2020 = { { { 0.6274040f, 0.0690970f, 0.0163916f }, { 0.3292820f, 0.9195400f, 0.0880132f }, { 0.0433136f, 0.0113612f, 0.8955950f } } };
constexpr RotateMatrix kRotate2020to709 = { { { 1.6604910f, -0.1245505f, -0.0181508f }, { -0.5876411f, 1.1328999f, -0.1005789f }, { -0.0728499f, -0.0083494f, 1.1187297f } } };
constexpr RotateMatrix kRotateP3D65to2020 = { { { 0.753845f, 0.0457456f, -0.00121055f }, { 0.198593f, 0.941777f, 0.0176041f }, { 0.047562f, 0.0124772f, 0.983607f } } };
constexpr RotateMatrix kRotate709toP3D65 = { { { 0.822461969f, 0.033194199f, 0.017082631f }, { 0.1775380f, 0.9668058f, 0.0723974f }, { 0.0000000f, 0.0000000f, 0.9105199f } } };
constexpr RotateMatrix kRotateP3D65to709 = { { { 1.224940176f, -0.042056955f, -0.019637555f }, { -0.224940176f, 1.042056955f, -0.078636046f }, { 0.0000000f, 0.0000000f, 1.098273600f } } };

// the matrix and the curve of rotate = ROTATE_*; false for a value outside 1..8
inline bool rotate_resolve(uint32_t rotate, float nits, RotateArgs& a, int& curve)
{
    const RotateMatrix* m = nullptr;
    curve = ROTATE_CURVE_NONE;
    switch (rotate)
    {
    case ROTATE_709_TO_HDR10: m = &kRotate709to2020; curve = ROTATE_CURVE_TO_ST2084; break;
    case ROTATE_HDR10_TO_709: m = &kRotate2020to709; curve = ROTATE_CURVE_FROM_ST2084; break;
    case ROTATE_709_TO_2020: m = &kRotate709to2020; break;
    case ROTATE_2020_TO_709: m = &kRotate2020to709; break;
    case ROTATE_P3D65_TO_HDR10: m = &kRotateP3D65to2020; curve = ROTATE_CURVE_TO_ST2084; break;
    case ROTATE_P3D65_TO_2020: m = &kRotateP3D65to2020; break;
    case ROTATE_709_TO_P3D65: m = &kRotate709toP3D65; break;
    case ROTATE_P3D65_TO_709: m = &kRotateP3D65to709; break;
    default: return false;
    }
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) a.m[r][k] = m->m[r][k];
    a.nits = nits;
    return true;
}
// texconv's rule for -nits (texconv.cpp:1898), which a NaN fails too
inline bool rotate_nits_valid(float nits) { return nits > 0.0f && nits <= 10000.0f; }

// the correctly rounded powf
__host__ __device__ inline float rc_pow(float x, float y) { return float(pow(double(x), double(y))); }

__host__ __device__ inline void rc_transform(float (&v)[3], const float (&m)[3][3])
{
    const float x = v[0], y = v[1], z = v[2];
#pragma unroll
    for (int k = 0; k < 3; ++k)
    {
        float t = z * m[2][k];
        t = t + 0.0f;
        t = y * m[1][k] + t;
        t = x * m[0][k] + t;
        v[k] = t;
    }
}

__host__ __device__ inline float rc_linear_to_st2084(float v)
{
    const float p = rc_pow(fabsf(v), 0.1593017578f);
    return rc_pow((0.8359375f + 18.8515625f * p) / (1.0f + 18.6875f * p), 78.84375f);
}

__host__ __device__ inline float rc_st2084_to_linear(float v)
{
    const float p = rc_pow(fabsf(v), 1.0f / 78.84375f);
    float n = p - 0.8359375f;
    n = (n < 0.0f) ? 0.0f : n;
    return rc_pow(n / (18.8515625f - 18.6875f * p), 1.0f / 0.1593017578f);
}

// r, g and b of one texel (c[3], the alpha, is not read or written)
template<int CURVE>
__host__ __device__ inline void rc_apply(float (&c)[4], const RotateArgs& a)
{
    float v[3] = { c[0], c[1], c[2] };
    if constexpr (CURVE == ROTATE_CURVE_FROM_ST2084)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = (rc_st2084_to_linear(v[k]) * 10000.0f) / a.nits;
    }
    rc_transform(v, a.m);
    if constexpr (CURVE == ROTATE_CURVE_TO_ST2084)
    {
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = rc_linear_to_st2084((v[k] * a.nits) / 10000.0f);
    }
    c[0] = v[0]; c[1] = v[1]; c[2] = v[2];
}
} // namespace dxtex
