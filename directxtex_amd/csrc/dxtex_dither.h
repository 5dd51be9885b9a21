// StoreScanlineDither (DirectXTexConvert.cpp:4049-4562): the dithered stores of ConvertCustom's two dither branches (:4804-4913),
// shared by the GPU kernels (scanline.hip) and the host check (tests/cpp/dither_check.cpp), so everything here is __host__ __device__.
//
// Per texel, in the reference's order (the leaf arithmetic is oracle/shim/DirectXMath.h's statement of DirectXMath's SSE2 path):
//   v = swizzle(src); v = Saturate(v) or Clamp(v, lo, hi)      the format's pre-step
//   v = (v + vError) * scale                                    (XR_BIAS: v * scale + vError, mul then add)
//   ordered:   target = Round(v + g_Dither[(z & 3) + (y & 3) * 8 + (x & 3)])     vError stays zero
//   diffusion: target = Round(v); e = (v - target) / scale; e feeds three slots of the next row's error buffer with 3/16, 5/16, 1/16;
//              vError = e * 7/16
//   target (+ bias for XR_BIAS), clamped, truncated, masked, packed.
// Non-normalised formats (UINT / SINT) have scale 1 here: x * 1 and x / 1 are exact, which is the reference's "no multiply, no divide".
//
// Error diffusion is one serial chain per row (vError). dither_segment runs a contiguous piece of the row (in processing order) from a
// given state and, when asked, stops at the first texel whose divided error equals - bit for bit, on the lanes that reach memory - the
// one stored by an earlier run of the same piece: from there on the earlier run is the chain of the new state too. dither_row_segmented
// is the whole speculate-and-merge scheme written serially (the host check runs it); the GPU kernel runs the same steps with one lane per
// segment and barriers between the phases.
#pragma once
#include "dxtex_device.h"

namespace dxtex
{
struct alignas(16) F4 { float v[4]; };

struct DitherSpec
{
    int valid;          // 0: the format has no dithered store (StoreScanline runs; under diffusion after the zero error row was added)
    int bgr;            // XMVectorSwizzle<2, 1, 0, 3> first
    int rev;            // XMVectorSwizzle<3, 2, 1, 0> (A4B4G4R4)
    int sat;            // pre-step XMVectorSaturate (NaN -> 0); else XMVectorClamp(v, preLo, preHi) (NaN survives)
    int xr;             // R10G10B10_XR_BIAS_A2: MultiplyAdd(v, scale, vError), bias added after rounding
    int bytes;          // texel size: 1, 2, 4 or 8
    int alphaBit;       // B5G5R5A1: bit 15 = (target.w > threshold)
    uint32_t lanes;     // lanes whose value reaches memory (bit i = lane i); the merge compares only these
    float preLo[4], preHi[4], scale[4], postLo[4], postHi[4], bias[4];
    uint32_t mask[4], shift[4];
};

__host__ __device__ inline uint32_t f4_bits(float f) { union { float f; uint32_t u; } c; c.f = f; return c.u; }
__host__ __device__ inline float f4_float(uint32_t u) { union { uint32_t u; float f; } c; c.u = u; return c.f; }

__host__ __device__ inline void spec_lanes(DitherSpec& s, const float* scale, const float* lo, const float* hi, const float* plo, const float* phi)
{
    for (int i = 0; i < 4; ++i)
    {
        s.scale[i] = scale[i]; s.preLo[i] = lo[i]; s.preHi[i] = hi[i]; s.postLo[i] = plo[i]; s.postHi[i] = phi[i]; s.bias[i] = 0.0f;
    }
}

// STORE_SCANLINE / STORE_SCANLINE2 / STORE_SCANLINE1 (:3887-4040): scalev, clampzero, norm -> the pre-step and the final clamp
__host__ __device__ inline void spec_macro(DitherSpec& s, float scalev, bool clampzero, bool norm)
{
    const float sv[4] = { scalev, scalev, scalev, scalev };
    const float one[4] = { 1.0f, 1.0f, 1.0f, 1.0f };
    const float neg1[4] = { -1.0f, -1.0f, -1.0f, -1.0f };
    const float zero[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    const float lo = (0.0f - scalev) + 1.0f;                         // XMVectorAdd(XMVectorNegate(scalev), g_XMOne)
    const float lov[4] = { lo, lo, lo, lo };
    s.sat = norm && clampzero;
    spec_lanes(s, norm ? sv : one, clampzero ? zero : (norm ? neg1 : lov), (norm && !clampzero) ? one : sv, clampzero ? zero : lov, sv);
}

__host__ __device__ inline void spec_pack(DitherSpec& s, int bytes, uint32_t lanes, uint32_t m0, uint32_t m1, uint32_t m2, uint32_t m3,
                                          uint32_t s0, uint32_t s1, uint32_t s2, uint32_t s3)
{
    s.bytes = bytes; s.lanes = lanes;
    s.mask[0] = m0; s.mask[1] = m1; s.mask[2] = m2; s.mask[3] = m3;
    s.shift[0] = s0; s.shift[1] = s1; s.shift[2] = s2; s.shift[3] = s3;
}

// The formats with a dithered store (every case of :4127-4557); valid = 0 for every other format (R10G10B10_7E3_A2_FLOAT and
// R10G10B10_6E4_A2_FLOAT among them: :4558-4559 hands them to StoreScanline).
__host__ __device__ inline DitherSpec dither_spec(int format)
{
    DitherSpec s = {};
    s.valid = 1;
    const float s10[4] = { 1023.0f, 1023.0f, 1023.0f, 3.0f };
    switch (format)
    {
    case FMT_R16G16B16A16_UNORM: spec_macro(s, 65535.0f, true, true); spec_pack(s, 8, 15, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0, 16, 32, 48); break;
    case FMT_R16G16B16A16_UINT: spec_macro(s, 65535.0f, true, false); spec_pack(s, 8, 15, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0, 16, 32, 48); break;
    case FMT_R16G16B16A16_SNORM: spec_macro(s, 32767.0f, false, true); spec_pack(s, 8, 15, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0, 16, 32, 48); break;
    case FMT_R16G16B16A16_SINT: spec_macro(s, 32767.0f, false, false); spec_pack(s, 8, 15, 0xFFFF, 0xFFFF, 0xFFFF, 0xFFFF, 0, 16, 32, 48); break;
    case FMT_R10G10B10A2_UNORM:          // STORE_SCANLINE(XMUDECN4, g_Scale10pc, true, true, ...): per-lane scale (1023, 1023, 1023, 3)
    {
        const float one[4] = { 1.0f, 1.0f, 1.0f, 1.0f }, zero[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        s.sat = 1; spec_lanes(s, s10, zero, one, zero, s10);
        spec_pack(s, 4, 15, 0x3FF, 0x3FF, 0x3FF, 0x3, 0, 10, 20, 30); break;
    }
    case FMT_R10G10B10A2_UINT:           // clampzero, not norm: Clamp(v, 0, g_Scale10pc), no scaling
    {
        const float one[4] = { 1.0f, 1.0f, 1.0f, 1.0f }, zero[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        spec_lanes(s, one, zero, s10, zero, s10);
        spec_pack(s, 4, 15, 0x3FF, 0x3FF, 0x3FF, 0x3, 0, 10, 20, 30); break;
    }
    case FMT_R10G10B10_XR_BIAS_A2_UNORM: // :4156-4208
    {
        const float sc[4] = { 510.0f, 510.0f, 510.0f, 3.0f }, lo[4] = { -0.7529f, -0.7529f, -0.7529f, 0.0f }, hi[4] = { 1.2529f, 1.2529f, 1.2529f, 1.0f };
        const float zero[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        spec_lanes(s, sc, lo, hi, zero, s10);
        s.xr = 1; s.bias[0] = s.bias[1] = s.bias[2] = 384.0f;
        spec_pack(s, 4, 15, 0x3FF, 0x3FF, 0x3FF, 0x3, 0, 10, 20, 30); break;
    }
    case FMT_R8G8B8A8_UNORM: case FMT_R8G8B8A8_UNORM_SRGB: spec_macro(s, 255.0f, true, true); spec_pack(s, 4, 15, 0xFF, 0xFF, 0xFF, 0xFF, 0, 8, 16, 24); break;
    case FMT_R8G8B8A8_UINT: spec_macro(s, 255.0f, true, false); spec_pack(s, 4, 15, 0xFF, 0xFF, 0xFF, 0xFF, 0, 8, 16, 24); break;
    case FMT_R8G8B8A8_SNORM: spec_macro(s, 127.0f, false, true); spec_pack(s, 4, 15, 0xFF, 0xFF, 0xFF, 0xFF, 0, 8, 16, 24); break;
    case FMT_R8G8B8A8_SINT: spec_macro(s, 127.0f, false, false); spec_pack(s, 4, 15, 0xFF, 0xFF, 0xFF, 0xFF, 0, 8, 16, 24); break;
    case FMT_R16G16_UNORM: spec_macro(s, 65535.0f, true, true); spec_pack(s, 4, 3, 0xFFFF, 0xFFFF, 0, 0, 0, 16, 0, 0); break;
    case FMT_R16G16_UINT: spec_macro(s, 65535.0f, true, false); spec_pack(s, 4, 3, 0xFFFF, 0xFFFF, 0, 0, 0, 16, 0, 0); break;
    case FMT_R16G16_SNORM: spec_macro(s, 32767.0f, false, true); spec_pack(s, 4, 3, 0xFFFF, 0xFFFF, 0, 0, 0, 16, 0, 0); break;
    case FMT_R16G16_SINT: spec_macro(s, 32767.0f, false, false); spec_pack(s, 4, 3, 0xFFFF, 0xFFFF, 0, 0, 0, 16, 0, 0); break;
    case FMT_D24_UNORM_S8_UINT:          // :4240-4287: Clamp(v, 0, (1, 255)), scale (16777215, 1), final clamp to (16777215, 255)
    {
        const float sc[4] = { 16777215.0f, 1.0f, 0.0f, 0.0f }, zero[4] = { 0.0f, 0.0f, 0.0f, 0.0f }, hi[4] = { 1.0f, 255.0f, 0.0f, 0.0f };
        const float phi[4] = { 16777215.0f, 255.0f, 0.0f, 0.0f };
        spec_lanes(s, sc, zero, hi, zero, phi);
        spec_pack(s, 4, 3, 0xFFFFFF, 0xFF, 0, 0, 0, 24, 0, 0); break;
    }
    case FMT_R8G8_UNORM: spec_macro(s, 255.0f, true, true); spec_pack(s, 2, 3, 0xFF, 0xFF, 0, 0, 0, 8, 0, 0); break;
    case FMT_R8G8_UINT: spec_macro(s, 255.0f, true, false); spec_pack(s, 2, 3, 0xFF, 0xFF, 0, 0, 0, 8, 0, 0); break;
    case FMT_R8G8_SNORM: spec_macro(s, 127.0f, false, true); spec_pack(s, 2, 3, 0xFF, 0xFF, 0, 0, 0, 8, 0, 0); break;
    case FMT_R8G8_SINT: spec_macro(s, 127.0f, false, false); spec_pack(s, 2, 3, 0xFF, 0xFF, 0, 0, 0, 8, 0, 0); break;
    case FMT_D16_UNORM: case FMT_R16_UNORM: spec_macro(s, 65535.0f, true, true); spec_pack(s, 2, 1, 0xFFFF, 0, 0, 0, 0, 0, 0, 0); break;
    case FMT_R16_UINT: spec_macro(s, 65535.0f, true, false); spec_pack(s, 2, 1, 0xFFFF, 0, 0, 0, 0, 0, 0, 0); break;
    case FMT_R16_SNORM: spec_macro(s, 32767.0f, false, true); spec_pack(s, 2, 1, 0xFFFF, 0, 0, 0, 0, 0, 0, 0); break;
    case FMT_R16_SINT: spec_macro(s, 32767.0f, false, false); spec_pack(s, 2, 1, 0xFFFF, 0, 0, 0, 0, 0, 0, 0); break;
    case FMT_R8_UNORM: spec_macro(s, 255.0f, true, true); spec_pack(s, 1, 1, 0xFF, 0, 0, 0, 0, 0, 0, 0); break;
    case FMT_R8_UINT: spec_macro(s, 255.0f, true, false); spec_pack(s, 1, 1, 0xFF, 0, 0, 0, 0, 0, 0, 0); break;
    case FMT_R8_SNORM: spec_macro(s, 127.0f, false, true); spec_pack(s, 1, 1, 0xFF, 0, 0, 0, 0, 0, 0, 0); break;
    case FMT_R8_SINT: spec_macro(s, 127.0f, false, false); spec_pack(s, 1, 1, 0xFF, 0, 0, 0, 0, 0, 0, 0); break;
    case FMT_A8_UNORM: spec_macro(s, 255.0f, true, true); spec_pack(s, 1, 8, 0, 0, 0, 0xFF, 0, 0, 0, 0); break;      // selectw
    case FMT_B5G6R5_UNORM:               // :4343-4387: Saturate after the swizzle, clamp to g_Scale565pc
    {
        const float sc[4] = { 31.0f, 63.0f, 31.0f, 1.0f }, zero[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        s.bgr = 1; s.sat = 1; spec_lanes(s, sc, zero, zero, zero, sc);
        spec_pack(s, 2, 7, 0x1F, 0x3F, 0x1F, 0, 0, 5, 11, 0); break;
    }
    case FMT_B5G5R5A1_UNORM:             // :4389-4434: the alpha bit is target.w > threshold
    {
        const float sc[4] = { 31.0f, 31.0f, 31.0f, 1.0f }, zero[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
        s.bgr = 1; s.sat = 1; s.alphaBit = 1; spec_lanes(s, sc, zero, zero, zero, sc);
        spec_pack(s, 2, 15, 0x1F, 0x1F, 0x1F, 0, 0, 5, 10, 0); break;
    }
    case FMT_B8G8R8A8_UNORM: case FMT_B8G8R8A8_UNORM_SRGB: spec_macro(s, 255.0f, true, true); s.bgr = 1; spec_pack(s, 4, 15, 0xFF, 0xFF, 0xFF, 0xFF, 0, 8, 16, 24); break;
    case FMT_B8G8R8X8_UNORM: case FMT_B8G8R8X8_UNORM_SRGB:     // :4440-4484: the X byte is written as 0
        spec_macro(s, 255.0f, true, true); s.bgr = 1; spec_pack(s, 4, 7, 0xFF, 0xFF, 0xFF, 0, 0, 8, 16, 0); break;
    case FMT_B4G4R4A4_UNORM: spec_macro(s, 15.0f, true, true); s.bgr = 1; spec_pack(s, 2, 15, 0xF, 0xF, 0xF, 0xF, 0, 4, 8, 12); break;
    case FMT_A4B4G4R4_UNORM:             // :4489-4533: Saturate, then XMVectorSwizzle<3, 2, 1, 0>
        spec_macro(s, 15.0f, true, true); s.rev = 1; spec_pack(s, 2, 15, 0xF, 0xF, 0xF, 0xF, 0, 4, 8, 12); break;
    case FMT_R10G10B10_SNORM_A2_UNORM:   // STORE_SCANLINE(XMXDECN4, g_Scale9pc, false, true, ...) (:4509-4510): per-lane scale (511, 511, 511, 3);
    {                                    // alpha is clamped to [-1, 1] like the colours, and its low two bits are what the bitfield keeps
        const float s9[4] = { 511.0f, 511.0f, 511.0f, 3.0f }, one[4] = { 1.0f, 1.0f, 1.0f, 1.0f }, neg1[4] = { -1.0f, -1.0f, -1.0f, -1.0f };
        const float lo[4] = { (0.0f - 511.0f) + 1.0f, (0.0f - 511.0f) + 1.0f, (0.0f - 511.0f) + 1.0f, (0.0f - 3.0f) + 1.0f };
        spec_lanes(s, s9, neg1, one, lo, s9);
        spec_pack(s, 4, 15, 0x3FF, 0x3FF, 0x3FF, 0x3, 0, 10, 20, 30); break;
    }
    case FMT_R4G4_UNORM:                 // :4512-4556: Saturate, g_Scale4pc, x and y into one byte
        spec_macro(s, 15.0f, true, true); spec_pack(s, 1, 3, 0xF, 0xF, 0, 0, 0, 4, 0, 0); break;
    default:
        s.valid = 0;
        break;
    }
    return s;
}

// g_Dither (:3863-3868): every 8-wide row is a 4-wide row twice, so (z & 3) + (x & 3) is taken mod 4. Entries are k / 32.
__host__ __device__ inline float dither_offset(uint32_t x, uint32_t y, uint32_t z)
{
    // rows of the 4 x 4 pattern as four signed bytes (column 0 in the low byte)
    const uint32_t r = y & 3u;
    const uint32_t w = (r == 0) ? 0xFB0BFF0Fu : (r == 1) ? 0x03F307F7u : (r == 2) ? 0xFD0DF909u : 0x05F501F1u;
    return float(int8_t(uint8_t(w >> (8u * ((x + z) & 3u))))) * 0.03125f;
}

// XMVectorRound, SSE2 form: (v + 2^23) - 2^23 with v's sign where |v| <= 2^23, v itself elsewhere (NaN included). Small negatives give +0.
__host__ __device__ inline float dither_round(float v)
{
    const uint32_t u = f4_bits(v);
    const float magic = f4_float(0x4B000000u | (u & 0x80000000u));
    const float t = v + magic;
    const float r = t - magic;
    return (f4_float(u & 0x7FFFFFFFu) <= 8388608.0f) ? r : v;
}

// the format's swizzle and pre-step on a converted texel (src + error row already added by the caller under diffusion)
__host__ __device__ inline F4 dither_pre(const DitherSpec& s, float r, float g, float b, float a)
{
    F4 v;
    if (s.bgr) { v.v[0] = b; v.v[1] = g; v.v[2] = r; v.v[3] = a; }
    else if (s.rev) { v.v[0] = a; v.v[1] = b; v.v[2] = g; v.v[3] = r; }
    else { v.v[0] = r; v.v[1] = g; v.v[2] = b; v.v[3] = a; }
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        float x = v.v[i];
        if (s.sat) { x = (x > 0.0f) ? x : 0.0f; x = (x < 1.0f) ? x : 1.0f; }
        else { x = (s.preLo[i] > x) ? s.preLo[i] : x; x = (s.preHi[i] < x) ? s.preHi[i] : x; }     // maxps(lo, v), minps(hi, .)
        v.v[i] = x;
    }
    return v;
}

// v from the pre-stepped texel and vError
__host__ __device__ inline float dither_v(const DitherSpec& s, int i, float pre, float err)
{
    return s.xr ? pre * s.scale[i] + err : (pre + err) * s.scale[i];
}

// rounded target -> the clamped value the store truncates
__host__ __device__ inline float dither_final(const DitherSpec& s, int i, float target)
{
    float t = s.xr ? target + s.bias[i] : target;
    t = (s.postLo[i] > t) ? s.postLo[i] : t;
    return (s.postHi[i] < t) ? s.postHi[i] : t;
}

// static_cast<integer>(float) of an integral, in-range value; NaN gives 0 (x86-64's cvttss2si leaves 0 in the 8- / 16- / 24-bit fields)
__host__ __device__ inline uint32_t dither_cast(float f) { return (f == f) ? uint32_t(int32_t(f)) : 0u; }

__host__ __device__ inline uint64_t dither_pack(const DitherSpec& s, const F4& fin, float threshold)
{
    uint64_t w = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) w |= uint64_t(dither_cast(fin.v[i]) & s.mask[i]) << s.shift[i];
    if (s.alphaBit && fin.v[3] > threshold) w |= 0x8000u;
    return w;
}

__host__ __device__ inline void dither_write(uint8_t* row, uint32_t x, int bytes, uint64_t w)
{
    switch (bytes)
    {
    case 1: row[x] = uint8_t(w); break;
    case 2: reinterpret_cast<uint16_t*>(row)[x] = uint16_t(w); break;
    case 4: reinterpret_cast<uint32_t*>(row)[x] = uint32_t(w); break;
    default:
    {
        uint32_t* p = reinterpret_cast<uint32_t*>(row) + 2 * size_t(x);
        p[0] = uint32_t(w); p[1] = uint32_t(w >> 32);
        break;
    }
    }
}

// Ordered dithering of one converted texel: the packed destination texel
__host__ __device__ inline uint64_t dither_ordered(const DitherSpec& s, float r, float g, float b, float a, uint32_t x, uint32_t y, uint32_t z, float threshold)
{
    const F4 p = dither_pre(s, r, g, b, a);
    const float d = dither_offset(x, y, z);
    F4 fin;
#pragma unroll
    for (int i = 0; i < 4; ++i) fin.v[i] = dither_final(s, i, dither_round(dither_v(s, i, p.v[i], 0.0f) + d));      // vError = XMVectorZero()
    return dither_pack(s, fin, threshold);
}

// One step of the diffusion chain: packed texel and divided error e from the pre-stepped texel and the incoming vError.
__host__ __device__ inline uint64_t dither_diffuse(const DitherSpec& s, const F4& pre, const F4& state, F4& e, float threshold)
{
    F4 fin;
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        const float v = dither_v(s, i, pre.v[i], state.v[i]);
        const float t = dither_round(v);
        e.v[i] = (v - t) / s.scale[i];
        fin.v[i] = dither_final(s, i, t);
    }
    return dither_pack(s, fin, threshold);
}

__host__ __device__ inline F4 dither_next_state(const F4& e)
{
    F4 n;
#pragma unroll
    for (int i = 0; i < 4; ++i) n.v[i] = e.v[i] * 0.4375f;      // XMVectorMultiply(vError, g_ErrorWeight7)
    return n;
}

__host__ __device__ inline bool dither_same(const DitherSpec& s, const F4& a, const F4& b)
{
    bool same = true;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if ((s.lanes >> i) & 1u) same = same && f4_bits(a.v[i]) == f4_bits(b.v[i]);
    return same;
}

// The next row's error slot of the texel at processing position p (the slot of its column): MultiplyAdd(w, e, slot) in processing order,
// from +0. The texel before p in processing order gives 1/16, p itself 5/16, the one after 3/16; contributions past the row's ends are dropped.
__host__ __device__ inline F4 dither_slot(const F4* e, uint32_t p, uint32_t n)
{
    F4 acc;
#pragma unroll
    for (int i = 0; i < 4; ++i)
    {
        float a = 0.0f;
        if (p > 0) a = 0.0625f * e[p - 1].v[i] + a;
        a = 0.3125f * e[p].v[i] + a;
        if (p + 1 < n) a = 0.1875f * e[p + 1].v[i] + a;
        acc.v[i] = a;
    }
    return acc;
}

// Positions [p0, p1) of a row from vError `state`: out(p, packed) per texel, e[p] stored. With merge, the run stops after the first
// position whose new e equals the stored one on the written lanes (the chain from there on is the stored one). Returns the texels run.
template<class Out>
__host__ __device__ inline uint32_t dither_segment(const DitherSpec& s, const F4* pre, F4* e, uint32_t p0, uint32_t p1, F4 state, bool merge,
                                                   float threshold, Out out)
{
    for (uint32_t p = p0; p < p1; ++p)
    {
        F4 ep;
        out(p, dither_diffuse(s, pre[p], state, ep, threshold));
        const bool merged = merge && dither_same(s, ep, e[p]);
        e[p] = ep;
        if (merged) return p - p0 + 1;
        state = dither_next_state(ep);
    }
    return p1 - p0;
}

// The incoming vError of segment k (k >= 1): the state after the last texel of segment k - 1
__host__ __device__ inline F4 dither_seg_input(const F4* e, uint32_t k, uint32_t segLen) { return dither_next_state(e[k * segLen - 1]); }

// The speculate-and-merge scheme for one row, serially: segments of segLen positions each run from vError = 0 (segment 0 is exact: a row
// starts at zero); then rounds re-run every segment whose incoming state changed, from that state, until it merges with its stored run;
// no change in a round = every segment continues its predecessor exactly. `in` and `pending` hold one state per segment. Returns the
// texels re-run after the speculative pass.
template<class Out>
__host__ __device__ inline uint64_t dither_row_segmented(const DitherSpec& s, const F4* pre, F4* e, uint32_t n, uint32_t segLen, F4* in,
                                                         F4* pending, float threshold, Out out)
{
    const uint32_t nseg = (n + segLen - 1) / segLen;
    const F4 zero = { { 0.0f, 0.0f, 0.0f, 0.0f } };
    for (uint32_t k = 0; k < nseg; ++k)
    {
        in[k] = zero;
        dither_segment(s, pre, e, k * segLen, (k + 1) * segLen < n ? (k + 1) * segLen : n, zero, false, threshold, out);
    }
    uint64_t rerun = 0;
    for (;;)
    {
        for (uint32_t k = 1; k < nseg; ++k) pending[k] = dither_seg_input(e, k, segLen);     // read phase (a barrier follows on the GPU)
        bool changed = false;
        for (uint32_t k = 1; k < nseg; ++k)
        {
            if (dither_same(s, pending[k], in[k])) continue;
            in[k] = pending[k];
            rerun += dither_segment(s, pre, e, k * segLen, (k + 1) * segLen < n ? (k + 1) * segLen : n, in[k], true, threshold, out);
            changed = true;
        }
        if (!changed) break;
    }
    return rerun;
}

} // namespace dxtex
