// Radiance RGBE (.hdr) texels, both directions, per texel: shared by the GPU kernels (rgbe.hip), the host codec
// (host/DirectXTexAMD_HDR.cpp, a plain C++ build) and the host check (tests/cpp/rgbe_check.cpp). Compiled with -ffp-contract=off
// -fno-fast-math where the compiler could fuse: every product below rounds on its own.
//
//   rgbe_decode   DirectXTexHDR.cpp:887-901 (LoadFromHDRMemory's second pass): out[c] = scale * ldexpf(float(in[c]) + 0.5f, in[3] - 136),
//                 alpha 1. scale = 1 / exposure, computed once by the caller. There is no special case for a zero exponent, as the reference
//                 has none: (0, 0, 0, 0) decodes to 2^-137, a denormal. The ldexpf is exact (nine significant bits, no result below
//                 2^-137); the multiply is the correctly rounded one, denormal results included.
//   rgbe_encode   FloatToRGBE / HalfToRGBE (:328-407): a negative or NaN channel counts as 0; a maximum that is not above 1e-32f gives four
//                 zero bytes; otherwise top = frexpf(max, &e) * 256.f / max, left to right with an IEEE divide, every channel is its product
//                 with top truncated to a byte (the largest channel's lies in [128, 256) for every finite input), and the exponent byte
//                 is e + 128 unless all three mantissa bytes are zero. Halves are widened exactly first (rgbe_half_to_float).
//
// +Inf: the reference's top is then a NaN whose conversion to uint8_t is undefined. Here it is defined: a maximum that is not finite writes
// four zero bytes.
#pragma once
#include "dxtex_stream.h"
#include <math.h>

namespace dxtex
{
// The format table, for the C ABI and the host codec alike: the bytes of a texel of a format the encoder reads (the decoder writes
// R32G32B32A32_FLOAT only); 0 for one it does not
DXTEX_FN constexpr uint32_t rgbe_source_bytes(int format)
{
    return format == FMT_R32G32B32A32_FLOAT ? 16u : format == FMT_R32G32B32_FLOAT ? 12u : format == FMT_R16G16B16A16_FLOAT ? 8u : 0u;
}

DXTEX_FN void rgbe_decode(const uint8_t in[4], float scale, float out[4])
{
    const int e = int(in[3]) - (128 + 8);
    out[0] = scale * ldexpf(float(in[0]) + 0.5f, e);
    out[1] = scale * ldexpf(float(in[1]) + 0.5f, e);
    out[2] = scale * ldexpf(float(in[2]) + 0.5f, e);
    out[3] = 1.0f;
}

DXTEX_FN void rgbe_encode(float r, float g, float b, uint8_t out[4])
{
    r = (r >= 0.f) ? r : 0.f; g = (g >= 0.f) ? g : 0.f; b = (b >= 0.f) ? b : 0.f;         // negatives (and NaN) count as 0
    const float rg = (r > g) ? r : g;
    const float mx = (rg > b) ? rg : b;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!(mx > 1e-32f) || mx > 3.402823466e+38f) return;                                  // nothing to hold, or +Inf (this project's rule)
    int e;
    const float top = frexpf(mx, &e) * 256.f / mx;
    const uint8_t red = uint8_t(int(r * top)), green = uint8_t(int(g * top)), blue = uint8_t(int(b * top));
    out[0] = red; out[1] = green; out[2] = blue;
    out[3] = (red || green || blue) ? uint8_t((e + 128) & 0xff) : uint8_t(0);
}

// XMConvertHalfToFloat's value: exact for every half, denormals included
DXTEX_FN float rgbe_half_to_float(uint16_t h)
{
    const uint32_t sign = uint32_t(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
    if (e == 0)
    {
        const float f = float(m) * 5.9604644775390625e-8f;          // m * 2^-24
        return sign ? -f : f;
    }
    const uint32_t bits = sign | ((e == 31u ? 0xffu : e + 112u) << 23) | (m << 13);
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
}
} // namespace dxtex
