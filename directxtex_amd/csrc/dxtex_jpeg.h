// JPEG samples (jpeg.hip holds the kernels): what a baseline or progressive .jpg needs after the host's Huffman walk, which is the only
// byte-serial part. The quantised coefficients go up as the file has them; dequantisation, the inverse DCT, chroma upsampling, YCbCr -> RGB
// and the clamp are these functions, one 8 x 8 block or one texel at a time, for the kernels, the host loader
// (host/DirectXTexAMD_JPEG.cpp) and a host check (tests/cpp/jpeg_check.cpp). They follow libjpeg's defaults, which the reference's
// Auxiliary/DirectXTexJPEG.cpp leaves as they are: jidctint.c (JDCT_ISLOW), jdsample.c with fancy upsampling, jdcolor.c.
//
// All arithmetic is 32-bit. Additions, multiplications and left shifts are written on uint32_t, so that nothing is undefined and host and
// device agree on every input, nonsense coefficients included; right shifts are arithmetic shifts of the int32_t value. Parity with
// libjpeg holds where nothing overflows 32 bits, which no coefficient an encoder writes comes near.
#pragma once
#include "dxtex_stream.h"

namespace dxtex
{
enum JpegColour : int { JPEG_GREY = 0, JPEG_YCBCR = 1, JPEG_RGB = 2 };

// zigzag position -> natural (row-major) index
static constexpr uint8_t kJpegNatural[64] = {
     0,  1,  8, 16,  9,  2,  3, 10, 17, 24, 32, 25, 18, 11,  4,  5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,  6,  7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };

DXTEX_FN constexpr int32_t jpeg_mul(int32_t a, int32_t b) { return int32_t(uint32_t(a) * uint32_t(b)); }
DXTEX_FN constexpr int32_t jpeg_add(int32_t a, int32_t b) { return int32_t(uint32_t(a) + uint32_t(b)); }
DXTEX_FN constexpr int32_t jpeg_sub(int32_t a, int32_t b) { return int32_t(uint32_t(a) - uint32_t(b)); }
DXTEX_FN constexpr int32_t jpeg_shl(int32_t a, uint32_t n) { return int32_t(uint32_t(a) << n); }
// DESCALE(x, n) = (x + (1 << (n - 1))) >> n
DXTEX_FN constexpr int32_t jpeg_descale(int32_t x, uint32_t n) { return jpeg_add(x, int32_t(1u << (n - 1u))) >> n; }

// the coefficient times its quantiser entry: what both passes start from
DXTEX_FN constexpr int32_t jpeg_dequant(int32_t coefficient, uint32_t quant) { return jpeg_mul(coefficient, int32_t(quant)); }

// One pass of jidctint.c (CONST_BITS 13) over in[0..7], descaled by `shift`: 11 down a column (CONST_BITS - PASS1_BITS), 18 along a row
// (CONST_BITS + PASS1_BITS + 3). libjpeg's shortcut for a column whose AC terms are all zero gives what this gives.
DXTEX_FN void jpeg_idct_pass(const int32_t (&in)[8], int32_t (&out)[8], uint32_t shift)
{
    int32_t z1 = jpeg_mul(jpeg_add(in[2], in[6]), 4433);
    const int32_t t2 = jpeg_sub(z1, jpeg_mul(in[6], 15137)), t3 = jpeg_add(z1, jpeg_mul(in[2], 6270));
    const int32_t t0 = jpeg_shl(jpeg_add(in[0], in[4]), 13), t1 = jpeg_shl(jpeg_sub(in[0], in[4]), 13);
    const int32_t t10 = jpeg_add(t0, t3), t13 = jpeg_sub(t0, t3), t11 = jpeg_add(t1, t2), t12 = jpeg_sub(t1, t2);
    int32_t o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
    z1 = jpeg_add(o0, o3);
    int32_t z2 = jpeg_add(o1, o2), z3 = jpeg_add(o0, o2), z4 = jpeg_add(o1, o3);
    const int32_t z5 = jpeg_mul(jpeg_add(z3, z4), 9633);
    o0 = jpeg_mul(o0, 2446); o1 = jpeg_mul(o1, 16819); o2 = jpeg_mul(o2, 25172); o3 = jpeg_mul(o3, 12299);
    z1 = jpeg_mul(z1, -7373); z2 = jpeg_mul(z2, -20995);
    z3 = jpeg_add(jpeg_mul(z3, -16069), z5); z4 = jpeg_add(jpeg_mul(z4, -3196), z5);
    o0 = jpeg_add(o0, jpeg_add(z1, z3)); o1 = jpeg_add(o1, jpeg_add(z2, z4));
    o2 = jpeg_add(o2, jpeg_add(z2, z3)); o3 = jpeg_add(o3, jpeg_add(z1, z4));
    out[0] = jpeg_descale(jpeg_add(t10, o3), shift); out[7] = jpeg_descale(jpeg_sub(t10, o3), shift);
    out[1] = jpeg_descale(jpeg_add(t11, o2), shift); out[6] = jpeg_descale(jpeg_sub(t11, o2), shift);
    out[2] = jpeg_descale(jpeg_add(t12, o1), shift); out[5] = jpeg_descale(jpeg_sub(t12, o1), shift);
    out[3] = jpeg_descale(jpeg_add(t13, o0), shift); out[4] = jpeg_descale(jpeg_sub(t13, o0), shift);
}

// libjpeg's masked range-limit table: the value wrapped to signed 10 bits, plus 128, clamped to a sample
DXTEX_FN constexpr uint32_t jpeg_range_limit(int32_t x)
{
    const int32_t w = int32_t((uint32_t(x) + 512u) & 1023u) - 512 + 128;
    return uint32_t(w < 0 ? 0 : w > 255 ? 255 : w);
}

// a whole block: 64 quantised coefficients and the component's table, both in natural order -> 64 samples, row-major
DXTEX_FN void jpeg_idct_block(const int16_t* coefficients, const uint16_t* quant, uint8_t* samples)
{
    int32_t ws[64];
    for (uint32_t c = 0; c < 8; ++c)
    {
        int32_t in[8], out[8];
        for (uint32_t r = 0; r < 8; ++r) in[r] = jpeg_dequant(coefficients[r * 8 + c], quant[r * 8 + c]);
        jpeg_idct_pass(in, out, 11);
        for (uint32_t r = 0; r < 8; ++r) ws[r * 8 + c] = out[r];
    }
    for (uint32_t r = 0; r < 8; ++r)
    {
        int32_t in[8], out[8];
        for (uint32_t c = 0; c < 8; ++c) in[c] = ws[r * 8 + c];
        jpeg_idct_pass(in, out, 18);
        for (uint32_t c = 0; c < 8; ++c) samples[r * 8 + c] = uint8_t(jpeg_range_limit(out[c]));
    }
}

// A component's samples after the inverse DCT: block-padded rows of `pitch` bytes, of which dw x dh are the component's own
// (dw = ceil(width * h / hmax), dh likewise). hs and vs are the luma factors over this component's: 1 or 2.
struct JpegPlane
{
    const uint8_t* samples;
    uint32_t pitch, dw, dh, hs, vs;
};

// jdsample.c: the component's sample at texel (x, y) of the image. 1 x 1 copies. 2 x 1 and 2 x 2 with dw > 2 are the fancy (triangle)
// filters; with dw <= 2 libjpeg replicates instead. Nothing outside the plane's dw x dh is read.
DXTEX_FN uint32_t jpeg_upsample(const JpegPlane& p, uint32_t x, uint32_t y)
{
    if (p.hs == 1u) return p.samples[uint64_t(y) * p.pitch + x];
    const uint32_t c = x >> 1, r = p.vs == 2u ? y >> 1 : y;
    const uint8_t* cur = p.samples + uint64_t(r) * p.pitch;
    if (p.dw <= 2u) return cur[c];
    const bool odd = (x & 1u) != 0;
    if (p.vs == 1u)
    {
        if (!odd) return c == 0 ? cur[0] : (3u * cur[c] + cur[c - 1] + 1u) >> 2;
        return c == p.dw - 1u ? cur[c] : (3u * cur[c] + cur[c + 1] + 2u) >> 2;
    }
    const uint32_t nr = (y & 1u) ? (r + 1u < p.dh ? r + 1u : p.dh - 1u) : (r ? r - 1u : 0u);
    const uint8_t* nb = p.samples + uint64_t(nr) * p.pitch;
    const uint32_t s = 3u * cur[c] + nb[c];
    if (!odd) return c == 0 ? (4u * s + 8u) >> 4 : (3u * s + (3u * cur[c - 1] + nb[c - 1]) + 8u) >> 4;
    return c == p.dw - 1u ? (4u * s + 7u) >> 4 : (3u * s + (3u * cur[c + 1] + nb[c + 1]) + 7u) >> 4;
}

DXTEX_FN constexpr uint32_t jpeg_clamp(int32_t v) { return uint32_t(v < 0 ? 0 : v > 255 ? 255 : v); }

// jdcolor.c: three samples -> R | G << 8 | B << 16 | 0xff << 24. RGB-coded files skip the transform.
DXTEX_FN constexpr uint32_t jpeg_texel(int colour, uint32_t a, uint32_t b, uint32_t c)
{
    if (colour == JPEG_RGB) return a | (b << 8) | (c << 16) | 0xFF000000u;
    const int32_t y = int32_t(a), cb = int32_t(b) - 128, cr = int32_t(c) - 128;
    const uint32_t R = jpeg_clamp(y + ((91881 * cr + 32768) >> 16));
    const uint32_t G = jpeg_clamp(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    const uint32_t B = jpeg_clamp(y + ((116130 * cb + 32768) >> 16));
    return R | (G << 8) | (B << 16) | 0xFF000000u;
}

// the blocks a component is padded to: whole MCUs. factor = the component's h (or v), maxFactor = the frame's largest
DXTEX_FN constexpr uint32_t jpeg_padded_blocks(uint32_t extent, uint32_t factor, uint32_t maxFactor) { return (extent + 8u * maxFactor - 1u) / (8u * maxFactor) * factor; }
// the component's own samples along one axis
DXTEX_FN constexpr uint32_t jpeg_downsampled(uint32_t extent, uint32_t factor, uint32_t maxFactor) { return (extent * factor + maxFactor - 1u) / maxFactor; }
} // namespace dxtex
