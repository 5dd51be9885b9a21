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

// ---- The writer's direction (jpeg_encode.hip holds the kernels): what libjpeg does to a texel before its Huffman coder, which is the only
// byte-serial part - jccolor.c, jcprepct.c's edge padding, jcsample.c without smoothing, jfdctint.c (JDCT_ISLOW), jcdctmgr.c's quantiser and
// jccoefct.c's dummy blocks - for the kernels, the host saver and a host check (tests/cpp/jpeg_write_check.cpp). The coefficients come out
// in the layout the reader takes.

// The format table, for the C ABI and the host codec alike: what an image format is to the coder, -1 for one that is neither read into
// nor written. A grey frame is JPEG_TEXEL_GREY on both sides; a colour frame decodes into JPEG_TEXEL_RGBA only and encodes from
// JPEG_TEXEL_RGBA or JPEG_TEXEL_BGRX (`bgr` below).
enum JpegTexel : int { JPEG_TEXEL_GREY = 0, JPEG_TEXEL_RGBA, JPEG_TEXEL_BGRX };
DXTEX_FN constexpr int jpeg_texel_of(int format)
{
    switch (format)
    {
    case FMT_R8_UNORM: return JPEG_TEXEL_GREY;
    case FMT_R8G8B8A8_UNORM: case FMT_R8G8B8A8_UNORM_SRGB: return JPEG_TEXEL_RGBA;
    case FMT_B8G8R8A8_UNORM: case FMT_B8G8R8A8_UNORM_SRGB: case FMT_B8G8R8X8_UNORM: case FMT_B8G8R8X8_UNORM_SRGB: return JPEG_TEXEL_BGRX;
    default: return -1;
    }
}

// jccolor.c: an R8G8B8A8 texel word (B8G8R8x8 with `bgr`) -> Y | Cb << 8 | Cr << 16. Alpha or X is ignored. No term is negative.
DXTEX_FN constexpr uint32_t jpeg_ycc(uint32_t texel, bool bgr)
{
    const uint32_t r = (bgr ? texel >> 16 : texel) & 0xFFu, g = (texel >> 8) & 0xFFu, b = (bgr ? texel : texel >> 16) & 0xFFu;
    const uint32_t y = (19595u * r + 38470u * g + 7471u * b + 32768u) >> 16;
    const uint32_t cb = ((128u << 16) + 32767u + 32768u * b - 11059u * r - 21709u * g) >> 16;
    const uint32_t cr = ((128u << 16) + 32767u + 32768u * r - 27439u * g - 5329u * b) >> 16;
    return y | (cb << 8) | (cr << 16);
}

// jcsample.c's rounding: 2 x 2 adds 1 to an even output column and 2 to an odd one, 2 x 1 adds 0 and 1
DXTEX_FN constexpr uint32_t jpeg_downsample_bias(uint32_t vs, uint32_t cx) { return (vs == 2u ? 1u : 0u) + (cx & 1u); }

// The image a frame is made from: R8_UNORM (grey) or one of the 32-bit colour formats, read through its pitch, never past width x height
struct JpegSource
{
    const uint8_t* pixels;
    uint64_t pitch;
    uint32_t width, height;
    bool grey, bgr;
};

// component c (0 Y, 1 Cb, 2 Cr; grey: the sample) of the texel at (x, y), both clamped to the image: jcprepct.c's edge replication
DXTEX_FN uint32_t jpeg_source_sample(const JpegSource& s, uint32_t c, uint32_t x, uint32_t y)
{
    x = x < s.width ? x : s.width - 1u; y = y < s.height ? y : s.height - 1u;
    const uint8_t* p = s.pixels + uint64_t(y) * s.pitch + uint64_t(x) * (s.grey ? 1u : 4u);
    return s.grey ? p[0] : (jpeg_ycc(le_load32(p, 4), s.bgr) >> (8u * c)) & 0xFFu;
}

// The sample at (cx, cy) of component c's block-padded plane; hs and vs are the luma factors over this component's (1 x 1, 2 x 1 or 2 x 2).
// A full-size component replicates the image's last column and row. A downsampled one averages hs x vs texels whose columns and rows are
// clamped to the image, and past its own ceil(height / vs) rows it repeats its last ROW, not the image's: h2v2 of an image of odd
// height + 1 rows differs from that.
DXTEX_FN uint32_t jpeg_plane_sample(const JpegSource& s, uint32_t c, uint32_t hs, uint32_t vs, uint32_t cx, uint32_t cy)
{
    if (hs == 1u) return jpeg_source_sample(s, c, cx, cy);
    const uint32_t dh = (s.height + vs - 1u) / vs;
    cy = cy < dh ? cy : dh - 1u;
    uint32_t sum = jpeg_downsample_bias(vs, cx);
    for (uint32_t j = 0; j < vs; ++j)
        for (uint32_t i = 0; i < 2u; ++i) sum += jpeg_source_sample(s, c, 2u * cx + i, vs * cy + j);
    return sum >> vs;
}

// One pass of jfdctint.c (CONST_BITS 13, PASS1_BITS 2) over in[0..7]. Along a row (`rows`): outputs 0 and 4 are scaled up by PASS1_BITS, the
// rest descaled by CONST_BITS - PASS1_BITS. Down a column: 0 and 4 are descaled by PASS1_BITS, the rest by CONST_BITS + PASS1_BITS. The
// results are 8 times the DCT's; the quantiser divides that out.
DXTEX_FN void jpeg_fdct_pass(const int32_t (&in)[8], int32_t (&out)[8], bool rows)
{
    const int32_t t0 = jpeg_add(in[0], in[7]), t7 = jpeg_sub(in[0], in[7]), t1 = jpeg_add(in[1], in[6]), t6 = jpeg_sub(in[1], in[6]);
    const int32_t t2 = jpeg_add(in[2], in[5]), t5 = jpeg_sub(in[2], in[5]), t3 = jpeg_add(in[3], in[4]), t4 = jpeg_sub(in[3], in[4]);
    const int32_t t10 = jpeg_add(t0, t3), t13 = jpeg_sub(t0, t3), t11 = jpeg_add(t1, t2), t12 = jpeg_sub(t1, t2);
    const uint32_t shift = rows ? 11u : 15u;
    out[0] = rows ? jpeg_shl(jpeg_add(t10, t11), 2) : jpeg_descale(jpeg_add(t10, t11), 2);
    out[4] = rows ? jpeg_shl(jpeg_sub(t10, t11), 2) : jpeg_descale(jpeg_sub(t10, t11), 2);
    int32_t z1 = jpeg_mul(jpeg_add(t12, t13), 4433);
    out[2] = jpeg_descale(jpeg_add(z1, jpeg_mul(t13, 6270)), shift);
    out[6] = jpeg_descale(jpeg_sub(z1, jpeg_mul(t12, 15137)), shift);
    z1 = jpeg_add(t4, t7);
    int32_t z2 = jpeg_add(t5, t6), z3 = jpeg_add(t4, t6), z4 = jpeg_add(t5, t7);
    const int32_t z5 = jpeg_mul(jpeg_add(z3, z4), 9633);
    const int32_t o4 = jpeg_mul(t4, 2446), o5 = jpeg_mul(t5, 16819), o6 = jpeg_mul(t6, 25172), o7 = jpeg_mul(t7, 12299);
    z1 = jpeg_mul(z1, -7373); z2 = jpeg_mul(z2, -20995);
    z3 = jpeg_add(jpeg_mul(z3, -16069), z5); z4 = jpeg_add(jpeg_mul(z4, -3196), z5);
    out[7] = jpeg_descale(jpeg_add(o4, jpeg_add(z1, z3)), shift); out[5] = jpeg_descale(jpeg_add(o5, jpeg_add(z2, z4)), shift);
    out[3] = jpeg_descale(jpeg_add(o6, jpeg_add(z2, z3)), shift); out[1] = jpeg_descale(jpeg_add(o7, jpeg_add(z1, z4)), shift);
}

// jcdctmgr.c: the transform's output over 8 * quant, rounded half away from zero. quant is 1 to 65535; the entry points refuse 0.
DXTEX_FN constexpr int16_t jpeg_quantise(int32_t c, uint32_t quant)
{
    const uint32_t d = 8u * quant, a = c < 0 ? 0u - uint32_t(c) : uint32_t(c), r = (a + (d >> 1)) / d;
    return int16_t(uint16_t(c < 0 ? 0u - r : r));
}

// a whole block: 8 rows of 8 samples `pitch` bytes apart and the component's table in natural order -> 64 quantised coefficients, natural order
DXTEX_FN void jpeg_fdct_block(const uint8_t* samples, uint64_t pitch, const uint16_t* quant, int16_t* coefficients)
{
    int32_t ws[64];
    for (uint32_t r = 0; r < 8; ++r)
    {
        int32_t in[8], out[8];
        for (uint32_t c = 0; c < 8; ++c) in[c] = int32_t(samples[r * pitch + c]) - 128;
        jpeg_fdct_pass(in, out, true);
        for (uint32_t c = 0; c < 8; ++c) ws[r * 8 + c] = out[c];
    }
    for (uint32_t c = 0; c < 8; ++c)
    {
        int32_t in[8], out[8];
        for (uint32_t r = 0; r < 8; ++r) in[r] = ws[r * 8 + c];
        jpeg_fdct_pass(in, out, false);
        for (uint32_t r = 0; r < 8; ++r) coefficients[r * 8 + c] = jpeg_quantise(out[r], quant[r * 8 + c]);
    }
}

// jccoefct.c's dummy blocks. A component's plane is padded to whole MCUs, of which rw x rh blocks hold its own samples; h is its horizontal
// factor. A block outside them has all AC zero and the DC of the block coded before it in its MCU: in a real row, the row's last real block;
// in a dummy row, the last block of the MCU's row above - itself the last real block where that one is a dummy. True for a dummy, with
// the block whose DC it takes.
DXTEX_FN constexpr bool jpeg_dummy_block(uint32_t bx, uint32_t by, uint32_t rw, uint32_t rh, uint32_t h, uint32_t& sx, uint32_t& sy)
{
    if (by < rh && bx < rw) return false;
    const uint32_t last = (bx / h) * h + h - 1u;
    sx = by < rh || last > rw - 1u ? rw - 1u : last;
    sy = by < rh ? by : rh - 1u;
    return true;
}
// the blocks that hold a component's own samples along one axis
DXTEX_FN constexpr uint32_t jpeg_real_blocks(uint32_t extent, uint32_t factor, uint32_t maxFactor) { return (jpeg_downsampled(extent, factor, maxFactor) + 7u) / 8u; }
} // namespace dxtex
