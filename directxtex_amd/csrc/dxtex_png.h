// PNG texels (.png), both directions, per texel: shared by the GPU kernels (png.hip), the host codec (host/DirectXTexAMD_PNG.cpp, a plain
// C++ build) and the host check (tests/cpp/png_check.cpp). Integer code: bits move, nothing is computed but a sub-byte grey's multiply.
//
// The file side is the unfiltered image data: tight rows of png_row_bytes(kind, width) = ceil(width * bits / 8) bytes, no filter byte.
// Chunks, CRCs, inflate and the row filters are byte-serial and stay with the host codec.
//
// The reader's kinds (Auxiliary/DirectXTexPNG.cpp; Update :126-178, GuessFormat :181-225, GetHeader :228-251):
//   PNG_G1/G2/G4   grey, 1, 2, 4 bits   -> R8_UNORM              sample * 255, 85, 17; the first texel sits in the byte's high bits and every
//                                                                row starts on a byte (png_set_expand)
//   PNG_G8         grey, 8 bits         -> R8_UNORM              the byte
//   PNG_G16        grey, 16 bits        -> R16_UNORM             the sample, big-endian in the file (png_set_swap)
//   PNG_GA8/GA16   grey + alpha         -> R8G8B8A8_UNORM / R16G16B16A16_UNORM   g, g, g, a (png_set_gray_to_rgb)
//   PNG_RGB8/RGB16 colour               -> R8G8B8A8_UNORM[_SRGB] or, with PNG_BGR, B8G8R8X8_UNORM[_SRGB] / R16G16B16A16_UNORM
//                                                                the filler is 0xff / 0xffff (png_set_filler); a tRNS colour key is ignored
//   PNG_RGBA8/16   colour + alpha       -> R8G8B8A8 or, with PNG_BGR, B8G8R8A8_UNORM[_SRGB] / R16G16B16A16_UNORM
//   PNG_P1/2/4/8   palette index        -> as PNG_RGB8           table[index]: 256 words R, G, B, A (png_palette_table), A from tRNS or 255,
//                                                                opaque black at and past the palette's end; A lands in the fourth byte
//                                                                whatever the format calls it
// PNG_BGR exchanges the first and third byte of an 8-bit colour texel (png_set_bgr); the 16-bit kinds and the grey ones ignore it.
// Departures from the reference, as include/dxtex_amd.h and host/DirectXTexAMD.h state them: no alpha association and no gamma
// correction - every sample is the file's sample.
//
// The writer (WriteImage :315-404), one PngSource per image format it takes:
//   PNG_SRC_R8 -> grey 8, PNG_SRC_R16 -> grey 16, PNG_SRC_RGBA8 / PNG_SRC_BGRA8 -> RGBA 8 (B and R exchanged for the latter),
//   PNG_SRC_RGBA16 -> RGBA 16, PNG_SRC_BGRX8 -> RGB 8 (exchanged, X dropped). 16-bit samples are written big-endian.
#pragma once
#include "dxtex_stream.h"

namespace dxtex
{
enum PngKind : int { PNG_G1 = 0, PNG_G2, PNG_G4, PNG_G8, PNG_G16, PNG_GA8, PNG_GA16, PNG_RGB8, PNG_RGB16, PNG_RGBA8, PNG_RGBA16, PNG_P1, PNG_P2, PNG_P4, PNG_P8, PNG_KINDS };
enum PngFlags : uint32_t { PNG_BGR = 0x1 };          // DXTEX_PNG_BGR of include/dxtex_amd.h
enum PngSource : int { PNG_SRC_R8 = 0, PNG_SRC_R16, PNG_SRC_RGBA8, PNG_SRC_BGRA8, PNG_SRC_RGBA16, PNG_SRC_BGRX8, PNG_SOURCES };

// bits of a file texel, bytes of an image texel, per reader kind
DXTEX_FN constexpr uint32_t png_file_bits(int kind)
{
    return (kind == PNG_G1 || kind == PNG_P1) ? 1u : (kind == PNG_G2 || kind == PNG_P2) ? 2u : (kind == PNG_G4 || kind == PNG_P4) ? 4u :
           (kind == PNG_G8 || kind == PNG_P8) ? 8u : (kind == PNG_G16 || kind == PNG_GA8) ? 16u : kind == PNG_RGB8 ? 24u :
           (kind == PNG_GA16 || kind == PNG_RGBA8) ? 32u : kind == PNG_RGB16 ? 48u : 64u;
}
DXTEX_FN constexpr uint32_t png_image_bytes(int kind)
{
    return kind <= PNG_G8 ? 1u : kind == PNG_G16 ? 2u : (kind == PNG_GA16 || kind == PNG_RGB16 || kind == PNG_RGBA16) ? 8u : 4u;
}
DXTEX_FN constexpr bool png_is_palette(int kind) { return kind >= PNG_P1 && kind <= PNG_P8; }
DXTEX_FN constexpr bool png_is_sub_byte(int kind) { return png_file_bits(kind) < 8u; }
// the kinds PNG_BGR changes
DXTEX_FN constexpr bool png_takes_bgr(int kind) { return kind == PNG_RGB8 || kind == PNG_RGBA8 || png_is_palette(kind); }
// bytes of one unfiltered row of the file
DXTEX_FN constexpr uint64_t png_row_bytes(int kind, uint64_t width) { return (width * png_file_bits(kind) + 7u) / 8u; }
// a sub-byte grey sample to 8 bits
DXTEX_FN constexpr uint32_t png_grey_scale(uint32_t bits) { return bits == 1u ? 255u : bits == 2u ? 85u : 17u; }

// the writer's side: bytes of an image texel and of a file texel per source
DXTEX_FN constexpr uint32_t png_source_bytes(int src) { return src == PNG_SRC_R8 ? 1u : src == PNG_SRC_R16 ? 2u : src == PNG_SRC_RGBA16 ? 8u : 4u; }
DXTEX_FN constexpr uint32_t png_source_file_bytes(int src) { return src == PNG_SRC_BGRX8 ? 3u : png_source_bytes(src); }

// The two format tables, for the C ABI and the host codec alike. The reader's: whether a kind under these flags unpacks into this format
// (the host codec chooses one of them from the file's colour chunks and its PNG_FLAGS).
DXTEX_FN constexpr bool png_unpack_pairs(int kind, uint32_t flags, int format)
{
    const bool bgr = (flags & PNG_BGR) != 0;
    switch (kind)
    {
    case PNG_G1: case PNG_G2: case PNG_G4: case PNG_G8: return format == FMT_R8_UNORM;
    case PNG_G16: return format == FMT_R16_UNORM;
    case PNG_GA8: return format == (bgr ? FMT_B8G8R8A8_UNORM : FMT_R8G8B8A8_UNORM);          // g, g, g, a either way
    case PNG_GA16: case PNG_RGB16: case PNG_RGBA16: return format == FMT_R16G16B16A16_UNORM;
    case PNG_RGBA8: return bgr ? (format == FMT_B8G8R8A8_UNORM || format == FMT_B8G8R8A8_UNORM_SRGB) : (format == FMT_R8G8B8A8_UNORM || format == FMT_R8G8B8A8_UNORM_SRGB);
    default: return bgr ? (format == FMT_B8G8R8X8_UNORM || format == FMT_B8G8R8X8_UNORM_SRGB) : (format == FMT_R8G8B8A8_UNORM || format == FMT_R8G8B8A8_UNORM_SRGB);          // RGB 8, palette
    }
}
// The writer's (WriteImage): the PngSource of a format; -1 for one that is not written
DXTEX_FN constexpr int png_pack_source(int format)
{
    switch (format)
    {
    case FMT_R8_UNORM: return PNG_SRC_R8;
    case FMT_R16_UNORM: return PNG_SRC_R16;
    case FMT_R8G8B8A8_UNORM: case FMT_R8G8B8A8_UNORM_SRGB: return PNG_SRC_RGBA8;
    case FMT_B8G8R8A8_UNORM: case FMT_B8G8R8A8_UNORM_SRGB: return PNG_SRC_BGRA8;
    case FMT_R16G16B16A16_UNORM: return PNG_SRC_RGBA16;
    case FMT_B8G8R8X8_UNORM: case FMT_B8G8R8X8_UNORM_SRGB: return PNG_SRC_BGRX8;
    default: return -1;
    }
}

// The table a palette kind reads: 256 words. rgb = `count` entries of 3 bytes (PLTE), alpha = `alphaCount` bytes (tRNS) or null.
DXTEX_FN void png_palette_table(const uint8_t* rgb, uint32_t count, const uint8_t* alpha, uint32_t alphaCount, uint32_t (&table)[256])
{
    for (uint32_t i = 0; i < 256u; ++i)
    {
        uint32_t w = 0xFF000000u;
        if (i < count) w = uint32_t(rgb[3 * i]) | (uint32_t(rgb[3 * i + 1]) << 8) | (uint32_t(rgb[3 * i + 2]) << 16) | ((alpha && i < alphaCount) ? uint32_t(alpha[i]) << 24 : 0xFF000000u);
        table[i] = w;
    }
}

// One file texel of a kind with whole bytes, its bytes as a little-endian word -> the image texel likewise. table = the palette's 256
// words (PNG_P8), else unused.
DXTEX_FN uint64_t png_texel(int kind, uint64_t t, bool bgr, const uint32_t* table)
{
    switch (kind)
    {
    case PNG_G8: return t & 0xFFu;
    case PNG_G16: return swap16(uint32_t(t));
    case PNG_GA8: { const uint64_t g = t & 0xFFu; return g | (g << 8) | (g << 16) | (((t >> 8) & 0xFFu) << 24); }
    case PNG_GA16: { const uint64_t g = swap16(uint32_t(t)), a = swap16(uint32_t(t >> 16)); return g | (g << 16) | (g << 32) | (a << 48); }
    case PNG_RGB8: { const uint32_t w = (uint32_t(t) & 0x00FFFFFFu) | 0xFF000000u; return bgr ? swap_rb(w) : w; }
    case PNG_RGB16: return swap16x4(t & 0x0000FFFFFFFFFFFFull) | 0xFFFF000000000000ull;
    case PNG_RGBA8: return bgr ? swap_rb(uint32_t(t)) : uint32_t(t);
    case PNG_RGBA16: return swap16x4(t);
    case PNG_P8: { const uint32_t w = table[t & 0xFFu]; return bgr ? swap_rb(w) : w; }
    default: return 0;
    }
}

// Texel j (0 .. 8 / bits - 1) of a byte of a sub-byte kind: the first one sits in the high bits
DXTEX_FN constexpr uint32_t png_sample(uint32_t byte, uint32_t bits, uint32_t j) { return (byte >> (8u - bits * (j + 1u))) & ((1u << bits) - 1u); }
DXTEX_FN uint32_t png_sub_byte_texel(int kind, uint32_t byte, uint32_t j, bool bgr, const uint32_t* table)
{
    const uint32_t bits = png_file_bits(kind), s = png_sample(byte, bits, j);
    if (!png_is_palette(kind)) return s * png_grey_scale(bits);
    return bgr ? swap_rb(table[s]) : table[s];
}

// The writer's texel: an image texel as a little-endian word -> the file texel likewise (png_source_file_bytes(src) bytes of it count)
DXTEX_FN uint64_t png_pack(int src, uint64_t t)
{
    switch (src)
    {
    case PNG_SRC_R8: return t & 0xFFu;
    case PNG_SRC_R16: return swap16(uint32_t(t));
    case PNG_SRC_RGBA8: return uint32_t(t);
    case PNG_SRC_BGRA8: return swap_rb(uint32_t(t));
    case PNG_SRC_RGBA16: return swap16x4(t);
    case PNG_SRC_BGRX8: return swap_rb(uint32_t(t)) & 0x00FFFFFFu;
    default: return 0;
    }
}

// Texel x of an unfiltered file row -> one image texel at d, byte by byte: the host codec's loop body and what the kernels' narrow route
// does. Reads the byte(s) of texel x in `row`, writes png_image_bytes(kind).
DXTEX_FN void png_unpack_texel(const uint8_t* row, uint64_t x, uint8_t* d, int kind, bool bgr, const uint32_t* table)
{
    const uint32_t bits = png_file_bits(kind), D = png_image_bytes(kind);
    if (bits < 8u)
    {
        const uint32_t per = 8u / bits;
        le_store64(d, png_sub_byte_texel(kind, row[x / per], uint32_t(x % per), bgr, table), D);
    }
    else le_store64(d, png_texel(kind, le_load64(row + x * (bits / 8u), bits / 8u), bgr, table), D);
}

// One image texel at s -> one file texel at d, byte by byte
DXTEX_FN void png_pack_texel(const uint8_t* s, uint8_t* d, int src)
{
    le_store64(d, png_pack(src, le_load64(s, png_source_bytes(src))), png_source_file_bytes(src));
}
} // namespace dxtex
