// Truevision TGA texels, both directions, per texel: shared by the GPU kernels (tga.hip), the host codec (host/DirectXTexAMD_TGA.cpp, a
// plain C++ build) and the host check (tests/cpp/tga_check.cpp). Integer code: bytes move, nothing rounds.
//
// A file texel is its B = 1, 2, 3 or 4 bytes as a little-endian word (le_load32); what the reader makes of it is one of seven kinds, the
// cases of DecodeTGAHeader / CopyPixels (DirectXTexTGA.cpp:110-258, :738-1180):
//   TGA_GREY       1 byte            -> R8_UNORM        the byte
//   TGA_5551       2 bytes           -> B5G5R5A1_UNORM  the word; alpha counts as 255 with bit 15 set, else as 0
//   TGA_RGB_RGBA   3 bytes B, G, R   -> R8G8B8A8_UNORM  R, G, B, 255: opaque by construction
//   TGA_RGB_BGRX   3 bytes           -> B8G8R8X8_UNORM  B, G, R, 0 (TGA_FLAGS_BGR); no alpha rule
//   TGA_BGRA_RGBA  4 bytes B, G, R, A-> R8G8B8A8_UNORM  R, G, B, A
//   TGA_BGRA_BGRA  4 bytes           -> B8G8R8A8_UNORM  the word (TGA_FLAGS_BGR)
//   TGA_PALETTE    1 byte index      -> 4 bytes         the index's word of the 256-word table ReadPalette makes; no alpha rule
// Only TGA_5551 and the two four-byte kinds have an alpha rule (tga_has_alpha_rule): the reader ORs every texel's alpha and, separately,
// every texel's alpha ^ 255. The first is zero if every alpha is zero, the second if every alpha is 255 - the two facts the loader needs,
// whatever the order of the texels (tga_alpha_answer).
//
// The writer's three row kinds (SaveToTGAMemory, :2249-2330; Copy24bppScanline, :1288): copy (B = 1, 2 or 4), swap R and B
// (R8G8B8A8[_SRGB], B = 4), drop X (B8G8R8X8[_SRGB], B = 3).
#pragma once
#include "dxtex_stream.h"

namespace dxtex
{
enum TgaKind : int { TGA_GREY = 0, TGA_5551, TGA_RGB_RGBA, TGA_RGB_BGRX, TGA_BGRA_RGBA, TGA_BGRA_BGRA, TGA_PALETTE, TGA_KINDS };
enum TgaRow : int { TGA_ROW_COPY = 0, TGA_ROW_SWAP_RB, TGA_ROW_DROP_X };
// how the stream is ordered (the descriptor's bits 4 and 5) and the reader's TGA_FLAGS_ALLOW_ALL_ZERO_ALPHA: the DXTEX_TGA_* of include/dxtex_amd.h
enum TgaFlags : uint32_t { TGA_RIGHT_TO_LEFT = 0x1, TGA_TOP_DOWN = 0x2, TGA_ALLOW_ALL_ZERO_ALPHA = 0x4 };

// bytes of a file texel / of an image texel, per kind
DXTEX_FN constexpr uint32_t tga_file_bytes(int kind) { return kind == TGA_GREY || kind == TGA_PALETTE ? 1u : kind == TGA_5551 ? 2u : (kind == TGA_RGB_RGBA || kind == TGA_RGB_BGRX) ? 3u : 4u; }
DXTEX_FN constexpr uint32_t tga_image_bytes(int kind) { return kind == TGA_GREY ? 1u : kind == TGA_5551 ? 2u : 4u; }
DXTEX_FN constexpr bool tga_has_alpha_rule(int kind) { return kind == TGA_5551 || kind == TGA_BGRA_RGBA || kind == TGA_BGRA_BGRA; }

// The reader's table, for the C ABI and the host codec alike: which kind a (destination format before any sRGB relabel, bytes of a file
// texel, colour-mapped or not) is; -1 for a triple outside it
DXTEX_FN constexpr int tga_unpack_kind(int format, uint32_t bytesPerTexel, bool paletted)
{
    if (paletted) return (bytesPerTexel == 1 && (format == FMT_R8G8B8A8_UNORM || format == FMT_B8G8R8X8_UNORM)) ? TGA_PALETTE : -1;
    switch (format)
    {
    case FMT_R8_UNORM: return bytesPerTexel == 1 ? TGA_GREY : -1;
    case FMT_B5G5R5A1_UNORM: return bytesPerTexel == 2 ? TGA_5551 : -1;
    case FMT_R8G8B8A8_UNORM: return bytesPerTexel == 3 ? TGA_RGB_RGBA : bytesPerTexel == 4 ? TGA_BGRA_RGBA : -1;
    case FMT_B8G8R8X8_UNORM: return bytesPerTexel == 3 ? TGA_RGB_BGRX : -1;
    case FMT_B8G8R8A8_UNORM: return bytesPerTexel == 4 ? TGA_BGRA_BGRA : -1;
    default: return -1;
    }
}

// The writer's table (SaveToTGAMemory) likewise: the bytes of a file texel and the row kind of a format; 0 bytes for a format that is
// not written. An image texel has 4 bytes under TGA_ROW_DROP_X, else the file texel's.
struct TgaPackRow { uint32_t bytesPerTexel; int row; };
DXTEX_FN constexpr TgaPackRow tga_pack_row(int format)
{
    switch (format)
    {
    case FMT_R8G8B8A8_UNORM: case FMT_R8G8B8A8_UNORM_SRGB: return { 4u, TGA_ROW_SWAP_RB };
    case FMT_B8G8R8A8_UNORM: case FMT_B8G8R8A8_UNORM_SRGB: return { 4u, TGA_ROW_COPY };
    case FMT_B8G8R8X8_UNORM: case FMT_B8G8R8X8_UNORM_SRGB: return { 3u, TGA_ROW_DROP_X };
    case FMT_R8_UNORM: case FMT_A8_UNORM: return { 1u, TGA_ROW_COPY };
    case FMT_B5G5R5A1_UNORM: return { 2u, TGA_ROW_COPY };
    default: return { 0u, -1 };
    }
}
DXTEX_FN constexpr uint32_t tga_row_image_bytes(const TgaPackRow& r) { return r.row == TGA_ROW_DROP_X ? 4u : r.bytesPerTexel; }

// One file texel (its bytes as a word, the rest zero) as the image stores it; alpha = what the alpha rule sees of it (255 where the kind
// has no alpha). palette is read by TGA_PALETTE only.
DXTEX_FN uint32_t tga_unpack_texel(uint32_t t, int kind, const uint32_t* palette, uint32_t& alpha)
{
    alpha = 255u;
    switch (kind)
    {
    case TGA_5551: alpha = (t & 0x8000u) ? 255u : 0u; return t;
    case TGA_RGB_RGBA: return swap_rb(t) | 0xFF000000u;
    case TGA_BGRA_RGBA: alpha = t >> 24; return swap_rb(t);
    case TGA_BGRA_BGRA: alpha = t >> 24; return t;
    case TGA_PALETTE: return palette[t & 0xFFu];
    default: return t;          // TGA_GREY, and TGA_RGB_BGRX: X stays 0
    }
}

// The loader's answer from the two ORs over an image with an alpha rule (CopyPixels' tail, :1150-1180). 1: opaque - every alpha is 255, or
// every alpha is zero and the caller did not allow that, in which case makeOpaque tells it to set them (alpha 255; bit 15 of a 5:5:5:1
// word). 0: alpha is in use.
DXTEX_FN uint32_t tga_alpha_answer(uint32_t orOfAlpha, uint32_t orOfNotAlpha, bool allowAllZero, bool& makeOpaque)
{
    makeOpaque = orOfAlpha == 0u && !allowAllZero;
    return (makeOpaque || orOfNotAlpha == 0u) ? 1u : 0u;
}

// One image texel (its bytes as a word) as the file stores it; the low 3 bytes count for TGA_ROW_DROP_X
DXTEX_FN constexpr uint32_t tga_pack_texel(uint32_t t, int row)
{
    return row == TGA_ROW_SWAP_RB ? swap_rb(t) : row == TGA_ROW_DROP_X ? (t & 0x00FFFFFFu) : t;
}
} // namespace dxtex
