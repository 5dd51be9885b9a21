// Portable pixmap texels (.ppm, .pfm, .phm), both directions, per texel: shared by the GPU kernels (pnm.hip), the host codec
// (host/DirectXTexAMD_PNM.cpp, a plain C++ build) and the host check (tests/cpp/pnm_check.cpp). Integer code: bits move, and the one
// place that computes (a .ppm sample's rescale) is an integer division.
//
// The reader's five kinds (Texconv/PortablePixMap.cpp; LoadFromPortablePixMap :152-358, LoadFromPortablePixMapHDR :452-684):
//   PNM_P6   3 bytes R, G, B -> R8G8B8A8_UNORM        c_i = 255 * byte_i / maxval, word = c_0 | c_1 << 8 | c_2 << 16 | 0xff000000 (:216-219)
//   PNM_PF   3 x f32         -> R32G32B32A32_FLOAT    the three elements, alpha 0x3f800000 (:656-678)
//   PNM_Pf   1 x f32         -> R32_FLOAT             the element (:644-652)
//   PNM_PH   3 x f16         -> R16G16B16A16_FLOAT    the three elements, alpha 0x3c00 (:612-635)
//   PNM_Ph   1 x f16         -> R16_FLOAT             the element (:600-608)
// PNM_P6 has no clamp. A sample above maxval gives a c_i above 255 and its high bits are ORed into the next channel (or, for c_2, into
// alpha, where 0xff already stands). The expression is evaluated in 32-bit unsigned arithmetic, modulo 2^32, which is what the reference's
// int arithmetic stores into its uint32_t: c_2 << 16 passes 2^31 for a small maxval (255 * 255 / 1 << 16 = 0xfe010000). maxval == 255 is
// the identity, 255 * b / 255 == b, and is taken without a division or a table (a null `scale`): the word is the three bytes and 0xff.
// Every other maxval reads c from a 256-entry table of pnm_scale(i, maxval) - pnm.hip builds it once per workgroup in LDS, one division
// per lane, the host codec once per file.
// The float kinds move bits: PNM_BIG_ENDIAN swaps the bytes of every 2- or 4-byte element, nothing else looks at them, so NaN payloads,
// signalling NaNs, denormals and infinities pass as they are. File row y of a float kind is image row height - 1 - y; a .ppm is top-down.
//
// The writer (SaveToPortablePixMap :361-443, SaveToPortablePixMapHDR :688-758), one PnmSource per image format it takes:
//   PNM_P6   R8G8B8A8_UNORM[_SRGB] (PNM_SRC_RGBA8), B8G8R8A8 / B8G8R8X8_UNORM[_SRGB] (PNM_SRC_BGRA8: Convert's swizzle) -> R, G, B, top-down
//   PNM_PF   R32G32B32A32_FLOAT, R32G32B32_FLOAT, R16G16B16A16_FLOAT -> 3 little-endian floats, bottom row first
//   PNM_Pf   R32_FLOAT -> 1 little-endian float, bottom row first
// A half is widened as the reference's Convert(R16G16B16A16_FLOAT -> R32G32B32_FLOAT) does, XMConvertHalfToFloat on the way in and a
// plain store on the way out: exact for every finite half, a NaN keeps its sign, its payload (shifted up 13 bits) and its quiet bit as it
// is. That is dxtex_rgbe.h's rgbe_half_to_float, the widening the .hdr writer already uses; the bits of its result are taken as they are.
// The reference's flip is FlipRotate's TEX_FR_FLIP_VERTICAL, of which only "row y becomes row height - 1 - y" is taken.
#pragma once
#include "dxtex_rgbe.h"

namespace dxtex
{
enum PnmKind : int { PNM_P6 = 0, PNM_PF, PNM_Pf, PNM_PH, PNM_Ph, PNM_KINDS };
enum PnmFlags : uint32_t { PNM_BIG_ENDIAN = 0x1 };          // DXTEX_PNM_BIG_ENDIAN of include/dxtex_amd.h
enum PnmSource : int { PNM_SRC_RGBA8 = 0, PNM_SRC_BGRA8, PNM_SRC_RGBA32F, PNM_SRC_RGB32F, PNM_SRC_RGBA16F, PNM_SRC_R32F, PNM_SOURCES };

// bytes of one element (a sample), elements of a file texel and of an image texel, per reader kind
DXTEX_FN constexpr uint32_t pnm_element_bytes(int kind) { return kind == PNM_P6 ? 1u : (kind == PNM_PF || kind == PNM_Pf) ? 4u : 2u; }
DXTEX_FN constexpr uint32_t pnm_file_elements(int kind) { return (kind == PNM_Pf || kind == PNM_Ph) ? 1u : 3u; }
DXTEX_FN constexpr uint32_t pnm_image_elements(int kind) { return (kind == PNM_Pf || kind == PNM_Ph) ? 1u : 4u; }
DXTEX_FN constexpr uint32_t pnm_file_bytes(int kind) { return pnm_element_bytes(kind) * pnm_file_elements(kind); }
DXTEX_FN constexpr uint32_t pnm_image_bytes(int kind) { return pnm_element_bytes(kind) * pnm_image_elements(kind); }
// the element that stands for an alpha of one
DXTEX_FN constexpr uint32_t pnm_one(int kind) { return kind == PNM_P6 ? 0xFFu : (kind == PNM_PF || kind == PNM_Pf) ? 0x3F800000u : 0x3C00u; }
// file row y is image row pnm_image_row(kind, y, height)
DXTEX_FN constexpr uint32_t pnm_image_row(int kind, uint32_t y, uint32_t height) { return kind == PNM_P6 ? y : height - 1u - y; }

// the writer's side: bytes of an image texel per source, the kind it is written as, bytes of a file texel
DXTEX_FN constexpr uint32_t pnm_source_bytes(int src) { return src == PNM_SRC_RGBA32F ? 16u : src == PNM_SRC_RGB32F ? 12u : src == PNM_SRC_RGBA16F ? 8u : 4u; }
DXTEX_FN constexpr int pnm_source_kind(int src) { return (src == PNM_SRC_RGBA8 || src == PNM_SRC_BGRA8) ? PNM_P6 : src == PNM_SRC_R32F ? PNM_Pf : PNM_PF; }

// The two format tables, for the C ABI and the host codec alike. The reader's: the one format a kind unpacks into.
DXTEX_FN constexpr int pnm_unpack_format(int kind)
{
    return kind == PNM_P6 ? FMT_R8G8B8A8_UNORM : kind == PNM_PF ? FMT_R32G32B32A32_FLOAT : kind == PNM_Pf ? FMT_R32_FLOAT : kind == PNM_PH ? FMT_R16G16B16A16_FLOAT : FMT_R16_FLOAT;
}
// The writer's (SaveToPortablePixMap, SaveToPortablePixMapHDR): the PnmSource of a format, -1 for one that is not written;
// pnm_source_kind() of it is the kind it is written as.
DXTEX_FN constexpr int pnm_pack_source(int format)
{
    switch (format)
    {
    case FMT_R8G8B8A8_UNORM: case FMT_R8G8B8A8_UNORM_SRGB: return PNM_SRC_RGBA8;
    case FMT_B8G8R8A8_UNORM: case FMT_B8G8R8A8_UNORM_SRGB: case FMT_B8G8R8X8_UNORM: case FMT_B8G8R8X8_UNORM_SRGB: return PNM_SRC_BGRA8;
    case FMT_R32G32B32A32_FLOAT: return PNM_SRC_RGBA32F;
    case FMT_R32G32B32_FLOAT: return PNM_SRC_RGB32F;
    case FMT_R16G16B16A16_FLOAT: return PNM_SRC_RGBA16F;
    case FMT_R32_FLOAT: return PNM_SRC_R32F;
    default: return -1;
    }
}

// 255 * i / maxval in uint32_t; 1 <= maxval <= 255 and i <= 255, so nothing wraps here
DXTEX_FN constexpr uint32_t pnm_scale(uint32_t i, uint32_t maxval) { return 255u * i / maxval; }

// One P6 texel, its three bytes as a little-endian word (the top byte is ignored). scale = the table of pnm_scale(i, maxval), or null for
// maxval == 255.
DXTEX_FN uint32_t pnm_p6_texel(uint32_t rgb, const uint32_t* scale)
{
    if (!scale) return rgb | 0xFF000000u;
    return scale[rgb & 0xFFu] | (scale[(rgb >> 8) & 0xFFu] << 8) | (scale[(rgb >> 16) & 0xFFu] << 16) | 0xFF000000u;          // modulo 2^32
}

// One element of a float kind, its bytes as a little-endian word, as the image holds it
DXTEX_FN constexpr uint32_t pnm_element(uint32_t e, uint32_t bytes, bool bigEndian) { return !bigEndian ? e : bytes == 2u ? swap16(e) : swap32(e); }

// The writer's P6 texel: an image word -> R, G, B in the low three bytes
DXTEX_FN constexpr uint32_t pnm_pack_p6(uint32_t t, bool bgr)
{
    return (bgr ? swap_rb(t) : t) & 0x00FFFFFFu;
}

// The writer's half -> float, as bits
DXTEX_FN uint32_t pnm_half_to_float_bits(uint32_t h)
{
    const float f = rgbe_half_to_float(uint16_t(h));
    uint32_t bits;
    __builtin_memcpy(&bits, &f, 4);
    return bits;
}

// One file texel at s -> one image texel at d, byte by byte: the host codec's loop body and what the kernels' narrow route does where
// nothing is aligned. Reads pnm_file_bytes(kind) bytes, writes pnm_image_bytes(kind).
DXTEX_FN void pnm_unpack_texel(const uint8_t* s, uint8_t* d, int kind, bool bigEndian, const uint32_t* scale)
{
    if (kind == PNM_P6) { le_store32(d, pnm_p6_texel(le_load32(s, 3u), scale), 4u); return; }
    const uint32_t E = pnm_element_bytes(kind), n = pnm_file_elements(kind);
    for (uint32_t c = 0; c < n; ++c) le_store32(d + c * E, pnm_element(le_load32(s + c * E, E), E, bigEndian), E);
    if (n == 3u) le_store32(d + 3u * E, pnm_one(kind), E);
}

// One image texel at s -> one file texel at d, byte by byte. Reads pnm_source_bytes(src) bytes, writes pnm_file_bytes(pnm_source_kind(src)).
DXTEX_FN void pnm_pack_texel(const uint8_t* s, uint8_t* d, int src)
{
    switch (src)
    {
    case PNM_SRC_RGBA8: case PNM_SRC_BGRA8: le_store32(d, pnm_pack_p6(le_load32(s, 4u), src == PNM_SRC_BGRA8), 3u); break;
    case PNM_SRC_RGBA16F: for (uint32_t c = 0; c < 3u; ++c) le_store32(d + 4u * c, pnm_half_to_float_bits(le_load32(s + 2u * c, 2u)), 4u); break;
    case PNM_SRC_R32F: le_store32(d, le_load32(s, 4u), 4u); break;
    default: for (uint32_t c = 0; c < 3u; ++c) le_store32(d + 4u * c, le_load32(s + 4u * c, 4u), 4u); break;          // RGBA32F, RGB32F
    }
}
} // namespace dxtex
