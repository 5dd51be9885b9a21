// TIFF files (.tif, .tiff): the rules behind the byte-serial half of the codec, for host and device (tiff.hip, the host codec
// DirectXTexAMD_TIFF.cpp and tests/cpp/tiff_check.cpp build this header). tests/tiff_ref.py restates them.
//
// THE STREAM. The host's Raw loader leaves the expanded bytes of every strip or tile in one stream, with a descriptor per segment. A segment
// holds `rows` rows of rowBytes each - a strip's row is the image's width, a tile's row the tile's width, a separate plane's row one sample
// a pixel - still predictor-coded, in the file's byte order, at the file's bits per sample. Rows start on byte boundaries.
//
// THE UNDO (tiff_undo in tiff.hip, tiff_undo_row_serial here), in place, row by row:
//   predictor 2   an inclusive prefix sum over the row's 8- or 16-bit elements with a stride of samples per pixel (1 in a separate plane),
//                 modulo the element's width; a big-endian 16-bit row is swapped on the way and left little-endian
//   predictor 3   the same sum over the row's bytes, with the stride in bytes equal to samples per pixel. What it leaves is four byte
//                 planes of rowBytes / 4 each, the most significant first whatever the file's byte order; they are never regrouped in
//                 memory: byte b of float i is read at (3 - b) * (rowBytes / 4) + i (tiff_sample)
// so predictor 3 is predictor 2 over 8-bit elements of a row four times as long.
//
// THE TEXEL. tiff_texel makes texel x of a chunky row: 1- and 4-bit samples are taken from the top of each byte and multiplied out (255,
// 17), WhiteIsZero inverts at the sample's depth, a palette index reads a 256-word table, RGB gets the alpha of its depth's maximum (1.0
// for floats) and so does a fourth sample that is not alpha (`opaque`), big-endian samples the undo did not touch are swapped. A separate
// plane's row gives one component of every texel (tiff_plane_component); plane 0 also fills the alpha that RGB lacks.
#pragma once
#include "dxtex_stream.h"

namespace dxtex
{
// A strip or a tile (of one plane, where planes are separate): `rows` rows of rowBytes at `offset` of the stream, rows firstRow .. and
// columns firstCol .. firstCol + cols - 1 of the image; a tile's row may hold more columns than `cols` (padding)
struct TiffSegment { uint64_t offset; uint32_t firstRow, rows, firstCol, cols, rowBytes, plane; };

// file kinds; the table below gives bits, samples, destination format and bytes of an image texel
enum : uint32_t
{
    TIFF_GREY1 = 0, TIFF_GREY4, TIFF_GREY8, TIFF_GREY16, TIFF_GREY32F, TIFF_PAL1, TIFF_PAL4, TIFF_PAL8,
    TIFF_RGB8, TIFF_RGBA8, TIFF_RGB16, TIFF_RGBA16, TIFF_RGB32F, TIFF_RGBA32F, TIFF_KINDS
};
struct TiffKindRow { uint32_t bits, samples; int format; uint32_t imageBytes; };
DXTEX_FN constexpr TiffKindRow tiff_kind_row(uint32_t kind)
{
    return kind == TIFF_GREY1 ? TiffKindRow{ 1, 1, FMT_R8_UNORM, 1 } : kind == TIFF_GREY4 ? TiffKindRow{ 4, 1, FMT_R8_UNORM, 1 } :
           kind == TIFF_GREY8 ? TiffKindRow{ 8, 1, FMT_R8_UNORM, 1 } : kind == TIFF_GREY16 ? TiffKindRow{ 16, 1, FMT_R16_UNORM, 2 } :
           kind == TIFF_GREY32F ? TiffKindRow{ 32, 1, FMT_R32_FLOAT, 4 } : kind == TIFF_PAL1 ? TiffKindRow{ 1, 1, FMT_R8G8B8A8_UNORM, 4 } :
           kind == TIFF_PAL4 ? TiffKindRow{ 4, 1, FMT_R8G8B8A8_UNORM, 4 } : kind == TIFF_PAL8 ? TiffKindRow{ 8, 1, FMT_R8G8B8A8_UNORM, 4 } :
           kind == TIFF_RGB8 ? TiffKindRow{ 8, 3, FMT_R8G8B8A8_UNORM, 4 } : kind == TIFF_RGBA8 ? TiffKindRow{ 8, 4, FMT_R8G8B8A8_UNORM, 4 } :
           kind == TIFF_RGB16 ? TiffKindRow{ 16, 3, FMT_R16G16B16A16_UNORM, 8 } : kind == TIFF_RGBA16 ? TiffKindRow{ 16, 4, FMT_R16G16B16A16_UNORM, 8 } :
           kind == TIFF_RGB32F ? TiffKindRow{ 32, 3, FMT_R32G32B32_FLOAT, 12 } : kind == TIFF_RGBA32F ? TiffKindRow{ 32, 4, FMT_R32G32B32A32_FLOAT, 16 } :
           TiffKindRow{ 0, 0, FMT_UNKNOWN, 0 };
}
DXTEX_FN constexpr bool tiff_is_palette(uint32_t kind) { return kind >= TIFF_PAL1 && kind <= TIFF_PAL8; }
// the 8-bit colour kinds, whose destination may be the _SRGB twin
DXTEX_FN constexpr bool tiff_may_be_srgb(uint32_t kind) { return tiff_is_palette(kind) || kind == TIFF_RGB8 || kind == TIFF_RGBA8; }
DXTEX_FN constexpr bool tiff_unpacks_into(uint32_t kind, int format)
{
    return kind < TIFF_KINDS && (format == tiff_kind_row(kind).format || (tiff_may_be_srgb(kind) && format == FMT_R8G8B8A8_UNORM_SRGB));
}

// The file as the kernels see it. bits and samples are the kind's; predictor 1, 2 or 3; opaque: the fourth sample is not alpha and reads
// as the maximum
struct TiffLayout { uint32_t width, height, bits, samples, kind, predictor, bigEndian, planar, whiteIsZero, opaque; };

DXTEX_FN constexpr uint32_t tiff_row_bytes(uint32_t columns, uint32_t samples, uint32_t bits) { return uint32_t((uint64_t(columns) * samples * bits + 7u) / 8u); }
// the alpha a kind without one gets: the maximum of its depth, 1.0 for floats
DXTEX_FN constexpr uint32_t tiff_alpha_max(uint32_t bits) { return bits == 32u ? 0x3F800000u : bits == 16u ? 0xFFFFu : 0xFFu; }

// the undo's element width in bytes, its stride in elements and whether it swaps: predictor 2 or 3 (tiff_undo_row_serial, tiff.hip)
DXTEX_FN constexpr uint32_t tiff_undo_element(const TiffLayout& l) { return l.predictor == 2u && l.bits == 16u ? 2u : 1u; }
DXTEX_FN constexpr uint32_t tiff_undo_stride(const TiffLayout& l) { return l.planar ? 1u : l.samples; }
DXTEX_FN constexpr bool tiff_undo_swaps(const TiffLayout& l) { return l.predictor == 2u && l.bits == 16u && l.bigEndian != 0u; }
// what predictor 2 runs over (the rest is HRESULT_E_NOT_SUPPORTED), and predictor 3
DXTEX_FN constexpr bool tiff_predictor_fits(uint32_t predictor, uint32_t bits)
{
    return predictor == 1u || (predictor == 2u && (bits == 8u || bits == 16u)) || (predictor == 3u && bits == 32u);
}

// tiff_undo's tile: the bytes of a row that one workgroup of 256 lanes scans in one pass, 48 a lane - a whole number of pixels of 1, 2,
// 3, 4, 6 and 8 bytes. A longer row is walked tile by tile with a carry.
constexpr uint32_t kTiffUndoLaneBytes = 48u;
constexpr uint32_t kTiffUndoTile = 256u * kTiffUndoLaneBytes;
// segment descriptors travel in the kernels' arguments, this many a launch
constexpr uint32_t kTiffBatchMax = 64u;

// the undo of one row on one core
inline void tiff_undo_row_serial(uint8_t* row, uint32_t rowBytes, uint32_t element, uint32_t stride, bool swap)
{
    if (element == 1u) { for (uint32_t i = stride; i < rowBytes; ++i) row[i] = uint8_t(row[i] + row[i - stride]); return; }
    for (uint32_t i = 0; i < rowBytes / 2u; ++i)
    {
        uint32_t v = le_load32(row + 2u * i, 2u);
        if (swap) v = swap16(v);
        if (i >= stride) v += le_load32(row + 2u * (i - stride), 2u);
        le_store32(row + 2u * i, v, 2u);
    }
}
inline void tiff_undo_segment_serial(uint8_t* stream, const TiffSegment& s, const TiffLayout& l)
{
    if (l.predictor < 2u) return;
    for (uint32_t r = 0; r < s.rows; ++r) tiff_undo_row_serial(stream + s.offset + uint64_t(r) * s.rowBytes, s.rowBytes, tiff_undo_element(l), tiff_undo_stride(l), tiff_undo_swaps(l));
}

// sample i of an undone row as a little-endian value
DXTEX_FN uint32_t tiff_sample(const uint8_t* row, uint32_t rowBytes, const TiffLayout& l, uint32_t i)
{
    if (l.bits == 1u) return (row[i >> 3] >> (7u - (i & 7u))) & 1u;
    if (l.bits == 4u) return (row[i >> 1] >> ((i & 1u) ? 0u : 4u)) & 15u;
    if (l.bits == 8u) return row[i];
    if (l.bits == 16u) { const uint32_t v = le_load32(row + 2u * i, 2u); return l.bigEndian && l.predictor != 2u ? swap16(v) : v; }
    if (l.predictor == 3u)
    {
        const uint32_t plane = rowBytes / 4u;
        return (uint32_t(row[i]) << 24) | (uint32_t(row[plane + i]) << 16) | (uint32_t(row[2u * plane + i]) << 8) | row[3u * plane + i];
    }
    const uint32_t v = le_load32(row + 4u * i, 4u);
    return l.bigEndian ? swap32(v) : v;
}

// texel x of a chunky row -> its imageBytes as little-endian words. palette: 256 words, for the palette kinds.
DXTEX_FN void tiff_texel(const uint8_t* row, uint32_t rowBytes, const TiffLayout& l, const uint32_t* palette, uint32_t x, uint32_t (&out)[4])
{
    out[0] = out[1] = out[2] = out[3] = 0u;
    if (l.samples == 1u)
    {
        uint32_t v = tiff_sample(row, rowBytes, l, x);
        if (tiff_is_palette(l.kind)) { out[0] = palette[v]; return; }
        if (l.whiteIsZero) v = l.bits == 32u ? v : ((l.bits == 16u ? 0xFFFFu : (1u << l.bits) - 1u) - v);
        out[0] = l.bits == 1u ? v * 255u : l.bits == 4u ? v * 17u : v;
        return;
    }
    const uint32_t S = l.samples, r = tiff_sample(row, rowBytes, l, x * S), g = tiff_sample(row, rowBytes, l, x * S + 1u), b = tiff_sample(row, rowBytes, l, x * S + 2u);
    const uint32_t a = S == 4u && !l.opaque ? tiff_sample(row, rowBytes, l, x * S + 3u) : tiff_alpha_max(l.bits);
    if (l.bits == 8u) out[0] = r | (g << 8) | (b << 16) | (a << 24);
    else if (l.bits == 16u) { out[0] = r | (g << 16); out[1] = b | (a << 16); }
    else { out[0] = r; out[1] = g; out[2] = b; out[3] = a; }
}

// column x of a separate plane's row -> component `plane` of the texel: its value, where it lies in the texel and its bytes
DXTEX_FN uint32_t tiff_plane_component(const uint8_t* row, uint32_t rowBytes, const TiffLayout& l, uint32_t plane, uint32_t x)
{
    return plane == 3u && l.opaque ? tiff_alpha_max(l.bits) : tiff_sample(row, rowBytes, l, x);
}
// whether the image's texel has a fourth component that a file of three samples does not bring: plane 0 fills it
DXTEX_FN constexpr bool tiff_fills_alpha(const TiffLayout& l) { return l.samples == 3u && l.bits != 32u; }

// A file that is its image already: chunky (or one sample), strips, no predictor, little-endian or 8-bit, the kind's texel the image's,
// nothing inverted or forced. Its rows are copied and no kernel runs.
DXTEX_FN constexpr bool tiff_is_native(const TiffLayout& l)
{
    return l.predictor == 1u && (!l.planar || l.samples == 1u) && (!l.bigEndian || l.bits == 8u) && !l.whiteIsZero && !l.opaque &&
           (l.kind == TIFF_GREY8 || l.kind == TIFF_GREY16 || l.kind == TIFF_GREY32F || l.kind == TIFF_RGBA8 || l.kind == TIFF_RGBA16 || l.kind == TIFF_RGBA32F || l.kind == TIFF_RGB32F);
}

// The writer's sources, by format. A source moves as tight rows, except the BGR ones, which tiff_pack swizzles: B8G8R8A8 is written RGBA,
// B8G8R8X8 RGB at 3 bytes.
struct TiffSource { uint32_t bits, samples, sampleFormat, imageBytes, fileBytes; bool bgr, srgb; };
DXTEX_FN constexpr TiffSource tiff_pack_source(int format)
{
    return format == FMT_R8_UNORM ? TiffSource{ 8, 1, 1, 1, 1, false, false } : format == FMT_R16_UNORM ? TiffSource{ 16, 1, 1, 2, 2, false, false } :
           format == FMT_R32_FLOAT ? TiffSource{ 32, 1, 3, 4, 4, false, false } :
           format == FMT_R8G8B8A8_UNORM ? TiffSource{ 8, 4, 1, 4, 4, false, false } : format == FMT_R8G8B8A8_UNORM_SRGB ? TiffSource{ 8, 4, 1, 4, 4, false, true } :
           format == FMT_R16G16B16A16_UNORM ? TiffSource{ 16, 4, 1, 8, 8, false, false } :
           format == FMT_R32G32B32_FLOAT ? TiffSource{ 32, 3, 3, 12, 12, false, false } : format == FMT_R32G32B32A32_FLOAT ? TiffSource{ 32, 4, 3, 16, 16, false, false } :
           format == FMT_B8G8R8A8_UNORM ? TiffSource{ 8, 4, 1, 4, 4, true, false } : format == FMT_B8G8R8A8_UNORM_SRGB ? TiffSource{ 8, 4, 1, 4, 4, true, true } :
           format == FMT_B8G8R8X8_UNORM ? TiffSource{ 8, 3, 1, 4, 3, true, false } : format == FMT_B8G8R8X8_UNORM_SRGB ? TiffSource{ 8, 3, 1, 4, 3, true, true } :
           TiffSource{ 0, 0, 0, 0, 0, false, false };
}
// a BGR source texel -> the file's: R and B exchanged; the fourth byte is dropped by a 3-byte file texel
DXTEX_FN constexpr uint32_t tiff_pack_bgr(uint32_t texel) { return swap_rb(texel); }
} // namespace dxtex
