// OpenEXR scanline files (.exr): the rules behind the byte-serial half of the codec, for host and device (exr.hip, the host codec
// DirectXTexAMD_EXR.cpp and tests/cpp/exr_check.cpp build this header). tests/exr_ref.py restates them.
//
// THE STREAM. The host's Raw loader leaves the expanded bytes of every chunk in one stream, with a descriptor per chunk. A chunk of n
// bytes is either
//   plain   for each of its scanlines, for each channel of the file in name order, `width` samples of 2 (HALF) or 4 (UINT, FLOAT) bytes,
//           little-endian; or
//   coded   what a ZIP / ZIPS / RLE chunk expands to: t[0..n), with  u[0] = t[0], u[i] = (u[i-1] + t[i] - 128) mod 256  and
//           plain[2k] = u[k], plain[2k+1] = u[(n+1)/2 + k].
// The first step is a byte-wise inclusive prefix sum: u[i] = (t[0] + ... + t[i] - 128 i) mod 256, and 128 i mod 256 is 128 for an odd i
// and 0 for an even one. exr_undo runs it in place (exr.hip); the host runs exr_undo_serial. The second step is never carried out in
// memory: a chunk whose first step is done is UNDONE, and byte q of its plain layout is read at exr_plain_index(n, q). So the stream is
// never copied.
//
// THE TEXEL. R, G, B and A are each a channel of the file (its byte offset within a scanline and its type) or absent; a texel of
// R16G16B16A16_FLOAT is their four samples converted by exr_sample_to_half, an absent R, G or B reading 0 and an absent A 1.0
// (RgbaInputFile's fill). A file with Y and none of R, G, B names Y's channel three times.
//
// THE SAMPLE CONVERSION (ImfConvert.h's floatToHalf / uintToHalf, which the RGBA interface applies to a channel that is not HALF):
//   HALF    moves as bits
//   FLOAT   a finite value above 65504 is +Inf and one below -65504 is -Inf - also in (65504, 65520), where rounding to nearest would give
//           65504; a NaN is sign | 0x7c00 | mantissa >> 13, with bit 0 set where that leaves the mantissa zero; everything else is
//           rounded to nearest even, denormal halves included
//   UINT    above 65504 +Inf, otherwise its value rounded likewise
// THE WRITER'S CONVERSION is another one: XMConvertFloatToHalf (the reference stores through XMStoreHalf4), which rounds to nearest even
// and lets the overflow become infinity, so that 65519.996 is still 65504; a NaN is sign | 0x7e00 | mantissa >> 13.
#pragma once
#include "dxtex_stream.h"

namespace dxtex
{
enum : uint32_t { EXR_UINT = 0, EXR_HALF = 1, EXR_FLOAT = 2, EXR_ABSENT = 3 };
DXTEX_FN constexpr uint32_t exr_type_bytes(uint32_t type) { return type == EXR_HALF ? 2u : 4u; }

// One of R, G, B, A: where its `width` samples start within a scanline, and their type (EXR_ABSENT: none, offset ignored)
struct ExrChannel { uint32_t offset, type; };
// The window as the kernels see it: `rows` scanlines of scanlineBytes each; row y belongs to item y / itemRows of the destination
struct ExrLayout { uint32_t width, rows, itemRows, scanlineBytes; ExrChannel channel[4]; };
// A chunk of the stream: `bytes` = rows * scanlineBytes at `offset`, holding scanlines firstRow .. firstRow + rows - 1 of the window
struct ExrChunk { uint64_t offset; uint32_t bytes, firstRow, rows, coded; };

// exr_undo's tile: the bytes of a coded chunk that one workgroup of 256 lanes scans, 64 a lane. A chunk of more than one tile takes the
// two-launch form (partial sums, then apply).
constexpr uint32_t kExrUndoLaneBytes = 64u;
constexpr uint32_t kExrUndoTile = 256u * kExrUndoLaneBytes;
// chunk descriptors travel in the kernels' arguments, this many a launch
constexpr uint32_t kExrBatchMax = 64u;
// the most items (array slices) one window is cut into: the six faces of an environment map
constexpr uint32_t kExrItemsMax = 6u;

// bits of a float's magnitude below 2^16 -> half bits, rounded to nearest even (denormal halves included; at and above 65520 the result is
// 0x7c00)
DXTEX_FN uint32_t exr_round_half(uint32_t x)
{
    if (x < 0x38800000u)
    {
        if (x < 0x33000000u) return 0;          // below half the smallest denormal
        const uint32_t e = x >> 23, m = (x & 0x7FFFFFu) | 0x800000u, shift = 126u - e;          // 14..24
        const uint32_t q = m >> shift, rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1u);
        return q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);
    }
    const uint32_t y = x - 0x38000000u;
    return (y + 0x0FFFu + ((y >> 13) & 1u)) >> 13;
}

// the reader's FLOAT
DXTEX_FN uint32_t exr_float_to_half(uint32_t bits)
{
    const uint32_t sign = (bits >> 16) & 0x8000u, x = bits & 0x7FFFFFFFu;
    if (x > 0x7F800000u) { const uint32_t m = (x >> 13) & 0x3FFu; return sign | 0x7C00u | m | (m == 0u ? 1u : 0u); }
    if (x > 0x477FE000u) return sign | 0x7C00u;          // above 65504, infinity included
    return sign | exr_round_half(x);
}

// the reader's UINT: a value of up to 65504 is a float exactly
DXTEX_FN uint32_t exr_uint_to_half(uint32_t u)
{
    if (u > 65504u) return 0x7C00u;
    if (u == 0u) return 0u;
    uint32_t top = 31u;
    while (!(u >> top)) --top;
    return exr_round_half(((127u + top) << 23) | ((u << (23u - top)) & 0x7FFFFFu));
}

DXTEX_FN uint32_t exr_sample_to_half(uint32_t type, uint32_t raw)
{
    return type == EXR_HALF ? (raw & 0xFFFFu) : type == EXR_FLOAT ? exr_float_to_half(raw) : exr_uint_to_half(raw);
}

// the writer's float: XMConvertFloatToHalf
DXTEX_FN uint32_t exr_xm_float_to_half(uint32_t bits)
{
    const uint32_t sign = (bits >> 16) & 0x8000u, x = bits & 0x7FFFFFFFu;
    if (x > 0x7F800000u) return sign | 0x7E00u | ((x >> 13) & 0x3FFu);
    if (x >= 0x47800000u) return sign | 0x7C00u;
    return sign | exr_round_half(x);
}

// where byte q of the plain layout lies in an undone chunk of n bytes
DXTEX_FN constexpr uint32_t exr_plain_index(uint32_t n, uint32_t q) { return (q & 1u) ? (n + 1u) / 2u + (q >> 1) : (q >> 1); }

// `bytes` (2 or 4) bytes of the plain layout from byte q on, as a little-endian word. chunk: the chunk's first byte.
DXTEX_FN uint32_t exr_load(const uint8_t* chunk, bool coded, uint32_t n, uint32_t q, uint32_t bytes)
{
    if (!coded) return le_load32(chunk + q, bytes);
    uint32_t t = 0;
    for (uint32_t b = 0; b < bytes; ++b) t |= uint32_t(chunk[exr_plain_index(n, q + b)]) << (8u * b);
    return t;
}

// texel x of the scanline that starts at byte `line` of the chunk's plain layout
DXTEX_FN uint64_t exr_texel(const uint8_t* chunk, bool coded, uint32_t n, uint32_t line, const ExrChannel (&channel)[4], uint32_t x)
{
    uint64_t t = 0;
    for (uint32_t c = 0; c < 4u; ++c)
    {
        const uint32_t type = channel[c].type;
        uint32_t h = c == 3u ? 0x3C00u : 0u;
        if (type != EXR_ABSENT)
        {
            const uint32_t e = exr_type_bytes(type);
            h = exr_sample_to_half(type, exr_load(chunk, coded, n, line + channel[c].offset + x * e, e));
        }
        t |= uint64_t(h) << (16u * c);
    }
    return t;
}

// the first step on one core: t[0..n) in place
inline void exr_undo_serial(uint8_t* t, size_t n)
{
    for (size_t i = 1; i < n; ++i) t[i] = uint8_t(t[i - 1] + t[i] - 128);
}

// The writer's sources, by format; -1: none. A file texel is the four halves A, B, G, R, each in its own plane of a scanline.
enum : int { EXR_SRC_RGBA16F = 0, EXR_SRC_RGBA32F = 1, EXR_SRC_RGB32F = 2, EXR_SOURCES = 3 };
DXTEX_FN constexpr int exr_pack_source(int format)
{
    return format == FMT_R16G16B16A16_FLOAT ? EXR_SRC_RGBA16F : format == FMT_R32G32B32A32_FLOAT ? EXR_SRC_RGBA32F : format == FMT_R32G32B32_FLOAT ? EXR_SRC_RGB32F : -1;
}
DXTEX_FN constexpr uint32_t exr_source_bytes(int source) { return source == EXR_SRC_RGBA16F ? 8u : source == EXR_SRC_RGBA32F ? 16u : 12u; }
constexpr uint32_t kExrFileTexelBytes = 8u;

// a source texel held as S / 4 little-endian dwords -> its halves R, G, B, A in the four quarters of the result; R32G32B32 gets alpha 1.0
template<int SRC>
DXTEX_FN uint64_t exr_pack_halves(const uint32_t* w)
{
    if (SRC == EXR_SRC_RGBA16F) return uint64_t(w[0]) | (uint64_t(w[1]) << 32);
    uint64_t t = uint64_t(exr_xm_float_to_half(w[0])) | (uint64_t(exr_xm_float_to_half(w[1])) << 16) | (uint64_t(exr_xm_float_to_half(w[2])) << 32);
    return t | (uint64_t(SRC == EXR_SRC_RGBA32F ? exr_xm_float_to_half(w[3]) : 0x3C00u) << 48);
}

// the plane of a scanline that holds channel c of R, G, B, A: the file's order is A, B, G, R
DXTEX_FN constexpr uint32_t exr_file_plane(uint32_t c) { return c == 3u ? 0u : 3u - c; }

// texel x of a source row -> its four halves into their planes of the scanline at `line` (8 * width bytes)
inline void exr_pack_texel(const uint8_t* s, uint8_t* line, uint32_t width, uint32_t x, int source)
{
    uint32_t w[4] = { 0, 0, 0, 0 };
    const uint32_t S = exr_source_bytes(source);
    for (uint32_t i = 0; i < S / 4u; ++i) w[i] = le_load32(s + size_t(x) * S + 4u * i, 4u);
    const uint64_t t = source == EXR_SRC_RGBA16F ? exr_pack_halves<EXR_SRC_RGBA16F>(w) : source == EXR_SRC_RGBA32F ? exr_pack_halves<EXR_SRC_RGBA32F>(w) : exr_pack_halves<EXR_SRC_RGB32F>(w);
    for (uint32_t c = 0; c < 4u; ++c) le_store32(line + (size_t(exr_file_plane(c)) * width + x) * 2u, uint32_t(t >> (16u * c)) & 0xFFFFu, 2u);
}
} // namespace dxtex
