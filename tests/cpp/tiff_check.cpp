// tiff_check: csrc/dxtex_tiff.h as plain C++ - the serial predictor undo against sums written out here, the sample and texel rules on bytes
// spelled out, the kind and source tables. Run by tests/test_tiff_cpu.py; prints nothing and exits 0 when every check holds.
#include "dxtex_tiff.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace dxtex;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static TiffLayout layout(uint32_t kind, uint32_t predictor = 1, bool be = false, bool planar = false, bool wiz = false, bool opaque = false)
{
    const TiffKindRow k = tiff_kind_row(kind);
    return TiffLayout{ 4, 1, k.bits, k.samples, kind, predictor, be ? 1u : 0u, planar ? 1u : 0u, wiz ? 1u : 0u, opaque ? 1u : 0u };
}

static void tables()
{
    static const struct { uint32_t kind, bits, samples; int format; uint32_t bytes; } rows[] = {
        { TIFF_GREY1, 1, 1, FMT_R8_UNORM, 1 }, { TIFF_GREY4, 4, 1, FMT_R8_UNORM, 1 }, { TIFF_GREY8, 8, 1, FMT_R8_UNORM, 1 }, { TIFF_GREY16, 16, 1, FMT_R16_UNORM, 2 },
        { TIFF_GREY32F, 32, 1, FMT_R32_FLOAT, 4 }, { TIFF_PAL1, 1, 1, FMT_R8G8B8A8_UNORM, 4 }, { TIFF_PAL4, 4, 1, FMT_R8G8B8A8_UNORM, 4 }, { TIFF_PAL8, 8, 1, FMT_R8G8B8A8_UNORM, 4 },
        { TIFF_RGB8, 8, 3, FMT_R8G8B8A8_UNORM, 4 }, { TIFF_RGBA8, 8, 4, FMT_R8G8B8A8_UNORM, 4 }, { TIFF_RGB16, 16, 3, FMT_R16G16B16A16_UNORM, 8 },
        { TIFF_RGBA16, 16, 4, FMT_R16G16B16A16_UNORM, 8 }, { TIFF_RGB32F, 32, 3, FMT_R32G32B32_FLOAT, 12 }, { TIFF_RGBA32F, 32, 4, FMT_R32G32B32A32_FLOAT, 16 },
    };
    EXPECT(sizeof(rows) / sizeof(rows[0]) == TIFF_KINDS);
    for (const auto& r : rows)
    {
        const TiffKindRow k = tiff_kind_row(r.kind);
        EXPECT(k.bits == r.bits && k.samples == r.samples && k.format == r.format && k.imageBytes == r.bytes);
        EXPECT(tiff_unpacks_into(r.kind, r.format) && !tiff_unpacks_into(r.kind, FMT_BC1_UNORM));
        const bool colour8 = r.format == FMT_R8G8B8A8_UNORM;
        EXPECT(tiff_unpacks_into(r.kind, FMT_R8G8B8A8_UNORM_SRGB) == colour8 && tiff_may_be_srgb(r.kind) == colour8);
    }
    EXPECT(tiff_kind_row(TIFF_KINDS).bits == 0 && !tiff_unpacks_into(TIFF_KINDS, FMT_R8_UNORM));
    EXPECT(tiff_predictor_fits(1, 1) && tiff_predictor_fits(2, 8) && tiff_predictor_fits(2, 16) && tiff_predictor_fits(3, 32));
    EXPECT(!tiff_predictor_fits(2, 1) && !tiff_predictor_fits(2, 4) && !tiff_predictor_fits(2, 32) && !tiff_predictor_fits(3, 16) && !tiff_predictor_fits(4, 8) && !tiff_predictor_fits(0, 8));
    EXPECT(tiff_row_bytes(11, 1, 1) == 2 && tiff_row_bytes(7, 1, 4) == 4 && tiff_row_bytes(7, 3, 8) == 21 && tiff_row_bytes(5, 4, 16) == 40 && tiff_row_bytes(0x0FFFFFFF, 1, 1) == 0x02000000);
    EXPECT(kTiffUndoTile == 12288 && kTiffUndoLaneBytes % 8 == 0 && kTiffUndoLaneBytes % 6 == 0);
    // the writer's sources
    static const struct { int format; uint32_t bits, samples, sf, image, file; bool bgr, srgb; } sources[] = {
        { FMT_R8_UNORM, 8, 1, 1, 1, 1, false, false }, { FMT_R16_UNORM, 16, 1, 1, 2, 2, false, false }, { FMT_R32_FLOAT, 32, 1, 3, 4, 4, false, false },
        { FMT_R8G8B8A8_UNORM, 8, 4, 1, 4, 4, false, false }, { FMT_R8G8B8A8_UNORM_SRGB, 8, 4, 1, 4, 4, false, true }, { FMT_R16G16B16A16_UNORM, 16, 4, 1, 8, 8, false, false },
        { FMT_R32G32B32_FLOAT, 32, 3, 3, 12, 12, false, false }, { FMT_R32G32B32A32_FLOAT, 32, 4, 3, 16, 16, false, false }, { FMT_B8G8R8A8_UNORM, 8, 4, 1, 4, 4, true, false },
        { FMT_B8G8R8A8_UNORM_SRGB, 8, 4, 1, 4, 4, true, true }, { FMT_B8G8R8X8_UNORM, 8, 3, 1, 4, 3, true, false }, { FMT_B8G8R8X8_UNORM_SRGB, 8, 3, 1, 4, 3, true, true },
    };
    for (const auto& s : sources)
    {
        const TiffSource t = tiff_pack_source(s.format);
        EXPECT(t.bits == s.bits && t.samples == s.samples && t.sampleFormat == s.sf && t.imageBytes == s.image && t.fileBytes == s.file && t.bgr == s.bgr && t.srgb == s.srgb);
    }
    for (int f : { FMT_UNKNOWN, FMT_R16G16B16A16_FLOAT, FMT_R8G8_UNORM, FMT_BC7_UNORM, FMT_B5G6R5_UNORM, FMT_R10G10B10A2_UNORM, FMT_R16_FLOAT, FMT_A8_UNORM }) EXPECT(tiff_pack_source(f).bits == 0);
    EXPECT(tiff_pack_bgr(0x44332211u) == 0x44112233u);
}

static void undo()
{
    // every element width, stride and length up to past three pixels; the sums are written out again here
    uint32_t seed = 12345;
    auto next = [&] { seed = seed * 1664525u + 1013904223u; return seed >> 24; };
    for (uint32_t E = 1; E <= 2; ++E)
        for (uint32_t S : { 1u, 3u, 4u })
            for (uint32_t pixels = 1; pixels <= 9; ++pixels)
                for (int swap = 0; swap <= int(E == 2); ++swap)
                {
                    const uint32_t n = pixels * S;
                    std::vector<uint8_t> row(n * E), want(n * E);
                    std::vector<uint32_t> v(n);
                    for (uint32_t i = 0; i < n; ++i)
                    {
                        v[i] = E == 1 ? next() : (next() << 8) | next();
                        if (E == 1) row[i] = uint8_t(v[i]);
                        else { row[2 * i + (swap ? 1 : 0)] = uint8_t(v[i]); row[2 * i + (swap ? 0 : 1)] = uint8_t(v[i] >> 8); }
                    }
                    for (uint32_t i = 0; i < n; ++i)
                    {
                        uint32_t sum = 0;
                        for (uint32_t k = i % S; k <= i; k += S) sum += v[k];
                        le_store32(want.data() + i * E, sum & (E == 1 ? 0xFFu : 0xFFFFu), E);
                    }
                    tiff_undo_row_serial(row.data(), n * E, E, S, swap != 0);
                    EXPECT(row == want);
                }
    // the parameters by layout
    EXPECT(tiff_undo_element(layout(TIFF_RGB8, 2)) == 1 && tiff_undo_stride(layout(TIFF_RGB8, 2)) == 3 && !tiff_undo_swaps(layout(TIFF_RGB8, 2, true)));
    EXPECT(tiff_undo_element(layout(TIFF_RGBA16, 2)) == 2 && tiff_undo_stride(layout(TIFF_RGBA16, 2)) == 4 && tiff_undo_swaps(layout(TIFF_RGBA16, 2, true)) && !tiff_undo_swaps(layout(TIFF_RGBA16, 2)));
    EXPECT(tiff_undo_element(layout(TIFF_RGB32F, 3, true)) == 1 && tiff_undo_stride(layout(TIFF_RGB32F, 3)) == 3 && !tiff_undo_swaps(layout(TIFF_RGB32F, 3, true)));
    EXPECT(tiff_undo_stride(layout(TIFF_RGB16, 2, false, true)) == 1);
    // a segment: predictor 1 leaves it alone, predictor 2 runs every row on its own
    uint8_t two[6] = { 1, 2, 3, 4, 5, 6 };
    tiff_undo_segment_serial(two, TiffSegment{ 0, 0, 2, 0, 3, 3, 0 }, layout(TIFF_GREY8, 1));
    EXPECT(two[1] == 2 && two[5] == 6);
    tiff_undo_segment_serial(two, TiffSegment{ 0, 0, 2, 0, 3, 3, 0 }, layout(TIFF_GREY8, 2));
    EXPECT(two[0] == 1 && two[1] == 3 && two[2] == 6 && two[3] == 4 && two[4] == 9 && two[5] == 15);
}

static void texels()
{
    uint32_t t[4], pal[256];
    for (uint32_t i = 0; i < 256; ++i) pal[i] = 0xFF000000u | (i * 0x010203u);
    // bilevel and 4-bit samples come from the top of each byte; WhiteIsZero inverts before the multiplication
    const uint8_t bits[2] = { 0xA5, 0x80 };
    const uint32_t want1[9] = { 255, 0, 255, 0, 0, 255, 0, 255, 255 };
    for (uint32_t x = 0; x < 9; ++x)
    {
        tiff_texel(bits, 2, layout(TIFF_GREY1), nullptr, x, t); EXPECT(t[0] == want1[x]);
        tiff_texel(bits, 2, layout(TIFF_GREY1, 1, false, false, true), nullptr, x, t); EXPECT(t[0] == 255 - want1[x]);
        tiff_texel(bits, 2, layout(TIFF_PAL1), pal, x, t); EXPECT(t[0] == pal[want1[x] / 255]);
    }
    const uint8_t nib[2] = { 0x3C, 0xF0 };
    tiff_texel(nib, 2, layout(TIFF_GREY4), nullptr, 0, t); EXPECT(t[0] == 3 * 17);
    tiff_texel(nib, 2, layout(TIFF_GREY4), nullptr, 1, t); EXPECT(t[0] == 12 * 17);
    tiff_texel(nib, 2, layout(TIFF_GREY4, 1, false, false, true), nullptr, 2, t); EXPECT(t[0] == 0);
    tiff_texel(nib, 2, layout(TIFF_PAL4), pal, 1, t); EXPECT(t[0] == pal[12]);
    const uint8_t g8[2] = { 7, 200 };
    tiff_texel(g8, 2, layout(TIFF_GREY8, 1, false, false, true), nullptr, 1, t); EXPECT(t[0] == 55);
    tiff_texel(g8, 2, layout(TIFF_PAL8), pal, 1, t); EXPECT(t[0] == pal[200]);
    // 16 bits: a big-endian sample is swapped unless predictor 2 already did
    const uint8_t g16[2] = { 0x12, 0x34 };
    tiff_texel(g16, 2, layout(TIFF_GREY16), nullptr, 0, t); EXPECT(t[0] == 0x3412);
    tiff_texel(g16, 2, layout(TIFF_GREY16, 1, true), nullptr, 0, t); EXPECT(t[0] == 0x1234);
    tiff_texel(g16, 2, layout(TIFF_GREY16, 2, true), nullptr, 0, t); EXPECT(t[0] == 0x3412);
    tiff_texel(g16, 2, layout(TIFF_GREY16, 1, false, false, true), nullptr, 0, t); EXPECT(t[0] == 0xFFFF - 0x3412);
    // colour: RGB gets the maximum alpha, and so does a fourth sample under `opaque`
    const uint8_t c8[8] = { 1, 2, 3, 4, 5, 6, 7, 8 };
    tiff_texel(c8, 8, layout(TIFF_RGB8), nullptr, 1, t); EXPECT(t[0] == 0xFF060504u);
    tiff_texel(c8, 8, layout(TIFF_RGBA8), nullptr, 1, t); EXPECT(t[0] == 0x08070605u);
    tiff_texel(c8, 8, layout(TIFF_RGBA8, 1, false, false, false, true), nullptr, 1, t); EXPECT(t[0] == 0xFF070605u);
    tiff_texel(c8, 8, layout(TIFF_RGB16, 1, true), nullptr, 0, t); EXPECT(t[0] == 0x03040102u && t[1] == 0xFFFF0506u);
    tiff_texel(c8, 8, layout(TIFF_RGBA16), nullptr, 0, t); EXPECT(t[0] == 0x04030201u && t[1] == 0x08070605u);
    // floats: little-endian, big-endian, and the four byte planes of predictor 3 (the most significant first, whatever the byte order)
    const uint8_t f32[12] = { 0x00, 0x00, 0x80, 0x3F, 0x40, 0x00, 0x00, 0x00, 0x11, 0x22, 0x33, 0x44 };
    tiff_texel(f32, 12, layout(TIFF_RGB32F), nullptr, 0, t); EXPECT(t[0] == 0x3F800000u && t[1] == 0x00000040u && t[2] == 0x44332211u);
    tiff_texel(f32, 12, layout(TIFF_RGB32F, 1, true), nullptr, 0, t); EXPECT(t[0] == 0x0000803Fu && t[1] == 0x40000000u && t[2] == 0x11223344u);
    const uint8_t planes[12] = { 0x3F, 0x40, 0xC0, 0x80, 0x00, 0x40, 0x00, 0x00, 0x00, 0x00, 0x00, 0x01 };          // 1.0, 2.0, -3.0 + 1 ulp
    tiff_texel(planes, 12, layout(TIFF_RGB32F, 3), nullptr, 0, t); EXPECT(t[0] == 0x3F800000u && t[1] == 0x40000000u && t[2] == 0xC0400001u);
    tiff_texel(planes, 12, layout(TIFF_RGB32F, 3, true), nullptr, 0, t); EXPECT(t[0] == 0x3F800000u && t[2] == 0xC0400001u);
    const uint8_t four[16] = { 0, 0, 0x80, 0x3F, 0, 0, 0, 0x40, 0, 0, 0x40, 0x40, 0, 0, 0, 0x3F };
    tiff_texel(four, 16, layout(TIFF_RGBA32F), nullptr, 0, t); EXPECT(t[3] == 0x3F000000u);
    tiff_texel(four, 16, layout(TIFF_RGBA32F, 1, false, false, false, true), nullptr, 0, t); EXPECT(t[3] == 0x3F800000u && t[2] == 0x40400000u);
    // separate planes: one component each; the fourth under `opaque` is the maximum, and RGB of 8 and 16 bits has an alpha to fill
    EXPECT(tiff_plane_component(c8, 8, layout(TIFF_RGBA8, 1, false, true), 2, 5) == 6);
    EXPECT(tiff_plane_component(c8, 8, layout(TIFF_RGBA16, 1, false, true, false, true), 3, 1) == 0xFFFF);
    EXPECT(tiff_fills_alpha(layout(TIFF_RGB8)) && tiff_fills_alpha(layout(TIFF_RGB16)) && !tiff_fills_alpha(layout(TIFF_RGB32F)) && !tiff_fills_alpha(layout(TIFF_RGBA8)));
    EXPECT(tiff_alpha_max(8) == 0xFF && tiff_alpha_max(16) == 0xFFFF && tiff_alpha_max(32) == 0x3F800000u);
    // the no-kernel route
    for (uint32_t k : { TIFF_GREY8, TIFF_GREY16, TIFF_GREY32F, TIFF_RGBA8, TIFF_RGBA16, TIFF_RGBA32F, TIFF_RGB32F }) EXPECT(tiff_is_native(layout(k)));
    for (uint32_t k : { TIFF_GREY1, TIFF_GREY4, TIFF_PAL1, TIFF_PAL4, TIFF_PAL8, TIFF_RGB8, TIFF_RGB16 }) EXPECT(!tiff_is_native(layout(k)));
    EXPECT(!tiff_is_native(layout(TIFF_GREY8, 2)) && !tiff_is_native(layout(TIFF_GREY16, 1, true)) && tiff_is_native(layout(TIFF_GREY8, 1, true)));
    EXPECT(!tiff_is_native(layout(TIFF_RGBA8, 1, false, true)) && !tiff_is_native(layout(TIFF_GREY8, 1, false, false, true)) && !tiff_is_native(layout(TIFF_RGBA8, 1, false, false, false, true)));
    EXPECT(!tiff_is_native(layout(TIFF_RGB32F, 3)));
}

int main()
{
    tables();
    undo();
    texels();
    if (failures) std::printf("%d checks failed\n", failures);
    return failures ? 1 : 0;
}
