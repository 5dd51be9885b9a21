// Host build of csrc/dxtex_stream.h for tests/test_stream_cpu.py: the pieces under the five file codecs that no codec's own check reaches
// on their own, each against the plainest statement of what it computes.
//
//   stream_check texel_of   texel_of<B>, B = 1..4, k = 0..3, over random dwords against byte loads of the same memory
//   stream_check pack3x4    the four-texel three-byte repack against byte stores
//   stream_check le         le_load32 / le_store32 (1..4 bytes) and le_load64 / le_store64 (1..8) at every offset 0..7 of a buffer with
//                           sentinel bytes either side: the value, and no byte outside the range written
//   stream_check grid       stream_grid_x / stream_grid_y over the widths, heights and groups listed below
//   stream_check align      multiple_of over pointer and pitch values 0..31 for 1, 2, 4, 8 and 16 bytes
// Prints "<what>: <cases> cases, <failures> failures" and returns 1 where one failed.
#include "dxtex_stream.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>

using namespace dxtex;

static unsigned long long g_cases = 0, g_failures = 0;
static void check(bool ok, const char* what, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0)
{
    ++g_cases;
    if (ok) return;
    if (++g_failures <= 20) std::printf("FAIL %s (%llu, %llu, %llu)\n", what, a, b, c);
}

// B little-endian dwords as the 4 * B bytes they are in memory
template<uint32_t B>
static void bytes_of(const uint32_t (&w)[B], uint8_t (&bytes)[4 * B])
{
    for (uint32_t i = 0; i < 4 * B; ++i) bytes[i] = uint8_t(w[i / 4] >> (8 * (i % 4)));
}

template<uint32_t B>
static void texel_of_cases(std::mt19937& rng)
{
    for (int n = 0; n < 10000; ++n)
    {
        uint32_t w[B]; uint8_t bytes[4 * B];
        for (uint32_t& d : w) d = rng();
        bytes_of(w, bytes);
        for (uint32_t k = 0; k < 4; ++k)
        {
            uint32_t want = 0;
            for (uint32_t b = 0; b < B; ++b) want |= uint32_t(bytes[k * B + b]) << (8 * b);
            check(texel_of<B>(w, k) == want, "texel_of", B, k, want);
        }
    }
}

static void pack3x4_cases(std::mt19937& rng)
{
    for (int n = 0; n < 10000; ++n)
    {
        uint32_t t[4], out[3]; uint8_t want[12], got[12];
        for (uint32_t k = 0; k < 4; ++k)
        {
            t[k] = rng() & 0x00FFFFFFu;
            for (uint32_t b = 0; b < 3; ++b) want[3 * k + b] = uint8_t(t[k] >> (8 * b));
        }
        pack3x4(t, out);
        bytes_of(out, got);
        check(std::memcmp(got, want, 12) == 0, "pack3x4", t[0], t[1], t[2]);
    }
}

static void le_cases(std::mt19937& rng)
{
    constexpr uint32_t kPad = 8, kSize = kPad + 7 + 8 + kPad;
    for (uint32_t bytes = 1; bytes <= 8; ++bytes)
        for (uint32_t off = 0; off < 8; ++off)
            for (int n = 0; n < 50; ++n)
            {
                uint8_t buf[kSize], before[kSize];
                for (uint8_t& b : buf) b = uint8_t(rng());
                uint8_t* p = buf + kPad + off;
                uint64_t want = 0;
                for (uint32_t b = 0; b < bytes; ++b) want |= uint64_t(p[b]) << (8 * b);
                check(le_load64(p, bytes) == want, "le_load64", bytes, off);
                if (bytes <= 4) check(le_load32(p, bytes) == uint32_t(want), "le_load32", bytes, off);

                // a store of a value with every byte set differently from what is there leaves the bytes around it alone
                const uint64_t v = (uint64_t(rng()) << 32) | rng();
                for (int wide = 0; wide < 2; ++wide)
                {
                    if (!wide && bytes > 4) continue;
                    std::memcpy(before, buf, kSize);
                    if (wide) le_store64(p, v, bytes); else le_store32(p, uint32_t(v), bytes);
                    bool ok = true;
                    for (uint32_t i = 0; i < kSize; ++i)
                    {
                        const bool inside = i >= kPad + off && i < kPad + off + bytes;
                        ok = ok && buf[i] == (inside ? uint8_t(v >> (8 * (i - kPad - off))) : before[i]);
                    }
                    check(ok, wide ? "le_store64" : "le_store32", bytes, off);
                }
            }
}

static void grid_cases()
{
    const uint32_t widths[] = { 1, 3, 4, 255, 256, 257, 1025, (1u << 20) + 1, 0x3FFFFFFFu };
    const uint32_t heights[] = { 1, 2, 65535, 65536, 1u << 20 };
    const uint32_t groups[] = { 1, 2, 4, 8, 16 };
    for (uint32_t width : widths)
        for (uint32_t height : heights)
            for (uint32_t group : groups)
            {
                const uint64_t gx = stream_grid_x(width, group), gy = stream_grid_y(uint32_t(gx), height);
                // gx is the least value with gx * 256 * group >= width
                check(gx >= 1 && gx * 256 * group >= width && (gx - 1) * 256 * group < width, "grid x", width, group, gx);
                check(gy >= 1 && gy <= std::min<uint64_t>(height, 65535), "grid y range", width, height, gy);
                check(gy == std::min<uint64_t>(std::min<uint64_t>(height, 65535), std::max<uint64_t>(1, 8192 / gx)), "grid y", width, height, gy);
            }
}

static void align_cases()
{
    const uint32_t sizes[] = { 1, 2, 4, 8, 16 };
    for (uint32_t bytes : sizes)
        for (uintptr_t p = 0; p < 32; ++p)
            for (uint64_t pitch = 0; pitch < 32; ++pitch)
                check(multiple_of(reinterpret_cast<const void*>(p), pitch, bytes) == (p % bytes == 0 && pitch % bytes == 0), "multiple_of", p, pitch, bytes);
}

int main(int argc, char** argv)
{
    const char* what = argc > 1 ? argv[1] : "";
    std::mt19937 rng(12345);
    if (!std::strcmp(what, "texel_of")) { texel_of_cases<1>(rng); texel_of_cases<2>(rng); texel_of_cases<3>(rng); texel_of_cases<4>(rng); }
    else if (!std::strcmp(what, "pack3x4")) pack3x4_cases(rng);
    else if (!std::strcmp(what, "le")) le_cases(rng);
    else if (!std::strcmp(what, "grid")) grid_cases();
    else if (!std::strcmp(what, "align")) align_cases();
    else { std::fprintf(stderr, "usage: stream_check texel_of | pack3x4 | le | grid | align\n"); return 2; }
    std::printf("%s: %llu cases, %llu failures\n", what, g_cases, g_failures);
    return g_failures ? 1 : 0;
}
