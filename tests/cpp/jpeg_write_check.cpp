// Host build of csrc/dxtex_jpeg.h's forward functions for tests/test_jpeg_write_cpu.py: the functions the kernels of jpeg_encode.hip and the
// host saver share, run serially on pixels the test supplies, so that tests/jpeg_write_ref.py can be held against them without a file in
// between.
//
//   jpeg_write_check coefficients <width> <height> <format> <pitch> <h> <v> <quant: 4 * 64 uint16> <pixels> <out>
//       the frame whose luma is h x v over 1 x 1 chroma (format 61, R8_UNORM: grey, 1 x 1), component c with table c, from rows of `pitch`
//       bytes of format 28 / 29 (R8G8B8A8), 87 / 91 (B8G8R8A8) or 88 / 93 (B8G8R8X8): the coefficients as include/dxtex_amd.h lays them out
//   jpeg_write_check formats
//       the format table over its whole domain: "texel <format> <JpegTexel, -1 for a format the coder does not take>" for every format 0..191
#include "dxtex_jpeg.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dxtex;

static bool read_file(const char* path, std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END); const long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    buf.resize(n > 0 ? size_t(n) : 0);
    const bool ok = buf.empty() || std::fread(buf.data(), 1, buf.size(), f) == buf.size();
    std::fclose(f);
    return ok;
}

static int coefficients(char** a)
{
    const uint32_t width = uint32_t(std::atoi(a[0])), height = uint32_t(std::atoi(a[1])), pitch = uint32_t(std::atoi(a[3]));
    const int format = std::atoi(a[2]);
    const bool grey = jpeg_texel_of(format) == JPEG_TEXEL_GREY, bgr = jpeg_texel_of(format) == JPEG_TEXEL_BGRX;
    const uint32_t hmax = grey ? 1u : uint32_t(std::atoi(a[4])), vmax = grey ? 1u : uint32_t(std::atoi(a[5])), ncomp = grey ? 1u : 3u;
    std::vector<uint8_t> q, px;
    if (!read_file(a[6], q) || !read_file(a[7], px) || q.size() != 512 || !width || !height) return 1;
    if (pitch < width * (grey ? 1u : 4u) || px.size() < size_t(pitch) * (height - 1) + width * (grey ? 1u : 4u)) return 1;
    const uint16_t* quant = reinterpret_cast<const uint16_t*>(q.data());
    const JpegSource source = { px.data(), pitch, width, height, grey, bgr };
    std::vector<int16_t> out;
    for (uint32_t c = 0; c < ncomp; ++c)
    {
        const uint32_t h = c ? 1u : hmax, v = c ? 1u : vmax;
        const uint32_t bw = jpeg_padded_blocks(width, h, hmax), bh = jpeg_padded_blocks(height, v, vmax);
        const uint32_t rw = jpeg_real_blocks(width, h, hmax), rh = jpeg_real_blocks(height, v, vmax);
        for (uint32_t by = 0; by < bh; ++by)
            for (uint32_t bx = 0; bx < bw; ++bx)
            {
                uint32_t sx = bx, sy = by;
                const bool dummy = jpeg_dummy_block(bx, by, rw, rh, h, sx, sy);
                uint8_t samples[64];
                for (uint32_t y = 0; y < 8; ++y)
                    for (uint32_t x = 0; x < 8; ++x) samples[y * 8 + x] = uint8_t(jpeg_plane_sample(source, c, hmax / h, vmax / v, sx * 8 + x, sy * 8 + y));
                int16_t block[64];
                jpeg_fdct_block(samples, 8, quant + 64 * c, block);
                if (dummy) std::memset(block + 1, 0, 63 * sizeof(int16_t));
                out.insert(out.end(), block, block + 64);
            }
    }
    FILE* f = std::fopen(a[8], "wb");
    if (!f) return 1;
    const bool ok = std::fwrite(out.data(), 2, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 1;
}

static int formats()
{
    for (int f = 0; f < 192; ++f) std::printf("texel %d %d\n", f, jpeg_texel_of(f));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "formats")) return formats();
    if (argc == 11 && !std::strcmp(argv[1], "coefficients")) return coefficients(argv + 2);
    std::fprintf(stderr, "usage: jpeg_write_check coefficients <width> <height> <format> <pitch> <h> <v> <quant> <pixels> <out> | formats\n");
    return 2;
}
