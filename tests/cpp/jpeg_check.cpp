// Host build of csrc/dxtex_jpeg.h for tests/test_jpeg_cpu.py: the functions the kernels and the host loader share, run serially on
// coefficients the test supplies, so that tests/jpeg_ref.py can be held against them without a file in between.
//
//   jpeg_check idct <quant: 64 uint16> <coefficients: n * 64 int16> <out: n * 64 uint8>
//       dequantisation, both passes and the range limit of every block
//   jpeg_check pixels <width> <height> <colour 0|1|2> <h> <v> <quant: 4 * 64 uint16> <coefficients> <out>
//       the whole pixel stage of a frame whose luma is h x v over 1 x 1 chroma (grey: 1 x 1), component c with table c, coefficients laid
//       out as include/dxtex_amd.h states: tight rows of R8_UNORM or R8G8B8A8_UNORM texels
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

static bool write_file(const char* path, const std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = buf.empty() || std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    return (std::fclose(f) == 0) && ok;
}

static int idct(char** a)
{
    std::vector<uint8_t> q, c;
    if (!read_file(a[0], q) || !read_file(a[1], c) || q.size() != 128 || c.size() % 128) return 1;
    std::vector<uint8_t> out(c.size() / 2);
    for (size_t b = 0; b < c.size() / 128; ++b)
        jpeg_idct_block(reinterpret_cast<const int16_t*>(c.data()) + b * 64, reinterpret_cast<const uint16_t*>(q.data()), out.data() + b * 64);
    return write_file(a[2], out) ? 0 : 1;
}

static int pixels(char** a)
{
    const uint32_t width = uint32_t(std::atoi(a[0])), height = uint32_t(std::atoi(a[1])), hmax = uint32_t(std::atoi(a[3])), vmax = uint32_t(std::atoi(a[4]));
    const int colour = std::atoi(a[2]);
    const uint32_t ncomp = colour == JPEG_GREY ? 1u : 3u;
    std::vector<uint8_t> q, c;
    if (!read_file(a[5], q) || !read_file(a[6], c) || q.size() != 512 || !width || !height) return 1;
    const uint16_t* quant = reinterpret_cast<const uint16_t*>(q.data());
    const int16_t* coef = reinterpret_cast<const int16_t*>(c.data());
    std::vector<std::vector<uint8_t>> store(ncomp);
    JpegPlane plane[3] = {};
    size_t at = 0;
    for (uint32_t k = 0; k < ncomp; ++k)
    {
        const uint32_t h = k ? 1u : hmax, v = k ? 1u : vmax;
        const uint32_t bw = jpeg_padded_blocks(width, h, hmax), bh = jpeg_padded_blocks(height, v, vmax), pitch = bw * 8;
        if ((at + size_t(bw) * bh * 64) * 2 > c.size()) return 1;
        store[k].resize(size_t(pitch) * bh * 8);
        for (uint32_t by = 0; by < bh; ++by)
            for (uint32_t bx = 0; bx < bw; ++bx)
            {
                uint8_t s[64];
                jpeg_idct_block(coef + at + (size_t(by) * bw + bx) * 64, quant + 64 * k, s);
                for (uint32_t r = 0; r < 8; ++r) std::memcpy(store[k].data() + size_t(by * 8 + r) * pitch + bx * 8, s + r * 8, 8);
            }
        plane[k] = JpegPlane{ store[k].data(), pitch, jpeg_downsampled(width, h, hmax), jpeg_downsampled(height, v, vmax), hmax / h, vmax / v };
        at += size_t(bw) * bh * 64;
    }
    const uint32_t texel = ncomp == 1 ? 1u : 4u;
    std::vector<uint8_t> out(size_t(width) * height * texel);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x)
        {
            uint8_t* d = out.data() + (size_t(y) * width + x) * texel;
            if (ncomp == 1) d[0] = uint8_t(jpeg_upsample(plane[0], x, y));
            else le_store32(d, jpeg_texel(colour, jpeg_upsample(plane[0], x, y), jpeg_upsample(plane[1], x, y), jpeg_upsample(plane[2], x, y)), 4);
        }
    return write_file(a[7], out) ? 0 : 1;
}

int main(int argc, char** argv)
{
    if (argc == 5 && !std::strcmp(argv[1], "idct")) return idct(argv + 2);
    if (argc == 10 && !std::strcmp(argv[1], "pixels")) return pixels(argv + 2);
    std::fprintf(stderr, "usage: jpeg_check idct <quant> <coefficients> <out> | pixels <width> <height> <colour> <h> <v> <quant> <coefficients> <out>\n");
    return 2;
}
