// Host build of dxtex_rgbe.h (the Radiance RGBE texel, both directions) for tests/test_rgbe_cpu.py, which compares it bit for bit with
// the reference's .hdr reader and writer (oracle/_ref).
//
//   rgbe_check decode <exposure> <in.rgbe> <out.f32>
//       every four bytes of in.rgbe through rgbe_decode with scale = 1 / exposure, four floats each to out.f32. <exposure> is a decimal
//       number read as the .hdr header's is (atof, then float), or 0x followed by the bits of a float
//   rgbe_check encode <format 2 | 6 | 10> <in.bin> <out.rgbe>
//       the tightly packed R32G32B32A32_FLOAT (2), R32G32B32_FLOAT (6) or R16G16B16A16_FLOAT (10) texels of in.bin through rgbe_encode
#include "dxtex_rgbe.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dxtex;

static bool read_all(const char* path, std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    uint8_t chunk[65536];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    std::fclose(f);
    return true;
}

static bool write_all(const char* path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = std::fwrite(p, 1, bytes, f) == bytes;
    return (std::fclose(f) == 0) && ok;
}

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: rgbe_check decode <exposure> <in.rgbe> <out.f32> | encode <format> <in.bin> <out.rgbe>\n"); return 2; }
    std::vector<uint8_t> in;
    if (!read_all(argv[3], in)) return 1;
    if (!std::strcmp(argv[1], "decode"))
    {
        float exposure;
        if (!std::strncmp(argv[2], "0x", 2)) { const uint32_t bits = uint32_t(std::strtoul(argv[2], nullptr, 16)); std::memcpy(&exposure, &bits, 4); }
        else exposure = float(std::atof(argv[2]));
        const float scale = 1.0f / exposure;
        std::vector<float> out(in.size() / 4 * 4);
        for (size_t i = 0; i + 3 < in.size(); i += 4) rgbe_decode(&in[i], scale, &out[i]);
        return write_all(argv[4], out.data(), out.size() * sizeof(float)) ? 0 : 1;
    }
    if (!std::strcmp(argv[1], "encode"))
    {
        const int format = std::atoi(argv[2]);
        const size_t texel = format == 2 ? 16 : format == 6 ? 12 : format == 10 ? 8 : 0;
        if (!texel) return 2;
        const size_t n = in.size() / texel;
        std::vector<uint8_t> out(n * 4);
        for (size_t i = 0; i < n; ++i)
        {
            float c[3];
            if (format == 10)
            {
                uint16_t h[3];
                std::memcpy(h, &in[i * texel], 6);
                for (int k = 0; k < 3; ++k) c[k] = rgbe_half_to_float(h[k]);
            }
            else std::memcpy(c, &in[i * texel], 12);
            rgbe_encode(c[0], c[1], c[2], &out[i * 4]);
        }
        return write_all(argv[4], out.data(), out.size()) ? 0 : 1;
    }
    return 2;
}
