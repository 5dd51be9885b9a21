// Host build of directxtex_amd/csrc/dxtex_exr.h for tests/test_exr_cpu.py: the rules the kernels of exr.hip and the host codec share, one
// value at a time. All files are little-endian.
//
//   exr_check convert <in.bin> <out.bin>
//       in: records of two uint32, a channel type (0 UINT, 1 HALF, 2 FLOAT) and a sample's bits; out: one uint16 each, exr_sample_to_half
//   exr_check xm <in.bin> <out.bin>
//       in: float bits, uint32 each; out: two uint16 each - exr_xm_float_to_half, the writer's conversion, and XMConvertFloatToHalf of
//       oracle/shim/DirectXPackedVector.h, which this program includes
//   exr_check undo <in.bin> <out.bin>
//       in: one coded chunk; out: its plain layout - exr_undo_serial, then every byte through exr_plain_index
//   exr_check texels <in.bin> <width> <rows> <scanlineBytes> <coded 0|1> <oR> <tR> <oG> <tG> <oB> <tB> <oA> <tA> <out.bin>
//       in: one chunk of rows * scanlineBytes bytes (coded: still to be undone); out: width * rows texels of 8 bytes, exr_texel
//   exr_check pack <in.bin> <width> <height> <format> <out.bin>
//       in: tight rows of R16G16B16A16_FLOAT (10), R32G32B32A32_FLOAT (2) or R32G32B32_FLOAT (6); out: 8 * width * height bytes, exr_pack_texel
//   exr_check constants
//       prints kExrUndoTile, kExrBatchMax and kExrItemsMax
#include "dxtex_exr.h"
#include "DirectXPackedVector.h"

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

int main(int argc, char** argv)
{
    std::vector<uint8_t> in, out;
    if (argc == 2 && !std::strcmp(argv[1], "constants")) { std::printf("%u %u %u\n", kExrUndoTile, kExrBatchMax, kExrItemsMax); return 0; }
    if (argc < 4 || !read_file(argv[2], in)) { std::fprintf(stderr, "usage: exr_check convert|xm|undo|texels|pack|constants ...\n"); return 2; }
    if (!std::strcmp(argv[1], "convert") && argc == 4)
    {
        for (size_t i = 0; i + 8 <= in.size(); i += 8)
        {
            const uint32_t h = exr_sample_to_half(le_load32(&in[i], 4), le_load32(&in[i + 4], 4));
            out.push_back(uint8_t(h)); out.push_back(uint8_t(h >> 8));
        }
        return write_file(argv[3], out) ? 0 : 1;
    }
    if (!std::strcmp(argv[1], "xm") && argc == 4)
    {
        for (size_t i = 0; i + 4 <= in.size(); i += 4)
        {
            const uint32_t bits = le_load32(&in[i], 4);
            float f; std::memcpy(&f, &bits, 4);
            const uint32_t mine = exr_xm_float_to_half(bits), theirs = DirectX::PackedVector::XMConvertFloatToHalf(f);
            out.push_back(uint8_t(mine)); out.push_back(uint8_t(mine >> 8)); out.push_back(uint8_t(theirs)); out.push_back(uint8_t(theirs >> 8));
        }
        return write_file(argv[3], out) ? 0 : 1;
    }
    if (!std::strcmp(argv[1], "undo") && argc == 4)
    {
        exr_undo_serial(in.data(), in.size());
        out.resize(in.size());
        for (size_t q = 0; q < in.size(); ++q) out[q] = in[exr_plain_index(uint32_t(in.size()), uint32_t(q))];
        return write_file(argv[3], out) ? 0 : 1;
    }
    if (!std::strcmp(argv[1], "texels") && argc == 16)
    {
        const uint32_t width = uint32_t(std::atoll(argv[3])), rows = uint32_t(std::atoll(argv[4])), line = uint32_t(std::atoll(argv[5]));
        const bool coded = std::atoi(argv[6]) != 0;
        ExrChannel channel[4];
        for (int c = 0; c < 4; ++c) channel[c] = { uint32_t(std::atoll(argv[7 + 2 * c])), uint32_t(std::atoll(argv[8 + 2 * c])) };
        if (in.size() != size_t(rows) * line) return 1;
        for (int c = 0; c < 4; ++c) if (channel[c].type != EXR_ABSENT && channel[c].offset + uint64_t(width) * exr_type_bytes(channel[c].type) > line) return 1;
        if (coded) exr_undo_serial(in.data(), in.size());
        out.resize(size_t(width) * rows * 8);
        for (uint32_t r = 0; r < rows; ++r)
            for (uint32_t x = 0; x < width; ++x) le_store64(&out[(size_t(r) * width + x) * 8], exr_texel(in.data(), coded, uint32_t(in.size()), r * line, channel, x), 8);
        return write_file(argv[15], out) ? 0 : 1;
    }
    if (!std::strcmp(argv[1], "pack") && argc == 7)
    {
        const uint32_t width = uint32_t(std::atoll(argv[3])), height = uint32_t(std::atoll(argv[4]));
        const int source = exr_pack_source(std::atoi(argv[5]));
        if (source < 0 || in.size() != size_t(width) * height * exr_source_bytes(source)) return 1;
        out.resize(size_t(width) * height * kExrFileTexelBytes);
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x)
                exr_pack_texel(&in[size_t(y) * width * exr_source_bytes(source)], &out[size_t(y) * width * kExrFileTexelBytes], width, x, source);
        return write_file(argv[6], out) ? 0 : 1;
    }
    std::fprintf(stderr, "usage: exr_check convert|xm|undo|texels|pack|constants ...\n");
    return 2;
}
