// Host build of csrc/dxtex_png.h, the per-texel rules the GPU kernels and the host codec share, for tests/test_png_cpu.py, which compares
// every answer with tests/png_ref.py.
//
//   png_check unpack <kind> <bgr> <width> <height> <rows> <palette words | -> <out>
//       the unfiltered rows of <rows> through png_unpack_texel -> the image's tight rows. <palette words>: 256 little-endian words, the table
//       a palette kind reads
//   png_check pack <source> <width> <height> <in> <out>
//       tight image rows through png_pack_texel -> the file's rows
//   png_check table <plte> <trns | -> <out>
//       png_palette_table of a PLTE chunk's and a tRNS chunk's bytes: 256 little-endian words
//   png_check formats
//       the two format tables over their whole domain: "pack <format> <source>" for every format 0..191, and "unpack <kind> <flags> <format>"
//       for every (kind, PNG_BGR or not, format 0..191) that png_unpack_pairs accepts
#include "dxtex_png.h"

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

static bool write_file(const char* path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path, "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    return (std::fclose(f) == 0) && ok;
}

static int unpack(char** a)
{
    const int kind = std::atoi(a[0]);
    const bool bgr = std::atoi(a[1]) != 0;
    const uint32_t width = uint32_t(std::atoi(a[2])), height = uint32_t(std::atoi(a[3]));
    std::vector<uint8_t> in, pal;
    if (kind < 0 || kind >= PNG_KINDS || !read_file(a[4], in)) return 1;
    uint32_t table[256] = {};
    if (std::strcmp(a[5], "-") != 0)
    {
        if (!read_file(a[5], pal) || pal.size() != 1024) return 1;
        std::memcpy(table, pal.data(), 1024);
    }
    const size_t rowBytes = size_t(png_row_bytes(kind, width)), D = png_image_bytes(kind);
    if (in.size() < rowBytes * height) return 1;
    std::vector<uint8_t> image(size_t(width) * height * D);
    for (uint32_t y = 0; y < height; ++y)
        for (uint32_t x = 0; x < width; ++x) png_unpack_texel(in.data() + y * rowBytes, x, image.data() + (size_t(y) * width + x) * D, kind, bgr && png_takes_bgr(kind), table);
    return write_file(a[6], image.data(), image.size()) ? 0 : 1;
}

static int pack(char** a)
{
    const int source = std::atoi(a[0]);
    const uint32_t width = uint32_t(std::atoi(a[1])), height = uint32_t(std::atoi(a[2]));
    std::vector<uint8_t> in;
    if (source < 0 || source >= PNG_SOURCES || !read_file(a[3], in)) return 1;
    const size_t S = png_source_bytes(source), F = png_source_file_bytes(source);
    if (in.size() < size_t(width) * height * S) return 1;
    std::vector<uint8_t> file(size_t(width) * height * F);
    for (size_t i = 0; i < size_t(width) * height; ++i) png_pack_texel(in.data() + i * S, file.data() + i * F, source);
    return write_file(a[4], file.data(), file.size()) ? 0 : 1;
}

static int table(char** a)
{
    std::vector<uint8_t> plte, trns;
    if (!read_file(a[0], plte) || plte.size() % 3 != 0 || plte.size() > 768) return 1;
    const bool hasTrns = std::strcmp(a[1], "-") != 0;
    if (hasTrns && (!read_file(a[1], trns) || trns.size() > 256)) return 1;
    uint32_t words[256];
    png_palette_table(plte.data(), uint32_t(plte.size() / 3), hasTrns ? trns.data() : nullptr, uint32_t(trns.size()), words);
    return write_file(a[2], words, sizeof(words)) ? 0 : 1;
}

static int formats()
{
    for (int f = 0; f < 192; ++f) std::printf("pack %d %d\n", f, png_pack_source(f));
    for (int kind = 0; kind < PNG_KINDS; ++kind)
        for (uint32_t flags = 0; flags < 2; ++flags)
            for (int f = 0; f < 192; ++f)
                if (png_unpack_pairs(kind, flags, f)) std::printf("unpack %d %u %d\n", kind, flags, f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "formats")) return formats();
    if (argc == 9 && !std::strcmp(argv[1], "unpack")) return unpack(argv + 2);
    if (argc == 7 && !std::strcmp(argv[1], "pack")) return pack(argv + 2);
    if (argc == 5 && !std::strcmp(argv[1], "table")) return table(argv + 2);
    std::fprintf(stderr, "usage: png_check unpack <kind> <bgr> <w> <h> <rows> <palette|-> <out> | pack <source> <w> <h> <in> <out> | table <plte> <trns|-> <out> | formats\n");
    return 2;
}
