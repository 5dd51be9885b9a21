// Host build of csrc/dxtex_pnm.h, the per-texel rules the GPU kernels and the host codec share, for tests/test_pnm_cpu.py, which compares
// every answer with tests/pnm_ref.py.
//
//   pnm_check p6 <out>
//       for maxval 1..255 and byte b 0..255 (the whole domain of a sample, 65 280 cases): the word of the texel (b, 255 - b, b ^ 0x5a), so
//       that every byte stands in every channel under every maxval, the ones above maxval - whose c spills into the next channel -
//       included; little-endian uint32 each. maxval 255 goes the identity route (no table), and once more through a table of its own,
//       appended as a 256th block of 256 words: the two must agree.
//   pnm_check unpack <kind> <big endian> <maxval> <width> <height> <in> <out>
//       the samples of <in> through pnm_unpack_texel and pnm_image_row -> the image's tight rows
//   pnm_check pack <source> <width> <height> <in> <out>
//       tight image rows through pnm_pack_texel and pnm_image_row -> the file's samples
//   pnm_check half <out>
//       pnm_half_to_float_bits of every half 0..65535, little-endian uint32 each
//   pnm_check formats
//       the two format tables over their whole domain: "pack <format> <source> <kind it is written as, -1 without a source>" for every
//       format 0..191, and "unpack <kind> <format>" for every kind
#include "dxtex_pnm.h"

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

static void scale_table(uint32_t maxval, uint32_t (&table)[256]) { for (uint32_t i = 0; i < 256; ++i) table[i] = pnm_scale(i, maxval); }

static int p6(const char* out)
{
    std::vector<uint32_t> words;
    uint32_t table[256];
    for (uint32_t pass = 1; pass <= 256; ++pass)
    {
        const uint32_t maxval = pass <= 255 ? pass : 255;
        scale_table(maxval, table);
        for (uint32_t b = 0; b < 256; ++b)
            words.push_back(pnm_p6_texel(b | ((255u - b) << 8) | ((b ^ 0x5Au) << 16) | 0xAB000000u, pass == 255 ? nullptr : table));
    }
    return write_file(out, words.data(), words.size() * 4) ? 0 : 1;
}

static int unpack(char** a)
{
    const int kind = std::atoi(a[0]);
    const bool bigEndian = std::atoi(a[1]) != 0;
    const uint32_t maxval = uint32_t(std::atoi(a[2])), width = uint32_t(std::atoi(a[3])), height = uint32_t(std::atoi(a[4]));
    std::vector<uint8_t> in;
    if (kind < 0 || kind >= PNM_KINDS || !read_file(a[5], in)) return 1;
    const size_t B = pnm_file_bytes(kind), D = pnm_image_bytes(kind);
    if (in.size() < size_t(width) * height * B) return 1;
    uint32_t table[256];
    scale_table(maxval ? maxval : 1, table);
    std::vector<uint8_t> image(size_t(width) * height * D);
    const uint8_t* s = in.data();
    for (uint32_t y = 0; y < height; ++y)
    {
        uint8_t* d = image.data() + size_t(pnm_image_row(kind, y, height)) * width * D;
        for (uint32_t x = 0; x < width; ++x, s += B, d += D) pnm_unpack_texel(s, d, kind, bigEndian, (kind == PNM_P6 && maxval != 255) ? table : nullptr);
    }
    return write_file(a[6], image.data(), image.size()) ? 0 : 1;
}

static int pack(char** a)
{
    const int source = std::atoi(a[0]);
    const uint32_t width = uint32_t(std::atoi(a[1])), height = uint32_t(std::atoi(a[2]));
    std::vector<uint8_t> in;
    if (source < 0 || source >= PNM_SOURCES || !read_file(a[3], in)) return 1;
    const int kind = pnm_source_kind(source);
    const size_t S = pnm_source_bytes(source), B = pnm_file_bytes(kind);
    if (in.size() < size_t(width) * height * S) return 1;
    std::vector<uint8_t> file(size_t(width) * height * B);
    uint8_t* d = file.data();
    for (uint32_t y = 0; y < height; ++y)
    {
        const uint8_t* s = in.data() + size_t(pnm_image_row(kind, y, height)) * width * S;
        for (uint32_t x = 0; x < width; ++x, s += S, d += B) pnm_pack_texel(s, d, source);
    }
    return write_file(a[4], file.data(), file.size()) ? 0 : 1;
}

static int half(const char* out)
{
    std::vector<uint32_t> bits(65536);
    for (uint32_t h = 0; h < 65536; ++h) bits[h] = pnm_half_to_float_bits(h);
    return write_file(out, bits.data(), bits.size() * 4) ? 0 : 1;
}

static int formats()
{
    for (int f = 0; f < 192; ++f) { const int src = pnm_pack_source(f); std::printf("pack %d %d %d\n", f, src, src < 0 ? -1 : pnm_source_kind(src)); }
    for (int kind = 0; kind < PNM_KINDS; ++kind) std::printf("unpack %d %d\n", kind, pnm_unpack_format(kind));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "formats")) return formats();
    if (argc == 3 && !std::strcmp(argv[1], "p6")) return p6(argv[2]);
    if (argc == 9 && !std::strcmp(argv[1], "unpack")) return unpack(argv + 2);
    if (argc == 7 && !std::strcmp(argv[1], "pack")) return pack(argv + 2);
    if (argc == 3 && !std::strcmp(argv[1], "half")) return half(argv[2]);
    std::fprintf(stderr, "usage: pnm_check p6 <out> | unpack <kind> <big endian> <maxval> <w> <h> <in> <out> | pack <source> <w> <h> <in> <out> | half <out> | formats\n");
    return 2;
}
