// Host build of csrc/dxtex_tga.h for tests/test_tga_cpu.py: the per-texel rules the GPU kernels (tga.hip) and the host codec share, run
// here over whole images the way the kernels run them - the flips, the image's pitch, the two alpha ORs and the opaque pass.
//
//   tga_check unpack_many <list>
//       one image per line: "<texels file> <kind> <flags> <width> <height> <rowPitch> <palette file or -> <out file>". kind = a TgaKind,
//       flags = TgaFlags, the texels are in file order, the palette file holds 256 words. Writes rowPitch * height bytes (zero where no
//       texel lands) and prints the alpha answer, one line per image.
//   tga_check pack <row> <bytesPerTexel> <width> <height> <rowPitch> <pixels file> <out file>
//       row = a TgaRow; writes the width * height * bytesPerTexel bytes of the file's rows
//   tga_check formats
//       the two format tables over their whole domain: "pack <format> <bytes per texel> <row>" for every format 0..191, and "unpack <format>
//       <bytes per texel> <paletted> <kind>" for every format, bytes per texel 0..5 and both palette states
#include "dxtex_tga.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace dxtex;

static bool read_file(const std::string& path, std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END); const long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
    buf.resize(size_t(n > 0 ? n : 0));
    const bool ok = buf.empty() || std::fread(buf.data(), 1, buf.size(), f) == buf.size();
    std::fclose(f);
    return ok;
}

static bool write_file(const std::string& path, const std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = buf.empty() || std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    return (std::fclose(f) == 0) && ok;
}

static int unpack_many(const char* list)
{
    std::ifstream in(list);
    for (std::string line; std::getline(in, line);)
    {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string texelsPath, palettePath, outPath;
        int kind; unsigned flags; size_t width, height, pitch;
        if (!(ss >> texelsPath >> kind >> flags >> width >> height >> pitch >> palettePath >> outPath)) return 2;
        if (kind < 0 || kind >= TGA_KINDS) return 2;
        const uint32_t B = tga_file_bytes(kind), D = tga_image_bytes(kind);
        std::vector<uint8_t> texels, pal;
        if (!read_file(texelsPath, texels) || texels.size() != width * height * B || pitch < width * D) return 3;
        uint32_t palette[256] = {};
        if (kind == TGA_PALETTE) { if (!read_file(palettePath, pal) || pal.size() != sizeof(palette)) return 3; std::memcpy(palette, pal.data(), sizeof(palette)); }
        std::vector<uint8_t> out(pitch * height, 0);
        uint32_t orAlpha = 0, orNotAlpha = 0;
        for (size_t y = 0; y < height; ++y)
            for (size_t x = 0; x < width; ++x)
            {
                uint32_t alpha;
                const uint32_t t = tga_unpack_texel(le_load32(texels.data() + (y * width + x) * B, B), kind, palette, alpha);
                const size_t dy = (flags & TGA_TOP_DOWN) ? y : height - 1 - y, dx = (flags & TGA_RIGHT_TO_LEFT) ? width - 1 - x : x;
                le_store32(out.data() + dy * pitch + dx * D, t, D);
                orAlpha |= alpha; orNotAlpha |= alpha ^ 255u;
            }
        uint32_t answer = kind == TGA_RGB_RGBA ? 1u : 0u;
        if (tga_has_alpha_rule(kind))
        {
            bool makeOpaque;
            answer = tga_alpha_answer(orAlpha, orNotAlpha, (flags & TGA_ALLOW_ALL_ZERO_ALPHA) != 0, makeOpaque);
            if (makeOpaque)
                for (size_t y = 0; y < height; ++y)
                    for (size_t x = 0; x < width; ++x)
                    {
                        uint8_t& top = out[y * pitch + x * D + (D - 1)];
                        top = D == 2 ? uint8_t(top | 0x80) : uint8_t(0xFF);
                    }
        }
        if (!write_file(outPath, out)) return 4;
        std::printf("%u\n", answer);
    }
    return 0;
}

static int pack(char** a)
{
    const int row = std::atoi(a[0]);
    const uint32_t B = uint32_t(std::atoi(a[1])), D = row == TGA_ROW_DROP_X ? 4u : B;
    const size_t width = size_t(std::atoll(a[2])), height = size_t(std::atoll(a[3])), pitch = size_t(std::atoll(a[4]));
    std::vector<uint8_t> px;
    if (B < 1 || B > 4 || !read_file(a[5], px) || pitch < width * D || px.size() < pitch * (height - 1) + width * D) return 3;
    std::vector<uint8_t> out(width * height * B);
    for (size_t y = 0; y < height; ++y)
        for (size_t x = 0; x < width; ++x)
            le_store32(out.data() + (y * width + x) * B, tga_pack_texel(le_load32(px.data() + y * pitch + x * D, D), row), B);
    return write_file(a[6], out) ? 0 : 4;
}

static int formats()
{
    for (int f = 0; f < 192; ++f) { const TgaPackRow r = tga_pack_row(f); std::printf("pack %d %u %d\n", f, r.bytesPerTexel, r.row); }
    for (int f = 0; f < 192; ++f)
        for (uint32_t B = 0; B <= 5; ++B)
            for (int paletted = 0; paletted < 2; ++paletted) std::printf("unpack %d %u %d %d\n", f, B, paletted, tga_unpack_kind(f, B, paletted != 0));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "formats")) return formats();
    if (argc == 3 && !std::strcmp(argv[1], "unpack_many")) return unpack_many(argv[2]);
    if (argc == 9 && !std::strcmp(argv[1], "pack")) return pack(argv + 2);
    std::fprintf(stderr, "usage: tga_check unpack_many <list> | pack <row> <bytesPerTexel> <width> <height> <rowPitch> <pixels> <out> | formats\n");
    return 2;
}
