// Host build of csrc/dxtex_dds.h for tests/test_dds_texel_cpu.py: the per-texel rules the GPU kernels (dds.hip) and the host codec share,
// run here over one row of file texels the way a lane runs them.
//
//   dds_check rows <list>
//       one row per line: "<texels file> <op> <format> <opaque> <palette file or -> <out file>". op = a DdsRowOp, format = the result's
//       DXGI_FORMAT, the palette file holds 256 words. Writes the row's image bytes: whole texels only. Prints "ok" per row, or "refused"
//       where dds_target() refuses the pair (nothing is written then).
#include "dxtex_dds.h"

#include <cstdio>
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

static int rows(const char* list)
{
    std::ifstream in(list);
    for (std::string line; std::getline(in, line);)
    {
        if (line.empty()) continue;
        std::istringstream ss(line);
        std::string texelsPath, palettePath, outPath;
        int op, format, opaque;
        if (!(ss >> texelsPath >> op >> format >> opaque >> palettePath >> outPath)) return 2;
        std::vector<uint8_t> texels, pal, out;
        if (!read_file(texelsPath, texels)) return 3;
        uint32_t palette[256] = {};
        if (dds_has_palette(op)) { if (!read_file(palettePath, pal) || pal.size() != sizeof(palette)) return 3; std::memcpy(palette, pal.data(), sizeof(palette)); }
        const int target = dds_target(op, format);
        if (target < 0) { std::printf("refused\n"); continue; }
        if (op == ROW_COPY || target == DDS_TO_BYTES)
        {
            // the forced alpha on the last word of every whole texel; a format without one passes its bytes
            const DdsOpaque o = (op == ROW_COPY && opaque) ? dds_opaque_of(format) : DdsOpaque{ 0u, 0xffffffffu, 0u };
            out = texels;
            if (o.texelBytes)
            {
                const size_t T = o.texelBytes, W = T < 4 ? T : 4;
                out.resize(texels.size() / T * T);
                for (size_t i = 0; i + T <= out.size(); i += T) le_store64(out.data() + i + T - W, dds_opaque_word(le_load32(texels.data() + i + T - W, uint32_t(W)), o), uint32_t(W));
            }
        }
        else
        {
            const size_t B = dds_file_bytes(op), D = dds_image_bytes(target), n = texels.size() / B;
            out.resize(n * D);
            for (size_t x = 0; x < n; ++x) le_store64(out.data() + x * D, dds_unpack_texel(le_load32(texels.data() + x * B, uint32_t(B)), op, target, opaque != 0, palette), uint32_t(D));
        }
        if (!write_file(outPath, out)) return 4;
        std::printf("ok\n");
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "rows")) return rows(argv[2]);
    std::fprintf(stderr, "usage: dds_check rows <list>\n");
    return 2;
}
