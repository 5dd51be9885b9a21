// Host run of dxtex_nmap.h (ComputeNormalMap's per-texel arithmetic, the code the GPU's nmap_kernel runs) over LoadScanline rows, for
// tests/test_normalmap_cpu.py:
//   nmap_check <in.f32> <width> <height> <flags> <amplitude as fp32 bits, hex> <unorm 0|1> <out.f32>
// in.f32 holds height x width float4 (what LoadScanline produces); out.f32 receives the float4 rows ComputeNMap hands to StoreScanline.
// The neighbours come from nmap_edge, as in the kernel (wrap, or the edge texel under CNMAP_MIRROR_U / _V).
#include "dxtex_nmap.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dxtex;

int main(int argc, char** argv)
{
    if (argc != 8) { std::fprintf(stderr, "usage: nmap_check in.f32 width height flags amplitude-bits unorm out.f32\n"); return 2; }
    const uint32_t w = uint32_t(std::strtoul(argv[2], nullptr, 10)), h = uint32_t(std::strtoul(argv[3], nullptr, 10));
    const uint32_t flags = uint32_t(std::strtoul(argv[4], nullptr, 0));
    const float amplitude = nmap_float(uint32_t(std::strtoul(argv[5], nullptr, 16)));
    const bool unorm = std::atoi(argv[6]) != 0;
    if (!w || !h) { std::fprintf(stderr, "empty image\n"); return 2; }
    std::vector<float> src(size_t(w) * h * 4), out(size_t(w) * h * 4);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(src.data(), sizeof(float), src.size(), f) != src.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fclose(f);
    const auto height = [&](int64_t x, int64_t y)
    {
        const float* t = &src[(size_t(nmap_edge(y, h, (flags & NMAP_MIRROR_V) != 0)) * w + nmap_edge(x, w, (flags & NMAP_MIRROR_U) != 0)) * 4];
        return nmap_height(t[0], t[1], t[2], t[3], flags);
    };
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x)
        {
            float hv[3][3];
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) hv[r][c] = height(int64_t(x) + c - 1, int64_t(y) + r - 1);
            const NmapOut o = nmap_texel(hv, flags, amplitude, unorm);
            float* d = &out[(size_t(y) * w + x) * 4];
            d[0] = o.x; d[1] = o.y; d[2] = o.z; d[3] = o.w;
        }
    f = std::fopen(argv[7], "wb");
    if (!f || std::fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[7]); return 2; }
    std::fclose(f);
    return 0;
}
