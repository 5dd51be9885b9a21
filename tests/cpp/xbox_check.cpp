// Host sweep of the 10-bit float pack / unpack helpers behind R10G10B10_7E3_A2_FLOAT (116) and R10G10B10_6E4_A2_FLOAT (117)
// (dxtex_device.h: float_from_7e3 / float_from_6e4 / unpack_small10_a2; dxtex_store.h: float_to_7e3 / float_to_6e4 / pack_small10_a2)
// against the reference's own LoadScanline / StoreScanline, for tests/test_xbox_formats_cpu.py:
//   xbox_check <libdxtex_ref.so> load                     every 10-bit code in every colour field with every alpha code, both formats
//   xbox_check <libdxtex_ref.so> store <texels.f32>       the file's R32G32B32A32_FLOAT texels packed into both formats
// Prints "texels <n> mismatches <m>" per format and returns 1 if any m is not 0. The reference library is opened at run time, so that
// the program builds where the reference is absent.
#include "dxtex_store.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <vector>

using namespace dxtex;

typedef int (*LoadFn)(const uint8_t* src, size_t size, int fmt, float* rgba, size_t count);
typedef int (*StoreFn)(uint8_t* dst, size_t size, int fmt, const float* rgba, size_t count, float threshold);

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: xbox_check libdxtex_ref.so load | store texels.f32\n"); return 2; }
    void* lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) { std::fprintf(stderr, "cannot open %s: %s\n", argv[1], dlerror()); return 2; }
    const LoadFn refLoad = LoadFn(dlsym(lib, "dxtex_ref_load_scanline"));
    const StoreFn refStore = StoreFn(dlsym(lib, "dxtex_ref_store_scanline"));
    if (!refLoad || !refStore) { std::fprintf(stderr, "%s lacks the scanline entry points\n", argv[1]); return 2; }
    const int formats[2] = { FMT_R10G10B10_7E3_A2_FLOAT, FMT_R10G10B10_6E4_A2_FLOAT };
    const int mbits[2] = { 7, 6 };
    bool bad = false;

    if (!std::strcmp(argv[2], "load"))
    {
        // texel i of pass p holds code i in field p and other codes in the other two; alpha runs through its four codes
        std::vector<uint32_t> src;
        for (uint32_t p = 0; p < 3; ++p)
            for (uint32_t i = 0; i < 1024; ++i)
                for (uint32_t a = 0; a < 4; ++a)
                {
                    const uint32_t f[3] = { i, (7u * i + 1u) & 1023u, 1023u - i };
                    src.push_back(f[p % 3] | (f[(p + 1) % 3] << 10) | (f[(p + 2) % 3] << 20) | (a << 30));
                }
        std::vector<float> want(src.size() * 4);
        for (int k = 0; k < 2; ++k)
        {
            if (refLoad(reinterpret_cast<const uint8_t*>(src.data()), src.size() * 4, formats[k], want.data(), src.size()) != 0) { std::fprintf(stderr, "reference load failed\n"); return 2; }
            size_t mismatches = 0;
            for (size_t i = 0; i < src.size(); ++i)
            {
                float got[4];
                unpack_small10_a2(src[i], mbits[k], got[0], got[1], got[2], got[3]);
                const float one[3] = { k ? float_from_6e4(src[i] & 0x3FFu) : float_from_7e3(src[i] & 0x3FFu), got[1], got[2] };
                if (std::memcmp(got, &want[i * 4], 16) != 0 || std::memcmp(&one[0], &want[i * 4], 4) != 0)
                {
                    if (mismatches++ < 8) std::fprintf(stderr, "format %d code %08x: got %a %a %a %a want %a %a %a %a\n", formats[k], src[i], got[0], got[1], got[2], got[3],
                                                       want[i * 4], want[i * 4 + 1], want[i * 4 + 2], want[i * 4 + 3]);
                }
            }
            std::printf("format %d texels %zu mismatches %zu\n", formats[k], src.size(), mismatches);
            bad = bad || mismatches != 0;
        }
    }
    else if (!std::strcmp(argv[2], "store") && argc == 4)
    {
        FILE* f = std::fopen(argv[3], "rb");
        if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
        std::fseek(f, 0, SEEK_END);
        const size_t n = size_t(std::ftell(f)) / 16;
        std::fseek(f, 0, SEEK_SET);
        std::vector<float> texels(n * 4);
        if (!n || std::fread(texels.data(), 16, n, f) != n) { std::fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
        std::fclose(f);
        std::vector<uint32_t> want(n);
        for (int k = 0; k < 2; ++k)
        {
            if (refStore(reinterpret_cast<uint8_t*>(want.data()), n * 4, formats[k], texels.data(), n, 0.0f) != 0) { std::fprintf(stderr, "reference store failed\n"); return 2; }
            size_t mismatches = 0;
            for (size_t i = 0; i < n; ++i)
            {
                const float* t = &texels[i * 4];
                const uint32_t got = pack_small10_a2(t[0], t[1], t[2], t[3], mbits[k]);
                if (got != want[i] && mismatches++ < 8)
                    std::fprintf(stderr, "format %d texel %zu (%a %a %a %a): got %08x want %08x\n", formats[k], i, t[0], t[1], t[2], t[3], got, want[i]);
            }
            std::printf("format %d texels %zu mismatches %zu\n", formats[k], n, mismatches);
            bad = bad || mismatches != 0;
        }
    }
    else { std::fprintf(stderr, "unknown mode %s\n", argv[2]); return 2; }
    return bad ? 1 : 0;
}
