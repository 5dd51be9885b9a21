// The console formats through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_xbox_formats_host_gpu.py:
//   - IsSupportedOnDevice names the four, under their XBOX_DXGI_FORMAT_* enumerators;
//   - Convert into XBOX_DXGI_FORMAT_R10G10B10_7E3_A2_FLOAT through DeviceScratchImage equals the host-memory overload, which equals
//     dxtex_convert of the C ABI; the same for a 2-level array into the other three, and back to R32G32B32A32_FLOAT.
// Prints "xbox host checks passed" on success.
#include "../../directxtex_amd/host/DirectXTexAMD.h"
#include "../../include/dxtex_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace DirectXTexAMD;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool same(const ScratchImage& a, const ScratchImage& b)
{
    return a.GetPixelsSize() == b.GetPixelsSize() && std::memcmp(a.GetPixels(), b.GetPixels(), a.GetPixelsSize()) == 0;
}

int main()
{
    static_assert(XBOX_DXGI_FORMAT_R10G10B10_7E3_A2_FLOAT == 116 && XBOX_DXGI_FORMAT_R10G10B10_6E4_A2_FLOAT == 117, "numbering");
    static_assert(XBOX_DXGI_FORMAT_R10G10B10_SNORM_A2_UNORM == 189 && XBOX_DXGI_FORMAT_R4G4_UNORM == 190, "numbering");
    const DXGI_FORMAT four[4] = { XBOX_DXGI_FORMAT_R10G10B10_7E3_A2_FLOAT, XBOX_DXGI_FORMAT_R10G10B10_6E4_A2_FLOAT, XBOX_DXGI_FORMAT_R10G10B10_SNORM_A2_UNORM,
                                  XBOX_DXGI_FORMAT_R4G4_UNORM };
    for (DXGI_FORMAT f : four) CHECK(IsSupportedOnDevice(f));
    CHECK(BitsPerPixel(four[0]) == 32 && BitsPerPixel(four[1]) == 32 && BitsPerPixel(four[2]) == 32 && BitsPerPixel(four[3]) == 8);

    Device dev;
    CHECK(dev.Create(0) == S_OK);
    ScratchImage src;
    CHECK(src.Initialize2D(DXGI_FORMAT_R32G32B32A32_FLOAT, 37, 23, 2, 2) == S_OK);
    srand(116);
    for (size_t i = 0; i < src.GetImageCount(); ++i)
    {
        const Image& im = src.GetImages()[i];
        for (size_t y = 0; y < im.height; ++y)
        {
            float* row = reinterpret_cast<float*>(im.pixels + y * im.rowPitch);
            for (size_t k = 0; k < im.width * 4; ++k) row[k] = float(rand() % 4000) / 1000.0f - 1.5f;
        }
    }
    DeviceScratchImage dsrc;
    CHECK(dsrc.Upload(dev, src) == S_OK);
    for (DXGI_FORMAT f : four)
    {
        ScratchImage host;
        CHECK(Convert(dev, src.GetImages(), src.GetImageCount(), src.GetMetadata(), f, TEX_FILTER_DEFAULT, 0.5f, host) == S_OK);
        CHECK(host.GetMetadata().format == f && host.GetImageCount() == src.GetImageCount());
        for (size_t i = 0; i < src.GetImageCount(); ++i)
        {
            const Image& s = src.GetImages()[i];
            const Image& o = host.GetImages()[i];
            std::vector<uint8_t> want(o.slicePitch);
            dxtex_image sv = { s.width, s.height, int32_t(s.format), s.rowPitch, s.slicePitch, s.pixels };
            dxtex_image dv = { o.width, o.height, int32_t(o.format), o.rowPitch, o.slicePitch, want.data() };
            CHECK(dxtex_convert(dev.Get(), &sv, &dv, 0, 0.5f) == DXTEX_S_OK);
            CHECK(std::memcmp(want.data(), o.pixels, o.slicePitch) == 0);
        }
        DeviceScratchImage dout;
        CHECK(Convert(dev, dsrc, f, TEX_FILTER_DEFAULT, 0.5f, dout) == S_OK);
        ScratchImage back;
        CHECK(dout.Download(back) == S_OK);
        CHECK(same(host, back));
        // and back: device-resident source of the format
        DeviceScratchImage dfloat;
        CHECK(Convert(dev, dout, DXGI_FORMAT_R32G32B32A32_FLOAT, TEX_FILTER_DEFAULT, 0.5f, dfloat) == S_OK);
        ScratchImage f1, f2;
        CHECK(dfloat.Download(f1) == S_OK);
        CHECK(Convert(dev, host.GetImages(), host.GetImageCount(), host.GetMetadata(), DXGI_FORMAT_R32G32B32A32_FLOAT, TEX_FILTER_DEFAULT, 0.5f, f2) == S_OK);
        CHECK(same(f1, f2));
    }
    std::printf("xbox host checks passed\n");
    return 0;
}
