// The dithered Convert through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_dither_gpu.py:
//   - ConvertEx with a status callback and small progress bands gives the bytes of the call without one, under ordered dithering (bands
//     of whole multiples of 4 rows) and under error diffusion (one band: the callback runs at 0 and at the end only);
//   - Convert of a volume passes each slice's index within its mip level: every image equals dxtex_convert_slice of it with that z;
//   - the DeviceScratchImage overload equals the host overload.
// Prints "dither host checks passed" on success.
#include "../../directxtex_amd/host/DirectXTexAMD.h"
#include "../../include/dxtex_amd.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace DirectXTexAMD;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static dxtex_image view(const Image& im)
{
    dxtex_image v;
    v.width = im.width; v.height = im.height; v.format = int32_t(im.format); v.rowPitch = im.rowPitch; v.slicePitch = im.slicePitch; v.pixels = im.pixels;
    return v;
}

static bool same(const ScratchImage& a, const ScratchImage& b)
{
    return a.GetPixelsSize() == b.GetPixelsSize() && std::memcmp(a.GetPixels(), b.GetPixels(), a.GetPixelsSize()) == 0;
}

static void fill(const Image& im, unsigned seed)
{
    srand(seed);
    for (size_t y = 0; y < im.height; ++y)
    {
        float* row = reinterpret_cast<float*>(im.pixels + y * im.rowPitch);
        for (size_t i = 0; i < im.width * 4; ++i) row[i] = float(rand() % 1200) / 1000.0f - 0.1f;
    }
}

int main()
{
    Device dev;
    CHECK(dev.Create(0) == S_OK);
    const TEX_FILTER_FLAGS modes[2] = { TEX_FILTER_DITHER, TEX_FILTER_DITHER_DIFFUSION };
    const DXGI_FORMAT dsts[2] = { DXGI_FORMAT_B5G6R5_UNORM, DXGI_FORMAT_R8G8B8A8_UNORM };

    // ---- ConvertEx bands
    ScratchImage src;
    CHECK(src.Initialize2D(DXGI_FORMAT_R32G32B32A32_FLOAT, 67, 45, 1, 1) == S_OK);
    fill(*src.GetImage(0, 0, 0), 7);
    for (TEX_FILTER_FLAGS mode : modes)
        for (DXGI_FORMAT dst : dsts)
        {
            ConvertOptions opt = { mode, 0.5f };
            ScratchImage whole, banded;
            dev.SetProgressBands(0, 0);
            CHECK(ConvertEx(dev, *src.GetImage(0, 0, 0), dst, opt, whole) == S_OK);
            dev.SetProgressBands(0, 67 * 5);          // 5 rows a band: rounded up to 8 under ordered dithering
            size_t calls = 0;
            CHECK(ConvertEx(dev, *src.GetImage(0, 0, 0), dst, opt, banded, [&](size_t, size_t) { ++calls; return true; }) == S_OK);
            CHECK(same(whole, banded));
            CHECK(mode == TEX_FILTER_DITHER_DIFFUSION ? calls == 2 : calls == 2 + (45 - 1) / 8);
            ScratchImage plain;
            CHECK(Convert(dev, *src.GetImage(0, 0, 0), dst, TEX_FILTER_DEFAULT, 0.5f, plain) == S_OK);
            CHECK(!same(whole, plain));           // the dither bits are not ignored
        }
    dev.SetProgressBands(0, 0);

    // ---- a volume with its mip chain: slice phase, host and device overloads
    ScratchImage vol;
    CHECK(vol.Initialize3D(DXGI_FORMAT_R32G32B32A32_FLOAT, 33, 21, 6, 0) == S_OK);
    for (size_t i = 0; i < vol.GetImageCount(); ++i) fill(vol.GetImages()[i], unsigned(100 + i));
    // slice 1 repeats slice 0, so that only the phase can tell them apart
    std::memcpy(vol.GetImage(0, 0, 1)->pixels, vol.GetImage(0, 0, 0)->pixels, vol.GetImage(0, 0, 0)->slicePitch);
    DeviceScratchImage dvol;
    CHECK(dvol.Upload(dev, vol) == S_OK);
    for (TEX_FILTER_FLAGS mode : modes)
        for (DXGI_FORMAT dst : dsts)
        {
            ScratchImage out;
            CHECK(Convert(dev, vol.GetImages(), vol.GetImageCount(), vol.GetMetadata(), dst, mode, 0.5f, out) == S_OK);
            const TexMetadata& md = vol.GetMetadata();
            size_t index = 0;
            for (size_t level = 0, depth = md.depth; level < md.mipLevels; ++level, depth = depth > 1 ? depth >> 1 : 1)
                for (size_t z = 0; z < depth; ++z, ++index)
                {
                    const Image& s = vol.GetImages()[index];
                    const Image& o = out.GetImages()[index];
                    std::vector<uint8_t> want(o.slicePitch);
                    dxtex_image sv = view(s), dv = view(o);
                    dv.pixels = want.data();
                    CHECK(dxtex_convert_slice(dev.Get(), &sv, &dv, uint32_t(mode), 0.5f, uint32_t(z)) == DXTEX_S_OK);
                    CHECK(std::memcmp(want.data(), o.pixels, o.slicePitch) == 0);
                }
            CHECK(index == out.GetImageCount());
            const Image* s0 = out.GetImage(0, 0, 0);
            const Image* s1 = out.GetImage(0, 0, 1);
            const bool equal01 = std::memcmp(s0->pixels, s1->pixels, s0->slicePitch) == 0;
            CHECK(mode == TEX_FILTER_DITHER ? !equal01 : equal01);      // ordered dithering reads z; diffusion does not

            DeviceScratchImage dout;
            CHECK(Convert(dev, dvol, dst, mode, 0.5f, dout) == S_OK);
            ScratchImage back;
            CHECK(dout.Download(back) == S_OK);
            CHECK(same(out, back));
        }
    std::printf("dither host checks passed\n");
    return 0;
}
