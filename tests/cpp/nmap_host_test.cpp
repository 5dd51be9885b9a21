// ComputeNormalMap through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_normalmap_gpu.py:
//   - the array overload over a 3-item array (with mips) and a 4-slice volume equals one single-image call per image;
//   - the DeviceScratchImage overload equals the host overload;
//   - argument checks return the reference's HRESULTs and release the output.
// Prints "nmap host checks passed" on success.
#include "../../directxtex_amd/host/DirectXTexAMD.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace DirectXTexAMD;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static void fill(const Image& im, unsigned seed)
{
    srand(seed);
    for (size_t y = 0; y < im.height; ++y)
        for (size_t i = 0; i < im.rowPitch; ++i) im.pixels[y * im.rowPitch + i] = uint8_t(rand() & 0xFF);
}

static bool same(const ScratchImage& a, const ScratchImage& b)
{
    return a.GetPixelsSize() == b.GetPixelsSize() && std::memcmp(a.GetPixels(), b.GetPixels(), a.GetPixelsSize()) == 0;
}

static int check_array(Device& dev, const ScratchImage& src, CNMAP_FLAGS flags, float amp, DXGI_FORMAT fmt)
{
    ScratchImage out;
    CHECK(ComputeNormalMap(dev, src.GetImages(), src.GetImageCount(), src.GetMetadata(), flags, amp, fmt, out) == S_OK);
    CHECK(out.GetImageCount() == src.GetImageCount() && out.GetMetadata().format == fmt);
    for (size_t i = 0; i < src.GetImageCount(); ++i)
    {
        ScratchImage one;
        CHECK(ComputeNormalMap(dev, src.GetImages()[i], flags, amp, fmt, one) == S_OK);
        CHECK(std::memcmp(one.GetPixels(), out.GetImages()[i].pixels, out.GetImages()[i].slicePitch) == 0);
    }
    DeviceScratchImage dsrc, dout;
    CHECK(dsrc.Upload(dev, src) == S_OK);
    CHECK(ComputeNormalMap(dev, dsrc, flags, amp, fmt, dout) == S_OK);
    ScratchImage back;
    CHECK(dout.Download(back) == S_OK);
    CHECK(same(out, back));
    return 0;
}

int main()
{
    Device dev;
    CHECK(dev.Create(0) == S_OK);

    ScratchImage arr;
    CHECK(arr.Initialize2D(DXGI_FORMAT_R8G8B8A8_UNORM, 37, 21, 3, 0) == S_OK);
    for (size_t i = 0; i < arr.GetImageCount(); ++i) fill(arr.GetImages()[i], unsigned(10 + i));
    CHECK(check_array(dev, arr, CNMAP_CHANNEL_LUMINANCE | CNMAP_COMPUTE_OCCLUSION, 2.5f, DXGI_FORMAT_R8G8B8A8_UNORM) == 0);
    CHECK(check_array(dev, arr, CNMAP_CHANNEL_GREEN | CNMAP_MIRROR_U | CNMAP_INVERT_SIGN, 1.0f, DXGI_FORMAT_R16G16B16A16_SNORM) == 0);

    ScratchImage vol;
    CHECK(vol.Initialize3D(DXGI_FORMAT_R16G16B16A16_FLOAT, 19, 33, 4, 1) == S_OK);
    for (size_t i = 0; i < vol.GetImageCount(); ++i)
    {
        const Image& im = vol.GetImages()[i];
        srand(unsigned(50 + i));
        for (size_t y = 0; y < im.height; ++y)
        {
            uint16_t* row = reinterpret_cast<uint16_t*>(im.pixels + y * im.rowPitch);
            for (size_t k = 0; k < im.width * 4; ++k) row[k] = uint16_t(0x3000 + rand() % 0x0C00);      // halves in [0.125, 0.875)
        }
    }
    CHECK(vol.GetImageCount() == 4);
    CHECK(check_array(dev, vol, CNMAP_CHANNEL_RED | CNMAP_MIRROR, 3.7f, DXGI_FORMAT_R32G32B32A32_FLOAT) == 0);
    CHECK(check_array(dev, vol, CNMAP_CHANNEL_ALPHA, -2.0f, DXGI_FORMAT_R10G10B10A2_UNORM) == 0);

    // argument checks (DirectXTexNormalMaps.cpp:257-390): the output is released on failure
    const Image& img = *arr.GetImage(0, 0, 0);
    ScratchImage out;
    CHECK(ComputeNormalMap(dev, img, CNMAP_FLAGS(6), 1.0f, DXGI_FORMAT_R8G8B8A8_UNORM, out) == E_INVALIDARG);
    CHECK(ComputeNormalMap(dev, img, CNMAP_DEFAULT, 1.0f, DXGI_FORMAT_BC5_UNORM, out) == HRESULT_E_NOT_SUPPORTED);
    CHECK(ComputeNormalMap(dev, img, CNMAP_DEFAULT, 1.0f, DXGI_FORMAT_R8G8B8A8_TYPELESS, out) == HRESULT_E_NOT_SUPPORTED);
    CHECK(ComputeNormalMap(dev, img, CNMAP_DEFAULT, 1.0f, DXGI_FORMAT(0), out) == E_INVALIDARG);
    CHECK(ComputeNormalMap(dev, img, CNMAP_DEFAULT, 1.0f, DXGI_FORMAT_R8G8B8A8_UNORM, out) == S_OK);
    CHECK(ComputeNormalMap(dev, img, CNMAP_DEFAULT, 1.0f, DXGI_FORMAT_R8G8B8A8_UINT, out) == HRESULT_E_NOT_SUPPORTED);
    CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
    CHECK(ComputeNormalMap(dev, arr.GetImages(), arr.GetImageCount(), arr.GetMetadata(), CNMAP_FLAGS(7), 1.0f, DXGI_FORMAT_R8G8B8A8_UNORM, out) == E_INVALIDARG);
    std::printf("nmap host checks passed\n");
    return 0;
}
