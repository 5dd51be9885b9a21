// TransformImage with texconv's per-texel ops through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for
// tests/test_transform_gpu.py:
//   - for the ops that read one texel, the array overload over a 3-item array (with mips) and a 4-slice volume equals one single-image call
//     per image;
//   - the DeviceScratchImage overload equals the host array overload, the tone map (a maximum over the whole set) included;
//   - argument checks return the reference's HRESULTs and release the output.
// Prints "transform host checks passed" on success.
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

static TexTransform op(TEX_TRANSFORM_OP o, uint32_t key = 0)
{
    TexTransform t;
    t.op = o; t.colorKey = key;
    return t;
}

static int check_array(Device& dev, const ScratchImage& src, const TexTransform& t, bool perImage)
{
    ScratchImage out;
    CHECK(TransformImage(dev, src.GetImages(), src.GetImageCount(), src.GetMetadata(), t, out) == S_OK);
    CHECK(out.GetImageCount() == src.GetImageCount() && out.GetMetadata().format == src.GetMetadata().format);
    for (size_t i = 0; perImage && i < src.GetImageCount(); ++i)
    {
        ScratchImage one;
        CHECK(TransformImage(dev, src.GetImages()[i], t, one) == S_OK);
        CHECK(std::memcmp(one.GetPixels(), out.GetImages()[i].pixels, out.GetImages()[i].slicePitch) == 0);
    }
    DeviceScratchImage dsrc, dout;
    CHECK(dsrc.Upload(dev, src) == S_OK);
    CHECK(TransformImage(dev, dsrc, t, dout) == S_OK);
    ScratchImage back;
    CHECK(dout.Download(back) == S_OK);
    CHECK(same(out, back));
    return 0;
}

int main()
{
    Device dev;
    CHECK(dev.Create(0) == S_OK);

    TexTransform swz;
    CHECK(ParseSwizzleMask("bgr1", swz));
    ScratchImage arr;
    CHECK(arr.Initialize2D(DXGI_FORMAT_R8G8B8A8_UNORM, 37, 21, 3, 0) == S_OK);
    for (size_t i = 0; i < arr.GetImageCount(); ++i) fill(arr.GetImages()[i], unsigned(10 + i));
    CHECK(check_array(dev, arr, swz, true) == 0);
    CHECK(check_array(dev, arr, op(TEX_TRANSFORM_COLOR_KEY, 0x80FF20), true) == 0);
    CHECK(check_array(dev, arr, op(TEX_TRANSFORM_INVERT_Y), true) == 0);
    CHECK(check_array(dev, arr, op(TEX_TRANSFORM_RECONSTRUCT_Z), true) == 0);
    CHECK(check_array(dev, arr, op(TEX_TRANSFORM_TONEMAP), false) == 0);

    ScratchImage vol;
    CHECK(vol.Initialize3D(DXGI_FORMAT_R16G16B16A16_FLOAT, 19, 33, 4, 1) == S_OK);
    for (size_t i = 0; i < vol.GetImageCount(); ++i)
    {
        const Image& im = vol.GetImages()[i];
        srand(unsigned(50 + i));
        for (size_t y = 0; y < im.height; ++y)
        {
            uint16_t* row = reinterpret_cast<uint16_t*>(im.pixels + y * im.rowPitch);
            for (size_t k = 0; k < im.width * 4; ++k) row[k] = uint16_t(0x3000 + rand() % 0x1800);      // halves in [0.125, 3.5)
        }
    }
    CHECK(vol.GetImageCount() == 4);
    CHECK(check_array(dev, vol, op(TEX_TRANSFORM_RECONSTRUCT_Z), true) == 0);
    CHECK(check_array(dev, vol, swz, true) == 0);
    CHECK(check_array(dev, vol, op(TEX_TRANSFORM_TONEMAP), false) == 0);

    // the tone map of the set differs from the per-image one where an image does not hold the maximum
    {
        ScratchImage all, first;
        CHECK(TransformImage(dev, vol.GetImages(), vol.GetImageCount(), vol.GetMetadata(), op(TEX_TRANSFORM_TONEMAP), all) == S_OK);
        bool differs = false;
        for (size_t i = 0; i < vol.GetImageCount(); ++i)
        {
            CHECK(TransformImage(dev, vol.GetImages()[i], op(TEX_TRANSFORM_TONEMAP), first) == S_OK);
            differs |= std::memcmp(first.GetPixels(), all.GetImages()[i].pixels, all.GetImages()[i].slicePitch) != 0;
        }
        CHECK(differs);
    }

    // argument checks (DirectXTexMisc.cpp:606-700): the output is released on failure
    const Image& img = *arr.GetImage(0, 0, 0);
    ScratchImage out;
    CHECK(TransformImage(dev, img, swz, out) == S_OK);
    Image bad = img; bad.format = DXGI_FORMAT_BC1_UNORM;
    CHECK(TransformImage(dev, bad, swz, out) == HRESULT_E_NOT_SUPPORTED);          // refused before the result is touched, as there
    bad = img; bad.format = DXGI_FORMAT_R8G8B8A8_TYPELESS;
    CHECK(TransformImage(dev, bad, swz, out) == HRESULT_E_NOT_SUPPORTED);
    bad = img; bad.pixels = nullptr;
    CHECK(TransformImage(dev, img, swz, out) == S_OK);
    CHECK(TransformImage(dev, bad, swz, out) == E_POINTER);
    CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
    TexTransform wild = swz; wild.swizzle[2] = 4;
    CHECK(TransformImage(dev, img, wild, out) == E_INVALIDARG);
    TexMetadata md = arr.GetMetadata();
    CHECK(TransformImage(dev, arr.GetImages(), 0, md, swz, out) == E_INVALIDARG);
    CHECK(TransformImage(dev, arr.GetImages(), arr.GetImageCount() - 1, md, swz, out) == E_FAIL);
    md.format = DXGI_FORMAT_BC7_UNORM;
    CHECK(TransformImage(dev, arr.GetImages(), arr.GetImageCount(), md, swz, out) == HRESULT_E_NOT_SUPPORTED);
    md = arr.GetMetadata(); md.format = DXGI_FORMAT_B8G8R8A8_UNORM;            // same size, every image's format differs from the metadata's
    CHECK(TransformImage(dev, arr.GetImages(), arr.GetImageCount(), md, swz, out) == E_FAIL);
    CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
    md = arr.GetMetadata(); md.width = 38;
    CHECK(TransformImage(dev, arr.GetImages(), arr.GetImageCount(), md, swz, out) == E_FAIL);

    // ParseSwizzleMask: texconv's rules
    TexTransform p;
    CHECK(!ParseSwizzleMask("", p) && !ParseSwizzleMask("rgbar", p) && !ParseSwizzleMask("rgq", p) && !ParseSwizzleMask(nullptr, p));
    CHECK(ParseSwizzleMask("rgba", p) && IsIdentitySwizzle(p));
    CHECK(ParseSwizzleMask("w0", p) && p.swizzle[0] == 3 && p.zero[1] && p.zero[2] && p.zero[3] && !IsIdentitySwizzle(p));
    std::printf("transform host checks passed\n");
    return 0;
}
