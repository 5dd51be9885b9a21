// RotateColor (texconv's HDR colour rotation) through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for
// tests/test_rotate_host_gpu.py:
//   - the Image, array and DeviceScratchImage overloads on a 2-item, 3-mip R16G16B16A16_FLOAT texture equal the C ABI's dxtex_rotate_color
//     image by image, for an operation of each curve;
//   - argument checks return TransformImage's HRESULTs, E_INVALIDARG for a bad operation or paper-white level, and release the output;
//   - the resident form moves nothing between host and device: a pipeline around it is one upload and one download.
// Prints "rotate host checks passed" on success.
#include "../../directxtex_amd/host/DirectXTexAMD.h"
#include "../../include/dxtex_amd.h"

#include <cmath>
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

static int check_op(Device& dev, const ScratchImage& src, TEX_ROTATE_COLOR rotate, float nits)
{
    // the C ABI, image by image
    std::vector<std::vector<uint8_t>> want(src.GetImageCount());
    for (size_t i = 0; i < src.GetImageCount(); ++i)
    {
        const Image& im = src.GetImages()[i];
        want[i].assign(im.slicePitch, 0);
        const dxtex_image s = { im.width, im.height, int32_t(im.format), im.rowPitch, im.slicePitch, im.pixels };
        const dxtex_image d = { im.width, im.height, int32_t(im.format), im.rowPitch, im.slicePitch, want[i].data() };
        CHECK(dxtex_rotate_color(dev.Get(), &s, &d, uint32_t(rotate), nits) == DXTEX_S_OK);
        CHECK(std::memcmp(want[i].data(), im.pixels, im.slicePitch) != 0);          // the operation changed something
        ScratchImage one;
        CHECK(RotateColor(dev, im, rotate, nits, one) == S_OK);
        CHECK(one.GetImageCount() == 1 && one.GetImages()[0].slicePitch == im.slicePitch);
        CHECK(std::memcmp(one.GetPixels(), want[i].data(), im.slicePitch) == 0);
    }
    ScratchImage out;
    CHECK(RotateColor(dev, src.GetImages(), src.GetImageCount(), src.GetMetadata(), rotate, nits, out) == S_OK);
    CHECK(out.GetImageCount() == src.GetImageCount() && out.GetMetadata().format == src.GetMetadata().format);
    CHECK(out.GetMetadata().mipLevels == src.GetMetadata().mipLevels && out.GetMetadata().arraySize == src.GetMetadata().arraySize);
    for (size_t i = 0; i < src.GetImageCount(); ++i)
        CHECK(std::memcmp(out.GetImages()[i].pixels, want[i].data(), want[i].size()) == 0);

    // resident: one upload, the step, one download
    uint64_t up0 = 0, down0 = 0, up1 = 0, down1 = 0, up2 = 0, down2 = 0, up3 = 0, down3 = 0;
    GetTransferBytes(dev, up0, down0);
    DeviceScratchImage dsrc, dout;
    CHECK(dsrc.Upload(dev, src) == S_OK);
    GetTransferBytes(dev, up1, down1);
    CHECK(RotateColor(dev, dsrc, rotate, nits, dout) == S_OK);
    GetTransferBytes(dev, up2, down2);
    ScratchImage back;
    CHECK(dout.Download(back) == S_OK);
    GetTransferBytes(dev, up3, down3);
    CHECK(same(out, back));
    CHECK(up1 - up0 == src.GetPixelsSize() && down1 == down0);           // one upload of the texture
    CHECK(up2 == up1 && down2 == down1);                                 // the step itself transfers nothing
    CHECK(up3 == up2 && down3 - down2 == src.GetPixelsSize());           // one download
    return 0;
}

int main()
{
    Device dev;
    CHECK(dev.Create(0) == S_OK);

    ScratchImage tex;
    CHECK(tex.Initialize2D(DXGI_FORMAT_R16G16B16A16_FLOAT, 37, 21, 2, 3) == S_OK);
    CHECK(tex.GetImageCount() == 6);
    for (size_t i = 0; i < tex.GetImageCount(); ++i)
    {
        const Image& im = tex.GetImages()[i];
        srand(unsigned(70 + i));
        for (size_t y = 0; y < im.height; ++y)
        {
            uint16_t* row = reinterpret_cast<uint16_t*>(im.pixels + y * im.rowPitch);
            for (size_t k = 0; k < im.width * 4; ++k) row[k] = uint16_t(0x2C00 + rand() % 0x1000);      // halves in [0.0625, 1)
        }
    }
    CHECK(check_op(dev, tex, TEX_ROTATE_709_TO_2020, 200.f) == 0);
    CHECK(check_op(dev, tex, TEX_ROTATE_709_TO_HDR10, 200.f) == 0);
    CHECK(check_op(dev, tex, TEX_ROTATE_HDR10_TO_709, 80.f) == 0);
    CHECK(check_op(dev, tex, TEX_ROTATE_P3D65_TO_709, 200.f) == 0);

    // the paper-white level reaches the kernel: another level, another result, for the HDR10 operations only
    {
        ScratchImage a, b;
        CHECK(RotateColor(dev, tex.GetImages(), tex.GetImageCount(), tex.GetMetadata(), TEX_ROTATE_P3D65_TO_HDR10, 200.f, a) == S_OK);
        CHECK(RotateColor(dev, tex.GetImages(), tex.GetImageCount(), tex.GetMetadata(), TEX_ROTATE_P3D65_TO_HDR10, 400.f, b) == S_OK);
        CHECK(!same(a, b));
        CHECK(RotateColor(dev, tex.GetImages(), tex.GetImageCount(), tex.GetMetadata(), TEX_ROTATE_P3D65_TO_2020, 200.f, a) == S_OK);
        CHECK(RotateColor(dev, tex.GetImages(), tex.GetImageCount(), tex.GetMetadata(), TEX_ROTATE_P3D65_TO_2020, 400.f, b) == S_OK);
        CHECK(same(a, b));
    }

    // argument checks: the output is released on failure
    const Image& img = *tex.GetImage(0, 0, 0);
    const TEX_ROTATE_COLOR op = TEX_ROTATE_709_TO_HDR10;
    ScratchImage out;
    CHECK(RotateColor(dev, img, op, 200.f, out) == S_OK);
    Image bad = img; bad.format = DXGI_FORMAT_BC6H_UF16;
    CHECK(RotateColor(dev, bad, op, 200.f, out) == HRESULT_E_NOT_SUPPORTED);
    bad = img; bad.format = DXGI_FORMAT_R16G16B16A16_TYPELESS;
    CHECK(RotateColor(dev, bad, op, 200.f, out) == HRESULT_E_NOT_SUPPORTED);
    bad = img; bad.format = DXGI_FORMAT_NV12;
    CHECK(RotateColor(dev, bad, op, 200.f, out) == HRESULT_E_NOT_SUPPORTED);
    CHECK(RotateColor(dev, img, TEX_ROTATE_COLOR(0), 200.f, out) == E_INVALIDARG);
    CHECK(RotateColor(dev, img, TEX_ROTATE_COLOR(9), 200.f, out) == E_INVALIDARG);
    CHECK(RotateColor(dev, img, op, 0.f, out) == E_INVALIDARG);
    CHECK(RotateColor(dev, img, op, -1.f, out) == E_INVALIDARG);
    CHECK(RotateColor(dev, img, op, 10000.5f, out) == E_INVALIDARG);
    CHECK(RotateColor(dev, img, op, std::nanf(""), out) == E_INVALIDARG);
    CHECK(RotateColor(dev, img, op, 10000.f, out) == S_OK);
    bad = img; bad.pixels = nullptr;
    CHECK(RotateColor(dev, bad, op, 200.f, out) == E_POINTER);
    CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
    TexMetadata md = tex.GetMetadata();
    CHECK(RotateColor(dev, tex.GetImages(), 0, md, op, 200.f, out) == E_INVALIDARG);
    CHECK(RotateColor(dev, nullptr, 6, md, op, 200.f, out) == E_INVALIDARG);
    CHECK(RotateColor(dev, tex.GetImages(), tex.GetImageCount() - 1, md, op, 200.f, out) == E_FAIL);
    CHECK(RotateColor(dev, tex.GetImages(), tex.GetImageCount(), md, op, 20000.f, out) == E_INVALIDARG);
    md.format = DXGI_FORMAT_BC7_UNORM;
    CHECK(RotateColor(dev, tex.GetImages(), tex.GetImageCount(), md, op, 200.f, out) == HRESULT_E_NOT_SUPPORTED);
    md = tex.GetMetadata(); md.format = DXGI_FORMAT_R16G16B16A16_UNORM;          // same size, every image's format differs from the metadata's
    CHECK(RotateColor(dev, tex.GetImages(), tex.GetImageCount(), md, op, 200.f, out) == E_FAIL);
    CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
    md = tex.GetMetadata(); md.width = 38;
    CHECK(RotateColor(dev, tex.GetImages(), tex.GetImageCount(), md, op, 200.f, out) == E_FAIL);
    // resident: an image that is not on this device, a bad operation (the result is released)
    DeviceScratchImage none, dout;
    CHECK(RotateColor(dev, none, op, 200.f, dout) == E_INVALIDARG);
    DeviceScratchImage dsrc;
    CHECK(dsrc.Upload(dev, tex) == S_OK);
    CHECK(RotateColor(dev, dsrc, op, 200.f, dout) == S_OK && dout.GetImageCount() == 6);
    CHECK(RotateColor(dev, dsrc, TEX_ROTATE_COLOR(12), 200.f, dout) == E_INVALIDARG);
    std::printf("rotate host checks passed\n");
    return 0;
}
