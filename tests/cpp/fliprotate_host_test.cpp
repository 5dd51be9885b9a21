// FlipRotate and the turned cross through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_fliprotate_host_gpu.py:
//   - the Image, array and DeviceScratchImage overloads on a 2-item, 3-mip R8G8B8A8_UNORM texture equal the C ABI's dxtex_flip_rotate
//     image by image, for a word of each route and a combined one;
//   - the metadata of a cube with three mips under ROTATE90, and a 6 x 4 x 3 volume under ROTATE270 | FLIP_VERTICAL, slice by slice;
//   - the reference's HRESULT order, and the result released on failure;
//   - the resident form moves nothing between host and device;
//   - AssembleCross(..., TEX_FR_ROTATE180) equals CROSS_V_CROSS's result except for the -Z cell, which is the face turned by 180 written
//     out texel by texel here; CubeFromCross(..., TEX_FR_ROTATE180) on it returns the six faces byte for byte.
// Prints "fliprotate host checks passed" on success.
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

static void fill(const ScratchImage& tex, unsigned seed)
{
    srand(seed);
    for (size_t i = 0; i < tex.GetPixelsSize(); ++i) tex.GetPixels()[i] = uint8_t(rand());
}

static bool turns(TEX_FR_FLAGS f) { return (uint32_t(f) & 1u) != 0; }

// the C ABI's result for one image, with tight pitch
static int abi(Device& dev, const Image& im, TEX_FR_FLAGS flags, std::vector<uint8_t>& out, size_t& w, size_t& h)
{
    w = turns(flags) ? im.height : im.width; h = turns(flags) ? im.width : im.height;
    const size_t texel = BitsPerPixel(im.format) / 8;
    out.assign(w * h * texel, 0);
    const dxtex_image s = { im.width, im.height, int32_t(im.format), im.rowPitch, im.slicePitch, im.pixels };
    const dxtex_image d = { w, h, int32_t(im.format), w * texel, w * h * texel, out.data() };
    CHECK(dxtex_flip_rotate(dev.Get(), &s, &d, uint32_t(flags)) == DXTEX_S_OK);
    return 0;
}

static bool image_is(const Image& im, const std::vector<uint8_t>& want, size_t w, size_t h)
{
    const size_t row = w * (BitsPerPixel(im.format) / 8);
    if (im.width != w || im.height != h || want.size() != row * h) return false;
    for (size_t y = 0; y < h; ++y)
        if (std::memcmp(im.pixels + y * im.rowPitch, want.data() + y * row, row) != 0) return false;
    return true;
}

static int check_flags(Device& dev, const ScratchImage& src, TEX_FR_FLAGS flags)
{
    const size_t n = src.GetImageCount();
    std::vector<std::vector<uint8_t>> want(n);
    std::vector<size_t> w(n), h(n);
    for (size_t i = 0; i < n; ++i)
    {
        const Image& im = src.GetImages()[i];
        CHECK(abi(dev, im, flags, want[i], w[i], h[i]) == 0);
        ScratchImage one;
        CHECK(FlipRotate(dev, im, flags, one) == S_OK);
        CHECK(one.GetImageCount() == 1 && one.GetMetadata().mipLevels == 1 && one.GetMetadata().arraySize == 1 && one.GetMetadata().format == im.format);
        CHECK(image_is(one.GetImages()[0], want[i], w[i], h[i]));
    }
    const TexMetadata& md = src.GetMetadata();
    ScratchImage out;
    CHECK(FlipRotate(dev, src.GetImages(), n, md, flags, out) == S_OK);
    const TexMetadata& od = out.GetMetadata();
    CHECK(out.GetImageCount() == n && od.format == md.format && od.mipLevels == md.mipLevels && od.arraySize == md.arraySize && od.depth == md.depth);
    CHECK(od.dimension == md.dimension && od.miscFlags == md.miscFlags && od.miscFlags2 == md.miscFlags2);
    CHECK(od.width == (turns(flags) ? md.height : md.width) && od.height == (turns(flags) ? md.width : md.height));
    for (size_t i = 0; i < n; ++i) CHECK(image_is(out.GetImages()[i], want[i], w[i], h[i]));

    // resident: one upload, the step, one download
    uint64_t up0 = 0, down0 = 0, up1 = 0, down1 = 0, up2 = 0, down2 = 0, up3 = 0, down3 = 0;
    GetTransferBytes(dev, up0, down0);
    DeviceScratchImage dsrc, dout;
    CHECK(dsrc.Upload(dev, src) == S_OK);
    GetTransferBytes(dev, up1, down1);
    CHECK(FlipRotate(dev, dsrc, flags, dout) == S_OK);
    GetTransferBytes(dev, up2, down2);
    ScratchImage back;
    CHECK(dout.Download(back) == S_OK);
    GetTransferBytes(dev, up3, down3);
    CHECK(same(out, back));
    CHECK(up1 - up0 == src.GetPixelsSize() && down1 == down0);
    CHECK(up2 == up1 && down2 == down1);                                 // the step itself moves no byte between host and device
    CHECK(up3 == up2 && down3 - down2 == back.GetPixelsSize());
    return 0;
}

int main()
{
    Device dev;
    CHECK(dev.Create(0) == S_OK);

    ScratchImage tex;
    CHECK(tex.Initialize2D(DXGI_FORMAT_R8G8B8A8_UNORM, 37, 21, 2, 3) == S_OK);
    CHECK(tex.GetImageCount() == 6);
    fill(tex, 70);
    for (const TEX_FR_FLAGS f : { TEX_FR_FLIP_HORIZONTAL, TEX_FR_FLIP_VERTICAL, TEX_FR_ROTATE180, TEX_FR_ROTATE90, TEX_FR_ROTATE270 | TEX_FR_FLIP_HORIZONTAL })
        CHECK(check_flags(dev, tex, f) == 0);

    // a cube with three mips under ROTATE90: width and height exchanged, everything else kept
    {
        ScratchImage cube, out;
        CHECK(cube.InitializeCube(DXGI_FORMAT_R16G16B16A16_FLOAT, 12, 8, 1, 3) == S_OK);
        fill(cube, 71);
        TexMetadata md = cube.GetMetadata();
        md.SetAlphaMode(TEX_ALPHA_MODE_PREMULTIPLIED);
        CHECK(FlipRotate(dev, cube.GetImages(), cube.GetImageCount(), md, TEX_FR_ROTATE90, out) == S_OK);
        const TexMetadata& od = out.GetMetadata();
        CHECK(od.width == 8 && od.height == 12 && od.depth == 1 && od.arraySize == 6 && od.mipLevels == 3 && od.format == md.format);
        CHECK(od.IsCubemap() && od.dimension == TEX_DIMENSION_TEXTURE2D && od.GetAlphaMode() == TEX_ALPHA_MODE_PREMULTIPLIED && out.GetImageCount() == 18);
        CHECK(out.GetImage(2, 5, 0)->width == 2 && out.GetImage(2, 5, 0)->height == 3);
        CHECK(check_flags(dev, cube, TEX_FR_ROTATE90) == 0);
    }
    // a 6 x 4 x 3 volume under ROTATE270 | FLIP_VERTICAL: every depth slice of every mip
    {
        ScratchImage vol, out;
        CHECK(vol.Initialize3D(DXGI_FORMAT_R32G32B32_FLOAT, 6, 4, 3, 2) == S_OK);
        fill(vol, 72);
        CHECK(vol.GetImageCount() == 4);
        CHECK(check_flags(dev, vol, TEX_FR_ROTATE270 | TEX_FR_FLIP_VERTICAL) == 0);
        CHECK(FlipRotate(dev, vol.GetImages(), vol.GetImageCount(), vol.GetMetadata(), TEX_FR_ROTATE270 | TEX_FR_FLIP_VERTICAL, out) == S_OK);
        CHECK(out.GetMetadata().width == 4 && out.GetMetadata().height == 6 && out.GetMetadata().depth == 3 && out.GetMetadata().mipLevels == 2);
        CHECK(out.GetMetadata().dimension == TEX_DIMENSION_TEXTURE3D);
    }

    // the reference's checks, in its order (:191-203, :290-297, :335-381); the output is released on failure
    {
        const Image& img = *tex.GetImage(0, 0, 0);
        ScratchImage out;
        CHECK(FlipRotate(dev, img, TEX_FR_ROTATE90, out) == S_OK && out.GetImageCount() == 1);
        Image bad = img; bad.pixels = nullptr;
        CHECK(FlipRotate(dev, bad, TEX_FR_FLAGS(0), out) == E_POINTER);                   // null pixels before the flags
        bad = img; bad.format = DXGI_FORMAT_BC1_UNORM;
        CHECK(FlipRotate(dev, bad, TEX_FR_FLAGS(0), out) == E_INVALIDARG);                // the flags before the format
        CHECK(FlipRotate(dev, img, TEX_FR_FLAGS(4), out) == E_INVALIDARG);
        CHECK(FlipRotate(dev, img, TEX_FR_FLAGS(0x20), out) == E_INVALIDARG);
        CHECK(FlipRotate(dev, bad, TEX_FR_ROTATE90, out) == HRESULT_E_NOT_SUPPORTED);
        bad = img; bad.format = DXGI_FORMAT_YUY2;
        CHECK(FlipRotate(dev, bad, TEX_FR_ROTATE90, out) == HRESULT_E_NOT_SUPPORTED);     // refused here, converted by the reference
        CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
        bad = img; bad.format = DXGI_FORMAT_R8G8B8A8_TYPELESS;
        CHECK(FlipRotate(dev, bad, TEX_FR_FLIP_VERTICAL, out) == HRESULT_E_NOT_SUPPORTED);
        CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);

        TexMetadata md = tex.GetMetadata();
        CHECK(FlipRotate(dev, tex.GetImages(), 0, md, TEX_FR_ROTATE90, out) == E_INVALIDARG);
        CHECK(FlipRotate(dev, nullptr, 6, md, TEX_FR_ROTATE90, out) == E_INVALIDARG);
        md.format = DXGI_FORMAT_BC7_UNORM;
        CHECK(FlipRotate(dev, tex.GetImages(), 0, md, TEX_FR_ROTATE90, out) == E_INVALIDARG);          // no images before the format
        CHECK(FlipRotate(dev, tex.GetImages(), 6, md, TEX_FR_FLAGS(0), out) == HRESULT_E_NOT_SUPPORTED); // the format before the flags, as the reference's array form
        md = tex.GetMetadata();
        CHECK(FlipRotate(dev, tex.GetImages(), 6, md, TEX_FR_FLAGS(0x1F), out) == E_INVALIDARG);
        CHECK(FlipRotate(dev, tex.GetImages(), 5, md, TEX_FR_ROTATE90, out) == E_FAIL);                  // image count
        md.format = DXGI_FORMAT_B8G8R8A8_UNORM;
        CHECK(FlipRotate(dev, tex.GetImages(), 6, md, TEX_FR_ROTATE90, out) == E_FAIL);                  // every image's format differs from the metadata's
        md = tex.GetMetadata(); md.width = 38;
        CHECK(FlipRotate(dev, tex.GetImages(), 6, md, TEX_FR_ROTATE90, out) == E_FAIL);
        CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
        md = tex.GetMetadata(); md.mipLevels = 9;                                                        // what Initialize refuses is refused
        CHECK(FAILED(FlipRotate(dev, tex.GetImages(), 6, md, TEX_FR_ROTATE90, out)));
        CHECK(out.GetImageCount() == 0);

        DeviceScratchImage none, dout, dsrc;
        CHECK(FlipRotate(dev, none, TEX_FR_ROTATE90, dout) == E_INVALIDARG);
        CHECK(dsrc.Upload(dev, tex) == S_OK);
        CHECK(FlipRotate(dev, dsrc, TEX_FR_ROTATE90, dout) == S_OK && dout.GetImageCount() == 6);
        CHECK(FlipRotate(dev, dsrc, TEX_FR_FLAGS(4), dout) == E_INVALIDARG);
        CHECK(dsrc.OverrideFormat(DXGI_FORMAT_R8G8B8A8_TYPELESS));
        CHECK(FlipRotate(dev, dsrc, TEX_FR_ROTATE90, dout) == HRESULT_E_NOT_SUPPORTED);
        CHECK(dout.GetImageCount() == 0 && dout.GetPixels() == nullptr);                                 // released on failure
    }

    // the cross with a turned -Z face
    {
        const size_t w = 10, h = 6, texel = 4;
        ScratchImage faces;
        CHECK(faces.InitializeCube(DXGI_FORMAT_R8G8B8A8_UNORM, w, h, 1, 1) == S_OK);
        fill(faces, 73);
        DeviceScratchImage dfaces, plain, turned, cube;
        CHECK(dfaces.Upload(dev, faces) == S_OK);
        CHECK(AssembleCross(dev, CROSS_V_CROSS, dfaces, plain) == S_OK);
        uint64_t up0 = 0, down0 = 0, up1 = 0, down1 = 0;
        GetTransferBytes(dev, up0, down0);
        CHECK(AssembleCross(dev, CROSS_V_CROSS, dfaces, TEX_FR_ROTATE180, turned) == S_OK);
        CHECK(CubeFromCross(dev, CROSS_V_CROSS, turned, TEX_FR_ROTATE180, cube) == S_OK);
        GetTransferBytes(dev, up1, down1);
        CHECK(up1 == up0 && down1 == down0);
        ScratchImage a, b, c;
        CHECK(plain.Download(a) == S_OK && turned.Download(b) == S_OK && cube.Download(c) == S_OK);
        const CrossLayout* lay = GetCrossLayout(CROSS_V_CROSS);
        CHECK(a.GetMetadata().width == 3 * w && a.GetMetadata().height == 4 * h && b.GetMetadata().width == 3 * w && b.GetMetadata().height == 4 * h);
        const Image& ia = *a.GetImage(0, 0, 0);
        const Image& ib = *b.GetImage(0, 0, 0);
        const Image& nz = *faces.GetImage(0, 5, 0);
        const size_t cx = lay->x[5] * w, cy = lay->y[5] * h;
        for (size_t y = 0; y < ia.height; ++y)
            for (size_t x = 0; x < ia.width; ++x)
            {
                const bool cell = x >= cx && x < cx + w && y >= cy && y < cy + h;
                const uint8_t* want = cell ? nz.pixels + (h - 1 - (y - cy)) * nz.rowPitch + (w - 1 - (x - cx)) * texel : ia.pixels + y * ia.rowPitch + x * texel;
                CHECK(std::memcmp(ib.pixels + y * ib.rowPitch + x * texel, want, texel) == 0);
            }
        CHECK(c.GetMetadata().IsCubemap() && c.GetMetadata().arraySize == 6 && c.GetMetadata().width == w && c.GetMetadata().height == h);
        CHECK(same(c, faces));
        // flags that would exchange the face's width and height, and illegal ones; the plain forms are as they were
        CHECK(AssembleCross(dev, CROSS_V_CROSS, dfaces, TEX_FR_ROTATE90, turned) == E_INVALIDARG);
        CHECK(AssembleCross(dev, CROSS_V_CROSS, dfaces, TEX_FR_FLAGS(0), turned) == E_INVALIDARG);
        CHECK(CubeFromCross(dev, CROSS_V_CROSS, plain, TEX_FR_ROTATE270 | TEX_FR_FLIP_VERTICAL, cube) == E_INVALIDARG);
        CHECK(CubeFromCross(dev, CROSS_V_CROSS, plain, TEX_FR_FLAGS(4), cube) == E_INVALIDARG);
        CHECK(CubeFromCross(dev, CROSS_V_CROSS, plain, cube) == S_OK && cube.Download(c) == S_OK && same(c, faces));
        // another word that keeps the size, on the horizontal cross
        CHECK(AssembleCross(dev, CROSS_H_CROSS, dfaces, TEX_FR_FLIP_VERTICAL, turned) == S_OK);
        CHECK(CubeFromCross(dev, CROSS_H_CROSS, turned, TEX_FR_FLIP_VERTICAL, cube) == S_OK && cube.Download(c) == S_OK && same(c, faces));
    }
    std::printf("fliprotate host checks passed\n");
    return 0;
}
