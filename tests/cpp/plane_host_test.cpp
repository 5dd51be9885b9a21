// ConvertToSinglePlane through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_single_plane_host_gpu.py:
//
//   plane_host_test convert FORMAT WIDTH HEIGHT ITEMS MIPS IN EXPECTED RGBA
//     IN holds a planar texture as ScratchImage lays it out, EXPECTED what the reference's array overload makes of it (the same layout in
//     the single-plane format), RGBA the reference's Convert of that to R8G8B8A8_UNORM (R16G16B16A16_UNORM for the 16-bit formats). The
//     three overloads must reproduce EXPECTED byte for byte; the resident overload, followed by Convert on the same device image, must
//     reproduce RGBA with ONE upload of exactly the planar blob and ONE download.
//   plane_host_test errors
//     the argument checks, in the reference's order, with the result released on failure.
// Prints "plane host checks passed" on success.
#include "../../directxtex_amd/host/DirectXTexAMD.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace DirectXTexAMD;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "FAILED line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static bool read_file(const char* path, std::vector<uint8_t>& out)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    out.resize(size_t(std::ftell(f)));
    std::fseek(f, 0, SEEK_SET);
    const bool ok = out.empty() || std::fread(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    return ok;
}

static bool same(const ScratchImage& a, const std::vector<uint8_t>& b)
{
    return a.GetPixelsSize() == b.size() && std::memcmp(a.GetPixels(), b.data(), b.size()) == 0;
}

static int convert(Device& dev, char** a)
{
    const DXGI_FORMAT fmt = DXGI_FORMAT(std::atoi(a[0]));
    const size_t w = size_t(std::atol(a[1])), h = size_t(std::atol(a[2])), items = size_t(std::atol(a[3])), mips = size_t(std::atol(a[4]));
    std::vector<uint8_t> in, expected, rgba;
    CHECK(read_file(a[5], in) && read_file(a[6], expected) && read_file(a[7], rgba));
    ScratchImage src;
    CHECK(src.Initialize2D(fmt, w, h, items, mips) == S_OK);
    CHECK(src.GetPixelsSize() == in.size());
    std::memcpy(src.GetPixels(), in.data(), in.size());

    // one image
    ScratchImage one;
    CHECK(ConvertToSinglePlane(dev, *src.GetImage(0, 0, 0), one) == S_OK);
    CHECK(one.GetImageCount() == 1 && one.GetPixelsSize() <= expected.size());
    CHECK(std::memcmp(one.GetPixels(), expected.data(), one.GetPixelsSize()) == 0);

    // the array overload
    ScratchImage all;
    CHECK(ConvertToSinglePlane(dev, src.GetImages(), src.GetImageCount(), src.GetMetadata(), all) == S_OK);
    CHECK(all.GetImageCount() == src.GetImageCount() && all.GetMetadata().mipLevels == mips && all.GetMetadata().arraySize == items);
    CHECK(same(all, expected));

    // resident, then Convert on the same device image: the planar blob goes up once, the converted texture comes down once
    const DXGI_FORMAT target = (fmt == DXGI_FORMAT_P010 || fmt == DXGI_FORMAT_P016) ? DXGI_FORMAT_R16G16B16A16_UNORM : DXGI_FORMAT_R8G8B8A8_UNORM;
    uint64_t up = 0, down = 0;
    GetTransferBytes(dev, up, down, true);
    DeviceScratchImage dsrc, dsingle, dconv;
    CHECK(dsrc.Upload(dev, src) == S_OK);
    CHECK(ConvertToSinglePlane(dev, dsrc, dsingle) == S_OK);
    CHECK(dsingle.GetMetadata().format == all.GetMetadata().format && dsingle.GetImageCount() == all.GetImageCount());
    CHECK(Convert(dev, dsingle, target, TEX_FILTER_DEFAULT, TEX_THRESHOLD_DEFAULT, dconv) == S_OK);
    ScratchImage back;
    CHECK(dconv.Download(back) == S_OK);
    GetTransferBytes(dev, up, down);
    CHECK(up == src.GetPixelsSize());
    CHECK(down == back.GetPixelsSize());
    CHECK(same(back, rgba));
    ScratchImage single;
    CHECK(dsingle.Download(single) == S_OK);
    CHECK(same(single, expected));
    return 0;
}

static int errors(Device& dev)
{
    ScratchImage nv12, out;
    CHECK(nv12.Initialize2D(DXGI_FORMAT_NV12, 8, 8, 2, 3) == S_OK);
    CHECK(nv12.GetImageCount() == 6);
    const TexMetadata md = nv12.GetMetadata();
    CHECK(ConvertToSinglePlane(dev, nv12.GetImages(), nv12.GetImageCount(), md, out) == S_OK);
    CHECK(out.GetImageCount() == 6 && out.GetMetadata().format == DXGI_FORMAT_YUY2);

    // NV11 16 x 4 with four mips: the 2 x 1 level's width is no multiple of four. E_INVALIDARG, the result released.
    ScratchImage nv11;
    CHECK(nv11.Initialize2D(DXGI_FORMAT_NV11, 16, 4, 1, 4) == S_OK);
    CHECK(nv11.GetImageCount() == 4 && nv11.GetImages()[3].width == 2 && nv11.GetImages()[3].height == 1);
    CHECK(ConvertToSinglePlane(dev, nv11.GetImages(), nv11.GetImageCount(), nv11.GetMetadata(), out) == E_INVALIDARG);
    CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
    {
        DeviceScratchImage d, r;
        CHECK(d.Upload(dev, nv11) == S_OK);
        CHECK(ConvertToSinglePlane(dev, nv12.GetImages()[0], out) == S_OK);
        CHECK(ConvertToSinglePlane(dev, d, r) == E_INVALIDARG);
        CHECK(r.GetImageCount() == 0 && r.GetPixels() == nullptr);
        DeviceScratchImage other;
        CHECK(ConvertToSinglePlane(dev, other, r) == E_INVALIDARG);            // nothing resident
    }

    // the image overload (:5413-5424)
    Image img = nv12.GetImages()[0];
    Image bad = img; bad.format = DXGI_FORMAT_R8G8B8A8_UNORM;
    CHECK(ConvertToSinglePlane(dev, bad, out) == E_INVALIDARG);
    bad.pixels = nullptr;
    CHECK(ConvertToSinglePlane(dev, bad, out) == E_INVALIDARG);                 // not planar comes before null pixels
    bad = img; bad.pixels = nullptr;
    CHECK(ConvertToSinglePlane(dev, bad, out) == E_POINTER);
    bad.format = DXGI_FORMAT_420_OPAQUE;
    CHECK(ConvertToSinglePlane(dev, bad, out) == E_POINTER);                    // null pixels come before a format without a single-plane form
    bad = img; bad.format = DXGI_FORMAT_420_OPAQUE;
    CHECK(ConvertToSinglePlane(dev, bad, out) == HRESULT_E_NOT_SUPPORTED);
    bad.format = DXGI_FORMAT_P208;
    CHECK(ConvertToSinglePlane(dev, bad, out) == HRESULT_E_NOT_SUPPORTED);
    CHECK(ConvertToSinglePlane(dev, img, out) == S_OK);
    bad = img; bad.width = 7;
    CHECK(ConvertToSinglePlane(dev, bad, out) == E_INVALIDARG);
    CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
    bad = img; bad.height = 6; bad.width = 6; bad.format = DXGI_FORMAT_NV11;
    CHECK(ConvertToSinglePlane(dev, bad, out) == E_INVALIDARG);

    // the array overload (:5458-5520)
    CHECK(ConvertToSinglePlane(dev, nv12.GetImages(), 0, md, out) == E_INVALIDARG);
    CHECK(ConvertToSinglePlane(dev, nullptr, 6, md, out) == E_INVALIDARG);
    TexMetadata m = md; m.format = DXGI_FORMAT_YUY2;
    CHECK(ConvertToSinglePlane(dev, nv12.GetImages(), 6, m, out) == E_INVALIDARG);
    m = md; m.dimension = TEX_DIMENSION_TEXTURE3D;
    CHECK(ConvertToSinglePlane(dev, nv12.GetImages(), 6, m, out) == HRESULT_E_NOT_SUPPORTED);
    m = md; m.format = DXGI_FORMAT_420_OPAQUE;
    CHECK(ConvertToSinglePlane(dev, nv12.GetImages(), 6, m, out) == HRESULT_E_NOT_SUPPORTED);
    CHECK(ConvertToSinglePlane(dev, nv12.GetImages(), 6, md, out) == S_OK);
    CHECK(ConvertToSinglePlane(dev, nv12.GetImages(), 5, md, out) == E_FAIL);                   // image count
    CHECK(out.GetImageCount() == 0 && out.GetPixels() == nullptr);
    m = md; m.format = DXGI_FORMAT_P010;                                                        // every image's format differs from the metadata's
    CHECK(ConvertToSinglePlane(dev, nv12.GetImages(), 6, m, out) == E_FAIL);
    m = md; m.width = 16; m.height = 16;                                                        // sizes
    CHECK(ConvertToSinglePlane(dev, nv12.GetImages(), 6, m, out) == E_FAIL);

    // the planar formats stay outside the other entry points
    CHECK(!IsSupportedOnDevice(DXGI_FORMAT_NV12) && !IsSupportedOnDevice(DXGI_FORMAT_NV11));
    CHECK(!nv12.OverrideFormat(DXGI_FORMAT_P010));
    return 0;
}

int main(int argc, char** argv)
{
    Device dev;
    CHECK(dev.Create(0) == S_OK);
    if (argc == 10 && !std::strcmp(argv[1], "convert")) { if (convert(dev, argv + 2)) return 1; }
    else if (argc == 2 && !std::strcmp(argv[1], "errors")) { if (errors(dev)) return 1; }
    else { std::fprintf(stderr, "usage: plane_host_test convert FORMAT WIDTH HEIGHT ITEMS MIPS IN EXPECTED RGBA | errors\n"); return 2; }
    std::printf("plane host checks passed\n");
    return 0;
}
