// CopyRectangle (DirectXTexMisc.cpp:275-381) and texassemble's steps (Texassemble/texassemble.cpp:2013-2400) on the host layer, over the C
// ABI's dxtex_copy_rectangle, dxtex_copy_rectangles_device and dxtex_merge_image_device. The assemble steps work on DeviceScratchImages:
// the inputs go up once, every face, slice or item is one rectangle of ONE batched launch, and the result comes down once.
#include "DirectXTexAMD_Internal.h"

#include <new>
#include <vector>

namespace DirectXTexAMD
{
namespace
{
dxtex_rect View(const Rect& r) noexcept { return dxtex_rect{ r.x, r.y, r.w, r.h }; }

inline bool Resident(const Device& device, const DeviceScratchImage& src) noexcept { return src.GetImages() && src.GetDevice() == &device; }

// faces +X -X +Y -Y +Z -Z: the cell of each in a grid of cols x rows faces (texassemble.cpp:2106-2181; the strips are index * size)
const CrossLayout kLayouts[CROSS_KIND_COUNT] = {
    { "h-cross", 4, 3, { 2, 0, 1, 1, 1, 3 }, { 1, 1, 0, 2, 1, 1 } },
    { "v-cross", 3, 4, { 2, 0, 1, 1, 1, 1 }, { 1, 1, 0, 2, 1, 3 } },
    { "h-tee", 4, 3, { 1, 3, 0, 0, 0, 2 }, { 1, 1, 0, 2, 1, 1 } },
    { "h-strip", 6, 1, { 0, 1, 2, 3, 4, 5 }, { 0, 0, 0, 0, 0, 0 } },
    { "v-strip", 1, 6, { 0, 0, 0, 0, 0, 0 }, { 0, 1, 2, 3, 4, 5 } },
};

// one batched call: whole images `src[i]` into `dst[i]` at (x[i], y[i])
struct Batch
{
    std::vector<dxtex_image> src, dst;
    std::vector<dxtex_rect> rect;
    std::vector<size_t> x, y;
    void Add(const Image& s, const Rect& r, const Image& d, size_t xo, size_t yo)
    {
        src.push_back(ImageOf(s)); rect.push_back(View(r)); dst.push_back(ImageOf(d)); x.push_back(xo); y.push_back(yo);
    }
    HRESULT Run(Device& device) const noexcept
    {
        return dxtex_copy_rectangles_device(device.Get(), src.data(), rect.data(), dst.data(), x.data(), y.data(), src.size(), 0);
    }
};

TexMetadata Texture2D(DXGI_FORMAT format, size_t width, size_t height, size_t arraySize) noexcept
{
    TexMetadata m;
    m.width = width; m.height = height; m.depth = 1; m.arraySize = arraySize; m.mipLevels = 1;
    m.format = format; m.dimension = TEX_DIMENSION_TEXTURE2D;
    return m;
}
}

const CrossLayout* GetCrossLayout(CROSS_KIND kind) noexcept { return kind < CROSS_KIND_COUNT ? &kLayouts[kind] : nullptr; }

HRESULT CopyRectangle(Device& device, const Image& srcImage, const Rect& srcRect, const Image& dstImage, TEX_FILTER_FLAGS filter, size_t xOffset, size_t yOffset) noexcept
{
    if (!device) return E_POINTER;
    const dxtex_image s = ImageOf(srcImage), d = ImageOf(dstImage);
    const dxtex_rect r = View(srcRect);
    return dxtex_copy_rectangle(device.Get(), &s, &r, &d, uint32_t(filter), xOffset, yOffset);
}

HRESULT CopyRectangle(Device& device, const DeviceScratchImage& src, size_t srcMip, size_t srcItem, size_t srcSlice, const Rect& srcRect,
                      const DeviceScratchImage& dst, size_t dstMip, size_t dstItem, size_t dstSlice, TEX_FILTER_FLAGS filter, size_t xOffset, size_t yOffset) noexcept
{
    if (!device) return E_POINTER;
    if (!Resident(device, src) || !Resident(device, dst)) return E_INVALIDARG;
    const Image* s = src.GetImage(srcMip, srcItem, srcSlice);
    const Image* d = dst.GetImage(dstMip, dstItem, dstSlice);
    if (!s || !d) return E_INVALIDARG;
    const dxtex_image sv = ImageOf(*s), dv = ImageOf(*d);
    const dxtex_rect r = View(srcRect);
    return dxtex_copy_rectangles_device(device.Get(), &sv, &r, &dv, &xOffset, &yOffset, 1, uint32_t(filter));
}

HRESULT MergeImages(Device& device, const DeviceScratchImage& image1, const DeviceScratchImage& image2, TEX_FILTER_FLAGS filter, const uint32_t permute[4],
                    const uint32_t zero[4], const uint32_t one[4], DeviceScratchImage& result) noexcept
{
    if (!device || !permute || !zero || !one) return E_POINTER;
    if (!Resident(device, image1) || !Resident(device, image2)) return E_INVALIDARG;
    const Image* a = image1.GetImage(0, 0, 0);
    const Image* b = image2.GetImage(0, 0, 0);
    if (!a || !b) return E_POINTER;
    if (a->width != b->width || a->height != b->height) return E_FAIL;
    DeviceScratchImage bFloat;
    HRESULT hr = S_OK;
    if (b->format != DXGI_FORMAT_R32G32B32A32_FLOAT)
    {
        // Convert takes a whole resident texture; texassemble converts image 0 of the second input only, and merge refuses inputs with mips
        hr = Convert(device, image2, DXGI_FORMAT_R32G32B32A32_FLOAT, filter, TEX_THRESHOLD_DEFAULT, bFloat); if (FAILED(hr)) return hr;
        b = bFloat.GetImage(0, 0, 0);
    }
    hr = result.Initialize(device, Texture2D(a->format, a->width, a->height, 1)); if (FAILED(hr)) return hr;
    const dxtex_image av = ImageOf(*a), bv = ImageOf(*b), dv = ImageOf(*result.GetImage(0, 0, 0));
    hr = dxtex_merge_image_device(device.Get(), &av, &bv, &dv, permute, zero, one);
    if (FAILED(hr)) result.Release();
    return hr;
}

HRESULT MergeImages(Device& device, const Image& image1, const Image& image2, TEX_FILTER_FLAGS filter, const uint32_t permute[4], const bool zero[4],
                    const bool one[4], ScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    if (!image1.pixels || !image2.pixels || !permute || !zero || !one) return E_POINTER;
    DeviceScratchImage a, b, merged;
    HRESULT hr = a.Upload(device, &image1, 1, Texture2D(image1.format, image1.width, image1.height, 1)); if (FAILED(hr)) return hr;
    hr = b.Upload(device, &image2, 1, Texture2D(image2.format, image2.width, image2.height, 1)); if (FAILED(hr)) return hr;
    uint32_t z[4], o[4];
    for (int k = 0; k < 4; ++k) { z[k] = zero[k] ? 1u : 0u; o[k] = one[k] ? 1u : 0u; }
    hr = MergeImages(device, a, b, filter, permute, z, o, merged); if (FAILED(hr)) return hr;
    return merged.Download(result);
}

bool ParseMergeMask(const char* mask, uint32_t permute[4], uint32_t zero[4], uint32_t one[4]) noexcept
{
    if (!mask || !permute || !zero || !one || !mask[0]) return false;
    static const char kFirst[] = "rgbaxyzw", kSecond[] = "RGBAXYZW";
    for (uint32_t j = 0; j < 4 && mask[j]; ++j)
    {
        uint32_t p = 0, z = 0, o = 0;
        bool keep = false;          // 0 and 1 leave channel k on itself
        const char* f = nullptr;
        for (const char* q = kFirst; *q; ++q) if (*q == mask[j]) f = q;
        const char* g = nullptr;
        for (const char* q = kSecond; *q; ++q) if (*q == mask[j]) g = q;
        if (f) p = uint32_t(f - kFirst) & 3u;
        else if (g) p = 4u + (uint32_t(g - kSecond) & 3u);
        else if (mask[j] == '0') { z = 1; keep = true; }
        else if (mask[j] == '1') { o = 1; keep = true; }
        else return false;
        for (uint32_t k = j; k < 4; ++k) { permute[k] = keep ? k : p; zero[k] = z; one[k] = o; }
    }
    return true;
}

HRESULT AssembleCross(Device& device, CROSS_KIND kind, const DeviceScratchImage& faces, DeviceScratchImage& result) noexcept
{
    const CrossLayout* layout = GetCrossLayout(kind);
    if (!device) return E_POINTER;
    if (!layout || !Resident(device, faces) || faces.GetMetadata().arraySize < 6 || faces.GetMetadata().IsVolumemap()) return E_INVALIDARG;
    const TexMetadata& f = faces.GetMetadata();
    HRESULT hr = result.Initialize(device, Texture2D(f.format, f.width * layout->cols, f.height * layout->rows, 1));       // zero-filled: the background
    if (FAILED(hr)) return hr;
    try
    {
        Batch batch;
        for (size_t i = 0; i < 6; ++i)
            batch.Add(*faces.GetImage(0, i, 0), Rect(0, 0, f.width, f.height), *result.GetImage(0, 0, 0), layout->x[i] * f.width, layout->y[i] * f.height);
        hr = batch.Run(device);
    }
    catch (const std::bad_alloc&) { hr = E_OUTOFMEMORY; }
    if (FAILED(hr)) result.Release();
    return hr;
}

HRESULT CubeFromCross(Device& device, CROSS_KIND kind, const DeviceScratchImage& image, DeviceScratchImage& cube) noexcept
{
    const CrossLayout* layout = GetCrossLayout(kind);
    if (!device) return E_POINTER;
    if (!layout || !Resident(device, image) || image.GetMetadata().IsVolumemap()) return E_INVALIDARG;
    const TexMetadata& c = image.GetMetadata();
    if (!c.width || !c.height || c.width % layout->cols || c.height % layout->rows) return E_INVALIDARG;
    const size_t w = c.width / layout->cols, h = c.height / layout->rows;
    TexMetadata m = Texture2D(c.format, w, h, 6);
    m.miscFlags |= TEX_MISC_TEXTURECUBE;
    HRESULT hr = cube.Initialize(device, m);
    if (FAILED(hr)) return hr;
    try
    {
        Batch batch;
        for (size_t i = 0; i < 6; ++i)
            batch.Add(*image.GetImage(0, 0, 0), Rect(layout->x[i] * w, layout->y[i] * h, w, h), *cube.GetImage(0, i, 0), 0, 0);
        hr = batch.Run(device);
    }
    catch (const std::bad_alloc&) { hr = E_OUTOFMEMORY; }
    if (FAILED(hr)) cube.Release();
    return hr;
}

namespace
{
// a legal flag word that keeps the face's width and height
bool TurnKeepsSize(TEX_FR_FLAGS f) noexcept { return f != 0 && (uint32_t(f) & ~0x1Bu) == 0 && (uint32_t(f) & 1u) == 0; }

// the w x h cell at (x, y) of `image` as an image of its own: a pointer into it and its pitch
Image CellOf(const Image& image, size_t x, size_t y, size_t w, size_t h) noexcept
{
    Image cell = image;
    cell.pixels = image.pixels + y * image.rowPitch + x * (BitsPerPixel(image.format) / 8);
    cell.width = w; cell.height = h;
    cell.slicePitch = image.rowPitch * h;
    return cell;
}
}

HRESULT AssembleCross(Device& device, CROSS_KIND kind, const DeviceScratchImage& faces, TEX_FR_FLAGS negZ, DeviceScratchImage& result) noexcept
{
    const CrossLayout* layout = GetCrossLayout(kind);
    if (!device) return E_POINTER;
    if (!layout || !Resident(device, faces) || faces.GetMetadata().arraySize < 6 || faces.GetMetadata().IsVolumemap() || !TurnKeepsSize(negZ)) return E_INVALIDARG;
    const TexMetadata& f = faces.GetMetadata();
    HRESULT hr = result.Initialize(device, Texture2D(f.format, f.width * layout->cols, f.height * layout->rows, 1));       // zero-filled: the background
    if (FAILED(hr)) return hr;
    try
    {
        Batch batch;
        for (size_t i = 0; i < 5; ++i)
            batch.Add(*faces.GetImage(0, i, 0), Rect(0, 0, f.width, f.height), *result.GetImage(0, 0, 0), layout->x[i] * f.width, layout->y[i] * f.height);
        hr = batch.Run(device);
        if (SUCCEEDED(hr))
        {
            const dxtex_image s = ImageOf(*faces.GetImage(0, 5, 0));
            const dxtex_image d = ImageOf(CellOf(*result.GetImage(0, 0, 0), layout->x[5] * f.width, layout->y[5] * f.height, f.width, f.height));
            hr = dxtex_flip_rotate_device(device.Get(), &s, &d, 1, uint32_t(negZ));
        }
    }
    catch (const std::bad_alloc&) { hr = E_OUTOFMEMORY; }
    if (FAILED(hr)) result.Release();
    return hr;
}

HRESULT CubeFromCross(Device& device, CROSS_KIND kind, const DeviceScratchImage& image, TEX_FR_FLAGS negZ, DeviceScratchImage& cube) noexcept
{
    const CrossLayout* layout = GetCrossLayout(kind);
    if (!device) return E_POINTER;
    if (!layout || !Resident(device, image) || image.GetMetadata().IsVolumemap() || !TurnKeepsSize(negZ)) return E_INVALIDARG;
    const TexMetadata& c = image.GetMetadata();
    if (!c.width || !c.height || c.width % layout->cols || c.height % layout->rows) return E_INVALIDARG;
    const size_t w = c.width / layout->cols, h = c.height / layout->rows;
    TexMetadata m = Texture2D(c.format, w, h, 6);
    m.miscFlags |= TEX_MISC_TEXTURECUBE;
    HRESULT hr = cube.Initialize(device, m);
    if (FAILED(hr)) return hr;
    try
    {
        Batch batch;
        for (size_t i = 0; i < 5; ++i)
            batch.Add(*image.GetImage(0, 0, 0), Rect(layout->x[i] * w, layout->y[i] * h, w, h), *cube.GetImage(0, i, 0), 0, 0);
        hr = batch.Run(device);
        if (SUCCEEDED(hr))
        {
            const dxtex_image s = ImageOf(CellOf(*image.GetImage(0, 0, 0), layout->x[5] * w, layout->y[5] * h, w, h));
            const dxtex_image d = ImageOf(*cube.GetImage(0, 5, 0));
            hr = dxtex_flip_rotate_device(device.Get(), &s, &d, 1, uint32_t(negZ));
        }
    }
    catch (const std::bad_alloc&) { hr = E_OUTOFMEMORY; }
    if (FAILED(hr)) cube.Release();
    return hr;
}

HRESULT AssembleStrip(Device& device, const DeviceScratchImage& items, DeviceScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    if (!Resident(device, items) || items.GetMetadata().IsVolumemap() || !items.GetMetadata().arraySize) return E_INVALIDARG;
    const TexMetadata& f = items.GetMetadata();
    HRESULT hr = result.Initialize(device, Texture2D(f.format, f.width, f.height * f.arraySize, 1));
    if (FAILED(hr)) return hr;
    try
    {
        Batch batch;
        for (size_t i = 0; i < f.arraySize; ++i)
            batch.Add(*items.GetImage(0, i, 0), Rect(0, 0, f.width, f.height), *result.GetImage(0, 0, 0), 0, i * f.height);
        hr = batch.Run(device);
    }
    catch (const std::bad_alloc&) { hr = E_OUTOFMEMORY; }
    if (FAILED(hr)) result.Release();
    return hr;
}

HRESULT CopyImages(Device& device, const Image* srcDeviceImages, const Image* dstDeviceImages, size_t count, TEX_FILTER_FLAGS filter) noexcept
{
    if (!device) return E_POINTER;
    if (!srcDeviceImages || !dstDeviceImages || !count) return E_INVALIDARG;
    try
    {
        std::vector<dxtex_image> src(count), dst(count);
        std::vector<dxtex_rect> rect(count);
        std::vector<size_t> zero(count, 0);
        for (size_t i = 0; i < count; ++i)
        {
            if (srcDeviceImages[i].width != dstDeviceImages[i].width || srcDeviceImages[i].height != dstDeviceImages[i].height) return E_FAIL;
            src[i] = ImageOf(srcDeviceImages[i]); dst[i] = ImageOf(dstDeviceImages[i]);
            rect[i] = dxtex_rect{ 0, 0, src[i].width, src[i].height };
        }
        return dxtex_copy_rectangles_device(device.Get(), src.data(), rect.data(), dst.data(), zero.data(), zero.data(), count, uint32_t(filter));
    }
    catch (const std::bad_alloc&) { return E_OUTOFMEMORY; }
}

namespace
{
HRESULT Stack(Device& device, const Image* images, size_t count, const TexMetadata& m, DeviceScratchImage& result) noexcept
{
    HRESULT hr = result.Initialize(device, m);
    if (FAILED(hr)) return hr;
    try
    {
        std::vector<Image> dst(count);
        for (size_t i = 0; i < count; ++i) dst[i] = m.IsVolumemap() ? *result.GetImage(0, 0, i) : *result.GetImage(0, i, 0);
        hr = CopyImages(device, images, dst.data(), count);
    }
    catch (const std::bad_alloc&) { hr = E_OUTOFMEMORY; }
    if (FAILED(hr)) result.Release();
    return hr;
}

HRESULT CheckStack(Device& device, const Image* images, size_t count) noexcept
{
    if (!device) return E_POINTER;
    if (!images || !count) return E_INVALIDARG;
    for (size_t i = 0; i < count; ++i)
    {
        if (!images[i].pixels) return E_POINTER;
        if (images[i].width != images[0].width || images[i].height != images[0].height || images[i].format != images[0].format) return E_FAIL;
    }
    return S_OK;
}
}

HRESULT StackArray(Device& device, const Image* deviceImages, size_t count, bool asCube, DeviceScratchImage& result) noexcept
{
    const HRESULT hr = CheckStack(device, deviceImages, count);
    if (FAILED(hr)) return hr;
    if (asCube && count % 6) return E_INVALIDARG;
    TexMetadata m = Texture2D(deviceImages[0].format, deviceImages[0].width, deviceImages[0].height, count);
    if (asCube) m.miscFlags |= TEX_MISC_TEXTURECUBE;
    return Stack(device, deviceImages, count, m, result);
}

HRESULT StackVolume(Device& device, const Image* deviceImages, size_t count, DeviceScratchImage& result) noexcept
{
    const HRESULT hr = CheckStack(device, deviceImages, count);
    if (FAILED(hr)) return hr;
    TexMetadata m = Texture2D(deviceImages[0].format, deviceImages[0].width, deviceImages[0].height, 1);
    m.depth = count; m.dimension = TEX_DIMENSION_TEXTURE3D;
    return Stack(device, deviceImages, count, m, result);
}
} // namespace DirectXTexAMD
