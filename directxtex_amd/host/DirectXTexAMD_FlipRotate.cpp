// FlipRotate (DirectXTexFlipRotate.cpp:185-381) on the host layer, over the C ABI's dxtex_flip_rotate and dxtex_flip_rotate_device. What a
// flag word means is the C ABI's to say (include/dxtex_amd.h; dxtex_fliprotate.h's fr_resolve is the one function that does): this file
// only needs to know whether it exchanges width and height, which is FlipsWidthHeight() below and nothing else. The array and resident
// forms issue ONE batched call for every item, mip and depth slice.
#include "DirectXTexAMD_Internal.h"

#include <vector>

namespace DirectXTexAMD
{
namespace
{
// the reference's rotateMode test (:214-235): a quarter or three-quarter turn
bool FlipsWidthHeight(TEX_FR_FLAGS flags) noexcept { return (uint32_t(flags) & 1u) != 0; }
bool LegalFlags(TEX_FR_FLAGS flags) noexcept { return flags != 0 && (uint32_t(flags) & ~0x1Bu) == 0; }

// the array form's checks that come before the destination exists (:290-319)
HRESULT FlipSetChecks(const Image* srcImages, size_t nimages, const TexMetadata& metadata, TEX_FR_FLAGS flags) noexcept
{
    if (!srcImages || !nimages) return E_INVALIDARG;
    if (IsCompressed(metadata.format)) return HRESULT_E_NOT_SUPPORTED;
    if (!LegalFlags(flags)) return E_INVALIDARG;
    return S_OK;
}

TexMetadata Turned(const TexMetadata& metadata, TEX_FR_FLAGS flags) noexcept
{
    TexMetadata m = metadata;
    if (FlipsWidthHeight(flags)) { m.width = metadata.height; m.height = metadata.width; }
    return m;
}
}

HRESULT FlipRotate(Device& device, const Image& srcImage, TEX_FR_FLAGS flags, ScratchImage& image) noexcept
{
    if (!device) return E_POINTER;
    if (!srcImage.pixels) return E_POINTER;
    if (!LegalFlags(flags)) return E_INVALIDARG;
    if (srcImage.width > UINT32_MAX || srcImage.height > UINT32_MAX) return E_INVALIDARG;
    if (IsCompressed(srcImage.format)) return HRESULT_E_NOT_SUPPORTED;
    const bool turn = FlipsWidthHeight(flags);
    HRESULT hr = image.Initialize2D(srcImage.format, turn ? srcImage.height : srcImage.width, turn ? srcImage.width : srcImage.height, 1, 1);
    if (FAILED(hr)) return hr;
    const Image* rimage = image.GetImage(0, 0, 0);
    if (!rimage) { image.Release(); return E_POINTER; }
    const dxtex_image s = ImageOf(srcImage), d = ImageOf(*rimage);
    hr = dxtex_flip_rotate(device.Get(), &s, &d, uint32_t(flags));
    if (FAILED(hr)) image.Release();
    return hr;
}

HRESULT FlipRotate(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, TEX_FR_FLAGS flags, ScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    HRESULT hr = FlipSetChecks(srcImages, nimages, metadata, flags);
    if (FAILED(hr)) return hr;
    result.Release();
    // one upload of the set (it checks every image against the layout: E_FAIL for a count, format or size mismatch), the resident call, one download
    DeviceScratchImage in, out;
    hr = in.Upload(device, srcImages, nimages, metadata);
    if (SUCCEEDED(hr)) hr = FlipRotate(device, in, flags, out);
    if (SUCCEEDED(hr)) hr = out.Download(result);
    if (FAILED(hr)) result.Release();
    return hr;
}

HRESULT FlipRotate(Device& device, const DeviceScratchImage& src, TEX_FR_FLAGS flags, DeviceScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    if (!src.GetImages() || src.GetDevice() != &device) return E_INVALIDARG;
    const TexMetadata& metadata = src.GetMetadata();
    const size_t n = src.GetImageCount();
    HRESULT hr = FlipSetChecks(src.GetImages(), n, metadata, flags);
    if (FAILED(hr)) return hr;
    result.Release();
    hr = result.Initialize(device, Turned(metadata, flags));
    if (FAILED(hr)) return hr;
    if (n != result.GetImageCount()) { result.Release(); return E_FAIL; }
    try
    {
        const bool turn = FlipsWidthHeight(flags);
        std::vector<dxtex_image> s(n), d(n);
        for (size_t i = 0; i < n && SUCCEEDED(hr); ++i)
        {
            const Image& a = src.GetImages()[i];
            const Image& b = result.GetImages()[i];
            if (a.format != metadata.format || a.width > UINT32_MAX || a.height > UINT32_MAX) hr = E_FAIL;
            else if (turn ? (a.width != b.height || a.height != b.width) : (a.width != b.width || a.height != b.height)) hr = E_FAIL;
            s[i] = ImageOf(a); d[i] = ImageOf(b);
        }
        if (SUCCEEDED(hr)) hr = dxtex_flip_rotate_device(device.Get(), s.data(), d.data(), n, uint32_t(flags));
    }
    catch (...) { hr = E_OUTOFMEMORY; }
    if (FAILED(hr)) result.Release();
    return hr;
}
} // namespace DirectXTexAMD
