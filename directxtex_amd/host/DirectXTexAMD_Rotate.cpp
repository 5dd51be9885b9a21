// RotateColor: texconv's HDR colour rotation (Texconv/texconv.cpp:2696-2964) on the host layer, over the C ABI's dxtex_rotate_color and
// dxtex_rotate_color_device. The checks are TransformImage's (DirectXTexMisc.cpp:606-700), which the reference runs the lambdas through,
// plus texconv's own for the operation and the paper-white level. The array and resident forms issue ONE batched call for all images.
#include "DirectXTexAMD_Internal.h"

#include <vector>

namespace DirectXTexAMD
{
namespace
{

bool RotateUnsupported(DXGI_FORMAT f) noexcept { return IsPlanar(f) || IsPalettized(f) || IsCompressed(f) || IsTypeless(f); }

// what does not depend on the images: the operation and texconv's rule for -nits (texconv.cpp:1898), which a NaN fails too
HRESULT RotateArgChecks(TEX_ROTATE_COLOR rotate, float paperWhiteNits) noexcept
{
    if (rotate < TEX_ROTATE_709_TO_HDR10 || rotate > TEX_ROTATE_P3D65_TO_709) return E_INVALIDARG;
    if (!(paperWhiteNits > 0.f && paperWhiteNits <= 10000.f)) return E_INVALIDARG;
    return S_OK;
}

// the array form's checks that come before the destination exists (DirectXTexMisc.cpp:622-636)
HRESULT RotateSetChecks(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, TEX_ROTATE_COLOR rotate, float paperWhiteNits) noexcept
{
    if (!device) return E_POINTER;
    if (!srcImages || !nimages) return E_INVALIDARG;
    if (RotateUnsupported(metadata.format)) return HRESULT_E_NOT_SUPPORTED;
    if (metadata.width > UINT32_MAX || metadata.height > UINT32_MAX) return E_INVALIDARG;
    if (metadata.IsVolumemap() && metadata.depth > UINT16_MAX) return E_INVALIDARG;
    return RotateArgChecks(rotate, paperWhiteNits);
}
}

HRESULT RotateColor(Device& device, const Image& srcImage, TEX_ROTATE_COLOR rotate, float paperWhiteNits, ScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    if (srcImage.width > UINT32_MAX || srcImage.height > UINT32_MAX) return E_INVALIDARG;
    if (RotateUnsupported(srcImage.format)) return HRESULT_E_NOT_SUPPORTED;
    HRESULT hr = RotateArgChecks(rotate, paperWhiteNits);
    if (FAILED(hr)) return hr;
    result.Release();
    hr = result.Initialize2D(srcImage.format, srcImage.width, srcImage.height, 1, 1);
    if (FAILED(hr)) return hr;
    const Image* img = result.GetImage(0, 0, 0);
    if (!img) { result.Release(); return E_POINTER; }
    const dxtex_image s = ImageOf(srcImage), d = ImageOf(*img);
    hr = dxtex_rotate_color(device.Get(), &s, &d, uint32_t(rotate), paperWhiteNits);
    if (FAILED(hr)) result.Release();
    return hr;
}

HRESULT RotateColor(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, TEX_ROTATE_COLOR rotate, float paperWhiteNits,
                    ScratchImage& result) noexcept
{
    HRESULT hr = RotateSetChecks(device, srcImages, nimages, metadata, rotate, paperWhiteNits);
    if (FAILED(hr)) return hr;
    result.Release();
    // one upload of the set (it checks every image against the layout: E_FAIL for a format or size mismatch), the resident call, one download
    DeviceScratchImage in, out;
    hr = in.Upload(device, srcImages, nimages, metadata);
    if (SUCCEEDED(hr)) hr = RotateColor(device, in, rotate, paperWhiteNits, out);
    if (SUCCEEDED(hr)) hr = out.Download(result);
    if (FAILED(hr)) result.Release();
    return hr;
}

HRESULT RotateColor(Device& device, const DeviceScratchImage& src, TEX_ROTATE_COLOR rotate, float paperWhiteNits, DeviceScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    if (!src.GetImages() || src.GetDevice() != &device) return E_INVALIDARG;
    const TexMetadata& metadata = src.GetMetadata();
    HRESULT hr = RotateSetChecks(device, src.GetImages(), src.GetImageCount(), metadata, rotate, paperWhiteNits);
    if (FAILED(hr)) return hr;
    result.Release();
    hr = result.Initialize(device, metadata);
    if (FAILED(hr)) return hr;
    if (src.GetImageCount() != result.GetImageCount()) { result.Release(); return E_FAIL; }
    try
    {
        const size_t n = src.GetImageCount();
        std::vector<dxtex_image> s(n), d(n);
        for (size_t i = 0; i < n; ++i) { s[i] = ImageOf(src.GetImages()[i]); d[i] = ImageOf(result.GetImages()[i]); }
        hr = dxtex_rotate_color_device(device.Get(), s.data(), d.data(), n, uint32_t(rotate), paperWhiteNits);
    }
    catch (...) { hr = E_OUTOFMEMORY; }
    if (FAILED(hr)) result.Release();
    return hr;
}
} // namespace DirectXTexAMD
