// ConvertToSinglePlane (DirectXTexConvert.cpp:5411-5523) on the host layer, over the C ABI's dxtex_convert_to_single_plane and
// dxtex_convert_to_single_plane_device. The array and resident forms issue ONE batched submission for all images (array items x mips).
#include "DirectXTexAMD_Internal.h"

#include <new>
#include <vector>

namespace DirectXTexAMD
{
namespace
{

// the checks both array forms share, in the reference's order (:5458-5472); `format` receives PlanarToSingle(metadata.format)
HRESULT CheckPlanarSet(const Image* srcImages, size_t nimages, const TexMetadata& metadata, DXGI_FORMAT& format) noexcept
{
    if (!srcImages || !nimages || !IsPlanar(metadata.format)) return E_INVALIDARG;
    if (metadata.IsVolumemap()) return HRESULT_E_NOT_SUPPORTED;      // Direct3D has no planar Texture3D
    format = DXGI_FORMAT(dxtex_planar_to_single(int32_t(metadata.format)));
    if (format == DXGI_FORMAT_UNKNOWN) return HRESULT_E_NOT_SUPPORTED;
    if (metadata.width > UINT32_MAX || metadata.height > UINT32_MAX) return E_INVALIDARG;
    return S_OK;
}

// The reference's per-image loop (:5493-5520) up to the conversion itself: E_FAIL for an image-count, format or size mismatch, and - so
// that the FIRST failing image decides the code, as in a loop that converts image by image - what ConvertToSinglePlane_ answers before it
// touches a texel (:4998-5030). The batched submission repeats the second part (and this project's added checks) for every image.
HRESULT CheckPlanarImages(const Image* srcImages, size_t nimages, const TexMetadata& metadata, const Image* dest, size_t ndest) noexcept
{
    if (nimages != ndest) return E_FAIL;
    if (!dest) return E_POINTER;
    for (size_t i = 0; i < nimages; ++i)
    {
        const Image& src = srcImages[i];
        if (src.format != metadata.format) return E_FAIL;
        if (src.width > UINT32_MAX || src.height > UINT32_MAX) return E_FAIL;
        if (src.width != dest[i].width || src.height != dest[i].height) return E_FAIL;
        if (!src.pixels || !dest[i].pixels) return E_POINTER;
        if (src.format == DXGI_FORMAT_NV11 ? (src.width % 4) != 0 : ((src.width % 2) != 0 || (src.height % 2) != 0)) return E_INVALIDARG;
    }
    return S_OK;
}

// device memory freed on every way out (dxtex_device_free waits for the work that still uses it)
struct DeviceBlock
{
    Device& device;
    void* mem = nullptr;
    explicit DeviceBlock(Device& d) noexcept : device(d) {}
    DeviceBlock(const DeviceBlock&) = delete;
    DeviceBlock& operator=(const DeviceBlock&) = delete;
    ~DeviceBlock() { if (mem) dxtex_device_free(device.Get(), mem); }
};

HRESULT SubmitPlanes(Device& device, const dxtex_image* srcs, const Image* dest, size_t nimages)          // may throw bad_alloc: the callers catch
{
    std::vector<dxtex_image> d(nimages);
    for (size_t i = 0; i < nimages; ++i) d[i] = ImageOf(dest[i]);
    return dxtex_convert_to_single_plane_device(device.Get(), srcs, d.data(), nimages);
}
}

HRESULT ConvertToSinglePlane(Device& device, const Image& srcImage, ScratchImage& image) noexcept
{
    if (!device) return E_POINTER;
    if (!IsPlanar(srcImage.format)) return E_INVALIDARG;
    if (!srcImage.pixels) return E_POINTER;
    const DXGI_FORMAT format = DXGI_FORMAT(dxtex_planar_to_single(int32_t(srcImage.format)));
    if (format == DXGI_FORMAT_UNKNOWN) return HRESULT_E_NOT_SUPPORTED;
    if (srcImage.width > UINT32_MAX || srcImage.height > UINT32_MAX) return E_INVALIDARG;
    HRESULT hr = image.Initialize2D(format, srcImage.width, srcImage.height, 1, 1);
    if (FAILED(hr)) return hr;
    const Image* rimage = image.GetImage(0, 0, 0);
    if (!rimage) { image.Release(); return E_POINTER; }
    const dxtex_image s = ImageOf(srcImage), d = ImageOf(*rimage);
    hr = dxtex_convert_to_single_plane(device.Get(), &s, &d);
    if (FAILED(hr)) image.Release();
    return hr;
}

HRESULT ConvertToSinglePlane(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, ScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    DXGI_FORMAT format = DXGI_FORMAT_UNKNOWN;
    HRESULT hr = CheckPlanarSet(srcImages, nimages, metadata, format);
    if (FAILED(hr)) return hr;
    TexMetadata mdata2 = metadata;
    mdata2.format = format;
    try
    {
        DeviceScratchImage out;
        hr = out.Initialize(device, mdata2);
        if (FAILED(hr)) return hr;
        hr = CheckPlanarImages(srcImages, nimages, metadata, out.GetImages(), out.GetImageCount());
        if (FAILED(hr)) { result.Release(); return hr; }
        // every source goes up as the caller describes it - slicePitch bytes, its own pitches - into one allocation, 16-byte aligned each
        std::vector<dxtex_image> srcs(nimages);
        size_t total = 0;
        for (size_t i = 0; i < nimages; ++i)
        {
            srcs[i] = ImageOf(srcImages[i]);
            srcs[i].pixels = reinterpret_cast<uint8_t*>(total);
            total += (srcImages[i].slicePitch + 15) & ~size_t(15);
        }
        DeviceBlock block(device);
        hr = dxtex_device_alloc(device.Get(), total ? total : 16, &block.mem);
        if (FAILED(hr)) { result.Release(); return hr; }
        for (size_t i = 0; i < nimages && SUCCEEDED(hr); ++i)
        {
            srcs[i].pixels = static_cast<uint8_t*>(block.mem) + reinterpret_cast<size_t>(srcs[i].pixels);
            if (srcImages[i].slicePitch) hr = dxtex_memcpy_h2d_async(device.Get(), srcs[i].pixels, srcImages[i].pixels, srcImages[i].slicePitch);
        }
        if (SUCCEEDED(hr)) hr = SubmitPlanes(device, srcs.data(), out.GetImages(), nimages);
        if (SUCCEEDED(hr)) hr = out.Download(result);
        if (FAILED(hr)) result.Release();
        return hr;
    }
    catch (...) { result.Release(); return E_OUTOFMEMORY; }
}

HRESULT ConvertToSinglePlane(Device& device, const DeviceScratchImage& src, DeviceScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    if (!src.GetImages() || src.GetDevice() != &device) return E_INVALIDARG;
    const TexMetadata& metadata = src.GetMetadata();
    const size_t nimages = src.GetImageCount();
    DXGI_FORMAT format = DXGI_FORMAT_UNKNOWN;
    HRESULT hr = CheckPlanarSet(src.GetImages(), nimages, metadata, format);
    if (FAILED(hr)) return hr;
    TexMetadata mdata2 = metadata;
    mdata2.format = format;
    try
    {
        hr = result.Initialize(device, mdata2);
        if (FAILED(hr)) return hr;
        hr = CheckPlanarImages(src.GetImages(), nimages, metadata, result.GetImages(), result.GetImageCount());
        if (SUCCEEDED(hr))
        {
            std::vector<dxtex_image> srcs(nimages);
            for (size_t i = 0; i < nimages; ++i) srcs[i] = ImageOf(src.GetImages()[i]);
            hr = SubmitPlanes(device, srcs.data(), result.GetImages(), nimages);
        }
        if (FAILED(hr)) result.Release();
        return hr;
    }
    catch (...) { result.Release(); return E_OUTOFMEMORY; }
}
} // namespace DirectXTexAMD
