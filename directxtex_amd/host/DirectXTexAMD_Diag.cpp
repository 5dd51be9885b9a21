// texdiag's diagnostics on the host layer: ComputeMSE with CMSE_FLAGS (DirectXTexMisc.cpp:388-468), Analyze, AnalyzeBC and Difference
// (Texdiag/texdiag.cpp:698-787, :906-1226, :1229-1320) over the C ABI's dxtex_analyze_device, dxtex_analyze_bc_device,
// dxtex_compute_mse_flags_device and dxtex_difference_device. Every overload works on DeviceScratchImages: a host image goes up once,
// Decompress and Convert run on the device, and nothing but the figures (or Difference's finished map) comes back.
#include "DirectXTexAMD_Internal.h"

#include <cmath>
#include <new>
#include <vector>

namespace DirectXTexAMD
{
namespace
{

inline bool Resident(const Device& device, const DeviceScratchImage& src) noexcept { return src.GetImages() && src.GetDevice() == &device; }

TexMetadata SingleImage(const Image& image) noexcept
{
    TexMetadata m;
    m.width = image.width; m.height = image.height; m.depth = 1; m.arraySize = 1; m.mipLevels = 1;
    m.format = image.format; m.dimension = TEX_DIMENSION_TEXTURE2D;
    return m;
}

// the reference wrappers' format checks (DirectXTexMisc.cpp:401-407, :483-487)
HRESULT CheckFormat(DXGI_FORMAT f) noexcept
{
    if (!IsValid(f)) return E_INVALIDARG;
    if (IsPlanar(f) || IsPalettized(f) || IsTypeless(f)) return HRESULT_E_NOT_SUPPORTED;
    return S_OK;
}

// `src` as the kernels take it: itself, or its Decompress to R32G32B32A32_FLOAT in `expanded`
HRESULT Expanded(Device& device, const DeviceScratchImage& src, DeviceScratchImage& expanded, const DeviceScratchImage*& out) noexcept
{
    out = &src;
    if (!IsCompressed(src.GetMetadata().format)) return S_OK;
    const HRESULT hr = Decompress(device, src, DXGI_FORMAT_R32G32B32A32_FLOAT, expanded);
    if (SUCCEEDED(hr)) out = &expanded;
    return hr;
}

void Fill(AnalyzeData& r, const dxtex_image_stats& s) noexcept
{
    for (int c = 0; c < 4; ++c)
    {
        r.imageMin[c] = s.min[c]; r.imageMax[c] = s.max[c]; r.imageAvg[c] = s.avg[c]; r.imageVariance[c] = s.variance[c];
        r.imageStdDev[c] = std::sqrt(s.variance[c]); r.specials[c] = s.specials[c];
    }
    r.luminance = s.luminance;
}
}

// ---- ComputeMSE -------------------------------------------------------------------------------------------------------------------------
HRESULT ComputeMSE(Device& device, const DeviceScratchImage& image1, const DeviceScratchImage& image2, float& mse, float* mseV, CMSE_FLAGS flags) noexcept
{
    return ComputeMSE(device, image1, 0, image2, 0, mse, mseV, flags);
}

HRESULT ComputeMSE(Device& device, const DeviceScratchImage& image1, size_t index1, const DeviceScratchImage& image2, size_t index2, float& mse, float* mseV,
                   CMSE_FLAGS flags) noexcept
{
    if (!device) return E_POINTER;
    if (!Resident(device, image1) || !Resident(device, image2)) return E_INVALIDARG;
    if (index1 >= image1.GetImageCount() || index2 >= image2.GetImageCount()) return E_POINTER;
    const Image* a = image1.GetImages() + index1;
    const Image* b = image2.GetImages() + index2;
    if (a->width != b->width || a->height != b->height) return E_INVALIDARG;
    HRESULT hr = CheckFormat(a->format); if (FAILED(hr)) return hr;
    hr = CheckFormat(b->format); if (FAILED(hr)) return hr;
    DeviceScratchImage t1, t2;
    const DeviceScratchImage* ea = nullptr;
    const DeviceScratchImage* eb = nullptr;
    hr = Expanded(device, image1, t1, ea); if (FAILED(hr)) return hr;
    hr = Expanded(device, image2, t2, eb); if (FAILED(hr)) return hr;
    if (index1 >= ea->GetImageCount() || index2 >= eb->GetImageCount()) return E_POINTER;
    a = ea->GetImages() + index1; b = eb->GetImages() + index2;
    const dxtex_image va = ImageOf(*a), vb = ImageOf(*b);
    double v[4] = { 0, 0, 0, 0 };
    hr = dxtex_compute_mse_flags_device(device.Get(), &va, &vb, uint32_t(flags), v);
    if (FAILED(hr)) return hr;
    if (mseV) for (int c = 0; c < 4; ++c) mseV[c] = float(v[c]);
    mse = float(v[0]) + float(v[1]) + float(v[2]) + float(v[3]);
    return S_OK;
}

HRESULT ComputeMSE(Device& device, const Image& image1, const Image& image2, float& mse, float* mseV, CMSE_FLAGS flags) noexcept
{
    if (!device) return E_POINTER;
    if (!image1.pixels || !image2.pixels) return E_POINTER;
    if (image1.width != image2.width || image1.height != image2.height) return E_INVALIDARG;
    HRESULT hr = CheckFormat(image1.format); if (FAILED(hr)) return hr;
    hr = CheckFormat(image2.format); if (FAILED(hr)) return hr;
    DeviceScratchImage d1, d2;
    hr = d1.Upload(device, &image1, 1, SingleImage(image1)); if (FAILED(hr)) return hr;
    hr = d2.Upload(device, &image2, 1, SingleImage(image2)); if (FAILED(hr)) return hr;
    return ComputeMSE(device, d1, d2, mse, mseV, flags);
}

// ---- Analyze ----------------------------------------------------------------------------------------------------------------------------
HRESULT Analyze(Device& device, const DeviceScratchImage& images, AnalyzeData* results) noexcept
{
    if (!device || !results) return E_POINTER;
    if (!Resident(device, images)) return E_INVALIDARG;
    const TexMetadata& m = images.GetMetadata();
    if (m.width > UINT32_MAX || m.height > UINT32_MAX) return E_INVALIDARG;
    HRESULT hr = CheckFormat(m.format); if (FAILED(hr)) return hr;
    DeviceScratchImage temp;
    const DeviceScratchImage* e = nullptr;
    hr = Expanded(device, images, temp, e); if (FAILED(hr)) return hr;
    const size_t n = e->GetImageCount();
    if (n != images.GetImageCount()) return E_FAIL;
    try
    {
        std::vector<dxtex_image> v(n);
        std::vector<dxtex_image_stats> s(n);
        for (size_t i = 0; i < n; ++i) v[i] = ImageOf(e->GetImages()[i]);
        hr = dxtex_analyze_device(device.Get(), v.data(), n, s.data());
        if (FAILED(hr)) return hr;
        for (size_t i = 0; i < n; ++i) Fill(results[i], s[i]);
    }
    catch (const std::bad_alloc&) { return E_OUTOFMEMORY; }
    return S_OK;
}

HRESULT Analyze(Device& device, const Image* images, size_t nimages, const TexMetadata& metadata, AnalyzeData* results) noexcept
{
    if (!device || !results) return E_POINTER;
    if (!images || !nimages) return E_INVALIDARG;
    DeviceScratchImage d;
    const HRESULT hr = d.Upload(device, images, nimages, metadata);
    if (FAILED(hr)) return hr;
    return Analyze(device, d, results);
}

HRESULT Analyze(Device& device, const Image& image, AnalyzeData& result) noexcept
{
    if (!image.pixels) return E_POINTER;
    return Analyze(device, &image, 1, SingleImage(image), &result);
}

// ---- AnalyzeBC --------------------------------------------------------------------------------------------------------------------------
HRESULT AnalyzeBC(Device& device, const DeviceScratchImage& images, AnalyzeBCData* results) noexcept
{
    if (!device || !results) return E_POINTER;
    if (!Resident(device, images)) return E_INVALIDARG;
    if (!IsCompressed(images.GetMetadata().format)) return HRESULT_E_NOT_SUPPORTED;        // texdiag.cpp:933
    for (size_t i = 0; i < images.GetImageCount(); ++i)
    {
        const dxtex_image v = ImageOf(images.GetImages()[i]);
        const HRESULT hr = dxtex_analyze_bc_device(device.Get(), &v, results[i].blockHist, &results[i].blocks);
        if (FAILED(hr)) return hr;
    }
    return S_OK;
}

HRESULT AnalyzeBC(Device& device, const Image& image, AnalyzeBCData& result) noexcept
{
    if (!device || !image.pixels) return E_POINTER;
    if (!IsCompressed(image.format)) return HRESULT_E_NOT_SUPPORTED;
    DeviceScratchImage d;
    const HRESULT hr = d.Upload(device, &image, 1, SingleImage(image));
    if (FAILED(hr)) return hr;
    return AnalyzeBC(device, d, &result);
}

// ---- Difference -------------------------------------------------------------------------------------------------------------------------
HRESULT Difference(Device& device, const DeviceScratchImage& image1, const DeviceScratchImage& image2, TEX_FILTER_FLAGS dwFilter, DXGI_FORMAT format,
                   uint32_t diffColor, float threshold, DeviceScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    if (!Resident(device, image1) || !Resident(device, image2)) return E_INVALIDARG;
    const Image* a = image1.GetImage(0, 0, 0);
    const Image* b = image2.GetImage(0, 0, 0);
    if (!a || !b) return E_POINTER;
    if (a->width != b->width || a->height != b->height) return E_FAIL;                      // :1241-1243
    result.Release();
    DeviceScratchImage tempA, tempB;
    const DeviceScratchImage* ea = nullptr;
    HRESULT hr = Expanded(device, image1, tempA, ea); if (FAILED(hr)) return hr;           // :1247-1254
    const DeviceScratchImage* eb = &image2;
    if (b->format != DXGI_FORMAT_R32G32B32A32_FLOAT)                                        // :1258-1276
    {
        if (IsCompressed(b->format)) hr = Decompress(device, image2, DXGI_FORMAT_R32G32B32A32_FLOAT, tempB);
        else hr = Convert(device, image2, DXGI_FORMAT_R32G32B32A32_FLOAT, dwFilter, TEX_THRESHOLD_DEFAULT, tempB);
        if (FAILED(hr)) return hr;
        eb = &tempB;
    }
    a = ea->GetImage(0, 0, 0); b = eb->GetImage(0, 0, 0);
    if (!a || !b) return E_POINTER;
    DeviceScratchImage diff;
    hr = diff.Initialize(device, SingleImage(*a)); if (FAILED(hr)) return hr;
    const Image* d = diff.GetImage(0, 0, 0);
    if (!d) return E_POINTER;
    const dxtex_image va = ImageOf(*a), vb = ImageOf(*b), vd = ImageOf(*d);
    hr = dxtex_difference_device(device.Get(), &va, &vb, &vd, diffColor, threshold);
    if (FAILED(hr)) return hr;
    if (format == a->format) { result = static_cast<DeviceScratchImage&&>(diff); return S_OK; }        // :1313-1317
    hr = Convert(device, diff, format, dwFilter, TEX_THRESHOLD_DEFAULT, result);           // :1319
    if (FAILED(hr)) result.Release();
    return hr;
}

HRESULT Difference(Device& device, const Image& image1, const Image& image2, TEX_FILTER_FLAGS dwFilter, DXGI_FORMAT format, uint32_t diffColor,
                   float threshold, ScratchImage& result) noexcept
{
    if (!device) return E_POINTER;
    if (!image1.pixels || !image2.pixels) return E_POINTER;
    if (image1.width != image2.width || image1.height != image2.height) return E_FAIL;
    result.Release();
    DeviceScratchImage d1, d2, out;
    HRESULT hr = d1.Upload(device, &image1, 1, SingleImage(image1)); if (FAILED(hr)) return hr;
    hr = d2.Upload(device, &image2, 1, SingleImage(image2)); if (FAILED(hr)) return hr;
    hr = Difference(device, d1, d2, dwFilter, format, diffColor, threshold, out);
    if (SUCCEEDED(hr)) hr = out.Download(result);
    if (FAILED(hr)) result.Release();
    return hr;
}
} // namespace DirectXTexAMD
