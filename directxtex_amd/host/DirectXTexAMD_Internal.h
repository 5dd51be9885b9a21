// What the file codecs of the host layer share (DirectXTexAMD_DDS / _HDR / _TGA / _PNM / _PNG / _JPEG / _EXR.cpp): a whole file into a Blob, a
// Blob into a file, the file twins of the Memory forms, an Image as the C ABI takes it, device memory that lives as long as a scope, and
// the frame of a resident load and a resident save. Not part of the public interface. Header-only, and every definition has internal
// linkage: a translation unit compiled on its own, as the sanitised test programs compile one codec each, calls its own copy.
#pragma once
#include "DirectXTexAMD.h"
#include "../../include/dxtex_amd.h"
#include "../csrc/dxtex_stream.h"

#include <cstdio>

namespace DirectXTexAMD
{
// The codec tables of csrc/dxtex_{tga,dds,pnm,png,jpeg}.h are written over dxtex_stream.h's FMT_*, and the codecs hand them a DXGI_FORMAT:
// every number a codec's table names is the same in both lists
#define DXTEX_SAME_FORMAT(name) static_assert(int(DXGI_FORMAT_##name) == int(dxtex::FMT_##name), "DXGI_FORMAT_" #name " is not FMT_" #name)
DXTEX_SAME_FORMAT(UNKNOWN);
DXTEX_SAME_FORMAT(R32G32B32A32_TYPELESS); DXTEX_SAME_FORMAT(R32G32B32A32_FLOAT); DXTEX_SAME_FORMAT(R32G32B32A32_UINT); DXTEX_SAME_FORMAT(R32G32B32A32_SINT);
DXTEX_SAME_FORMAT(R32G32B32_FLOAT);
DXTEX_SAME_FORMAT(R16G16B16A16_TYPELESS); DXTEX_SAME_FORMAT(R16G16B16A16_FLOAT); DXTEX_SAME_FORMAT(R16G16B16A16_UNORM); DXTEX_SAME_FORMAT(R16G16B16A16_UINT);
DXTEX_SAME_FORMAT(R16G16B16A16_SNORM); DXTEX_SAME_FORMAT(R16G16B16A16_SINT);
DXTEX_SAME_FORMAT(R10G10B10A2_TYPELESS); DXTEX_SAME_FORMAT(R10G10B10A2_UNORM); DXTEX_SAME_FORMAT(R10G10B10A2_UINT);
DXTEX_SAME_FORMAT(R8G8B8A8_TYPELESS); DXTEX_SAME_FORMAT(R8G8B8A8_UNORM); DXTEX_SAME_FORMAT(R8G8B8A8_UNORM_SRGB); DXTEX_SAME_FORMAT(R8G8B8A8_UINT);
DXTEX_SAME_FORMAT(R8G8B8A8_SNORM); DXTEX_SAME_FORMAT(R8G8B8A8_SINT);
DXTEX_SAME_FORMAT(R32_FLOAT); DXTEX_SAME_FORMAT(R16_FLOAT); DXTEX_SAME_FORMAT(R16_UNORM); DXTEX_SAME_FORMAT(R8_UNORM); DXTEX_SAME_FORMAT(A8_UNORM);
DXTEX_SAME_FORMAT(B5G6R5_UNORM); DXTEX_SAME_FORMAT(B5G5R5A1_UNORM); DXTEX_SAME_FORMAT(B8G8R8A8_UNORM); DXTEX_SAME_FORMAT(B8G8R8X8_UNORM);
DXTEX_SAME_FORMAT(R10G10B10_XR_BIAS_A2_UNORM); DXTEX_SAME_FORMAT(B8G8R8A8_TYPELESS); DXTEX_SAME_FORMAT(B8G8R8A8_UNORM_SRGB);
DXTEX_SAME_FORMAT(B8G8R8X8_TYPELESS); DXTEX_SAME_FORMAT(B8G8R8X8_UNORM_SRGB);
DXTEX_SAME_FORMAT(AYUV); DXTEX_SAME_FORMAT(Y410); DXTEX_SAME_FORMAT(Y416); DXTEX_SAME_FORMAT(YUY2); DXTEX_SAME_FORMAT(B4G4R4A4_UNORM); DXTEX_SAME_FORMAT(A4B4G4R4_UNORM);
static_assert(int(XBOX_DXGI_FORMAT_R10G10B10_7E3_A2_FLOAT) == int(dxtex::FMT_R10G10B10_7E3_A2_FLOAT) && int(XBOX_DXGI_FORMAT_R10G10B10_6E4_A2_FLOAT) == int(dxtex::FMT_R10G10B10_6E4_A2_FLOAT) &&
              int(XBOX_DXGI_FORMAT_R10G10B10_SNORM_A2_UNORM) == int(dxtex::FMT_R10G10B10_SNORM_A2_UNORM), "the console formats are not their FMT_ twins");
#undef DXTEX_SAME_FORMAT

namespace
{
    // The whole file, which has at least `minimum` bytes and at most 4 GiB - 1: E_FAIL for a file that cannot be opened, sized or read
    // or that is shorter, HRESULT_E_FILE_TOO_LARGE, or what Blob::Initialize answers
    inline HRESULT ReadAll(const char* szFile, Blob& buf, size_t minimum) noexcept
    {
        FILE* f = std::fopen(szFile, "rb");
        if (!f) return E_FAIL;
        std::fseek(f, 0, SEEK_END); const long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
        if (n < 0) { std::fclose(f); return E_FAIL; }
        if (uint64_t(n) > UINT32_MAX) { std::fclose(f); return HRESULT_E_FILE_TOO_LARGE; }
        if (size_t(n) < minimum) { std::fclose(f); return E_FAIL; }
        const HRESULT hr = buf.Initialize(size_t(n));
        if (FAILED(hr)) { std::fclose(f); return hr; }
        const size_t got = std::fread(buf.GetBufferPointer(), 1, buf.GetBufferSize(), f);
        std::fclose(f);
        return got == buf.GetBufferSize() ? S_OK : E_FAIL;
    }

    inline HRESULT WriteBlob(const Blob& blob, const char* szFile) noexcept
    {
        FILE* f = std::fopen(szFile, "wb");
        if (!f) return E_FAIL;
        const size_t n = std::fwrite(blob.GetBufferPointer(), 1, blob.GetBufferSize(), f);
        const bool closed = std::fclose(f) == 0;
        if (n != blob.GetBufferSize() || !closed) { std::remove(szFile); return E_FAIL; }         // no partial files left behind
        return S_OK;
    }

    // "read the file, then the Memory form", the file twin of every loader: E_INVALIDARG for a null name, then `read`'s answer (ReadAll's
    // with `minimum`, or a codec's own reader), then load(bytes, size)'s. A Raw loader passes its result's storage as `keep`: where that
    // holds no bytes of its own after a load, the payload points into the file, and the storage takes the file's bytes over.
    template<class Load>
    inline HRESULT LoadFile(const char* szFile, HRESULT (*read)(const char*, Blob&) noexcept, Load&& load, Blob* keep = nullptr) noexcept
    {
        if (!szFile) return E_INVALIDARG;
        Blob file;
        HRESULT hr = read(szFile, file);
        if (SUCCEEDED(hr)) hr = load(file.GetBufferPointer(), file.GetBufferSize());
        if (SUCCEEDED(hr) && keep && !keep->GetBufferPointer()) keep->Swap(file);
        return hr;
    }
    template<size_t minimum>
    inline HRESULT ReadAtLeast(const char* szFile, Blob& buf) noexcept { return ReadAll(szFile, buf, minimum); }

    // "the Memory form, then WriteBlob", the file twin of every saver: E_INVALIDARG for a null name, then save(blob)'s answer, then WriteBlob's
    template<class Save>
    inline HRESULT SaveFile(const char* szFile, Save&& save) noexcept
    {
        if (!szFile) return E_INVALIDARG;
        Blob blob;
        const HRESULT hr = save(blob);
        return FAILED(hr) ? hr : WriteBlob(blob, szFile);
    }

    // an Image as the C ABI takes it
    inline dxtex_image ImageOf(const Image& i) noexcept { return dxtex_image{ i.width, i.height, int32_t(i.format), i.rowPitch, i.slicePitch, i.pixels }; }

    // device memory of the Device's context, freed on scope exit (the free waits for the work queued on it)
    struct DeviceTemp
    {
        Device& device; void* p = nullptr;
        explicit DeviceTemp(Device& d) noexcept : device(d) {}
        ~DeviceTemp() { if (p) dxtex_device_free(device.Get(), p); }
        DeviceTemp(const DeviceTemp&) = delete;
        DeviceTemp& operator=(const DeviceTemp&) = delete;
    };

    // The frame of a resident save: `bytes` of device memory for the scope of the call, pack(p) leaves the file's side there, and one
    // download brings it to `dst` and returns when it has landed
    template<class Pack>
    inline HRESULT PackAndDownload(Device& device, size_t bytes, void* dst, Pack&& pack) noexcept
    {
        DeviceTemp temp(device);
        HRESULT hr = dxtex_device_alloc(device.Get(), bytes, &temp.p);
        if (SUCCEEDED(hr)) hr = pack(temp.p);
        if (SUCCEEDED(hr)) hr = dxtex_memcpy_d2h(device.Get(), dst, temp.p, bytes);
        return hr;
    }

    // The frame of a resident load, behind the caller's own checks (and its image.Release() before them): the device image for `metadata`,
    // then fill(img) writes its one Image; any failure leaves `image` empty
    template<class Fill>
    inline HRESULT InitializeAndFill(Device& device, const TexMetadata& metadata, DeviceScratchImage& image, Fill&& fill) noexcept
    {
        HRESULT hr = image.Initialize(device, metadata);
        if (FAILED(hr)) return hr;
        const Image* img = image.GetImage(0, 0, 0);
        hr = img ? fill(*img) : E_POINTER;
        if (FAILED(hr)) image.Release();
        return hr;
    }

    // fill's usual body: `bytes` of the file's side go up to the start of an allocation of their own - aligned whatever the header's
    // length - with a copy that returns when the caller's bytes are free to go, then unpack(p) runs the kernels from there
    template<class Unpack>
    inline HRESULT UploadAndUnpack(Device& device, const void* src, size_t bytes, Unpack&& unpack) noexcept
    {
        DeviceTemp temp(device);
        HRESULT hr = dxtex_device_alloc(device.Get(), bytes, &temp.p);
        if (SUCCEEDED(hr)) hr = dxtex_memcpy_h2d(device.Get(), temp.p, src, bytes);
        if (SUCCEEDED(hr)) hr = unpack(temp.p);
        return hr;
    }
}
} // namespace DirectXTexAMD
