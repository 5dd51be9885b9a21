// What the file codecs of the host layer share (DirectXTexAMD_DDS / _HDR / _TGA / _PNM / _PNG.cpp): a whole file into a Blob, a Blob into a
// file, and device memory that lives as long as a scope. Not part of the public interface. Header-only, and every definition has internal
// linkage: a translation unit compiled on its own, as the sanitised test programs compile one codec each, calls its own copy.
#pragma once
#include "DirectXTexAMD.h"
#include "../../include/dxtex_amd.h"

#include <cstdio>

namespace DirectXTexAMD
{
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

    // device memory of the Device's context, freed on scope exit (the free waits for the work queued on it)
    struct DeviceTemp
    {
        Device& device; void* p = nullptr;
        explicit DeviceTemp(Device& d) noexcept : device(d) {}
        ~DeviceTemp() { if (p) dxtex_device_free(device.Get(), p); }
        DeviceTemp(const DeviceTemp&) = delete;
        DeviceTemp& operator=(const DeviceTemp&) = delete;
    };
}
} // namespace DirectXTexAMD
