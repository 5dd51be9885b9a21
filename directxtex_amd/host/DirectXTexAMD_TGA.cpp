// Truevision TGA reader / writer of the host layer. Behaviour follows DirectXTexTGA.cpp: which headers are accepted and the error
// code for each that is not (DecodeTGAHeader, :110-258); 8-bit grey, 16-bit 5:5:5:1, 24- and 32-bit true colour, raw or run-length
// encoded, and 8-bit colour-mapped with a 24-bit palette (:381-1180), either row order, either column order; the all-zero /
// all-opaque alpha rules; the TGA 2.0 extension area for the alpha mode and gamma -> sRGB (:1381-1440); on output the header choice
// per format, 24-bit rows for B8G8R8X8, the extension area and footer (:1183-1380, :2249-2330). One routine handles every texel
// size here where the reference has a copy per format; tests/test_hdr_tga_cpu.py checks files, pixels, metadata and HRESULTs
// against the reference's own codec (oracle/_ref), including truncated and mutated files. Host code.
// The reader is split in two. LoadFromTGAMemoryRaw does what is byte-serial - header, palette, extension area, undoing the run-length
// packets - and hands back the texels as the file orders them, B bytes each. What happens to a texel after that is dxtex_tga.h's, which
// the GPU kernels share: the host loader runs it here, the resident forms at the end of this file run it on the device, so that a file's
// texels cross PCIe as the bytes they are. The writer is split the same way around its rows.
#include "DirectXTexAMD_Internal.h"
#include "../csrc/dxtex_tga.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <new>
#include <vector>

namespace DirectXTexAMD
{
namespace
{
    const char kSignature[] = "TRUEVISION-XFILE.";            // 18 bytes with its NUL, as the footer stores it
    enum : uint8_t { IMG_NONE = 0, IMG_MAPPED = 1, IMG_TRUECOLOR = 2, IMG_GREY = 3, IMG_MAPPED_RLE = 9, IMG_TRUECOLOR_RLE = 10, IMG_GREY_RLE = 11 };
    enum : uint8_t { DESC_INVERTX = 0x10, DESC_INVERTY = 0x20, DESC_INTERLEAVED = 0xC0 };
    enum : uint8_t { ATTR_NONE = 0, ATTR_IGNORED = 1, ATTR_UNDEFINED = 2, ATTR_ALPHA = 3, ATTR_PREMULTIPLIED = 4 };
    constexpr size_t kHeaderLen = 18, kFooterLen = 26, kExtensionLen = 495;
    // offsets inside the extension area (TGA 2.0): size, time stamp, software id + version, gamma, attributes type
    constexpr size_t EXT_STAMP = 367, EXT_SOFTWARE = 426, EXT_VERSION = 467, EXT_VERSION_LETTER = 469, EXT_GAMMA = 478, EXT_ATTRIBUTES = 494;

    struct Header { uint8_t idLength, colorMapType, imageType; uint16_t colorMapFirst, colorMapLength; uint8_t colorMapSize; uint16_t width, height; uint8_t bitsPerPixel, descriptor; };
    inline uint16_t rd16(const uint8_t* p) noexcept { return uint16_t(p[0] | (p[1] << 8)); }
    inline uint32_t rd32(const uint8_t* p) noexcept { uint32_t v; std::memcpy(&v, p, 4); return v; }
    inline void wr16(uint8_t* p, uint32_t v) noexcept { p[0] = uint8_t(v); p[1] = uint8_t(v >> 8); }
    Header ParseHeader(const uint8_t* p) noexcept
    {
        Header h;
        h.idLength = p[0]; h.colorMapType = p[1]; h.imageType = p[2]; h.colorMapFirst = rd16(p + 3); h.colorMapLength = rd16(p + 5); h.colorMapSize = p[7];
        h.width = rd16(p + 12); h.height = rd16(p + 14); h.bitsPerPixel = p[16]; h.descriptor = p[17];
        return h;
    }

    enum : uint32_t { RD_EXPAND = 0x1, RD_INVERTX = 0x2, RD_INVERTY = 0x4, RD_RLE = 0x8, RD_PALETTED = 0x10 };

    HRESULT DecodeHeader(const uint8_t* pSource, size_t size, uint32_t flags, TexMetadata& metadata, size_t& offset, uint32_t* how) noexcept
    {
        if (!pSource) return E_POINTER;
        metadata = TexMetadata();
        metadata.dimension = TEX_DIMENSION(0);
        if (size < kHeaderLen) return HRESULT_E_INVALID_DATA;
        const Header h = ParseHeader(pSource);
        if (h.descriptor & DESC_INTERLEAVED) return HRESULT_E_NOT_SUPPORTED;
        if (!h.width || !h.height) return HRESULT_E_INVALID_DATA;
        const bool bgr = (flags & TGA_FLAGS_BGR) != 0;
        auto rgb24 = [&]()        // a 24-bit colour lands in RGBA8 (opaque) or, on request, stays BGR in B8G8R8X8
        {
            if (bgr) metadata.format = DXGI_FORMAT_B8G8R8X8_UNORM;
            else { metadata.format = DXGI_FORMAT_R8G8B8A8_UNORM; metadata.SetAlphaMode(TEX_ALPHA_MODE_OPAQUE); }
        };
        switch (h.imageType)
        {
        case IMG_NONE: case IMG_MAPPED_RLE:
            return HRESULT_E_NOT_SUPPORTED;
        case IMG_MAPPED:
            if (h.colorMapType != 1 || h.colorMapLength == 0 || h.bitsPerPixel != 8 || h.colorMapSize != 24) return HRESULT_E_NOT_SUPPORTED;
            rgb24();
            if (how) *how |= RD_PALETTED;
            break;
        case IMG_TRUECOLOR: case IMG_TRUECOLOR_RLE:
            if (h.colorMapType != 0 || h.colorMapLength != 0) return HRESULT_E_NOT_SUPPORTED;
            switch (h.bitsPerPixel)
            {
            case 16: metadata.format = DXGI_FORMAT_B5G5R5A1_UNORM; break;
            case 24: rgb24(); if (how) *how |= RD_EXPAND; break;
            case 32: metadata.format = bgr ? DXGI_FORMAT_B8G8R8A8_UNORM : DXGI_FORMAT_R8G8B8A8_UNORM; break;
            default: return HRESULT_E_NOT_SUPPORTED;
            }
            if (how && h.imageType == IMG_TRUECOLOR_RLE) *how |= RD_RLE;
            break;
        case IMG_GREY: case IMG_GREY_RLE:
            if (h.colorMapType != 0 || h.colorMapLength != 0 || h.bitsPerPixel != 8) return HRESULT_E_NOT_SUPPORTED;
            metadata.format = DXGI_FORMAT_R8_UNORM;
            if (how && h.imageType == IMG_GREY_RLE) *how |= RD_RLE;
            break;
        default:
            return HRESULT_E_INVALID_DATA;
        }
        if (uint64_t(h.width) * uint64_t(h.height) * uint64_t(h.bitsPerPixel) / 8 > UINT32_MAX) return HRESULT_E_ARITHMETIC_OVERFLOW;
        metadata.width = h.width; metadata.height = h.height;
        metadata.depth = metadata.arraySize = metadata.mipLevels = 1;
        metadata.dimension = TEX_DIMENSION_TEXTURE2D;
        if (how)
        {
            if (h.descriptor & DESC_INVERTX) *how |= RD_INVERTX;
            if (h.descriptor & DESC_INVERTY) *how |= RD_INVERTY;
        }
        offset = kHeaderLen + h.idLength;
        return S_OK;
    }

    // the 24-bit colour map as RGBA / BGRA words; entries outside [first, first + length) stay zero (ReadPalette, :260-310)
    HRESULT ReadPalette(const Header& h, const uint8_t* bytes, size_t size, uint32_t flags, uint32_t palette[256], size_t& mapBytes) noexcept
    {
        if (h.colorMapType != 1 || h.colorMapLength == 0 || h.colorMapLength > 256 || h.colorMapSize != 24) return HRESULT_E_NOT_SUPPORTED;
        const size_t last = size_t(h.colorMapFirst) + h.colorMapLength;
        if (last > 256) return HRESULT_E_NOT_SUPPORTED;
        mapBytes = size_t(h.colorMapLength) * 3;
        if (mapBytes > size) return HRESULT_E_INVALID_DATA;
        for (size_t i = h.colorMapFirst; i < last; ++i, bytes += 3)
            palette[i] = (flags & TGA_FLAGS_BGR) ? (uint32_t(bytes[0]) | (uint32_t(bytes[1]) << 8) | (uint32_t(bytes[2]) << 16) | 0xFF000000u)
                                                 : (uint32_t(bytes[2]) | (uint32_t(bytes[1]) << 8) | (uint32_t(bytes[0]) << 16) | 0xFF000000u);
        return S_OK;
    }

    // which of dxtex_tga.h's kinds a file is (its reader's table): every (format, bytes, colour-mapped) DecodeHeader gives is in it
    int KindOf(const TGARawImage& raw) noexcept { return dxtex::tga_unpack_kind(int(raw.format), raw.bytesPerTexel, raw.paletted); }

    // UncompressPixels' packets (:381-737) undone into file-order texels of B bytes. Packets do not cross rows; any truncation is E_FAIL.
    HRESULT ExpandPackets(const uint8_t* s, size_t size, size_t width, size_t height, size_t B, uint8_t* d) noexcept
    {
        const uint8_t* end = s + size;
        for (size_t y = 0; y < height; ++y)
            for (size_t x = 0; x < width;)
            {
                if (s >= end) return E_FAIL;
                const size_t n = size_t(*s & 0x7F) + 1;
                const bool run = (*s & 0x80) != 0;
                ++s;
                if (size_t(end - s) < (run ? B : n * B) || n > width - x) return E_FAIL;
                if (run) { for (size_t i = 0; i < n; ++i, d += B) std::memcpy(d, s, B); s += B; }
                else { std::memcpy(d, s, n * B); s += n * B; d += n * B; }
                x += n;
            }
        return S_OK;
    }

    // the extension area the footer points at, if the file has a TGA 2.0 footer and the area lies inside the file
    const uint8_t* FindExtension(const uint8_t* p, size_t size) noexcept
    {
        if (size < kFooterLen) return nullptr;
        const uint8_t* footer = p + size - kFooterLen;
        if (std::memcmp(footer + 8, kSignature, sizeof(kSignature)) != 0) return nullptr;
        const uint32_t at = rd32(footer);
        if (at == 0 || size_t(at) + kExtensionLen > size) return nullptr;
        return p + at;
    }

    TEX_ALPHA_MODE AlphaModeOf(const uint8_t* ext) noexcept
    {
        if (!ext || rd16(ext) != kExtensionLen) return TEX_ALPHA_MODE_UNKNOWN;
        switch (ext[EXT_ATTRIBUTES])
        {
        case ATTR_IGNORED: return TEX_ALPHA_MODE_OPAQUE;
        case ATTR_UNDEFINED: return TEX_ALPHA_MODE_CUSTOM;
        case ATTR_ALPHA: return TEX_ALPHA_MODE_STRAIGHT;
        case ATTR_PREMULTIPLIED: return TEX_ALPHA_MODE_PREMULTIPLIED;
        default: return TEX_ALPHA_MODE_UNKNOWN;
        }
    }

    // a gamma of 2.2 or 2.4 in the extension area means sRGB; with no usable gamma the caller's default decides (:1409-1440)
    DXGI_FORMAT ApplyGamma(const uint8_t* ext, DXGI_FORMAT format, uint32_t flags, ScratchImage* image) noexcept
    {
        bool srgb;
        if (ext && rd16(ext) == kExtensionLen && rd16(ext + EXT_GAMMA + 2) != 0)
        {
            const float gamma = float(rd16(ext + EXT_GAMMA)) / float(rd16(ext + EXT_GAMMA + 2));
            srgb = std::fabs(gamma - 2.2f) < 0.01f || std::fabs(gamma - 2.4f) < 0.01f;
        }
        else srgb = (flags & TGA_FLAGS_DEFAULT_SRGB) != 0;
        if (srgb)
        {
            format = MakeSRGB(format);
            if (image) image->OverrideFormat(format);
        }
        return format;
    }
}

HRESULT GetMetadataFromTGAMemory(const void* pSource, size_t size, TGA_FLAGS flags, TexMetadata& metadata) noexcept
{
    if (!pSource || size == 0) return E_INVALIDARG;
    const uint8_t* p = static_cast<const uint8_t*>(pSource);
    size_t offset;
    const HRESULT hr = DecodeHeader(p, size, flags, metadata, offset, nullptr);
    if (FAILED(hr)) return hr;
    const uint8_t* ext = FindExtension(p, size);
    if (ext) metadata.SetAlphaMode(AlphaModeOf(ext));
    if (!(flags & TGA_FLAGS_IGNORE_SRGB)) metadata.format = ApplyGamma(ext, metadata.format, flags, nullptr);
    return S_OK;
}

HRESULT GetMetadataFromTGAFile(const char* szFile, TGA_FLAGS flags, TexMetadata& metadata) noexcept
{
    return LoadFile(szFile, ReadAtLeast<kHeaderLen>, [&](const uint8_t* p, size_t n) { return GetMetadataFromTGAMemory(p, n, flags, metadata); });
}

// LoadFromTGAMemory's byte-serial half (DirectXTexTGA.cpp:1640-1745 around CopyPixels): header, palette, extension area, the size check of a
// raw file, the packets of a run-length one
HRESULT LoadFromTGAMemoryRaw(const void* pSource, size_t size, TGA_FLAGS flags, TexMetadata* metadata, TGARawImage& raw) noexcept
{
    raw.Release();          // on any failure the result is empty
    if (!pSource || size == 0) return E_INVALIDARG;
    const uint8_t* p = static_cast<const uint8_t*>(pSource);
    size_t offset; uint32_t how = 0;
    TexMetadata mdata;
    HRESULT hr = DecodeHeader(p, size, flags, mdata, offset, &how);
    if (FAILED(hr)) return hr;
    if (offset > size) return HRESULT_E_INVALID_DATA;
    size_t mapBytes = 0;
    if (how & RD_PALETTED)
    {
        if (size - offset == 0) return E_FAIL;
        hr = ReadPalette(ParseHeader(p), p + offset, size - offset, flags, raw.palette, mapBytes);
        if (FAILED(hr)) { raw.Release(); return hr; }
    }
    const size_t remaining = size - offset - mapBytes;
    if (remaining == 0) { raw.Release(); return HRESULT_E_HANDLE_EOF; }
    const size_t B = (how & RD_PALETTED) ? 1 : ParseHeader(p).bitsPerPixel / 8, texels = mdata.width * mdata.height;
    const uint8_t* s = p + offset + mapBytes;
    if (!(how & RD_RLE))
    {
        if (remaining < texels * B) { raw.Release(); return E_FAIL; }
        raw.texels = s;
    }
    else
    {
        // a packet of 1 + B bytes or more holds 128 texels at the most: a file too short for its size fails before anything is allocated
        if ((remaining / (1 + B) + 1) * 128 < texels) { raw.Release(); return E_FAIL; }
        hr = raw.storage.Initialize(texels * B);
        if (SUCCEEDED(hr)) hr = ExpandPackets(s, remaining, mdata.width, mdata.height, B, raw.storage.GetBufferPointer());
        if (FAILED(hr)) { raw.Release(); return hr; }
        raw.texels = raw.storage.GetBufferPointer();
    }
    raw.texelBytes = texels * B;
    raw.bytesPerTexel = uint32_t(B);
    raw.format = mdata.format;
    raw.paletted = (how & RD_PALETTED) != 0;
    raw.rightToLeft = (how & RD_INVERTX) != 0;
    raw.topDown = (how & RD_INVERTY) != 0;
    const uint8_t* ext = FindExtension(p, size);
    if (!(flags & TGA_FLAGS_IGNORE_SRGB)) mdata.format = ApplyGamma(ext, mdata.format, flags, nullptr);
    if (ext) mdata.SetAlphaMode(AlphaModeOf(ext));
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromTGAFileRaw(const char* szFile, TGA_FLAGS flags, TexMetadata* metadata, TGARawImage& raw) noexcept
{
    raw.Release();
    // a file without packets: the texels lie inside it, and raw keeps it
    return LoadFile(szFile, ReadAtLeast<kHeaderLen>, [&](const uint8_t* p, size_t n) { return LoadFromTGAMemoryRaw(p, n, flags, metadata, raw); }, &raw.storage);
}

// LoadFromTGAMemory (DirectXTexTGA.cpp:1640-1745)
HRESULT LoadFromTGAMemory(const void* pSource, size_t size, TGA_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept
{
    if (!pSource || size == 0) return E_INVALIDARG;
    image.Release();
    TexMetadata mdata; TGARawImage raw;
    HRESULT hr = LoadFromTGAMemoryRaw(pSource, size, flags, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = image.Initialize2D(raw.format, mdata.width, mdata.height, 1, 1);
    if (FAILED(hr)) return hr;
    const Image* img = image.GetImage(0, 0, 0);
    if (!img) { image.Release(); return E_POINTER; }
    // CopyPixels' texel half (:738-1180): the file's first row is the image's bottom row unless the descriptor says top-down; right-to-left likewise
    const int kind = KindOf(raw);
    const size_t B = raw.bytesPerTexel, D = dxtex::tga_image_bytes(kind);
    uint32_t orAlpha = 0, orNotAlpha = 0;
    const uint8_t* s = raw.texels;
    for (size_t y = 0; y < img->height; ++y)
    {
        uint8_t* row = img->pixels + img->rowPitch * (raw.topDown ? y : img->height - y - 1);
        for (size_t x = 0; x < img->width; ++x, s += B)
        {
            uint32_t alpha;
            const uint32_t t = dxtex::tga_unpack_texel(dxtex::le_load32(s, uint32_t(B)), kind, raw.palette, alpha);
            dxtex::le_store32(row + (raw.rightToLeft ? img->width - 1 - x : x) * D, t, uint32_t(D));
            orAlpha |= alpha; orNotAlpha |= alpha ^ 255u;
        }
    }
    bool opaque = kind == dxtex::TGA_RGB_RGBA;
    if (dxtex::tga_has_alpha_rule(kind))
    {
        bool makeOpaque;
        opaque = dxtex::tga_alpha_answer(orAlpha, orNotAlpha, (flags & TGA_FLAGS_ALLOW_ALL_ZERO_ALPHA) != 0, makeOpaque) != 0;
        if (makeOpaque)          // an alpha channel that is zero everywhere was not meant
            for (size_t y = 0; y < img->height; ++y)
            {
                uint8_t* top = img->pixels + y * img->rowPitch + (D - 1);
                for (size_t x = 0; x < img->width; ++x, top += D) *top = D == 2 ? uint8_t(*top | 0x80) : uint8_t(0xFF);
            }
    }
    image.OverrideFormat(mdata.format);
    if (opaque) mdata.SetAlphaMode(TEX_ALPHA_MODE_OPAQUE);
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromTGAFile(const char* szFile, TGA_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept
{
    if (szFile) image.Release();
    return LoadFile(szFile, ReadAtLeast<kHeaderLen>, [&](const uint8_t* p, size_t n) { return LoadFromTGAMemory(p, n, flags, metadata, image); });
}

namespace
{
    // SaveToTGAMemory's checks and header choice per format (DirectXTexTGA.cpp:1183-1287, :2249-2275)
    struct FileShape { uint8_t type, bits, descriptor; int row; };
    HRESULT SaveChecks(const Image& image, TGA_FLAGS flags, const TexMetadata* metadata, FileShape& f) noexcept
    {
        if ((flags & (TGA_FLAGS_FORCE_LINEAR | TGA_FLAGS_FORCE_SRGB)) != 0 && !metadata) return E_INVALIDARG;
        if (!image.pixels) return E_POINTER;
        if (image.width > UINT16_MAX || image.height > UINT16_MAX) return HRESULT_E_NOT_SUPPORTED;
        // the writer's table: a byte is grey, anything wider true colour; the descriptor's low bits count the alpha bits - 8 of 32, 1 of 16
        const dxtex::TgaPackRow r = dxtex::tga_pack_row(int(image.format));
        const uint32_t B = r.bytesPerTexel;
        if (!B) return HRESULT_E_NOT_SUPPORTED;
        f = { uint8_t(B == 1 ? IMG_GREY : IMG_TRUECOLOR), uint8_t(B * 8), uint8_t(DESC_INVERTY | (B == 4 ? 8 : B == 2 ? 1 : 0)), r.row };
        return S_OK;
    }

    // The file around the texels: the 18-byte header, then rows(d) leaves width * height texels of bits / 8 bytes at d, top-down and
    // tight; with metadata the TGA 2.0 extension area follows, and the footer.
    template<class Rows>
    HRESULT WriteFile(const Image& image, const FileShape& f, TGA_FLAGS flags, const TexMetadata* metadata, Blob& blob, Rows&& rows) noexcept
    {
        blob.Release();
        const size_t slicePitch = image.width * (f.bits / 8) * image.height;
        HRESULT hr = blob.Initialize(kHeaderLen + slicePitch + (metadata ? kExtensionLen : 0) + kFooterLen);
        if (FAILED(hr)) return hr;
        uint8_t* base = blob.GetBufferPointer();
        std::memset(base, 0, kHeaderLen);
        base[2] = f.type; wr16(base + 12, uint32_t(image.width)); wr16(base + 14, uint32_t(image.height)); base[16] = f.bits; base[17] = f.descriptor;
        hr = rows(base + kHeaderLen);
        if (FAILED(hr)) { blob.Release(); return hr; }
        uint8_t* d = base + kHeaderLen + slicePitch;
        uint32_t extOffset = 0;
        if (metadata)
        {
            // SetExtension (:1322-1380): who wrote it, gamma, what the alpha channel means, when
            std::memset(d, 0, kExtensionLen);
            wr16(d, kExtensionLen);
            std::memcpy(d + EXT_SOFTWARE, "DirectXTex", sizeof("DirectXTex"));
            wr16(d + EXT_VERSION, 211); d[EXT_VERSION_LETTER] = ' ';          // DIRECTX_TEX_VERSION of the reference this mirrors (DirectXTex.h:50)
            const bool srgb = !(flags & TGA_FLAGS_FORCE_LINEAR) && ((flags & TGA_FLAGS_FORCE_SRGB) || IsSRGB(metadata->format));
            if (srgb) { wr16(d + EXT_GAMMA, 22); wr16(d + EXT_GAMMA + 2, 10); }
            else if (flags & TGA_FLAGS_FORCE_LINEAR) { wr16(d + EXT_GAMMA, 1); wr16(d + EXT_GAMMA + 2, 1); }
            switch (metadata->GetAlphaMode())
            {
            case TEX_ALPHA_MODE_STRAIGHT: d[EXT_ATTRIBUTES] = ATTR_ALPHA; break;
            case TEX_ALPHA_MODE_PREMULTIPLIED: d[EXT_ATTRIBUTES] = ATTR_PREMULTIPLIED; break;
            case TEX_ALPHA_MODE_OPAQUE: d[EXT_ATTRIBUTES] = ATTR_IGNORED; break;
            case TEX_ALPHA_MODE_CUSTOM: d[EXT_ATTRIBUTES] = ATTR_UNDEFINED; break;
            default: d[EXT_ATTRIBUTES] = HasAlpha(metadata->format) ? ATTR_UNDEFINED : ATTR_NONE; break;
            }
            std::time_t now = {};
            std::time(&now);
            if (const std::tm* t = std::gmtime(&now))
            {
                wr16(d + EXT_STAMP, uint32_t(t->tm_mon + 1)); wr16(d + EXT_STAMP + 2, uint32_t(t->tm_mday)); wr16(d + EXT_STAMP + 4, uint32_t(t->tm_year + 1900));
                wr16(d + EXT_STAMP + 6, uint32_t(t->tm_hour)); wr16(d + EXT_STAMP + 8, uint32_t(t->tm_min)); wr16(d + EXT_STAMP + 10, uint32_t(t->tm_sec));
            }
            extOffset = uint32_t(d - base);
            d += kExtensionLen;
        }
        std::memcpy(d, &extOffset, 4);
        std::memset(d + 4, 0, 4);
        std::memcpy(d + 8, kSignature, sizeof(kSignature));
        return S_OK;
    }
}

// SaveToTGAMemory (DirectXTexTGA.cpp:2249-2330): uncompressed, top-down; with metadata a TGA 2.0 extension area is added
HRESULT SaveToTGAMemory(const Image& image, TGA_FLAGS flags, Blob& blob, const TexMetadata* metadata) noexcept
{
    FileShape f;
    const HRESULT hr = SaveChecks(image, flags, metadata, f);
    if (FAILED(hr)) return hr;
    const size_t B = f.bits / 8, D = f.row == dxtex::TGA_ROW_DROP_X ? 4 : B;
    return WriteFile(image, f, flags, metadata, blob, [&](uint8_t* d)
    {
        for (size_t y = 0; y < image.height; ++y)
        {
            const uint8_t* s = image.pixels + y * image.rowPitch;
            for (size_t x = 0; x < image.width && x * D + (D - 1) < image.rowPitch; ++x)          // a pitch below the row leaves the rest of it as allocated
                dxtex::le_store32(d + x * B, dxtex::tga_pack_texel(dxtex::le_load32(s + x * D, uint32_t(D)), f.row), uint32_t(B));
            d += image.width * B;
        }
        return S_OK;
    });
}

HRESULT SaveToTGAFile(const Image& image, TGA_FLAGS flags, const char* szFile, const TexMetadata* metadata) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveToTGAMemory(image, flags, blob, metadata); });
}

// ---- resident forms: the texels travel as the file has them, the per-texel pass runs on the device (dxtex_tga_unpack_device / dxtex_tga_pack_device) ----
void TGARawImage::Release() noexcept
{
    storage.Release();
    std::memset(palette, 0, sizeof(palette));
    texels = nullptr; texelBytes = 0; bytesPerTexel = 0; format = DXGI_FORMAT_UNKNOWN;
    paletted = rightToLeft = topDown = false;
}

void ApplyTGAAlphaRule(const TGARawImage& raw, TGA_FLAGS flags, TexMetadata& metadata) noexcept
{
    const int kind = KindOf(raw);
    bool opaque = kind == dxtex::TGA_RGB_RGBA;
    if (dxtex::tga_has_alpha_rule(kind) && raw.texels)
    {
        // the texel's top byte holds alpha (its top bit, for 5:5:5:1)
        const uint32_t B = raw.bytesPerTexel, mask = B == 2 ? 0x80u : 0xFFu;
        uint32_t orAlpha = 0, orNotAlpha = 0;
        for (const uint8_t* top = raw.texels + (B - 1), *end = raw.texels + raw.texelBytes; top < end; top += B) { orAlpha |= *top & mask; orNotAlpha |= ~*top & mask; }
        bool makeOpaque;
        opaque = dxtex::tga_alpha_answer(orAlpha, orNotAlpha, (flags & TGA_FLAGS_ALLOW_ALL_ZERO_ALPHA) != 0, makeOpaque) != 0;
    }
    if (opaque) metadata.SetAlphaMode(TEX_ALPHA_MODE_OPAQUE);
}

HRESULT UploadTGARaw(Device& device, TexMetadata& metadata, TGA_FLAGS flags, const TGARawImage& raw, DeviceScratchImage& image) noexcept
{
    image.Release();
    if (!device) return E_POINTER;
    if (!raw.texels || metadata.arraySize != 1 || metadata.mipLevels != 1 || metadata.depth != 1 ||
        raw.texelBytes != metadata.width * metadata.height * raw.bytesPerTexel) return E_INVALIDARG;
    TexMetadata plain = metadata;          // the image as ScratchImage::Initialize2D would describe it; the sRGB relabel follows the pixels
    plain.format = raw.format; plain.miscFlags = 0; plain.miscFlags2 = 0;
    const int kind = KindOf(raw);
    const bool rule = dxtex::tga_has_alpha_rule(kind);
    uint32_t opaque = kind == dxtex::TGA_RGB_RGBA ? 1u : 0u;
    const HRESULT hr = InitializeAndFill(device, plain, image, [&](const Image& img)
    {
        // the stream, and behind it (on a dword) the alpha answer
        const size_t answerAt = (raw.texelBytes + 3) & ~size_t(3);
        DeviceTemp temp(device);
        HRESULT hr2 = dxtex_device_alloc(device.Get(), answerAt + 4, &temp.p);
        // with an alpha rule the read-back of the answer below is the one wait, and the stream's copy has happened by then; without one the
        // synchronous copy is: the host texels are free to go when this returns
        if (SUCCEEDED(hr2)) hr2 = rule ? dxtex_memcpy_h2d_async(device.Get(), temp.p, raw.texels, raw.texelBytes) : dxtex_memcpy_h2d(device.Get(), temp.p, raw.texels, raw.texelBytes);
        if (FAILED(hr2)) return hr2;
        const uint32_t how = (raw.rightToLeft ? DXTEX_TGA_RIGHT_TO_LEFT : 0u) | (raw.topDown ? DXTEX_TGA_TOP_DOWN : 0u) |
                             ((flags & TGA_FLAGS_ALLOW_ALL_ZERO_ALPHA) ? DXTEX_TGA_ALLOW_ALL_ZERO_ALPHA : 0u);
        const dxtex_image d = ImageOf(img);
        uint32_t* answer = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(temp.p) + answerAt);
        hr2 = dxtex_tga_unpack_device(device.Get(), temp.p, raw.texelBytes, raw.bytesPerTexel, how, raw.paletted ? raw.palette : nullptr, &d, rule ? answer : nullptr);
        if (rule)
        {
            // queued or not, the stream's copy reads the caller's texels: wait for it either way
            const HRESULT waited = dxtex_memcpy_d2h(device.Get(), &opaque, answer, sizeof(opaque));
            if (SUCCEEDED(hr2)) hr2 = waited;
        }
        return hr2;
    });
    if (FAILED(hr)) return hr;
    image.OverrideFormat(metadata.format);
    if (opaque) metadata.SetAlphaMode(TEX_ALPHA_MODE_OPAQUE);
    return S_OK;
}

HRESULT LoadFromTGAMemory(Device& device, const void* pSource, size_t size, TGA_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();          // on any failure the result is empty
    if (!pSource || size == 0) return E_INVALIDARG;
    TexMetadata mdata; TGARawImage raw;
    HRESULT hr = LoadFromTGAMemoryRaw(pSource, size, flags, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = UploadTGARaw(device, mdata, flags, raw, image);
    if (FAILED(hr)) return hr;
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromTGAFile(Device& device, const char* szFile, TGA_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();
    return LoadFile(szFile, ReadAtLeast<kHeaderLen>, [&](const uint8_t* p, size_t n) { return LoadFromTGAMemory(device, p, n, flags, metadata, image); });
}

HRESULT SaveToTGAMemory(Device& device, const Image& deviceImage, TGA_FLAGS flags, Blob& blob, const TexMetadata* metadata) noexcept
{
    FileShape f;
    const HRESULT hr = SaveChecks(deviceImage, flags, metadata, f);
    if (FAILED(hr)) return hr;
    if (!device) return E_POINTER;
    const uint32_t B = f.bits / 8;
    const size_t bytes = deviceImage.width * deviceImage.height * B;
    const dxtex_image s = ImageOf(deviceImage);
    return WriteFile(deviceImage, f, flags, metadata, blob, [&](uint8_t* d)          // the rows land straight behind the header
    { return PackAndDownload(device, bytes, d, [&](void* p) { return dxtex_tga_pack_device(device.Get(), &s, B, p, bytes); }); });
}

HRESULT SaveToTGAFile(Device& device, const Image& deviceImage, TGA_FLAGS flags, const char* szFile, const TexMetadata* metadata) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveToTGAMemory(device, deviceImage, flags, blob, metadata); });
}
} // namespace DirectXTexAMD
