// PNG reader / writer of the host layer. Behaviour follows Auxiliary/DirectXTexPNG.cpp, the reference's codec over libpng; DirectXTexAMD.h
// states the four departures. No library is linked: the chunk walk, CRC-32 and the row filters are below, the inflater and Adler-32 in DirectXTexAMD_Inflate.h. libpng
// is not there to run the reference against, so the yardstick is tests/png_ref.py, a restatement of the rules over Python's zlib.
// The reader is split in two. LoadFromPNGMemoryRaw does what is byte-serial - signature, chunks, inflate, unfilter, every refusal - and
// hands back the unfiltered rows and how to read them. What happens to a texel after that is dxtex_png.h's, which the GPU kernels share:
// the host loader runs it here, the resident forms at the end of this file run it on the device, so that a file's rows cross PCIe as the
// bytes they are. The writer is split the same way around its rows.
// Unfiltering stays on the host: Average and Paeth chain every byte to its left neighbour and to the row above, which is one serial walk.
#include "DirectXTexAMD_Internal.h"
#include "DirectXTexAMD_Inflate.h"
#include "../csrc/dxtex_png.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>

namespace DirectXTexAMD
{
namespace
{
    constexpr uint8_t kSignature[8] = { 0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n' };
    constexpr uint32_t kSideLimit = 1000000;          // libpng's default png_set_user_limits
    constexpr size_t kIdatMax = size_t(1) << 24;      // the writer's IDAT payloads: well below 2^31

    inline uint32_t Be32(const uint8_t* p) noexcept { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]; }
    inline void PutBe32(uint8_t* p, uint32_t v) noexcept { p[0] = uint8_t(v >> 24); p[1] = uint8_t(v >> 16); p[2] = uint8_t(v >> 8); p[3] = uint8_t(v); }
    constexpr uint32_t Tag(char a, char b, char c, char d) noexcept { return (uint32_t(uint8_t(a)) << 24) | (uint32_t(uint8_t(b)) << 16) | (uint32_t(uint8_t(c)) << 8) | uint8_t(d); }

    // CRC-32 (ISO 3309, the PNG specification's), eight bytes a step over eight tables
    struct CrcTables
    {
        uint32_t t[8][256];
        CrcTables() noexcept
        {
            for (uint32_t n = 0; n < 256; ++n)
            {
                uint32_t c = n;
                for (int k = 0; k < 8; ++k) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
                t[0][n] = c;
            }
            for (uint32_t n = 0; n < 256; ++n)
                for (int s = 1; s < 8; ++s) t[s][n] = (t[s - 1][n] >> 8) ^ t[0][t[s - 1][n] & 0xFFu];
        }
    };
    const CrcTables& Crc() noexcept { static const CrcTables tables; return tables; }

    uint32_t Crc32(uint32_t crc, const uint8_t* p, size_t n) noexcept          // crc: the running value, 0xffffffff to start, inverted at the end
    {
        const CrcTables& T = Crc();
        while (n >= 8)
        {
            const uint32_t a = crc ^ (uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24));
            crc = T.t[7][a & 0xFFu] ^ T.t[6][(a >> 8) & 0xFFu] ^ T.t[5][(a >> 16) & 0xFFu] ^ T.t[4][a >> 24] ^ T.t[3][p[4]] ^ T.t[2][p[5]] ^ T.t[1][p[6]] ^ T.t[0][p[7]];
            p += 8; n -= 8;
        }
        while (n--) crc = T.t[0][(crc ^ *p++) & 0xFFu] ^ (crc >> 8);
        return crc;
    }

    // ---- the row filters ---------------------------------------------------------------------------------------------------------------
    inline int Paeth(int a, int b, int c) noexcept
    {
        const int p = a + b - c, pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
        return (pa <= pb && pa <= pc) ? a : (pb <= pc) ? b : c;
    }

    // `height` filtered rows of 1 + rowBytes at buf -> tight rows at the front of buf. bpp = max(1, bits per texel / 8); the row above the
    // first reads as zeros. The write position never passes the read position.
    bool Unfilter(uint8_t* buf, size_t height, size_t rowBytes, size_t bpp) noexcept
    {
        const uint8_t* prev = nullptr;
        for (size_t y = 0; y < height; ++y)
        {
            const uint8_t* s = buf + y * (rowBytes + 1);
            uint8_t* d = buf + y * rowBytes;
            const uint8_t f = *s++;
            const size_t head = std::min(bpp, rowBytes);
            switch (f)
            {
            case 0: std::memmove(d, s, rowBytes); break;
            case 1:
                for (size_t i = 0; i < head; ++i) d[i] = s[i];
                for (size_t i = head; i < rowBytes; ++i) d[i] = uint8_t(s[i] + d[i - bpp]);
                break;
            case 2:
                if (!prev) std::memmove(d, s, rowBytes);
                else for (size_t i = 0; i < rowBytes; ++i) d[i] = uint8_t(s[i] + prev[i]);
                break;
            case 3:
                for (size_t i = 0; i < head; ++i) d[i] = uint8_t(s[i] + ((prev ? prev[i] : 0) >> 1));
                for (size_t i = head; i < rowBytes; ++i) d[i] = uint8_t(s[i] + ((d[i - bpp] + (prev ? prev[i] : 0)) >> 1));
                break;
            case 4:
                for (size_t i = 0; i < head; ++i) d[i] = uint8_t(s[i] + (prev ? prev[i] : 0));          // Paeth(0, b, 0) is b
                for (size_t i = head; i < rowBytes; ++i) d[i] = uint8_t(s[i] + Paeth(d[i - bpp], prev ? prev[i] : 0, prev ? prev[i - bpp] : 0));
                break;
            default: return false;
            }
            prev = d;
        }
        return true;
    }

    // ---- the chunks ----------------------------------------------------------------------------------------------------------------------
    struct Header
    {
        uint32_t width = 0, height = 0;
        uint8_t depth = 0, colorType = 0;
        bool hasPalette = false, hasSRGB = false, hasGamma = false, greyKey = false;
        uint32_t gamma = 0;          // times 100000
        uint8_t plte[768] = {}; uint32_t plteCount = 0;
        uint8_t trns[256] = {}; uint32_t trnsCount = 0;
    };

    // a kind per colour type and depth; -1 for a pair the specification does not have
    int KindOf(uint8_t colorType, uint8_t depth) noexcept
    {
        switch (colorType)
        {
        case 0: return depth == 1 ? DXTEX_PNG_G1 : depth == 2 ? DXTEX_PNG_G2 : depth == 4 ? DXTEX_PNG_G4 : depth == 8 ? DXTEX_PNG_G8 : depth == 16 ? int(DXTEX_PNG_G16) : -1;
        case 2: return depth == 8 ? DXTEX_PNG_RGB8 : depth == 16 ? int(DXTEX_PNG_RGB16) : -1;
        case 3: return depth == 1 ? DXTEX_PNG_P1 : depth == 2 ? DXTEX_PNG_P2 : depth == 4 ? DXTEX_PNG_P4 : depth == 8 ? int(DXTEX_PNG_P8) : -1;
        case 4: return depth == 8 ? DXTEX_PNG_GA8 : depth == 16 ? int(DXTEX_PNG_GA16) : -1;
        case 6: return depth == 8 ? DXTEX_PNG_RGBA8 : depth == 16 ? int(DXTEX_PNG_RGBA16) : -1;
        default: return -1;
        }
    }

    // Update's flag change, GuessFormat and GetHeader (:126-251) from what the chunks said
    void FillMetadata(const Header& h, uint32_t flags, TexMetadata& m) noexcept
    {
        m = TexMetadata();
        m.width = h.width; m.height = h.height; m.depth = m.arraySize = m.mipLevels = 1;
        m.dimension = TEX_DIMENSION_TEXTURE2D;
        if (h.colorType == 4) flags |= PNG_FLAGS_IGNORE_SRGB;          // :145
        if (h.colorType == 0) m.format = h.depth == 16 ? DXGI_FORMAT_R16_UNORM : DXGI_FORMAT_R8_UNORM;
        else if (h.depth == 16) m.format = DXGI_FORMAT_R16G16B16A16_UNORM;
        else
        {
            const bool bgr = (flags & PNG_FLAGS_BGR) != 0;
            const DXGI_FORMAT linear = bgr ? DXGI_FORMAT_B8G8R8A8_UNORM : DXGI_FORMAT_R8G8B8A8_UNORM;
            const DXGI_FORMAT srgb = bgr ? DXGI_FORMAT_B8G8R8A8_UNORM_SRGB : DXGI_FORMAT_R8G8B8A8_UNORM_SRGB;
            const int64_t off = int64_t(h.gamma) - 100000;          // |gamma - 1.0| <= 1e-6 in units of 1e-5: the value itself
            if (flags & PNG_FLAGS_IGNORE_SRGB) m.format = linear;
            else if (h.hasSRGB) m.format = srgb;
            else if (h.hasGamma && off == 0) m.format = linear;
            else m.format = (flags & PNG_FLAGS_DEFAULT_LINEAR) ? linear : srgb;
        }
        const bool haveAlpha = (h.colorType & 4) != 0;
        if (!haveAlpha && m.format != DXGI_FORMAT_R8_UNORM && m.format != DXGI_FORMAT_R16_UNORM)
        {
            if (m.format == DXGI_FORMAT_B8G8R8A8_UNORM) m.format = DXGI_FORMAT_B8G8R8X8_UNORM;
            else if (m.format == DXGI_FORMAT_B8G8R8A8_UNORM_SRGB) m.format = DXGI_FORMAT_B8G8R8X8_UNORM_SRGB;
            else m.miscFlags2 |= TEX_ALPHA_MODE_OPAQUE;
        }
    }

    // The file's chunks. With `idat` null the walk stops at the first IDAT (metadata only); otherwise every IDAT's bytes are appended to
    // *idat and the file must end with IEND.
    HRESULT WalkChunks(const uint8_t* data, size_t size, Header& h, Blob* idat, size_t& idatBytes) noexcept
    {
        if (size < 8 || std::memcmp(data, kSignature, 8) != 0) return E_FAIL;
        size_t at = 8;
        bool first = true, sawIdat = false;
        // the IDAT bytes are no more than the file: one allocation
        if (idat) { const HRESULT hr = idat->Initialize(size); if (FAILED(hr)) return hr; }
        idatBytes = 0;
        for (;;)
        {
            if (size - at < 12) return E_FAIL;
            const uint32_t len = Be32(data + at), tag = Be32(data + at + 4);
            if (len > 0x7FFFFFFFu || size - at - 12 < len) return E_FAIL;
            const uint8_t* body = data + at + 8;
            if ((Crc32(0xFFFFFFFFu, data + at + 4, size_t(len) + 4) ^ 0xFFFFFFFFu) != Be32(body + len)) return E_FAIL;
            at += size_t(len) + 12;
            if (first != (tag == Tag('I', 'H', 'D', 'R'))) return E_FAIL;          // IHDR comes first, and once
            if (first)
            {
                first = false;
                if (len != 13) return E_FAIL;
                h.width = Be32(body); h.height = Be32(body + 4); h.depth = body[8]; h.colorType = body[9];
                if (!h.width || !h.height || h.width > kSideLimit || h.height > kSideLimit) return E_FAIL;
                if (KindOf(h.colorType, h.depth) < 0 || body[10] != 0 || body[11] != 0 || body[12] > 1) return E_FAIL;
                if (body[12] == 1) return HRESULT_E_NOT_SUPPORTED;          // Adam7
                continue;
            }
            if (tag == Tag('I', 'D', 'A', 'T'))
            {
                if (h.colorType == 3 && !h.hasPalette) return E_FAIL;
                if (!idat) return S_OK;
                sawIdat = true;
                if (len) std::memcpy(idat->GetBufferPointer() + idatBytes, body, len);
                idatBytes += len;
            }
            else if (tag == Tag('I', 'E', 'N', 'D')) return sawIdat ? S_OK : E_FAIL;
            else if (tag == Tag('P', 'L', 'T', 'E'))
            {
                if (sawIdat || h.hasPalette || len == 0 || len % 3 != 0 || len > 768) return E_FAIL;
                h.hasPalette = true; h.plteCount = len / 3;
                std::memcpy(h.plte, body, len);
            }
            else if (!(tag & 0x20000000u)) return E_FAIL;          // a critical chunk this reader does not know
            else if (sawIdat) continue;          // ancillary chunks behind the image data change nothing
            else if (tag == Tag('t', 'R', 'N', 'S'))
            {
                // a chunk of the wrong length or in the wrong place is passed over, as libpng does with a warning
                if (h.colorType == 3) { if (h.hasPalette && len >= 1 && len <= h.plteCount) { h.trnsCount = len; std::memcpy(h.trns, body, len); } }
                else if (h.colorType == 0 && len == 2) h.greyKey = true;
            }
            else if (tag == Tag('g', 'A', 'M', 'A')) { if (len == 4 && Be32(body) != 0 && Be32(body) <= 0x7FFFFFFFu) { h.hasGamma = true; h.gamma = Be32(body); } }
            else if (tag == Tag('s', 'R', 'G', 'B')) { if (len == 1) h.hasSRGB = true; }
        }
    }

    // this codec's own reader, not DirectXTexAMD_Internal.h's ReadAll: a missing file is ERROR_FILE_NOT_FOUND here and no size is too large
    HRESULT ReadPNGFile(const char* szFile, Blob& buf) noexcept
    {
        FILE* f = std::fopen(szFile, "rb");
        if (!f) return errno == ENOENT ? HRESULT_ERROR_FILE_NOT_FOUND : E_FAIL;
        std::fseek(f, 0, SEEK_END); const long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
        if (n < 1) { std::fclose(f); return E_FAIL; }
        const HRESULT hr = buf.Initialize(size_t(n));
        if (FAILED(hr)) { std::fclose(f); return hr; }
        const size_t got = std::fread(buf.GetBufferPointer(), 1, buf.GetBufferSize(), f);
        std::fclose(f);
        return got == buf.GetBufferSize() ? S_OK : E_FAIL;
    }

    HRESULT Metadata(const void* pSource, size_t size, PNG_FLAGS flags, TexMetadata& metadata, Header& h, Blob* idat, size_t& idatBytes) noexcept
    {
        if (!pSource) return E_INVALIDARG;
        const HRESULT hr = WalkChunks(static_cast<const uint8_t*>(pSource), size, h, idat, idatBytes);
        if (FAILED(hr)) return hr;
        if (h.greyKey) return HRESULT_E_NOT_SUPPORTED;
        FillMetadata(h, flags, metadata);
        return S_OK;
    }

    // ---- the writer ----------------------------------------------------------------------------------------------------------------------
    struct FileShape { int source; uint8_t depth, colorType; bool srgbFormat; };
    HRESULT SaveChecks(const Image& image, FileShape& f) noexcept
    {
        if (!image.pixels) return E_POINTER;
        // the writer's table (WriteImage :322-364): one channel is grey, B8G8R8X8 colour without alpha, the rest colour with it
        f.source = dxtex::png_pack_source(int(image.format));
        if (f.source < 0) return HRESULT_E_NOT_SUPPORTED;
        f.srgbFormat = IsSRGB(image.format);
        f.depth = (f.source == dxtex::PNG_SRC_R16 || f.source == dxtex::PNG_SRC_RGBA16) ? 16 : 8;
        f.colorType = (f.source == dxtex::PNG_SRC_R8 || f.source == dxtex::PNG_SRC_R16) ? 0 : f.source == dxtex::PNG_SRC_BGRX8 ? 2 : 6;
        if (!image.width || !image.height || image.width > kSideLimit || image.height > kSideLimit) return E_INVALIDARG;
        return S_OK;
    }

    uint8_t* PutChunk(uint8_t* p, uint32_t tag, const uint8_t* body, size_t len) noexcept
    {
        PutBe32(p, uint32_t(len)); PutBe32(p + 4, tag);
        if (len && body != p + 8) std::memcpy(p + 8, body, len);
        PutBe32(p + 8 + len, Crc32(0xFFFFFFFFu, p + 4, len + 4) ^ 0xFFFFFFFFu);
        return p + 12 + len;
    }

    // The file around the rows: rows(d, bytes) leaves the file's rows at d, tight; they are then wrapped - a filter byte 0 in front of each
    // row, the whole as stored deflate blocks in one zlib stream, that cut into IDAT chunks.
    template<class Rows>
    HRESULT WriteFile(const Image& image, PNG_FLAGS flags, const FileShape& f, Blob& blob, Rows&& rows) noexcept
    {
        blob.Release();
        const size_t rowBytes = image.width * dxtex::png_source_file_bytes(f.source);
        const size_t raw = image.height * (rowBytes + 1);
        const size_t blocks = (raw + 65534) / 65535;
        const size_t zbytes = 2 + blocks * 5 + raw + 4;
        const size_t idats = (zbytes + kIdatMax - 1) / kIdatMax;
        const bool gama = f.colorType != 0 && (flags & PNG_FLAGS_FORCE_LINEAR);
        const bool srgb = f.colorType != 0 && !gama && (f.srgbFormat || (flags & PNG_FLAGS_FORCE_SRGB));
        Blob tight, z;
        HRESULT hr = tight.Initialize(rowBytes * image.height);
        if (SUCCEEDED(hr)) hr = z.Initialize(zbytes);
        if (SUCCEEDED(hr)) hr = blob.Initialize(8 + 25 + (gama ? 16 : 0) + (srgb ? 13 : 0) + zbytes + idats * 12 + 12);
        if (SUCCEEDED(hr)) hr = rows(tight.GetBufferPointer(), tight.GetBufferSize());
        if (FAILED(hr)) { blob.Release(); return hr; }
        // the zlib stream: header, stored blocks that pay no heed to where rows end, the check value
        uint8_t* zp = z.GetBufferPointer();
        *zp++ = 0x78; *zp++ = 0x01;
        uint32_t a = 1, b = 0;          // Adler-32 as the bytes pass
        size_t inBlock = 0, left = raw;
        auto put = [&](const uint8_t* s, size_t n)
        {
            while (n)
            {
                if (!inBlock)
                {
                    inBlock = std::min<size_t>(left, 65535);
                    *zp++ = left <= 65535 ? 1 : 0;
                    *zp++ = uint8_t(inBlock); *zp++ = uint8_t(inBlock >> 8); *zp++ = uint8_t(~inBlock); *zp++ = uint8_t(~inBlock >> 8);
                }
                const size_t k = std::min(n, inBlock);
                std::memcpy(zp, s, k);
                zp += k; s += k; n -= k; inBlock -= k; left -= k;
            }
        };
        const uint8_t zero = 0;
        for (size_t y = 0; y < image.height; ++y) { put(&zero, 1); put(tight.GetBufferPointer() + y * rowBytes, rowBytes); }
        {
            // over the blocks' payloads: the filter bytes and the rows
            const uint8_t* t = tight.GetBufferPointer();
            for (size_t y = 0; y < image.height; ++y, t += rowBytes)
            {
                b += a;          // the filter byte: a += 0
                for (size_t i = 0; i < rowBytes; i += 5000)
                {
                    const size_t k = std::min<size_t>(5000, rowBytes - i);
                    for (size_t j = 0; j < k; ++j) { a += t[i + j]; b += a; }
                    a %= 65521u; b %= 65521u;
                }
                b %= 65521u;
            }
        }
        PutBe32(zp, (b << 16) | a);
        uint8_t* p = blob.GetBufferPointer();
        std::memcpy(p, kSignature, 8); p += 8;
        uint8_t ihdr[13];
        PutBe32(ihdr, uint32_t(image.width)); PutBe32(ihdr + 4, uint32_t(image.height));
        ihdr[8] = f.depth; ihdr[9] = f.colorType; ihdr[10] = ihdr[11] = ihdr[12] = 0;
        p = PutChunk(p, Tag('I', 'H', 'D', 'R'), ihdr, 13);
        if (gama) { uint8_t g[4]; PutBe32(g, 100000); p = PutChunk(p, Tag('g', 'A', 'M', 'A'), g, 4); }
        if (srgb) { const uint8_t intent = 0; p = PutChunk(p, Tag('s', 'R', 'G', 'B'), &intent, 1); }
        for (size_t at = 0; at < zbytes; at += kIdatMax) p = PutChunk(p, Tag('I', 'D', 'A', 'T'), z.GetBufferPointer() + at, std::min(kIdatMax, zbytes - at));
        p = PutChunk(p, Tag('I', 'E', 'N', 'D'), nullptr, 0);
        return size_t(p - blob.GetBufferPointer()) == blob.GetBufferSize() ? S_OK : E_UNEXPECTED;
    }

    HRESULT SaveHost(const Image& image, PNG_FLAGS flags, Blob& blob) noexcept
    {
        blob.Release();
        FileShape f;
        const HRESULT hr = SaveChecks(image, f);
        if (FAILED(hr)) return hr;
        const size_t S = dxtex::png_source_bytes(f.source), F = dxtex::png_source_file_bytes(f.source);
        if (image.rowPitch < image.width * S) return E_INVALIDARG;
        return WriteFile(image, flags, f, blob, [&](uint8_t* d, size_t)
        {
            for (size_t y = 0; y < image.height; ++y)
            {
                const uint8_t* s = image.pixels + y * image.rowPitch;
                for (size_t x = 0; x < image.width; ++x, s += S, d += F) dxtex::png_pack_texel(s, d, f.source);
            }
            return S_OK;
        });
    }

    HRESULT SaveResident(Device& device, const Image& deviceImage, PNG_FLAGS flags, Blob& blob) noexcept
    {
        blob.Release();
        FileShape f;
        const HRESULT hr = SaveChecks(deviceImage, f);
        if (FAILED(hr)) return hr;
        if (!device) return E_POINTER;
        const dxtex_image s = ImageOf(deviceImage);
        return WriteFile(deviceImage, flags, f, blob, [&](uint8_t* d, size_t bytes)
        { return PackAndDownload(device, bytes, d, [&](void* p) { return dxtex_png_pack_device(device.Get(), &s, p, bytes); }); });
    }
}

void PNGRawImage::Release() noexcept
{
    storage.Release();
    kind = flags = paletteCount = 0;
    std::memset(palette, 0, sizeof(palette));
    rowBytes = rowsBytes = 0;
    rows = nullptr;
}

HRESULT LoadFromPNGMemoryRaw(const void* pSource, size_t size, PNG_FLAGS flags, TexMetadata* metadata, PNGRawImage& raw) noexcept
{
    raw.Release();
    Header h; TexMetadata mdata; Blob idat; size_t idatBytes = 0;
    const HRESULT hr = Metadata(pSource, size, flags, mdata, h, &idat, idatBytes);
    if (FAILED(hr)) return hr;
    const int kind = KindOf(h.colorType, h.depth);
    const size_t rowBytes = size_t(dxtex::png_row_bytes(kind, h.width));
    const uint64_t need = uint64_t(h.height) * (rowBytes + 1);
    // deflate gives at most 1032 bytes for one (a stored byte of 258-byte matches): a stream too short for the image is refused before
    // memory is asked for
    if (need / 1032u > idatBytes || need > SIZE_MAX / 2) return E_FAIL;
    Blob out;
    HRESULT hr2 = out.Initialize(size_t(need));
    if (FAILED(hr2)) return hr2;
    if (!Inflate(idat.GetBufferPointer(), idatBytes, out.GetBufferPointer(), size_t(need))) return E_FAIL;
    idat.Release();
    if (!Unfilter(out.GetBufferPointer(), h.height, rowBytes, std::max<size_t>(1, dxtex::png_file_bits(kind) / 8))) return E_FAIL;
    hr2 = out.Trim(rowBytes * h.height);
    if (FAILED(hr2)) return hr2;
    raw.kind = uint32_t(kind);
    raw.flags = ((flags & PNG_FLAGS_BGR) && h.colorType != 0 && h.depth <= 8) ? DXTEX_PNG_BGR : 0u;
    if (h.colorType == 3)
    {
        dxtex::png_palette_table(h.plte, h.plteCount, h.trnsCount ? h.trns : nullptr, h.trnsCount, raw.palette);
        raw.paletteCount = h.plteCount;
    }
    raw.rowBytes = rowBytes; raw.rowsBytes = rowBytes * h.height;
    raw.storage.Swap(out);
    raw.rows = raw.storage.GetBufferPointer();
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromPNGFileRaw(const char* szFile, PNG_FLAGS flags, TexMetadata* metadata, PNGRawImage& raw) noexcept
{
    raw.Release();
    // the rows are always inflated into storage of their own: the file is not kept
    return LoadFile(szFile, ReadPNGFile, [&](const uint8_t* p, size_t n) { return LoadFromPNGMemoryRaw(p, n, flags, metadata, raw); });
}

HRESULT GetMetadataFromPNGMemory(const void* pSource, size_t size, PNG_FLAGS flags, TexMetadata& metadata) noexcept
{
    Header h; size_t idatBytes = 0;
    return Metadata(pSource, size, flags, metadata, h, nullptr, idatBytes);
}

HRESULT GetMetadataFromPNGFile(const char* szFile, PNG_FLAGS flags, TexMetadata& metadata) noexcept
{
    return LoadFile(szFile, ReadPNGFile, [&](const uint8_t* p, size_t n) { return GetMetadataFromPNGMemory(p, n, flags, metadata); });
}

HRESULT LoadFromPNGMemory(const void* pSource, size_t size, PNG_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept
{
    image.Release();          // on any failure the result is empty
    TexMetadata mdata; PNGRawImage raw;
    HRESULT hr = LoadFromPNGMemoryRaw(pSource, size, flags, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = image.Initialize2D(mdata.format, mdata.width, mdata.height, 1, 1);
    if (FAILED(hr)) return hr;
    const Image* img = image.GetImage(0, 0, 0);
    if (!img) { image.Release(); return E_POINTER; }
    const int kind = int(raw.kind);
    const size_t D = dxtex::png_image_bytes(kind);
    const bool bgr = (raw.flags & DXTEX_PNG_BGR) != 0;
    for (size_t y = 0; y < img->height; ++y)
    {
        const uint8_t* row = raw.rows + y * raw.rowBytes;
        uint8_t* d = img->pixels + y * img->rowPitch;
        for (size_t x = 0; x < img->width; ++x, d += D) dxtex::png_unpack_texel(row, x, d, kind, bgr, raw.palette);
    }
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromPNGFile(const char* szFile, PNG_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept
{
    image.Release();
    return LoadFile(szFile, ReadPNGFile, [&](const uint8_t* p, size_t n) { return LoadFromPNGMemory(p, n, flags, metadata, image); });
}

HRESULT SaveToPNGMemory(const Image& image, PNG_FLAGS flags, Blob& blob) noexcept { return SaveHost(image, flags, blob); }

HRESULT SaveToPNGFile(const Image& image, PNG_FLAGS flags, const char* szFile) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveHost(image, flags, blob); });
}

// ---- resident forms: the rows travel as the file has them, the per-texel pass runs on the device (dxtex_png_unpack_device / dxtex_png_pack_device) ----
HRESULT UploadPNGRaw(Device& device, const TexMetadata& metadata, const PNGRawImage& raw, DeviceScratchImage& image) noexcept
{
    image.Release();
    if (!device) return E_POINTER;
    if (!raw.rows || metadata.arraySize != 1 || metadata.mipLevels != 1 || metadata.depth != 1) return E_INVALIDARG;
    if (raw.rowsBytes != raw.rowBytes * metadata.height) return E_INVALIDARG;
    return InitializeAndFill(device, metadata, image, [&](const Image& img) -> HRESULT
    {
        const bool native = (raw.kind == DXTEX_PNG_G8 || raw.kind == DXTEX_PNG_RGBA8) && !(raw.flags & DXTEX_PNG_BGR);
        if (native && img.rowPitch == raw.rowBytes) return dxtex_memcpy_h2d(device.Get(), img.pixels, raw.rows, raw.rowsBytes);          // the rows are the image: one copy, no kernel
        // the rows start an allocation of their own: a width of whole groups takes the wide route
        const dxtex_image d = ImageOf(img);
        return UploadAndUnpack(device, raw.rows, raw.rowsBytes, [&](void* p)
        { return dxtex_png_unpack_device(device.Get(), p, raw.rowsBytes, raw.kind, raw.flags, raw.paletteCount ? raw.palette : nullptr, raw.paletteCount, &d); });
    });
}

HRESULT LoadFromPNGMemory(Device& device, const void* pSource, size_t size, PNG_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();          // on any failure the result is empty
    TexMetadata mdata; PNGRawImage raw;
    HRESULT hr = LoadFromPNGMemoryRaw(pSource, size, flags, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = UploadPNGRaw(device, mdata, raw, image);
    if (FAILED(hr)) return hr;
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromPNGFile(Device& device, const char* szFile, PNG_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();
    return LoadFile(szFile, ReadPNGFile, [&](const uint8_t* p, size_t n) { return LoadFromPNGMemory(device, p, n, flags, metadata, image); });
}

HRESULT SaveToPNGMemory(Device& device, const Image& deviceImage, PNG_FLAGS flags, Blob& blob) noexcept { return SaveResident(device, deviceImage, flags, blob); }

HRESULT SaveToPNGFile(Device& device, const Image& deviceImage, PNG_FLAGS flags, const char* szFile) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveResident(device, deviceImage, flags, blob); });
}
} // namespace DirectXTexAMD
