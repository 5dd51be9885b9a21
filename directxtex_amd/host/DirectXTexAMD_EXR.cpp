// OpenEXR reader / writer of the host layer. Behaviour follows Auxiliary/DirectXTexEXR.cpp, the reference's codec over the OpenEXR library's
// RgbaInputFile and RgbaOutputFile; DirectXTexAMD.h states the departures. No library is linked: the header walk, the offset table and the
// RLE packets are below, the inflater is DirectXTexAMD_Inflate.h's. The library is not there to run the reference against, so the yardstick
// is tests/exr_ref.py, a restatement of the rules over Python's zlib.
// The reader is split in two. LoadFromEXRMemoryRaw does what is byte-serial - header, every refusal, offset table, inflate, RLE - and ends
// in one stream of the chunks' expanded bytes with a descriptor per chunk. What happens to those bytes after that is csrc/dxtex_exr.h's,
// which the GPU kernels share: the host loader runs it here, the resident forms at the end of this file run it on the device, so that a
// file's chunks cross PCIe as they leave the inflater. The writer is split the same way around its scanlines.
#include "DirectXTexAMD_Internal.h"
#include "DirectXTexAMD_Inflate.h"
#include "../csrc/dxtex_exr.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

namespace DirectXTexAMD
{
static_assert(sizeof(EXRRawImage::Chunk) == sizeof(dxtex_exr_chunk) && sizeof(EXRRawImage::Chunk) == sizeof(dxtex::ExrChunk) &&
              sizeof(EXRRawImage::Channel) == sizeof(dxtex_exr_channel), "the raw image's tables are the C ABI's");

namespace
{
    constexpr uint8_t kMagic[4] = { 0x76, 0x2f, 0x31, 0x01 };
    enum : uint32_t { kTiled = 0x200, kLongNames = 0x400, kDeep = 0x800, kMultipart = 0x1000 };
    enum : uint32_t { kNone = 0, kRle = 1, kZips = 2, kZip = 3, kCompressions = 10 };
    constexpr size_t kNameMax = 255;
    constexpr size_t kChannelsMax = 1024;          // of one file; a list is name order, so every entry costs at least 18 bytes of it

    inline uint32_t Le32(const uint8_t* p) noexcept { return dxtex::le_load32(p, 4); }
    inline uint64_t Le64(const uint8_t* p) noexcept { return dxtex::le_load64(p, 8); }
    inline void PutLe32(uint8_t* p, uint32_t v) noexcept { dxtex::le_store32(p, v, 4); }

    // a NUL-terminated name of 1 to kNameMax bytes at p; its length, or 0 for none within `left`
    inline size_t NameAt(const uint8_t* p, size_t left) noexcept
    {
        const size_t most = std::min(left, kNameMax + 1);
        for (size_t n = 0; n < most; ++n) if (!p[n]) return n;
        return 0;
    }
    inline bool Is(const uint8_t* p, size_t n, const char* s) noexcept { return std::strlen(s) == n && !std::memcmp(p, s, n); }

    struct FileChannel { const uint8_t* name; size_t nameLen; uint32_t type; int32_t xs, ys; };
    struct Header
    {
        bool has[8] = {};          // the needed attributes, in name order
        bool envmap = false;
        uint32_t compression = 0;
        int32_t xMin = 0, yMin = 0, xMax = 0, yMax = 0;
        FileChannel channels[kChannelsMax]; size_t channelCount = 0;
        size_t end = 0;            // the first byte behind the header
    };

    bool NameLess(const FileChannel& a, const FileChannel& b) noexcept
    {
        const int c = std::memcmp(a.name, b.name, std::min(a.nameLen, b.nameLen));
        return c < 0 || (c == 0 && a.nameLen < b.nameLen);
    }

    HRESULT ParseChannels(const uint8_t* p, size_t size, Header& h) noexcept
    {
        size_t at = 0;
        for (;;)
        {
            if (at >= size) return E_FAIL;
            if (!p[at]) break;
            const size_t n = NameAt(p + at, size - at);
            if (!n || size - at - n - 1 < 16) return E_FAIL;
            if (h.channelCount == kChannelsMax) return E_FAIL;
            const uint8_t* e = p + at + n + 1;
            FileChannel c{ p + at, n, Le32(e), int32_t(Le32(e + 8)), int32_t(Le32(e + 12)) };
            if (c.type > dxtex::EXR_FLOAT || c.xs < 1 || c.ys < 1) return E_FAIL;
            h.channels[h.channelCount++] = c;
            at += n + 1 + 16;
        }
        if (!h.channelCount) return E_FAIL;
        // the file holds them in the byte order of their names, whatever order the list has
        std::sort(h.channels, h.channels + h.channelCount, NameLess);
        for (size_t i = 1; i < h.channelCount; ++i) if (!NameLess(h.channels[i - 1], h.channels[i])) return E_FAIL;          // the same name twice
        return S_OK;
    }

    HRESULT ParseHeader(const uint8_t* data, size_t size, Header& h) noexcept
    {
        if (size < 8 || std::memcmp(data, kMagic, 4) != 0) return E_FAIL;
        const uint32_t version = Le32(data + 4);
        if ((version & 0xFFu) != 2u) return E_FAIL;
        if (version & (kTiled | kDeep | kMultipart)) return HRESULT_E_NOT_SUPPORTED;
        if (version & ~(0xFFu | kLongNames)) return E_FAIL;
        static const struct { const char* name; const char* type; size_t size; } needed[8] =
        {
            { "channels", "chlist", 0 }, { "compression", "compression", 1 }, { "dataWindow", "box2i", 16 }, { "displayWindow", "box2i", 16 },
            { "lineOrder", "lineOrder", 1 }, { "pixelAspectRatio", "float", 4 }, { "screenWindowCenter", "v2f", 8 }, { "screenWindowWidth", "float", 4 },
        };
        size_t at = 8;
        for (;;)
        {
            if (at >= size) return E_FAIL;
            if (!data[at]) { ++at; break; }
            const size_t n = NameAt(data + at, size - at);
            if (!n) return E_FAIL;
            const uint8_t* name = data + at;
            at += n + 1;
            const size_t tn = at < size ? NameAt(data + at, size - at) : 0;
            if (!tn) return E_FAIL;
            const uint8_t* type = data + at;
            at += tn + 1;
            if (size - at < 4) return E_FAIL;
            const uint32_t bytes = Le32(data + at);
            at += 4;
            if (bytes > 0x7FFFFFFFu || bytes > size - at) return E_FAIL;
            const uint8_t* v = data + at;
            at += bytes;
            if (Is(name, n, "envmap")) { h.envmap = true; continue; }
            for (int k = 0; k < 8; ++k)
            {
                if (!Is(name, n, needed[k].name)) continue;
                if (!Is(type, tn, needed[k].type) || (needed[k].size && bytes != needed[k].size) || h.has[k]) return E_FAIL;
                h.has[k] = true;
                if (k == 0) { const HRESULT hr = ParseChannels(v, bytes, h); if (FAILED(hr)) return hr; }
                else if (k == 1) { h.compression = v[0]; if (h.compression >= kCompressions) return E_FAIL; }
                else if (k == 2) { h.xMin = int32_t(Le32(v)); h.yMin = int32_t(Le32(v + 4)); h.xMax = int32_t(Le32(v + 8)); h.yMax = int32_t(Le32(v + 12)); }
                else if (k == 4 && v[0] > 2) return E_FAIL;
            }
        }
        for (int k = 0; k < 8; ++k) if (!h.has[k]) return E_FAIL;
        h.end = at;
        return S_OK;
    }

    // what the header says of the image: the metadata, the scanline and where R, G, B, A lie in it
    struct Shape { size_t width = 0, height = 0; uint32_t scanlineBytes = 0; EXRRawImage::Channel channel[4]; };
    HRESULT ShapeOf(const Header& h, TexMetadata& m, Shape& s) noexcept
    {
        const int64_t w = int64_t(h.xMax) - h.xMin + 1, ht = int64_t(h.yMax) - h.yMin + 1;
        if (w < 1 || ht < 1 || w > INT32_MAX || ht > INT32_MAX) return E_FAIL;          // an empty or overflowing window
        if (h.compression > kZip) return HRESULT_E_NOT_SUPPORTED;
        s.width = size_t(w); s.height = size_t(ht);
        const FileChannel* named[5] = {};          // R, G, B, A, Y
        uint64_t line = 0, offset[kChannelsMax];
        for (size_t i = 0; i < h.channelCount; ++i)
        {
            const FileChannel& c = h.channels[i];
            if (Is(c.name, c.nameLen, "RY") || Is(c.name, c.nameLen, "BY")) return HRESULT_E_NOT_SUPPORTED;
            if (c.xs != 1 || c.ys != 1) return HRESULT_E_NOT_SUPPORTED;
            static const char* const names[5] = { "R", "G", "B", "A", "Y" };
            for (int k = 0; k < 5; ++k) if (Is(c.name, c.nameLen, names[k])) named[k] = &c;
            offset[i] = line;
            line += uint64_t(w) * dxtex::exr_type_bytes(c.type);
            if (line > 0x7FFFFFFFu / 16u) return E_FAIL;          // a chunk of 16 scanlines is an int32 dataSize
        }
        s.scanlineBytes = uint32_t(line);
        if (named[4] && !named[0] && !named[1] && !named[2]) named[0] = named[1] = named[2] = named[4];
        for (int k = 0; k < 4; ++k)
        {
            s.channel[k] = { 0, dxtex::EXR_ABSENT };
            if (named[k]) s.channel[k] = { uint32_t(offset[named[k] - h.channels]), named[k]->type };
        }
        m = TexMetadata();
        m.width = s.width; m.height = s.height; m.depth = m.arraySize = m.mipLevels = 1;
        m.format = DXGI_FORMAT_R16G16B16A16_FLOAT; m.dimension = TEX_DIMENSION_TEXTURE2D;
        if (h.envmap && s.width == s.height / 6)
        {
            // the reference takes six faces of width x width out of a window that may be up to five rows taller and reads all of its
            // rows into them; here such a window is refused
            if (s.height != s.width * 6) return E_FAIL;
            m.height = s.width; m.arraySize = 6;
        }
        return S_OK;
    }

    // the RLE packets at [in, in + n) into out[0, cap): true when they are used up as the last of cap bytes comes out
    bool Unrle(const uint8_t* in, size_t n, uint8_t* out, size_t cap) noexcept
    {
        size_t at = 0, pos = 0;
        while (at < n)
        {
            const int c = int8_t(in[at++]);
            if (c < 0)
            {
                const size_t k = size_t(-c);
                if (n - at < k || cap - pos < k) return false;
                std::memcpy(out + pos, in + at, k);
                at += k; pos += k;
            }
            else
            {
                const size_t k = size_t(c) + 1;
                if (at == n || cap - pos < k) return false;
                std::memset(out + pos, in[at++], k);
                pos += k;
            }
        }
        return pos == cap;
    }

    HRESULT ReadEXRFile(const char* szFile, Blob& buf) noexcept
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

    inline uint32_t LinesOf(uint32_t compression) noexcept { return compression == kZip ? 16u : 1u; }

    // ---- the writer: the file around its scanlines -----------------------------------------------------------------------------------------
    struct FileShape { int source; size_t headerBytes, tableBytes, lineBytes, fileBytes; };
    HRESULT SaveChecks(const Image& image, FileShape& f) noexcept
    {
        if (!image.pixels) return E_POINTER;
        f.source = dxtex::exr_pack_source(int(image.format));
        if (f.source < 0) return HRESULT_E_NOT_SUPPORTED;
        if (!image.width || !image.height) return E_INVALIDARG;
        if (image.width > size_t(INT32_MAX) / 8 || image.height > size_t(INT32_MAX)) return HRESULT_E_NOT_SUPPORTED;
        f.lineBytes = image.width * dxtex::kExrFileTexelBytes;
        f.headerBytes = 8 + (9 + 7 + 4 + 73) + (12 + 12 + 4 + 1) + (11 + 6 + 4 + 16) + (14 + 6 + 4 + 16) + (10 + 10 + 4 + 1) + (17 + 6 + 4 + 4) + (19 + 4 + 4 + 8) + (18 + 6 + 4 + 4) + 1;
        f.tableBytes = image.height * 8;
        if (image.height > (SIZE_MAX - f.headerBytes) / (f.lineBytes + 16)) return HRESULT_E_ARITHMETIC_OVERFLOW;
        f.fileBytes = f.headerBytes + f.tableBytes + image.height * (8 + f.lineBytes);
        return S_OK;
    }

    struct Writer
    {
        uint8_t* p;
        void Bytes(const void* s, size_t n) noexcept { std::memcpy(p, s, n); p += n; }
        void Str(const char* s) noexcept { Bytes(s, std::strlen(s) + 1); }
        void U32(uint32_t v) noexcept { PutLe32(p, v); p += 4; }
        void Attr(const char* name, const char* type, uint32_t size) noexcept { Str(name); Str(type); U32(size); }
    };

    // header, offset table and every chunk's y and dataSize; then rows(first, pitch) leaves scanline y at first + y * pitch
    template<class Rows>
    HRESULT WriteFile(const Image& image, const FileShape& f, Blob& blob, Rows&& rows) noexcept
    {
        blob.Release();
        HRESULT hr = blob.Initialize(f.fileBytes);
        if (FAILED(hr)) return hr;
        Writer w{ blob.GetBufferPointer() };
        const uint32_t xMax = uint32_t(image.width - 1), yMax = uint32_t(image.height - 1), one = 0x3F800000u;
        w.Bytes(kMagic, 4); w.U32(2);
        w.Attr("channels", "chlist", 73);
        for (const char* name : { "A", "B", "G", "R" }) { w.Str(name); w.U32(dxtex::EXR_HALF); w.U32(0); w.U32(1); w.U32(1); }
        *w.p++ = 0;
        w.Attr("compression", "compression", 1); *w.p++ = uint8_t(kNone);
        w.Attr("dataWindow", "box2i", 16); w.U32(0); w.U32(0); w.U32(xMax); w.U32(yMax);
        w.Attr("displayWindow", "box2i", 16); w.U32(0); w.U32(0); w.U32(xMax); w.U32(yMax);
        w.Attr("lineOrder", "lineOrder", 1); *w.p++ = 0;
        w.Attr("pixelAspectRatio", "float", 4); w.U32(one);
        w.Attr("screenWindowCenter", "v2f", 8); w.U32(0); w.U32(0);
        w.Attr("screenWindowWidth", "float", 4); w.U32(one);
        *w.p++ = 0;
        if (size_t(w.p - blob.GetBufferPointer()) != f.headerBytes) { blob.Release(); return E_UNEXPECTED; }
        const size_t first = f.headerBytes + f.tableBytes, pitch = 8 + f.lineBytes;
        for (size_t y = 0; y < image.height; ++y) dxtex::le_store64(w.p + y * 8, uint64_t(first + y * pitch), 8);
        uint8_t* chunk = blob.GetBufferPointer() + first;
        for (size_t y = 0; y < image.height; ++y) { PutLe32(chunk + y * pitch, uint32_t(y)); PutLe32(chunk + y * pitch + 4, uint32_t(f.lineBytes)); }
        hr = rows(chunk + 8, pitch);
        if (FAILED(hr)) blob.Release();
        return hr;
    }

    HRESULT SaveHost(const Image& image, Blob& blob) noexcept
    {
        blob.Release();
        FileShape f;
        const HRESULT hr = SaveChecks(image, f);
        if (FAILED(hr)) return hr;
        if (image.rowPitch < image.width * dxtex::exr_source_bytes(f.source)) return E_INVALIDARG;
        return WriteFile(image, f, blob, [&](uint8_t* first, size_t pitch)
        {
            for (size_t y = 0; y < image.height; ++y)
                for (size_t x = 0; x < image.width; ++x) dxtex::exr_pack_texel(image.pixels + y * image.rowPitch, first + y * pitch, uint32_t(image.width), uint32_t(x), f.source);
            return S_OK;
        });
    }

    HRESULT SaveResident(Device& device, const Image& deviceImage, Blob& blob) noexcept
    {
        blob.Release();
        FileShape f;
        HRESULT hr = SaveChecks(deviceImage, f);
        if (FAILED(hr)) return hr;
        if (!device) return E_POINTER;
        const dxtex_image s = ImageOf(deviceImage);
        return WriteFile(deviceImage, f, blob, [&](uint8_t* first, size_t pitch) -> HRESULT
        {
            // the scanlines are tight on the device and land between the chunk headers: one strided download of 8 bytes a texel
            const size_t bytes = f.lineBytes * deviceImage.height;
            DeviceTemp temp(device);
            HRESULT r = dxtex_device_alloc(device.Get(), bytes, &temp.p);
            if (SUCCEEDED(r)) r = dxtex_exr_pack_device(device.Get(), &s, temp.p, bytes);
            if (SUCCEEDED(r)) r = dxtex_memcpy_rows_d2h_async(device.Get(), first, pitch, temp.p, f.lineBytes, f.lineBytes, deviceImage.height);
            if (SUCCEEDED(r)) r = dxtex_ctx_synchronize(device.Get());
            return r;
        });
    }
}

void EXRRawImage::Release() noexcept
{
    storage.Release();
    chunks.reset();
    compression = scanlineBytes = 0;
    for (Channel& c : channel) c = Channel{ 0, 0 };
    chunkCount = deflatedBytes = streamBytes = 0;
    stream = nullptr;
}

HRESULT GetMetadataFromEXRMemory(const void* pSource, size_t size, TexMetadata& metadata) noexcept
{
    if (!pSource) return E_INVALIDARG;
    std::unique_ptr<Header> h(new (std::nothrow) Header);
    if (!h) return E_OUTOFMEMORY;
    const HRESULT hr = ParseHeader(static_cast<const uint8_t*>(pSource), size, *h);
    if (FAILED(hr)) return hr;
    Shape s;
    return ShapeOf(*h, metadata, s);
}

HRESULT GetMetadataFromEXRFile(const char* szFile, TexMetadata& metadata) noexcept
{
    return LoadFile(szFile, ReadEXRFile, [&](const uint8_t* p, size_t n) { return GetMetadataFromEXRMemory(p, n, metadata); });
}

HRESULT LoadFromEXRMemoryRaw(const void* pSource, size_t size, TexMetadata* metadata, EXRRawImage& raw) noexcept
{
    raw.Release();
    if (!pSource) return E_INVALIDARG;
    const uint8_t* data = static_cast<const uint8_t*>(pSource);
    std::unique_ptr<Header> h(new (std::nothrow) Header);
    if (!h) return E_OUTOFMEMORY;
    HRESULT hr = ParseHeader(data, size, *h);
    if (FAILED(hr)) return hr;
    TexMetadata mdata; Shape s;
    hr = ShapeOf(*h, mdata, s);
    if (FAILED(hr)) return hr;

    // the offset table: entry i is the chunk that starts at yMin + i * lines, whatever the line order
    const uint32_t lines = LinesOf(h->compression);
    const size_t count = (s.height + lines - 1) / lines;
    if ((size - h->end) / 8 < count) return E_FAIL;
    // neither a stored nor an expanded chunk gives more than 1032 bytes for one of the file's
    if (uint64_t(s.height) * s.scanlineBytes / 1032u > size) return E_FAIL;
    std::unique_ptr<EXRRawImage::Chunk[]> chunks(new (std::nothrow) EXRRawImage::Chunk[count]);
    std::unique_ptr<uint64_t[]> place(new (std::nothrow) uint64_t[count]);          // of each chunk in the stream
    if (!chunks || !place) return E_OUTOFMEMORY;
    const uint8_t* table = data + h->end;
    uint64_t streamBytes = 0, deflated = 0;
    for (size_t i = 0; i < count; ++i)
    {
        const uint64_t off = Le64(table + i * 8);
        if (!off || off > size || size - off < 8) return E_FAIL;
        const int64_t y = int32_t(Le32(data + off)), want = int64_t(h->yMin) + int64_t(i) * lines;
        const uint32_t dataSize = Le32(data + off + 4);
        if (y != want || dataSize > 0x7FFFFFFFu || dataSize > size - off - 8) return E_FAIL;
        const uint32_t rows = uint32_t(std::min<size_t>(lines, s.height - i * lines)), plain = rows * s.scanlineBytes;
        if (dataSize > plain || (h->compression == kNone && dataSize != plain)) return E_FAIL;
        const bool coded = dataSize != plain;          // the format stores a chunk raw when coding does not shrink it
        if (coded) streamBytes = (streamBytes + 15) & ~uint64_t(15);
        place[i] = streamBytes;
        chunks[i] = EXRRawImage::Chunk{ streamBytes, plain, uint32_t(i * lines), rows, coded ? 1u : 0u };
        streamBytes += plain;
        deflated += dataSize;
    }
    hr = raw.storage.Initialize(size_t(streamBytes));
    if (FAILED(hr)) return hr;
    uint8_t* stream = raw.storage.GetBufferPointer();
    size_t used = 0;          // descriptors
    uint64_t end = 0;
    for (size_t i = 0; i < count; ++i)
    {
        const EXRRawImage::Chunk c = chunks[i];
        const uint64_t off = Le64(table + i * 8);
        const uint8_t* body = data + off + 8;
        const uint32_t dataSize = Le32(data + off + 4);
        if (c.offset > end) std::memset(stream + end, 0, size_t(c.offset - end));          // the bytes in front of an aligned chunk
        uint8_t* out = stream + c.offset;
        bool ok = true;
        if (!c.coded) std::memcpy(out, body, c.bytes);
        else if (h->compression == kRle) ok = Unrle(body, dataSize, out, c.bytes);
        else
        {
            // exactly c.bytes: the inflater stops there, and a stream that ends there ends in their Adler-32 at the chunk's last bytes
            ok = dataSize >= 6 && Inflate(body, dataSize, out, c.bytes) &&
                 Adler32(out, c.bytes) == ((uint32_t(body[dataSize - 4]) << 24) | (uint32_t(body[dataSize - 3]) << 16) | (uint32_t(body[dataSize - 2]) << 8) | body[dataSize - 1]);
        }
        if (!ok) { raw.Release(); return E_FAIL; }
        end = c.offset + c.bytes;
        // a plain chunk right behind a plain one, in the stream and in the window, extends its descriptor
        EXRRawImage::Chunk* last = used ? &chunks[used - 1] : nullptr;
        if (last && !c.coded && !last->coded && last->offset + last->bytes == c.offset && last->firstRow + last->rows == c.firstRow &&
            uint64_t(last->bytes) + c.bytes <= 0x40000000u)
        { last->bytes += c.bytes; last->rows += c.rows; }
        else chunks[used++] = c;
    }
    raw.compression = h->compression; raw.scanlineBytes = s.scanlineBytes;
    for (int k = 0; k < 4; ++k) raw.channel[k] = s.channel[k];
    raw.chunks = std::move(chunks); raw.chunkCount = used; raw.deflatedBytes = size_t(deflated);
    raw.stream = stream; raw.streamBytes = size_t(streamBytes);
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromEXRFileRaw(const char* szFile, TexMetadata* metadata, EXRRawImage& raw) noexcept
{
    raw.Release();
    // the chunks are always expanded into storage of their own: the file is not kept
    return LoadFile(szFile, ReadEXRFile, [&](const uint8_t* p, size_t n) { return LoadFromEXRMemoryRaw(p, n, metadata, raw); });
}

HRESULT LoadFromEXRMemory(const void* pSource, size_t size, TexMetadata* metadata, ScratchImage& image) noexcept
{
    image.Release();          // on any failure the result is empty
    TexMetadata mdata; EXRRawImage raw;
    HRESULT hr = LoadFromEXRMemoryRaw(pSource, size, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = image.Initialize2D(mdata.format, mdata.width, mdata.height, mdata.arraySize, 1);
    if (FAILED(hr)) return hr;
    dxtex::ExrChannel channel[4];
    for (int k = 0; k < 4; ++k) channel[k] = { raw.channel[k].offset, raw.channel[k].type };
    uint8_t* stream = raw.storage.GetBufferPointer();
    for (size_t i = 0; i < raw.chunkCount; ++i)
    {
        const EXRRawImage::Chunk& c = raw.chunks[i];
        uint8_t* chunk = stream + c.offset;
        if (c.coded) dxtex::exr_undo_serial(chunk, c.bytes);
        for (uint32_t r = 0; r < c.rows; ++r)
        {
            const size_t y = c.firstRow + r;
            const Image* img = image.GetImage(0, y / mdata.height, 0);
            if (!img) { image.Release(); return E_POINTER; }
            uint8_t* d = img->pixels + (y % mdata.height) * img->rowPitch;
            for (uint32_t x = 0; x < uint32_t(mdata.width); ++x)
                dxtex::le_store64(d + size_t(x) * 8, dxtex::exr_texel(chunk, c.coded != 0, c.bytes, r * raw.scanlineBytes, channel, x), 8);
        }
    }
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromEXRFile(const char* szFile, TexMetadata* metadata, ScratchImage& image) noexcept
{
    image.Release();
    return LoadFile(szFile, ReadEXRFile, [&](const uint8_t* p, size_t n) { return LoadFromEXRMemory(p, n, metadata, image); });
}

HRESULT SaveToEXRMemory(const Image& image, Blob& blob) noexcept { return SaveHost(image, blob); }

HRESULT SaveToEXRFile(const Image& image, const char* szFile) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveHost(image, blob); });
}

// ---- resident forms: the stream travels as it left the inflater, everything behind it runs on the device (dxtex_exr_unpack_device / dxtex_exr_pack_device) ----
HRESULT UploadEXRRaw(Device& device, const TexMetadata& metadata, const EXRRawImage& raw, DeviceScratchImage& image) noexcept
{
    image.Release();
    if (!device) return E_POINTER;
    if (!raw.stream || !raw.chunks || !raw.chunkCount || metadata.mipLevels != 1 || metadata.depth != 1 || !metadata.arraySize || metadata.arraySize > dxtex::kExrItemsMax)
        return E_INVALIDARG;
    HRESULT hr = image.Initialize(device, metadata);
    if (FAILED(hr)) return hr;
    dxtex_image items[dxtex::kExrItemsMax];
    for (size_t i = 0; i < metadata.arraySize; ++i)
    {
        const Image* img = image.GetImage(0, i, 0);
        if (!img) { image.Release(); return E_POINTER; }
        items[i] = ImageOf(*img);
    }
    // the stream starts an allocation of its own, and its coded chunks lie on multiples of 16 bytes: exr_undo takes the wide route
    hr = UploadAndUnpack(device, raw.stream, raw.streamBytes, [&](void* p)
    {
        return dxtex_exr_unpack_device(device.Get(), p, raw.streamBytes, reinterpret_cast<const dxtex_exr_chunk*>(raw.chunks.get()), raw.chunkCount,
                                       reinterpret_cast<const dxtex_exr_channel*>(raw.channel), raw.scanlineBytes, items, metadata.arraySize);
    });
    if (FAILED(hr)) image.Release();
    return hr;
}

HRESULT LoadFromEXRMemory(Device& device, const void* pSource, size_t size, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();          // on any failure the result is empty
    TexMetadata mdata; EXRRawImage raw;
    HRESULT hr = LoadFromEXRMemoryRaw(pSource, size, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = UploadEXRRaw(device, mdata, raw, image);
    if (FAILED(hr)) return hr;
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromEXRFile(Device& device, const char* szFile, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();
    return LoadFile(szFile, ReadEXRFile, [&](const uint8_t* p, size_t n) { return LoadFromEXRMemory(device, p, n, metadata, image); });
}

HRESULT SaveToEXRMemory(Device& device, const Image& deviceImage, Blob& blob) noexcept { return SaveResident(device, deviceImage, blob); }

HRESULT SaveToEXRFile(Device& device, const Image& deviceImage, const char* szFile) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveResident(device, deviceImage, blob); });
}
} // namespace DirectXTexAMD
