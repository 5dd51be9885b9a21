// TIFF reader / writer of the host layer. The reference reads and writes TIFF through WIC (DirectXTexWIC.cpp); the kinds and formats
// follow its tables, DirectXTexAMD.h states the departures. No library is linked: the header, the IFD walk, LZW and PackBits are below, the
// inflater is DirectXTexAMD_Inflate.h's. WIC is not there to run the reference against, so the yardstick is tests/tiff_ref.py, a
// restatement of the rules over Python's zlib, held to Pillow's decodes where Pillow opens the file.
// The reader is split in two. LoadFromTIFFMemoryRaw does what is byte-serial - header, IFD, every refusal, LZW, PackBits, inflate - and
// ends in one stream of the segments' expanded bytes with a descriptor per segment. What happens to those bytes after that is
// csrc/dxtex_tiff.h's, which the GPU kernels share: the host loader runs it here, the resident forms at the end of this file run it on the
// device, so that a file's strips and tiles cross PCIe as they leave the decoder. The writer is split the same way around its rows.
#include "DirectXTexAMD_Internal.h"
#include "DirectXTexAMD_Inflate.h"
#include "../csrc/dxtex_tiff.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>

namespace DirectXTexAMD
{
static_assert(sizeof(TIFFRawImage::Segment) == sizeof(dxtex_tiff_segment) && sizeof(TIFFRawImage::Segment) == sizeof(dxtex::TiffSegment) &&
              sizeof(TIFFRawImage::Layout) == sizeof(dxtex_tiff_layout) && sizeof(TIFFRawImage::Layout) == sizeof(dxtex::TiffLayout), "the raw image's tables are the C ABI's");

namespace
{
    enum : uint16_t
    {
        kImageWidth = 256, kImageLength = 257, kBitsPerSample = 258, kCompression = 259, kPhotometric = 262, kFillOrder = 266, kStripOffsets = 273,
        kSamplesPerPixel = 277, kRowsPerStrip = 278, kStripByteCounts = 279, kXResolution = 282, kYResolution = 283, kPlanar = 284, kResolutionUnit = 296,
        kSoftware = 305, kPredictor = 317, kColorMap = 320, kTileWidth = 322, kTileLength = 323, kTileOffsets = 324, kTileByteCounts = 325,
        kExtraSamples = 338, kSampleFormat = 339, kExifIfd = 34665, kExifColorSpace = 40961,
    };
    enum : uint32_t { kNone = 1, kLzw = 5, kDeflate = 8, kAdobeDeflate = 32946, kPackBits = 32773 };
    enum : uint16_t { kByte = 1, kAscii = 2, kShort = 3, kLong = 4, kRational = 5 };
    constexpr size_t kDimensionMax = 0x0FFFFFFF;          // what the C ABI takes
    // no coder here makes more than this many bytes of one stored byte (LZW: a 12-bit code is a string of under 4096)
    constexpr uint64_t kExpansionMax = 4096;

    struct File
    {
        const uint8_t* d; size_t n; bool be;
        uint32_t U16(size_t at) const noexcept { return be ? (uint32_t(d[at]) << 8) | d[at + 1] : dxtex::le_load32(d + at, 2); }
        uint32_t U32(size_t at) const noexcept { return be ? dxtex::swap32(dxtex::le_load32(d + at, 4)) : dxtex::le_load32(d + at, 4); }
    };

    // one IFD entry: `count` values of `type` at `at` (checked against the file)
    struct Entry { uint32_t type = 0, count = 0; size_t at = 0; bool Has() const noexcept { return count != 0; } };

    inline size_t TypeBytes(uint32_t type) noexcept
    {
        static const uint8_t bytes[13] = { 0, 1, 1, 2, 4, 8, 1, 1, 2, 4, 8, 4, 8 };
        return type < 13 ? bytes[type] : 0;
    }

    // The entries of the IFD at `at` whose tags are tags[0..n): the first of each. E_FAIL for an IFD or a value that leaves the file.
    HRESULT ReadIfd(const File& f, size_t at, const uint16_t* tags, Entry* out, size_t n) noexcept
    {
        if (at < 8 || at > f.n || f.n - at < 6) return E_FAIL;
        const size_t count = f.U16(at);
        if ((f.n - at - 6) / 12 < count) return E_FAIL;          // the entries and the offset of the next IFD behind them
        for (size_t i = 0; i < count; ++i)
        {
            const size_t e = at + 2 + i * 12;
            const uint32_t tag = f.U16(e);
            for (size_t k = 0; k < n; ++k)
            {
                if (tags[k] != tag || out[k].Has()) continue;
                Entry v; v.type = f.U16(e + 2); v.count = f.U32(e + 4);
                const uint64_t bytes = uint64_t(TypeBytes(v.type)) * v.count;
                if (!bytes) return E_FAIL;          // a type this reader cannot size, or no values
                if (bytes <= 4) v.at = e + 8;
                else
                {
                    const uint32_t off = f.U32(e + 8);
                    if (off > f.n || bytes > f.n - off) return E_FAIL;
                    v.at = off;
                }
                out[k] = v;
            }
        }
        return S_OK;
    }

    // value k of an entry of BYTE, SHORT or LONG
    inline bool Value(const File& f, const Entry& e, size_t k, uint32_t& v) noexcept
    {
        if (k >= e.count) return false;
        if (e.type == kByte) v = f.d[e.at + k];
        else if (e.type == kShort) v = f.U16(e.at + 2 * k);
        else if (e.type == kLong) v = f.U32(e.at + 4 * k);
        else return false;
        return true;
    }
    // a tag of one value with a default
    inline HRESULT One(const File& f, const Entry& e, uint32_t fallback, uint32_t& v) noexcept
    {
        v = fallback;
        return !e.Has() || Value(f, e, 0, v) ? S_OK : E_FAIL;
    }
    // a tag of one value per sample, all equal; *equal = false where they are not
    inline HRESULT PerSample(const File& f, const Entry& e, uint32_t samples, uint32_t fallback, uint32_t& v, bool& equal) noexcept
    {
        v = fallback;
        if (!e.Has()) return S_OK;
        if (!Value(f, e, 0, v)) return E_FAIL;
        for (size_t k = 1; k < e.count && k < samples; ++k) { uint32_t o; if (!Value(f, e, k, o)) return E_FAIL; if (o != v) equal = false; }
        return S_OK;
    }

    enum Tag { T_WIDTH, T_LENGTH, T_BITS, T_COMPRESSION, T_PHOTOMETRIC, T_FILLORDER, T_STRIPOFFSETS, T_SAMPLES, T_ROWSPERSTRIP, T_STRIPCOUNTS, T_PLANAR, T_PREDICTOR,
               T_COLORMAP, T_TILEWIDTH, T_TILELENGTH, T_TILEOFFSETS, T_TILECOUNTS, T_EXTRA, T_FORMAT, T_EXIF, T_TAGS };
    constexpr uint16_t kTags[T_TAGS] = { kImageWidth, kImageLength, kBitsPerSample, kCompression, kPhotometric, kFillOrder, kStripOffsets, kSamplesPerPixel, kRowsPerStrip,
                                         kStripByteCounts, kPlanar, kPredictor, kColorMap, kTileWidth, kTileLength, kTileOffsets, kTileByteCounts, kExtraSamples, kSampleFormat, kExifIfd };

    // what the IFD says of the image
    struct Info
    {
        File file{};
        Entry tag[T_TAGS];
        TIFFRawImage::Layout layout{};
        uint32_t compression = kNone;
        bool tiled = false;
        uint32_t segRows = 0, segCols = 0;          // RowsPerStrip (at most the height) and the width, or a tile's size
        uint32_t across = 0, down = 0, planes = 1;          // segments across and down the image, and separate planes
        TexMetadata metadata;
    };

    HRESULT ParseInfo(const uint8_t* data, size_t size, TIFF_FLAGS flags, Info& info) noexcept
    {
        if (size < 8) return E_FAIL;
        File& f = info.file;
        if (data[0] == 'I' && data[1] == 'I') f = File{ data, size, false };
        else if (data[0] == 'M' && data[1] == 'M') f = File{ data, size, true };
        else return E_FAIL;
        const uint32_t magic = f.U16(2);
        if (magic == 43) return HRESULT_E_NOT_SUPPORTED;          // BigTIFF
        if (magic != 42) return E_FAIL;
        HRESULT hr = ReadIfd(f, f.U32(4), kTags, info.tag, T_TAGS);
        if (FAILED(hr)) return hr;
        const Entry* t = info.tag;
        uint32_t width = 0, height = 0, bits, format, samples, photometric, fillOrder, planar, predictor;
        if (!t[T_WIDTH].Has() || !t[T_LENGTH].Has() || !t[T_PHOTOMETRIC].Has()) return E_FAIL;
        if (!Value(f, t[T_WIDTH], 0, width) || !Value(f, t[T_LENGTH], 0, height) || !Value(f, t[T_PHOTOMETRIC], 0, photometric)) return E_FAIL;
        if (!width || !height || width > kDimensionMax || height > kDimensionMax) return E_FAIL;
        if (FAILED(One(f, t[T_SAMPLES], 1, samples)) || FAILED(One(f, t[T_COMPRESSION], kNone, info.compression)) || FAILED(One(f, t[T_FILLORDER], 1, fillOrder)) ||
            FAILED(One(f, t[T_PLANAR], 1, planar)) || FAILED(One(f, t[T_PREDICTOR], 1, predictor)))
            return E_FAIL;
        if (!samples || samples > 65535 || (planar != 1 && planar != 2) || (fillOrder != 1 && fillOrder != 2) || !predictor) return E_FAIL;
        if (info.compression == kNone || info.compression == kPackBits) predictor = 1;          // the predictor belongs to the LZW and deflate coders: libtiff ignores the tag elsewhere, and so does this reader
        bool equal = true;
        if (FAILED(PerSample(f, t[T_BITS], samples, 1, bits, equal)) || FAILED(PerSample(f, t[T_FORMAT], samples, 1, format, equal))) return E_FAIL;
        if ((t[T_BITS].Has() && t[T_BITS].count < samples) || (t[T_FORMAT].Has() && t[T_FORMAT].count < samples && t[T_FORMAT].count != 1)) return E_FAIL;

        // ---- the refusals ------------------------------------------------------------------------------------------------------------------
        if (info.compression != kNone && info.compression != kLzw && info.compression != kDeflate && info.compression != kAdobeDeflate && info.compression != kPackBits)
            return HRESULT_E_NOT_SUPPORTED;
        if (photometric > 3) return HRESULT_E_NOT_SUPPORTED;          // transparency masks, CMYK, YCbCr, CIELab and the rest
        if (fillOrder == 2) return HRESULT_E_NOT_SUPPORTED;
        if (!equal) return HRESULT_E_NOT_SUPPORTED;
        if (bits != 1 && bits != 4 && bits != 8 && bits != 16 && bits != 32) return HRESULT_E_NOT_SUPPORTED;
        if (format == 4) format = 1;
        if (format != 1 && format != 3) return HRESULT_E_NOT_SUPPORTED;          // signed, complex
        if ((format == 3) != (bits == 32)) return HRESULT_E_NOT_SUPPORTED;       // 16- and 64-bit floats (64 fell above), 32-bit integers
        const uint32_t colours = photometric == 2 ? 3u : 1u;
        if (samples < colours) return E_FAIL;
        const uint32_t extras = samples - colours;
        if (t[T_EXTRA].Has() && t[T_EXTRA].count != extras) return E_FAIL;
        if (extras > 1) return HRESULT_E_NOT_SUPPORTED;
        if (extras && colours == 1) return HRESULT_E_NOT_SUPPORTED;          // grey plus alpha, palette plus alpha
        if (colours == 3 && bits < 8) return HRESULT_E_NOT_SUPPORTED;
        if (photometric == 3 && bits > 8) return HRESULT_E_NOT_SUPPORTED;
        if (photometric == 0 && bits == 32) return HRESULT_E_NOT_SUPPORTED;
        if (!dxtex::tiff_predictor_fits(predictor, bits)) return HRESULT_E_NOT_SUPPORTED;
        if (photometric == 3 && (!t[T_COLORMAP].Has() || t[T_COLORMAP].type != kShort || t[T_COLORMAP].count < (3u << bits))) return E_FAIL;

        uint32_t kind;
        if (photometric == 3) kind = bits == 1 ? dxtex::TIFF_PAL1 : bits == 4 ? dxtex::TIFF_PAL4 : dxtex::TIFF_PAL8;
        else if (colours == 1) kind = bits == 1 ? dxtex::TIFF_GREY1 : bits == 4 ? dxtex::TIFF_GREY4 : bits == 8 ? dxtex::TIFF_GREY8 : bits == 16 ? dxtex::TIFF_GREY16 : dxtex::TIFF_GREY32F;
        else kind = (bits == 8 ? dxtex::TIFF_RGB8 : bits == 16 ? dxtex::TIFF_RGB16 : dxtex::TIFF_RGB32F) + extras;
        uint32_t extra = 0;          // unspecified
        if (extras && t[T_EXTRA].Has() && !Value(f, t[T_EXTRA], 0, extra)) return E_FAIL;
        const bool opaque = extras && extra != 1 && extra != 2;
        info.layout = TIFFRawImage::Layout{ width, height, bits, samples, kind, predictor, f.be ? 1u : 0u, planar == 2 && samples > 1 ? 1u : 0u, photometric == 0 ? 1u : 0u, opaque ? 1u : 0u };
        info.planes = info.layout.planar ? samples : 1u;

        // ---- strips or tiles -----------------------------------------------------------------------------------------------------------------
        info.tiled = t[T_TILEOFFSETS].Has();
        if (info.tiled)
        {
            if (!t[T_TILEWIDTH].Has() || !t[T_TILELENGTH].Has() || !t[T_TILECOUNTS].Has()) return E_FAIL;
            if (!Value(f, t[T_TILEWIDTH], 0, info.segCols) || !Value(f, t[T_TILELENGTH], 0, info.segRows)) return E_FAIL;
            if (!info.segCols || !info.segRows || info.segCols > kDimensionMax || info.segRows > kDimensionMax) return E_FAIL;
        }
        else
        {
            if (!t[T_STRIPOFFSETS].Has() || !t[T_STRIPCOUNTS].Has()) return E_FAIL;
            uint32_t rows;
            if (FAILED(One(f, t[T_ROWSPERSTRIP], 0xFFFFFFFFu, rows)) || !rows) return E_FAIL;
            info.segRows = std::min(rows, height); info.segCols = width;
        }
        info.across = (width + info.segCols - 1) / info.segCols; info.down = (height + info.segRows - 1) / info.segRows;
        const uint64_t count = uint64_t(info.across) * info.down * info.planes;
        const Entry& offsets = t[info.tiled ? T_TILEOFFSETS : T_STRIPOFFSETS]; const Entry& counts = t[info.tiled ? T_TILECOUNTS : T_STRIPCOUNTS];
        if (offsets.count < count || counts.count < count) return E_FAIL;
        if ((offsets.type != kShort && offsets.type != kLong) || (counts.type != kShort && counts.type != kLong)) return E_FAIL;
        if (uint64_t(dxtex::tiff_row_bytes(info.segCols, info.layout.planar ? 1u : samples, 32)) > 0x3FFFFFFFu) return E_FAIL;          // rowBytes is 32 bits

        // ---- the colour space: the Exif IFD's ColorSpace --------------------------------------------------------------------------------------
        bool srgb = false;
        if (dxtex::tiff_may_be_srgb(kind))
        {
            bool named = false;
            if (t[T_EXIF].Has())
            {
                uint32_t at;
                if (t[T_EXIF].type != kLong || !Value(f, t[T_EXIF], 0, at)) return E_FAIL;
                const uint16_t tag = kExifColorSpace; Entry space;
                hr = ReadIfd(f, at, &tag, &space, 1);
                if (FAILED(hr)) return hr;
                uint32_t v;
                if (space.Has()) { if (!Value(f, space, 0, v)) return E_FAIL; named = true; srgb = v == 1; }
            }
            if (!named && (flags & TIFF_FLAGS_DEFAULT_SRGB)) srgb = true;
            if (flags & TIFF_FLAGS_IGNORE_SRGB) srgb = false;
        }
        TexMetadata& m = info.metadata;
        m = TexMetadata();
        m.width = width; m.height = height; m.depth = m.arraySize = m.mipLevels = 1;
        m.format = srgb ? DXGI_FORMAT_R8G8B8A8_UNORM_SRGB : DXGI_FORMAT(dxtex::tiff_kind_row(kind).format);
        m.dimension = TEX_DIMENSION_TEXTURE2D;
        if (dxtex::tiff_is_palette(kind) || (colours == 3 && kind != dxtex::TIFF_RGB32F))          // the image has an alpha channel
        {
            if (!extras || opaque) m.SetAlphaMode(TEX_ALPHA_MODE_OPAQUE);
            else if (extra == 1) m.SetAlphaMode(TEX_ALPHA_MODE_PREMULTIPLIED);
        }
        return S_OK;
    }

    // PackBits at [in, in + n) into out[0, cap): true when cap bytes came out (a surplus is not decoded)
    bool Unpackbits(const uint8_t* in, size_t n, uint8_t* out, size_t cap) noexcept
    {
        size_t at = 0, pos = 0;
        while (pos < cap)
        {
            if (at == n) return false;
            const int c = int8_t(in[at++]);
            if (c == -128) continue;
            if (c < 0)
            {
                if (at == n) return false;
                const size_t k = std::min(size_t(1 - c), cap - pos);
                std::memset(out + pos, in[at++], k);
                pos += k;
            }
            else
            {
                const size_t k = size_t(c) + 1;
                if (n - at < k) return false;
                std::memcpy(out + pos, in + at, std::min(k, cap - pos));
                at += k; pos += std::min(k, cap - pos);
            }
        }
        return true;
    }

    // TIFF's LZW (MSB-first codes of 9 to 12 bits, the width changing one code early) at [in, in + n) into out[0, cap): S_OK when cap
    // bytes came out (a surplus is not decoded), HRESULT_E_NOT_SUPPORTED for the old LSB-first form, E_FAIL for every defect
    HRESULT Unlzw(const uint8_t* in, size_t n, uint8_t* out, size_t cap) noexcept
    {
        if (n >= 2 && in[0] == 0 && (in[1] & 1)) return HRESULT_E_NOT_SUPPORTED;          // a Clear code written LSB-first
        struct Table { uint16_t prefix[4096]; uint8_t suffix[4096], first[4096]; uint16_t length[4096]; };
        std::unique_ptr<Table> t(new (std::nothrow) Table);
        if (!t) return E_OUTOFMEMORY;
        for (uint32_t i = 0; i < 256; ++i) { t->prefix[i] = 0; t->suffix[i] = t->first[i] = uint8_t(i); t->length[i] = 1; }
        uint32_t next = 258, width = 9, buf = 0, have = 0;
        int old = -1;
        size_t at = 0, pos = 0;
        // string `code` at out[pos..), cut at cap
        auto emit = [&](uint32_t code)
        {
            const size_t len = t->length[code], room = cap - pos;
            for (size_t k = len; k-- > 0; code = t->prefix[code]) if (k < room) out[pos + k] = t->suffix[code];
            pos += std::min(len, room);
        };
        while (pos < cap)
        {
            while (have < width) { if (at == n) return E_FAIL; buf = (buf << 8) | in[at++]; have += 8; }
            const uint32_t code = (buf >> (have - width)) & ((1u << width) - 1u);
            have -= width;
            if (code == 257) return E_FAIL;          // the end, short of cap
            if (code == 256) { next = 258; width = 9; old = -1; continue; }
            if (old < 0)
            {
                if (code > 255) return E_FAIL;
                emit(code); old = int(code);
                continue;
            }
            // an entry, or the one this step makes
            if (code > next || (code == next && next > 4095)) return E_FAIL;
            if (next < 4096)
            {
                t->prefix[next] = uint16_t(old); t->first[next] = t->first[old]; t->length[next] = uint16_t(t->length[old] + 1);
                t->suffix[next] = code < next ? t->first[code] : t->first[old];
                ++next;
            }
            emit(code); old = int(code);
            if (next + 1 == (1u << width) && width < 12) ++width;
        }
        return S_OK;
    }

    HRESULT ReadTIFFFile(const char* szFile, Blob& buf) noexcept
    {
        FILE* f = std::fopen(szFile, "rb");
        if (!f) return errno == ENOENT ? HRESULT_ERROR_FILE_NOT_FOUND : E_FAIL;
        std::fseek(f, 0, SEEK_END); const long n = std::ftell(f); std::fseek(f, 0, SEEK_SET);
        if (n < 1) { std::fclose(f); return E_FAIL; }
        if (uint64_t(n) > UINT32_MAX) { std::fclose(f); return HRESULT_E_FILE_TOO_LARGE; }
        const HRESULT hr = buf.Initialize(size_t(n));
        if (FAILED(hr)) { std::fclose(f); return hr; }
        const size_t got = std::fread(buf.GetBufferPointer(), 1, buf.GetBufferSize(), f);
        std::fclose(f);
        return got == buf.GetBufferSize() ? S_OK : E_FAIL;
    }

    inline dxtex::TiffLayout LayoutOf(const TIFFRawImage::Layout& l) noexcept
    {
        return dxtex::TiffLayout{ l.width, l.height, l.bits, l.samples, l.kind, l.predictor, l.bigEndian, l.planar, l.whiteIsZero, l.opaque };
    }
    inline dxtex::TiffSegment SegmentOf(const TIFFRawImage::Segment& s) noexcept { return dxtex::TiffSegment{ s.offset, s.firstRow, s.rows, s.firstCol, s.cols, s.rowBytes, s.plane }; }

    // ---- the writer: the file around its rows --------------------------------------------------------------------------------------------------
    struct FileShape { dxtex::TiffSource source; bool srgb; size_t rowBytes, dataBytes, headBytes, fileBytes; uint32_t entries; };
    constexpr char kSoftwareName[] = "DirectXTex";          // 11 bytes with its NUL
    HRESULT SaveChecks(const Image& image, TIFF_FLAGS flags, FileShape& s) noexcept
    {
        if (!image.pixels) return E_POINTER;
        s.source = dxtex::tiff_pack_source(int(image.format));
        if (!s.source.bits) return HRESULT_E_NOT_SUPPORTED;
        if (!image.width || !image.height) return E_INVALIDARG;
        if (image.width > kDimensionMax || image.height > kDimensionMax) return HRESULT_E_NOT_SUPPORTED;
        s.srgb = (s.source.srgb || (flags & TIFF_FLAGS_FORCE_SRGB)) && !(flags & TIFF_FLAGS_FORCE_LINEAR);
        const uint32_t S = s.source.samples;
        s.entries = 15u + (S == 4 ? 1u : 0u) + (s.srgb ? 1u : 0u);
        // header, IFD, the values that do not fit an entry (bits and formats of more than two samples, two rationals, the software name),
        // the Exif IFD; the rows start on a multiple of 16
        size_t head = 8 + 2 + size_t(s.entries) * 12 + 4 + (S > 2 ? 2 * 2 * S : 0) + 16 + 12 + (s.srgb ? 2 + 12 + 4 : 0);
        s.headBytes = (head + 15) & ~size_t(15);
        s.rowBytes = image.width * s.source.fileBytes;
        if (image.height > (size_t(UINT32_MAX) - s.headBytes) / s.rowBytes) return HRESULT_E_NOT_SUPPORTED;          // classic TIFF holds 32-bit offsets
        s.dataBytes = s.rowBytes * image.height;
        s.fileBytes = s.headBytes + s.dataBytes;
        return S_OK;
    }

    struct Writer
    {
        uint8_t* base; uint8_t* p; uint8_t* extra;          // the next entry, and the next value that does not fit one
        void U16(uint32_t v) noexcept { dxtex::le_store32(p, v, 2); p += 2; }
        void U32(uint32_t v) noexcept { dxtex::le_store32(p, v, 4); p += 4; }
        void Entry(uint16_t tag, uint16_t type, uint32_t count, uint32_t value) noexcept { U16(tag); U16(type); U32(count); U32(value); }
        // `count` SHORTs of one value
        void Shorts(uint16_t tag, uint32_t count, uint32_t value) noexcept
        {
            if (count <= 2) { Entry(tag, kShort, count, count == 2 ? value | (value << 16) : value); return; }
            Entry(tag, kShort, count, uint32_t(extra - base));
            for (uint32_t i = 0; i < count; ++i) { dxtex::le_store32(extra, value, 2); extra += 2; }
        }
        void Rational(uint16_t tag, uint32_t num, uint32_t den) noexcept
        {
            Entry(tag, kRational, 1, uint32_t(extra - base));
            dxtex::le_store32(extra, num, 4); dxtex::le_store32(extra + 4, den, 4); extra += 8;
        }
    };

    // header and IFD; then rows(first) leaves the file's tight rows at `first`
    template<class Rows>
    HRESULT WriteFile(const Image& image, const FileShape& s, Blob& blob, Rows&& rows) noexcept
    {
        blob.Release();
        HRESULT hr = blob.Initialize(s.fileBytes);
        if (FAILED(hr)) return hr;
        uint8_t* b = blob.GetBufferPointer();
        std::memset(b, 0, s.headBytes);
        const uint32_t S = s.source.samples;
        Writer w{ b, b, b + 8 + 2 + size_t(s.entries) * 12 + 4 };
        w.U16(0x4949); w.U16(42); w.U32(8);
        w.U16(s.entries);
        w.Entry(kImageWidth, kLong, 1, uint32_t(image.width));
        w.Entry(kImageLength, kLong, 1, uint32_t(image.height));
        w.Shorts(kBitsPerSample, S, s.source.bits);
        w.Entry(kCompression, kShort, 1, kNone);
        w.Entry(kPhotometric, kShort, 1, S == 1 ? 1 : 2);
        w.Entry(kStripOffsets, kLong, 1, uint32_t(s.headBytes));
        w.Entry(kSamplesPerPixel, kShort, 1, S);
        w.Entry(kRowsPerStrip, kLong, 1, uint32_t(image.height));
        w.Entry(kStripByteCounts, kLong, 1, uint32_t(s.dataBytes));
        w.Rational(kXResolution, 72, 1);
        w.Rational(kYResolution, 72, 1);
        w.Entry(kPlanar, kShort, 1, 1);
        w.Entry(kResolutionUnit, kShort, 1, 2);
        w.Entry(kSoftware, kAscii, sizeof(kSoftwareName), uint32_t(w.extra - b));
        std::memcpy(w.extra, kSoftwareName, sizeof(kSoftwareName)); w.extra += 12;          // kept even
        if (S == 4) w.Entry(kExtraSamples, kShort, 1, 2);
        w.Shorts(kSampleFormat, S, s.source.sampleFormat);
        if (s.srgb)
        {
            w.Entry(kExifIfd, kLong, 1, uint32_t(w.extra - b));
            Writer e{ b, w.extra, nullptr };
            e.U16(1); e.Entry(kExifColorSpace, kShort, 1, 1); e.U32(0);
            w.extra = e.p;
        }
        w.U32(0);          // no further IFD
        if (size_t(w.extra - b) > s.headBytes || size_t(w.p - b) != 8 + 2 + size_t(s.entries) * 12 + 4) { blob.Release(); return E_UNEXPECTED; }
        hr = rows(b + s.headBytes);
        if (FAILED(hr)) blob.Release();
        return hr;
    }

    HRESULT SaveHost(const Image& image, TIFF_FLAGS flags, Blob& blob) noexcept
    {
        blob.Release();
        FileShape s;
        const HRESULT hr = SaveChecks(image, flags, s);
        if (FAILED(hr)) return hr;
        if (image.rowPitch < image.width * s.source.imageBytes) return E_INVALIDARG;
        return WriteFile(image, s, blob, [&](uint8_t* first)
        {
            for (size_t y = 0; y < image.height; ++y)
            {
                const uint8_t* src = image.pixels + y * image.rowPitch; uint8_t* d = first + y * s.rowBytes;
                if (!s.source.bgr) { std::memcpy(d, src, s.rowBytes); continue; }
                for (size_t x = 0; x < image.width; ++x) dxtex::le_store32(d + x * s.source.fileBytes, dxtex::tiff_pack_bgr(dxtex::le_load32(src + x * 4, 4)), s.source.fileBytes);
            }
            return S_OK;
        });
    }

    HRESULT SaveResident(Device& device, const Image& deviceImage, TIFF_FLAGS flags, Blob& blob) noexcept
    {
        blob.Release();
        FileShape s;
        const HRESULT hr = SaveChecks(deviceImage, flags, s);
        if (FAILED(hr)) return hr;
        if (!device) return E_POINTER;
        const dxtex_image src = ImageOf(deviceImage);
        return WriteFile(deviceImage, s, blob, [&](uint8_t* first) -> HRESULT
        {
            // a source whose rows are the file's comes down through its pitch; a BGR one is swizzled into tight rows first
            if (!s.source.bgr)
            {
                HRESULT r = dxtex_memcpy_rows_d2h_async(device.Get(), first, s.rowBytes, deviceImage.pixels, deviceImage.rowPitch, s.rowBytes, deviceImage.height);
                if (SUCCEEDED(r)) r = dxtex_ctx_synchronize(device.Get());
                return r;
            }
            return PackAndDownload(device, s.dataBytes, first, [&](void* p) { return dxtex_tiff_pack_device(device.Get(), &src, p, s.dataBytes); });
        });
    }
}

void TIFFRawImage::Release() noexcept
{
    storage.Release();
    segments.reset();
    compression = 0; layout = Layout{};
    std::memset(palette, 0, sizeof(palette));
    segmentCount = storedBytes = streamBytes = 0;
    stream = nullptr;
}

HRESULT GetMetadataFromTIFFMemory(const void* pSource, size_t size, TIFF_FLAGS flags, TexMetadata& metadata) noexcept
{
    if (!pSource) return E_INVALIDARG;
    Info info;
    const HRESULT hr = ParseInfo(static_cast<const uint8_t*>(pSource), size, flags, info);
    if (SUCCEEDED(hr)) metadata = info.metadata;
    return hr;
}

HRESULT GetMetadataFromTIFFFile(const char* szFile, TIFF_FLAGS flags, TexMetadata& metadata) noexcept
{
    return LoadFile(szFile, ReadTIFFFile, [&](const uint8_t* p, size_t n) { return GetMetadataFromTIFFMemory(p, n, flags, metadata); });
}

HRESULT LoadFromTIFFMemoryRaw(const void* pSource, size_t size, TIFF_FLAGS flags, TexMetadata* metadata, TIFFRawImage& raw) noexcept
{
    raw.Release();
    if (!pSource) return E_INVALIDARG;
    const uint8_t* data = static_cast<const uint8_t*>(pSource);
    Info info;
    HRESULT hr = ParseInfo(data, size, flags, info);
    if (FAILED(hr)) return hr;
    const File& f = info.file;
    const TIFFRawImage::Layout& l = info.layout;
    const Entry& offsets = info.tag[info.tiled ? T_TILEOFFSETS : T_STRIPOFFSETS]; const Entry& counts = info.tag[info.tiled ? T_TILECOUNTS : T_STRIPCOUNTS];
    const size_t perPlane = size_t(info.across) * info.down, count = perPlane * info.planes;
    const uint32_t rowBytes = dxtex::tiff_row_bytes(info.segCols, l.planar ? 1u : l.samples, l.bits);

    // where every segment lies in the file and in the stream: strips that follow one another share a descriptor, every other segment
    // starts on a multiple of 16 bytes
    if (count > size) return E_FAIL;          // every segment has an offset of at least two bytes in the file
    std::unique_ptr<TIFFRawImage::Segment[]> segments(new (std::nothrow) TIFFRawImage::Segment[count]);
    if (!segments) return E_OUTOFMEMORY;
    uint64_t streamBytes = 0, stored = 0;
    for (size_t i = 0; i < count; ++i)
    {
        uint32_t off = 0, n = 0;
        if (!Value(f, offsets, i, off) || !Value(f, counts, i, n)) return E_FAIL;
        if (off > size || n > size - off) return E_FAIL;
        const size_t plane = i / perPlane, j = i % perPlane, ty = j / info.across, tx = j % info.across;
        TIFFRawImage::Segment s{};
        s.firstRow = uint32_t(ty * info.segRows); s.rows = std::min(info.segRows, l.height - s.firstRow);
        s.firstCol = uint32_t(tx * info.segCols); s.cols = std::min(info.segCols, l.width - s.firstCol);
        s.rowBytes = rowBytes; s.plane = uint32_t(plane);
        const bool follows = !info.tiled && j != 0;
        if (!follows) streamBytes = (streamBytes + 15) & ~uint64_t(15);
        s.offset = streamBytes;
        streamBytes += uint64_t(s.rows) * rowBytes;
        stored += n;
        segments[i] = s;
    }
    if (streamBytes / kExpansionMax > size) return E_FAIL;
    hr = raw.storage.Initialize(size_t(streamBytes));
    if (FAILED(hr)) return hr;
    uint8_t* stream = raw.storage.GetBufferPointer();
    size_t used = 0;
    uint64_t end = 0;
    for (size_t i = 0; i < count; ++i)
    {
        const TIFFRawImage::Segment s = segments[i];
        uint32_t off = 0, n = 0;
        (void)Value(f, offsets, i, off); (void)Value(f, counts, i, n);
        const uint8_t* body = data + off;
        const size_t bytes = size_t(s.rows) * s.rowBytes;
        if (s.offset > end) std::memset(stream + end, 0, size_t(s.offset - end));          // the bytes in front of an aligned segment
        uint8_t* out = stream + s.offset;
        hr = S_OK;
        if (info.compression == kNone) { if (n < bytes) hr = E_FAIL; else std::memcpy(out, body, bytes); }
        else if (info.compression == kPackBits) hr = Unpackbits(body, n, out, bytes) ? S_OK : E_FAIL;
        else if (info.compression == kLzw) hr = Unlzw(body, n, out, bytes);
        else hr = Inflate(body, n, out, bytes) ? S_OK : E_FAIL;
        if (FAILED(hr)) { raw.Release(); return hr; }
        end = s.offset + bytes;
        TIFFRawImage::Segment* last = used ? &segments[used - 1] : nullptr;
        if (last && !info.tiled && last->plane == s.plane && last->offset + uint64_t(last->rows) * last->rowBytes == s.offset && last->firstRow + last->rows == s.firstRow)
            last->rows += s.rows;
        else segments[used++] = s;
    }
    if (dxtex::tiff_is_palette(l.kind))
    {
        const Entry& map = info.tag[T_COLORMAP];
        const uint32_t entries = 1u << l.bits;
        for (uint32_t i = 0; i < entries; ++i)
            raw.palette[i] = (f.U16(map.at + 2 * i) >> 8) | ((f.U16(map.at + 2 * (entries + i)) >> 8) << 8) | ((f.U16(map.at + 2 * (2 * entries + i)) >> 8) << 16) | 0xFF000000u;
    }
    raw.compression = info.compression; raw.layout = l;
    raw.segments = std::move(segments); raw.segmentCount = used; raw.storedBytes = size_t(stored);
    raw.stream = stream; raw.streamBytes = size_t(streamBytes);
    if (metadata) *metadata = info.metadata;
    return S_OK;
}

HRESULT LoadFromTIFFFileRaw(const char* szFile, TIFF_FLAGS flags, TexMetadata* metadata, TIFFRawImage& raw) noexcept
{
    raw.Release();
    // the segments are always expanded into storage of their own: the file is not kept
    return LoadFile(szFile, ReadTIFFFile, [&](const uint8_t* p, size_t n) { return LoadFromTIFFMemoryRaw(p, n, flags, metadata, raw); });
}

HRESULT LoadFromTIFFMemory(const void* pSource, size_t size, TIFF_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept
{
    image.Release();          // on any failure the result is empty
    TexMetadata mdata; TIFFRawImage raw;
    HRESULT hr = LoadFromTIFFMemoryRaw(pSource, size, flags, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = image.Initialize(mdata);          // the alpha mode stays with the image
    if (FAILED(hr)) return hr;
    const Image* img = image.GetImage(0, 0, 0);
    if (!img) { image.Release(); return E_POINTER; }
    const dxtex::TiffLayout l = LayoutOf(raw.layout);
    const uint32_t B = dxtex::tiff_kind_row(l.kind).imageBytes, E = l.bits / 8;
    uint8_t* stream = raw.storage.GetBufferPointer();
    for (size_t i = 0; i < raw.segmentCount; ++i)
    {
        const dxtex::TiffSegment s = SegmentOf(raw.segments[i]);
        dxtex::tiff_undo_segment_serial(stream, s, l);
        for (uint32_t r = 0; r < s.rows; ++r)
        {
            const uint8_t* row = stream + s.offset + uint64_t(r) * s.rowBytes;
            uint8_t* d = img->pixels + size_t(s.firstRow + r) * img->rowPitch + size_t(s.firstCol) * B;
            for (uint32_t x = 0; x < s.cols; ++x, d += B)
            {
                if (l.planar)
                {
                    dxtex::le_store32(d + s.plane * E, dxtex::tiff_plane_component(row, s.rowBytes, l, s.plane, x), E);
                    if (s.plane == 0 && dxtex::tiff_fills_alpha(l)) dxtex::le_store32(d + 3 * E, dxtex::tiff_alpha_max(l.bits), E);
                    continue;
                }
                uint32_t t[4];
                dxtex::tiff_texel(row, s.rowBytes, l, raw.palette, x, t);
                for (uint32_t b = 0; b < B; b += 4) dxtex::le_store32(d + b, t[b / 4], std::min(4u, B - b));
            }
        }
    }
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromTIFFFile(const char* szFile, TIFF_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept
{
    image.Release();
    return LoadFile(szFile, ReadTIFFFile, [&](const uint8_t* p, size_t n) { return LoadFromTIFFMemory(p, n, flags, metadata, image); });
}

HRESULT SaveToTIFFMemory(const Image& image, TIFF_FLAGS flags, Blob& blob) noexcept { return SaveHost(image, flags, blob); }

HRESULT SaveToTIFFFile(const Image& image, TIFF_FLAGS flags, const char* szFile) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveHost(image, flags, blob); });
}

// ---- resident forms: the stream travels as it left the decoder, everything behind it runs on the device (dxtex_tiff_unpack_device / dxtex_tiff_pack_device) ----
HRESULT UploadTIFFRaw(Device& device, const TexMetadata& metadata, const TIFFRawImage& raw, DeviceScratchImage& image) noexcept
{
    image.Release();
    if (!device) return E_POINTER;
    if (!raw.stream || !raw.segments || !raw.segmentCount || metadata.arraySize != 1 || metadata.mipLevels != 1 || metadata.depth != 1) return E_INVALIDARG;
    return InitializeAndFill(device, metadata, image, [&](const Image& img) -> HRESULT
    {
        const TIFFRawImage::Segment& s = raw.segments[0];
        if (dxtex::tiff_is_native(LayoutOf(raw.layout)) && raw.segmentCount == 1 && s.firstCol == 0 && s.cols == raw.layout.width && s.rows == raw.layout.height &&
            img.rowPitch == s.rowBytes && s.rowBytes == img.width * dxtex::tiff_kind_row(raw.layout.kind).imageBytes)
            return dxtex_memcpy_h2d(device.Get(), img.pixels, raw.stream + s.offset, size_t(s.rows) * s.rowBytes);          // the rows are the image: one copy, no kernel
        // the stream starts an allocation of its own, and its segments lie on multiples of 16 bytes
        const dxtex_image d = ImageOf(img);
        return UploadAndUnpack(device, raw.stream, raw.streamBytes, [&](void* p)
        {
            return dxtex_tiff_unpack_device(device.Get(), p, raw.streamBytes, reinterpret_cast<const dxtex_tiff_segment*>(raw.segments.get()), raw.segmentCount,
                                            reinterpret_cast<const dxtex_tiff_layout*>(&raw.layout), dxtex::tiff_is_palette(raw.layout.kind) ? raw.palette : nullptr, &d);
        });
    });
}

HRESULT LoadFromTIFFMemory(Device& device, const void* pSource, size_t size, TIFF_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();          // on any failure the result is empty
    TexMetadata mdata; TIFFRawImage raw;
    HRESULT hr = LoadFromTIFFMemoryRaw(pSource, size, flags, &mdata, raw);
    if (FAILED(hr)) return hr;
    hr = UploadTIFFRaw(device, mdata, raw, image);
    if (FAILED(hr)) return hr;
    if (metadata) *metadata = mdata;
    return S_OK;
}

HRESULT LoadFromTIFFFile(Device& device, const char* szFile, TIFF_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept
{
    image.Release();
    return LoadFile(szFile, ReadTIFFFile, [&](const uint8_t* p, size_t n) { return LoadFromTIFFMemory(device, p, n, flags, metadata, image); });
}

HRESULT SaveToTIFFMemory(Device& device, const Image& deviceImage, TIFF_FLAGS flags, Blob& blob) noexcept { return SaveResident(device, deviceImage, flags, blob); }

HRESULT SaveToTIFFFile(Device& device, const Image& deviceImage, TIFF_FLAGS flags, const char* szFile) noexcept
{
    return SaveFile(szFile, [&](Blob& blob) { return SaveResident(device, deviceImage, flags, blob); });
}
} // namespace DirectXTexAMD
