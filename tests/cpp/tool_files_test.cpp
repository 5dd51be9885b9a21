// tool_files_test: the tools' shared header (directxtex_amd/tools/tool_files.h) without a device. Driven by tests/test_tool_files_cpu.py.
//   tool_files_test tables            the file-type table and the format-name table against rules written out here
//   tool_files_test parse <file>...   SourceFile::Parse and GetMetadata against the codec's own calls, one line a file:
//                                     "<file> type <n> parse <hr> direct <hr> metadata <hr>"; any disagreement is reported and the exit code is 1
#include "../../directxtex_amd/tools/tool_files.h"

#include <cctype>

using namespace tool;

namespace
{
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

std::string Upper(std::string s) { for (char& c : s) c = char(std::toupper(static_cast<unsigned char>(c))); return s; }

void Tables()
{
    // every row, in both cases, with and without a directory; .jpg and .jpeg are one type
    size_t rows = 0;
    for (const FileTypeRow& r : kFileTypes)
    {
        ++rows;
        EXPECT(FileTypeOf(std::string("x") + r.ext) == r.type);
        EXPECT(FileTypeOf("dir.dds/" + Upper(std::string("name") + r.ext)) == r.type);
        EXPECT(FileTypeOf(r.ext) == r.type);                      // the one hasExt rule: a name that is only the extension
        EXPECT(hasExt(ExtensionOf(r.type), ExtensionOf(r.type)) && FileTypeOf(ExtensionOf(r.type)) == r.type);
        if (r.ft) { EXPECT(FileTypeOfFt(r.ft) == r.type); EXPECT(FileTypeOfFt(Upper(r.ft).c_str()) == r.type); EXPECT(std::string(".") + r.ft == r.ext); }
    }
    EXPECT(rows == 10);
    EXPECT(FileTypeOf("x.jpeg") == FileType::JPEG && FileTypeOf("x.jpg") == FileType::JPEG);
    EXPECT(FileTypeOf("x") == FileType::UNKNOWN);
    EXPECT(FileTypeOf("") == FileType::UNKNOWN);
    EXPECT(FileTypeOf(".dds") == FileType::DDS);
    EXPECT(FileTypeOf("a.dds.bak") == FileType::UNKNOWN);
    EXPECT(FileTypeOf("x.bmp") == FileType::UNKNOWN);
    EXPECT(FileTypeOf("xdds") == FileType::UNKNOWN);
    EXPECT(std::string(ExtensionOf(FileType::JPEG)) == ".jpg" && std::string(ExtensionOf(FileType::DDS)) == ".dds" && std::string(ExtensionOf(FileType::UNKNOWN)).empty());
    // -ft: the names dxtexconv takes; .phm is read only
    const struct { const char* ft; FileType type; } fts[] = {
        { "dds", FileType::DDS }, { "hdr", FileType::HDR }, { "tga", FileType::TGA }, { "ppm", FileType::PPM }, { "pfm", FileType::PFM }, { "png", FileType::PNG },
        { "exr", FileType::EXR }, { "jpg", FileType::JPEG }, { "jpeg", FileType::JPEG }, { "JPG", FileType::JPEG }, { "bmp", FileType::UNKNOWN }, { "phm", FileType::UNKNOWN },
        { "", FileType::UNKNOWN }, { ".png", FileType::UNKNOWN },
    };
    for (const auto& f : fts) EXPECT(FileTypeOfFt(f.ft) == f.type);

    // formats: every value answers with its first name, and that name finds the value again, in either case
    for (const Name& n : kFormats)
    {
        const char* canonical = FormatName(DXGI_FORMAT(n.value));
        const Name* first = nullptr;
        for (const Name& m : kFormats) if (m.value == n.value) { first = &m; break; }
        EXPECT(first && canonical == first->name);
        uint32_t v = 0;
        EXPECT(lookup(kFormats, n.name, v) && v == n.value);
        v = 0;
        EXPECT(lookup(kFormats, Upper(n.name).c_str(), v) && v == n.value);
    }
    // the aliases, as the three tools' own tables had them
    const Name aliases[] = { { "DXT1", 71 }, { "DXT2", 74 }, { "DXT3", 74 }, { "DXT4", 77 }, { "DXT5", 77 }, { "RGBA", 28 }, { "BGRA", 87 }, { "BGR", 88 }, { "FP16", 10 }, { "FP32", 2 } };
    for (const Name& a : aliases)
    {
        uint32_t v = 0;
        EXPECT(lookup(kFormats, a.name, v) && v == a.value);
        EXPECT(std::string(FormatName(DXGI_FORMAT(a.value))) != a.name);          // an alias is never the canonical name
    }
    EXPECT(std::string(FormatName(DXGI_FORMAT_BC1_UNORM)) == "BC1_UNORM" && std::string(FormatName(DXGI_FORMAT_R8G8B8A8_UNORM)) == "R8G8B8A8_UNORM");
    EXPECT(std::string(FormatName(DXGI_FORMAT_B8G8R8X8_UNORM)) == "B8G8R8X8_UNORM" && std::string(FormatName(DXGI_FORMAT_R32G32B32A32_FLOAT)) == "R32G32B32A32_FLOAT");
    EXPECT(std::string(FormatName(DXGI_FORMAT(0))) == "*UNKNOWN*" && std::string(FormatName(DXGI_FORMAT(0), "")).empty());
    // dxtexconv's block aliases are its own; numbers only where asked for
    uint32_t v = 0;
    for (const char* s : { "BC4", "BC5", "BC6H", "BC7", "28", "NOT_A_FORMAT", "" }) EXPECT(!lookup(kFormats, s, v));
    EXPECT(lookup(kFormats, "28", v, true) && v == 28);
    EXPECT(lookup(kFormats, "0x1C", v, true) && v == 28);
    EXPECT(!lookup(kFormats, "28x", v, true) && !lookup(kFormats, "", v, true));

    EXPECT(PngBgrFor(DXGI_FORMAT_B8G8R8A8_UNORM) == PNG_FLAGS_BGR && PngBgrFor(DXGI_FORMAT_B8G8R8X8_UNORM) == PNG_FLAGS_BGR);
    EXPECT(PngBgrFor(DXGI_FORMAT_B8G8R8A8_UNORM_SRGB) == PNG_FLAGS_BGR && PngBgrFor(DXGI_FORMAT_B8G8R8X8_UNORM_SRGB) == PNG_FLAGS_BGR);
    EXPECT(PngBgrFor(DXGI_FORMAT_R8G8B8A8_UNORM) == PNG_FLAGS_NONE && PngBgrFor(0) == PNG_FLAGS_NONE && PngBgrFor(DXGI_FORMAT_B5G6R5_UNORM) == PNG_FLAGS_NONE);
}

bool Same(const TexMetadata& a, const TexMetadata& b)
{
    return a.width == b.width && a.height == b.height && a.depth == b.depth && a.arraySize == b.arraySize && a.mipLevels == b.mipLevels &&
           a.miscFlags == b.miscFlags && a.miscFlags2 == b.miscFlags2 && a.format == b.format && a.dimension == b.dimension;
}

// the codec's own calls, as the tools wrote them out before there was a SourceFile
HRESULT Direct(const char* file, FileType type, const LoadFlags& flags, TexMetadata& info, TexMetadata& header, HRESULT& headerHr)
{
    switch (type)
    {
    case FileType::DDS:
    {
        DDSRawImage raw;
        headerHr = GetMetadataFromDDSFile(file, flags.dds, header);
        const HRESULT hr = LoadFromDDSFileRaw(file, flags.dds, nullptr, raw);
        if (SUCCEEDED(hr)) info = raw.metadata;
        return hr;
    }
    case FileType::HDR: { float exposure; Blob rgbe; headerHr = GetMetadataFromHDRFile(file, header); return LoadFromHDRFileRGBE(file, &info, exposure, rgbe); }
    case FileType::TGA:
    {
        TGARawImage raw;
        headerHr = GetMetadataFromTGAFile(file, flags.tga, header);
        const HRESULT hr = LoadFromTGAFileRaw(file, flags.tga, &info, raw);
        if (SUCCEEDED(hr)) ApplyTGAAlphaRule(raw, flags.tga, info);
        return hr;
    }
    case FileType::PPM: case FileType::PFM: case FileType::PHM: { PNMRawImage raw; headerHr = GetMetadataFromPortablePixMapFile(file, header); return LoadFromPortablePixMapFileRaw(file, &info, raw); }
    case FileType::PNG: { PNGRawImage raw; headerHr = GetMetadataFromPNGFile(file, flags.png, header); return LoadFromPNGFileRaw(file, flags.png, &info, raw); }
    case FileType::JPEG: { JPEGRawImage raw; headerHr = GetMetadataFromJPEGFile(file, flags.jpeg, header); return LoadFromJPEGFileRaw(file, flags.jpeg, &info, raw); }
    case FileType::EXR: { EXRRawImage raw; headerHr = GetMetadataFromEXRFile(file, header); return LoadFromEXRFileRaw(file, &info, raw); }
    default: headerHr = HRESULT_E_NOT_SUPPORTED; return HRESULT_E_NOT_SUPPORTED;
    }
}

void ParseOne(const char* file)
{
    const FileType type = FileTypeOf(file);
    for (int bgr = 0; bgr < 2; ++bgr)          // the flags reach the codec: a .png answers with the other format
    {
        LoadFlags flags;
        if (bgr) flags.png = PNG_FLAGS_BGR;
        TexMetadata direct, directHeader, header;
        HRESULT directHeaderHr = E_FAIL;
        const HRESULT directHr = Direct(file, type, flags, direct, directHeader, directHeaderHr);
        SourceFile source;
        const HRESULT hr = source.Parse(file, type, flags);
        const HRESULT headerHr = GetMetadata(file, type, flags, header);
        if (!bgr) std::printf("%s type %d parse %08X direct %08X metadata %08X\n", file, int(type), unsigned(hr), unsigned(directHr), unsigned(headerHr));
        EXPECT(source.type == type);
        EXPECT(hr == directHr);
        EXPECT(headerHr == directHeaderHr);
        if (SUCCEEDED(hr)) EXPECT(Same(source.info, direct));
        if (SUCCEEDED(headerHr)) EXPECT(Same(header, directHeader));
        if (SUCCEEDED(hr) && SUCCEEDED(headerHr))
            EXPECT(header.width == source.info.width && header.height == source.info.height && header.format == source.info.format && header.mipLevels == source.info.mipLevels);
        // what Parse kept is what the type's Upload takes, and Release lets it go
        if (SUCCEEDED(hr))
        {
            const bool pnm = type == FileType::PPM || type == FileType::PFM || type == FileType::PHM;
            EXPECT((type == FileType::DDS) == (source.dds.payload != nullptr));
            EXPECT((type == FileType::HDR) == (source.rgbe.GetBufferPointer() != nullptr));
            EXPECT((type == FileType::TGA) == (source.tga.texels != nullptr));
            EXPECT(pnm == (source.pnm.payload != nullptr));
            source.Release();
            EXPECT(!source.dds.payload && !source.rgbe.GetBufferPointer() && !source.tga.texels && !source.pnm.payload);
        }
    }
}
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "tables")) Tables();
    else if (argc >= 3 && !std::strcmp(argv[1], "parse")) for (int i = 2; i < argc; ++i) ParseOne(argv[i]);
    else { std::fprintf(stderr, "usage: tool_files_test tables | parse <file>...\n"); return 2; }
    if (failures) std::printf("%d checks failed\n", failures);
    return failures ? 1 : 0;
}
