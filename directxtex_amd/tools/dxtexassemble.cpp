// dxtexassemble: texassemble's commands (Texassemble/texassemble.cpp) on the MI355X host layer. DDS, HDR, TGA, PNG, JPEG and OpenEXR in; DDS out (TGA / HDR /
// PNG / JPEG / OpenEXR too for the single-image results). Every input is loaded on the host, checked, uploaded ONCE, run through texassemble's per-input
// pipeline on the device (decompress, -stripmips, -alpha, resize, -tonemap, convert), assembled there - every face, slice, item or mip a
// rectangle of one batched copy_rect launch - and the result is downloaded once.
//
//   dxtexassemble <command> [options] <files>
//   cube volume array cubearray          the images of the inputs become the faces / slices / items of one texture
//   h-cross v-cross h-tee h-strip v-strip   a cubemap .dds laid out as one image        array-strip   a 1D / 2D array .dds, items top to bottom
//   cube-from-hc -vc -ht -hs -vs         the reverse: one image cut into the six faces of a cubemap
//   merge                                rgb of image 1 and a channel of image 2 (-swizzle, default rgbB)
//   from-mips cube-from-mips             one input per mip level (per face: all levels of +X, then of -X, ...)
//   Not here: gif (WIC); v-cross-fnz and cube-from-vc-fnz, which still print their refusal: the host layer does them (AssembleCross /
//   CubeFromCross with TEX_FR_ROTATE180 for the -Z face), the commands are not turned on.
//
//   -w <n> -h <n> -m <n> -f <format> -if <filter> -srgb -srgbi -srgbo -wrap -mirror -sepalpha -alpha -tonemap -stripmips -swizzle <mask>
//   -o <file> -y -l -dx10 -fl <level> -nologo -gpu <n> -timing -help
//   The cross / strip commands default to a .bmp output in texassemble; there is no BMP writer here, so they want -o.
#include "tool_files.h"

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <sys/stat.h>
#include <vector>

using namespace tool;

namespace
{
const Name kFilters[] = {
    { "POINT", TEX_FILTER_POINT }, { "LINEAR", TEX_FILTER_LINEAR }, { "CUBIC", TEX_FILTER_CUBIC }, { "FANT", TEX_FILTER_FANT }, { "BOX", TEX_FILTER_BOX },
    { "TRIANGLE", TEX_FILTER_TRIANGLE }, { "POINT_DITHER", TEX_FILTER_POINT | TEX_FILTER_DITHER }, { "LINEAR_DITHER", TEX_FILTER_LINEAR | TEX_FILTER_DITHER },
    { "CUBIC_DITHER", TEX_FILTER_CUBIC | TEX_FILTER_DITHER }, { "TRIANGLE_DITHER", TEX_FILTER_TRIANGLE | TEX_FILTER_DITHER },
    { "POINT_DITHER_DIFFUSION", TEX_FILTER_POINT | TEX_FILTER_DITHER_DIFFUSION }, { "LINEAR_DITHER_DIFFUSION", TEX_FILTER_LINEAR | TEX_FILTER_DITHER_DIFFUSION },
};

constexpr uint32_t TEX_FILTER_SEPARATE_ALPHA = 0x100;      // DirectXTex.h: resize the alpha channel separately (as in dxtexconv)

enum Command
{
    CMD_CUBE, CMD_VOLUME, CMD_ARRAY, CMD_CUBEARRAY, CMD_H_CROSS, CMD_V_CROSS, CMD_H_TEE, CMD_H_STRIP, CMD_V_STRIP, CMD_ARRAY_STRIP, CMD_MERGE,
    CMD_CUBE_FROM_HC, CMD_CUBE_FROM_VC, CMD_CUBE_FROM_HT, CMD_CUBE_FROM_HS, CMD_CUBE_FROM_VS, CMD_FROM_MIPS, CMD_CUBE_FROM_MIPS,
    CMD_GIF, CMD_V_CROSS_FNZ, CMD_CUBE_FROM_VC_FNZ,
};
const Name kCommands[] = {
    { "cube", CMD_CUBE }, { "volume", CMD_VOLUME }, { "array", CMD_ARRAY }, { "cubearray", CMD_CUBEARRAY }, { "h-cross", CMD_H_CROSS }, { "v-cross", CMD_V_CROSS },
    { "v-cross-fnz", CMD_V_CROSS_FNZ }, { "h-tee", CMD_H_TEE }, { "h-strip", CMD_H_STRIP }, { "v-strip", CMD_V_STRIP }, { "array-strip", CMD_ARRAY_STRIP },
    { "merge", CMD_MERGE }, { "gif", CMD_GIF }, { "cube-from-hc", CMD_CUBE_FROM_HC }, { "cube-from-vc", CMD_CUBE_FROM_VC }, { "cube-from-vc-fnz", CMD_CUBE_FROM_VC_FNZ },
    { "cube-from-ht", CMD_CUBE_FROM_HT }, { "cube-from-hs", CMD_CUBE_FROM_HS }, { "cube-from-vs", CMD_CUBE_FROM_VS }, { "from-mips", CMD_FROM_MIPS },
    { "cube-from-mips", CMD_CUBE_FROM_MIPS },
};
const char* const kFeatureLevels[] = { "9.1", "9.2", "9.3", "10.0", "10.1", "11.0", "11.1", "12.0", "12.1", "12.2" };

bool IsCrossOut(uint32_t c) { return c == CMD_H_CROSS || c == CMD_V_CROSS || c == CMD_H_TEE || c == CMD_H_STRIP || c == CMD_V_STRIP; }
bool IsCubeFrom(uint32_t c) { return c >= CMD_CUBE_FROM_HC && c <= CMD_CUBE_FROM_VS; }
CROSS_KIND KindOf(uint32_t c)
{
    switch (c)
    {
    case CMD_H_CROSS: case CMD_CUBE_FROM_HC: return CROSS_H_CROSS;
    case CMD_V_CROSS: case CMD_CUBE_FROM_VC: return CROSS_V_CROSS;
    case CMD_H_TEE: case CMD_CUBE_FROM_HT: return CROSS_H_TEE;
    case CMD_H_STRIP: case CMD_CUBE_FROM_HS: return CROSS_H_STRIP;
    default: return CROSS_V_STRIP;
    }
}

struct Options
{
    uint32_t command = CMD_CUBE;
    std::string commandName, output;
    std::vector<std::string> files;
    size_t width = 0, height = 0, mipLevels = 0;
    uint32_t format = DXGI_FORMAT_UNKNOWN, filter = TEX_FILTER_DEFAULT, filterOpts = TEX_FILTER_DEFAULT, srgb = 0;
    uint32_t permute[4] = { 0, 1, 2, 6 }, zero[4] = {}, one[4] = {};
    bool overwrite = false, lower = false, nologo = false, dx10 = false, demulAlpha = false, tonemap = false, stripMips = false, timing = false, help = false;
    int gpu = 0;
};

void PrintUsage()
{
    std::printf("Usage: dxtexassemble <command> <options> <files>\n\n"
                "COMMANDS\n"
                "   cube                create cubemap\n   volume              create volume map\n   array               create texture array\n"
                "   cubearray           create cubemap array\n   h-cross or v-cross  create a cross image from a cubemap\n"
                "   h-tee               create a 'T' image from a cubemap\n   h-strip or v-strip  create a strip image from a cubemap\n"
                "   array-strip         create a strip image from a 1D/2D array\n   merge               create texture from rgb image and alpha image\n"
                "   cube-from-hc        create cubemap from a h-cross image\n   cube-from-vc        create cubemap from a v-cross image\n"
                "   cube-from-ht        create cubemap from a h-tee image\n   cube-from-hs        create cubemap from a h-strip image\n"
                "   cube-from-vs        create cubemap from a v-strip image\n   from-mips           create texture with provided mipmap images\n"
                "   cube-from-mips      create cubemap with provided mipmap images per face\n"
                "   (gif, v-cross-fnz and cube-from-vc-fnz are not supported)\n"
                "\nOPTIONS\n"
                "   -w <n>              width for output\n   -h <n>              height for output\n   -m <n>              miplevels for output (*-from-mips only)\n"
                "   -f <format>         pixel format for output\n   -if <filter>        image filtering\n   -srgb{i|o}          sRGB {input, output}\n"
                "   -o <filename>       output filename\n   -l                  force output filename to lower case\n   -y                  overwrite existing output file (if any)\n"
                "   -sepalpha           resize alpha channel separately from color channels\n   -wrap, -mirror      texture addressing mode (wrap, mirror, or clamp)\n"
                "   -alpha              convert premultiplied alpha to straight alpha\n   -dx10               Force use of 'DX10' extended header\n"
                "   -nologo             suppress copyright message\n   -fl <feature-level> Set maximum feature level target (defaults to 11.0)\n"
                "   -tonemap            Apply a tonemap operator based on maximum luminance\n   -swizzle <rgba>     Select channels for merge (defaults to rgbB)\n"
                "   -stripmips          Use only base image from input dds files\n   -gpu <n>            HIP device\n   -timing             Display elapsed processing time\n");
}

bool ParseSize(const char* v, size_t& out)
{
    char* end = nullptr;
    const unsigned long long n = std::strtoull(v, &end, 10);
    if (end == v || *end || v[0] == '-') return false;
    out = size_t(n);
    return true;
}

// 0: go on, 1: stop with exit code 1, 2: stop with exit code 0 (help)
int Parse(int argc, char** argv, Options& o)
{
    if (argc < 2) { PrintUsage(); return 2; }
    if (!std::strcmp(argv[1], "-help") || !std::strcmp(argv[1], "--help") || !std::strcmp(argv[1], "-?")) { PrintUsage(); return 2; }
    if (!lookup(kCommands, argv[1], o.command))
    {
        std::printf("Must use one of: cube, volume, array, cubearray, h-cross, v-cross, h-tee, h-strip, v-strip, array-strip,\n"
                    "   merge, cube-from-hc, cube-from-vc, cube-from-ht, cube-from-hs, cube-from-vs, from-mips, cube-from-mips\n\n");
        return 1;
    }
    o.commandName = argv[1];
    if (o.command == CMD_GIF) { std::printf("ERROR: gif is not supported (the reference reads animated GIFs through WIC)\n"); return 1; }
    if (o.command == CMD_V_CROSS_FNZ || o.command == CMD_CUBE_FROM_VC_FNZ)
    {
        std::printf("ERROR: %s is not supported (the host layer's AssembleCross / CubeFromCross with TEX_FR_ROTATE180 do it; the command is not turned on)\n", argv[1]);
        return 1;
    }
    for (int i = 2; i < argc; ++i)
    {
        const std::string a = argv[i];
        if (a.empty() || a[0] != '-') { o.files.push_back(a); continue; }
        const auto value = [&](const char*& v) { v = (i + 1 < argc) ? argv[++i] : nullptr; if (!v) PrintUsage(); return v != nullptr; };
        const char* v = nullptr;
        if (a == "-w" || a == "--width") { if (!value(v)) return 1; if (!ParseSize(v, o.width)) { std::printf("Invalid value specified with -w (%s)\n", v); return 1; } }
        else if (a == "-h" || a == "--height") { if (!value(v)) return 1; if (!ParseSize(v, o.height)) { std::printf("Invalid value specified with -h (%s)\n", v); return 1; } }
        else if (a == "-m" || a == "--mip-levels")
        {
            if (!value(v)) return 1;
            if (!ParseSize(v, o.mipLevels)) { std::printf("Invalid value specified with -m (%s)\n", v); return 1; }
            if (o.command != CMD_FROM_MIPS && o.command != CMD_CUBE_FROM_MIPS) { std::printf("-m only applies to from-mips and cube-from-mips commands\n"); return 1; }
        }
        else if (a == "-f" || a == "--format")
        {
            if (!value(v)) return 1;
            if (!lookup(kFormats, v, o.format)) { std::printf("Invalid value specified with -f (%s)\n", v); return 1; }
        }
        else if (a == "-if" || a == "--image-filter")
        {
            if (!value(v)) return 1;
            if (!lookup(kFilters, v, o.filter)) { std::printf("Invalid value specified with -if (%s)\n", v); return 1; }
        }
        else if (a == "-srgbi" || a == "--srgb-in") o.srgb |= TEX_FILTER_SRGB_IN;
        else if (a == "-srgbo" || a == "--srgb-out") o.srgb |= TEX_FILTER_SRGB_OUT;
        else if (a == "-srgb") o.srgb |= TEX_FILTER_SRGB;
        else if (a == "-sepalpha" || a == "--separate-alpha") o.filterOpts |= TEX_FILTER_SEPARATE_ALPHA;
        else if (a == "-wrap")
        {
            if (o.filterOpts & TEX_FILTER_MIRROR) { std::printf("Can't use -wrap and -mirror at same time\n\n"); return 1; }
            o.filterOpts |= TEX_FILTER_WRAP;
        }
        else if (a == "-mirror")
        {
            if (o.filterOpts & TEX_FILTER_WRAP) { std::printf("Can't use -wrap and -mirror at same time\n\n"); return 1; }
            o.filterOpts |= TEX_FILTER_MIRROR;
        }
        else if (a == "-alpha") o.demulAlpha = true;
        else if (a == "-tonemap") o.tonemap = true;
        else if (a == "-stripmips" || a == "--strip-mips")
        {
            if (o.command != CMD_CUBE && o.command != CMD_VOLUME && o.command != CMD_ARRAY && o.command != CMD_CUBEARRAY && o.command != CMD_MERGE)
            {
                std::printf("-stripmips only applies to cube, volume, array, cubearray, or merge commands\n");
                return 1;
            }
            o.stripMips = true;
        }
        else if (a == "-swizzle" || a == "--swizzle")
        {
            if (!value(v)) return 1;
            if (o.command != CMD_MERGE) { std::printf("-swizzle only applies to merge command\n"); return 1; }
            if (!*v || std::strlen(v) > 4) { std::printf("Invalid value specified with -swizzle (%s)\n\n", v); PrintUsage(); return 1; }
            if (!ParseMergeMask(v, o.permute, o.zero, o.one))
            {
                std::printf("-swizzle requires a 1 to 4 character mask composed of these letters: r, g, b, a, x, y, w, z, 0, 1.\n"
                            "    Lowercase letters are from the first image, upper-case letters are from the second image.\n");
                return 1;
            }
        }
        else if (a == "-o") { if (!value(v)) return 1; o.output = v; }
        else if (a == "-fl" || a == "--feature-level")
        {
            if (!value(v)) return 1;
            bool ok = false;
            for (const char* f : kFeatureLevels) ok = ok || !std::strcmp(f, v);
            if (!ok) { std::printf("Invalid value specified with -fl (%s)\n\n", v); return 1; }       // only texassemble's size warnings depend on it
        }
        else if (a == "-gpu") { if (!value(v)) return 1; o.gpu = std::atoi(v); }
        else if (a == "-y" || a == "--overwrite") o.overwrite = true;
        else if (a == "-l" || a == "--to-lowercase") o.lower = true;
        else if (a == "-dx10") o.dx10 = true;
        else if (a == "-nologo") o.nologo = true;
        else if (a == "-timing") o.timing = true;
        else if (a == "-help" || a == "--help" || a == "-?") { PrintUsage(); return 2; }
        else { std::printf("ERROR: Unknown option: `%s`\n\n", a.c_str()); PrintUsage(); return 1; }
    }
    if (o.files.empty()) { PrintUsage(); return 2; }
    // texassemble.cpp:1247-1330
    if ((IsCrossOut(o.command) || o.command == CMD_ARRAY_STRIP || IsCubeFrom(o.command)) && o.files.size() > 1)
    {
        std::printf("ERROR: cross/strip/gif/cube-from-* output only accepts 1 input file\n");
        return 1;
    }
    if (o.command == CMD_MERGE && o.files.size() > 2) { std::printf("ERROR: merge output only accepts 2 input files\n"); return 1; }
    if (o.command == CMD_FROM_MIPS && o.files.size() < 2) { std::printf("ERROR: from-mips command requires at least 2 input files\n"); return 1; }
    if (o.command == CMD_CUBE_FROM_MIPS)
    {
        if (o.files.size() < 12) { std::printf("ERROR: cube-from-mips command requires at least 12 input files\n"); return 1; }
        if (o.files.size() % 6) { std::printf("ERROR: cube-from-mips command requires the same number of input files for each of the 6 faces\n"); return 1; }
    }
    if (o.output.empty())
    {
        if (IsCrossOut(o.command) || o.command == CMD_ARRAY_STRIP) { std::printf("ERROR: Need to specify output file via -o (there is no .bmp writer)\n"); return 1; }
        if (FileTypeOf(o.files[0]) == FileType::DDS) { std::printf("ERROR: Need to specify output file via -o\n"); return 1; }
        std::string stem = o.files[0];
        const size_t slash = stem.find_last_of('/');
        if (slash != std::string::npos) stem = stem.substr(slash + 1);
        const size_t dot = stem.find_last_of('.');
        o.output = (dot == std::string::npos ? stem : stem.substr(0, dot)) + ".dds";
    }
    if (o.lower) std::transform(o.output.begin(), o.output.end(), o.output.begin(), [](unsigned char c) { return char(std::tolower(c)); });
    const bool single = IsCrossOut(o.command) || o.command == CMD_ARRAY_STRIP || o.command == CMD_MERGE;
    const FileType outType = FileTypeOf(o.output);
    if (outType != FileType::DDS && !(single && (outType == FileType::TGA || outType == FileType::HDR || outType == FileType::PNG || outType == FileType::JPEG || outType == FileType::EXR || outType == FileType::TIFF)))
    {
        std::printf("ERROR: the output file must be .dds%s\n", single ? ", .tga, .hdr, .png or .jpg" : "");
        return 1;
    }
    return 0;
}

void PrintInfo(const TexMetadata& info)
{
    std::printf(" (%zux%zu", info.width, info.height);
    if (info.dimension == TEX_DIMENSION_TEXTURE3D) std::printf("x%zu", info.depth);
    if (info.mipLevels > 1) std::printf(",%zu", info.mipLevels);
    if (info.arraySize > 1) std::printf(",%zu", info.arraySize);
    std::printf(" %s", FormatName(info.format));
    if (info.dimension == TEX_DIMENSION_TEXTURE1D) std::printf("%s", info.arraySize > 1 ? " 1DArray" : " 1D");
    else if (info.dimension == TEX_DIMENSION_TEXTURE3D) std::printf(" 3D");
    else if (info.IsCubemap()) std::printf("%s", info.arraySize > 6 ? " CubeArray" : " Cube");
    else std::printf("%s", info.arraySize > 1 ? " 2DArray" : " 2D");
    switch (info.GetAlphaMode())
    {
    case TEX_ALPHA_MODE_OPAQUE: std::printf(" \x61:Opaque"); break;
    case TEX_ALPHA_MODE_PREMULTIPLIED: std::printf(" \x61:PM"); break;
    case TEX_ALPHA_MODE_STRAIGHT: std::printf(" \x61:NonPM"); break;
    case TEX_ALPHA_MODE_CUSTOM: std::printf(" \x61:Custom"); break;
    default: break;
    }
    std::printf(")");
}

// texassemble.cpp:1360-1581: the files, read and checked on the host - no device yet
int LoadInputs(const Options& o, std::vector<std::unique_ptr<SourceFile>>& inputs)
{
    for (size_t i = 0; i < o.files.size(); ++i)
    {
        const std::string& file = o.files[i];
        if (i) std::printf("\n");
        std::printf("reading %s", file.c_str());
        std::fflush(stdout);
        const FileType type = FileTypeOf(file);
        const bool fromDds = IsCrossOut(o.command) || o.command == CMD_ARRAY_STRIP;
        if (fromDds && type != FileType::DDS) { std::printf("\nERROR: Input must be a dds of a %s\n", o.command == CMD_ARRAY_STRIP ? "1D/2D array" : "cubemap"); return 1; }
        // this tool takes no portable pixmaps
        if (type == FileType::UNKNOWN || type == FileType::PPM || type == FileType::PFM || type == FileType::PHM) { std::printf(" FAILED: only .dds, .tga, .hdr, .png and .jpg can be read (the reference reads the rest through WIC)\n"); return 1; }
        // the byte-serial half of every codec here, before there is a device; a .png headed for a BGR format is decoded as one
        // (texassemble.cpp:1526-1544). For a .tga this states the alpha mode the line below prints
        std::unique_ptr<SourceFile> in(new SourceFile);
        LoadFlags flags;
        flags.png = PngBgrFor(o.format);
        const HRESULT hr = in->Parse(file.c_str(), type, flags);
        if (FAILED(hr)) return Fail(" FAILED", hr);
        if (fromDds)
        {
            if (o.command == CMD_ARRAY_STRIP)
            {
                if (in->info.dimension == TEX_DIMENSION_TEXTURE3D || in->info.arraySize < 2 || in->info.IsCubemap()) { std::printf("\nERROR: Input must be a 1D/2D array\n"); return 1; }
            }
            else if (!in->info.IsCubemap()) { std::printf("\nERROR: Input must be a cubemap\n"); return 1; }
            else if (in->info.arraySize != 6) std::printf("\nWARNING: Only the first cubemap in an array is written out as a cross/strip\n");
        }
        else if (type == FileType::DDS)
        {
            if (in->info.IsVolumemap() || in->info.IsCubemap()) { std::printf("\nERROR: Can't assemble complex surfaces\n"); return 1; }
            if (in->info.mipLevels > 1 && !o.stripMips &&
                (o.command == CMD_CUBE || o.command == CMD_VOLUME || o.command == CMD_ARRAY || o.command == CMD_CUBEARRAY || o.command == CMD_MERGE))
            {
                std::printf("\nERROR: Can't assemble using input mips. To ignore mips, try again with -stripmips\n");
                return 1;
            }
        }
        PrintInfo(in->info);
        std::fflush(stdout);
        inputs.push_back(std::move(in));
    }
    // texassemble.cpp:1995-2035
    size_t images = 0;
    for (const auto& in : inputs) images += in->info.arraySize;
    if (o.command == CMD_CUBE && images != 6) { std::printf("\nERROR: cube requires six images to form the faces of the cubemap\n"); return 1; }
    if (o.command == CMD_CUBEARRAY && (images < 6 || images % 6)) { std::printf("cubearray requires a multiple of 6 images to form the faces of the cubemaps\n"); return 1; }
    if (!IsCrossOut(o.command) && !IsCubeFrom(o.command) && o.command != CMD_CUBE && o.command != CMD_CUBEARRAY && images < 2)
    {
        std::printf("\nERROR: Need at least 2 images to assemble\n\n");
        return 1;
    }
    return 0;
}

// CalculateMipLevels (DirectXTexMipmaps.cpp:62-91)
bool CalculateMipLevels(size_t width, size_t height, size_t& mipLevels)
{
    size_t full = 1;
    for (size_t w = width, h = height; w > 1 || h > 1; ++full) { if (w > 1) w >>= 1; if (h > 1) h >>= 1; }
    if (mipLevels > full) return false;
    if (!mipLevels) mipLevels = full;
    return true;
}

int Run(Device& dev, Options& o, std::vector<std::unique_ptr<SourceFile>>& inputs)
{
    std::vector<DeviceScratchImage> resident(inputs.size());
    size_t width = o.width, height = o.height, mipLevels = o.mipLevels;
    DXGI_FORMAT format = DXGI_FORMAT(o.format);
    const TEX_FILTER_FLAGS filter = TEX_FILTER_FLAGS(o.filter | o.filterOpts);
    for (size_t index = 0; index < inputs.size(); ++index)
    {
        DeviceScratchImage cur, next;
        SourceFile& in = *inputs[index];
        HRESULT hr = in.Upload(dev, cur);          // the file's own bytes go up; the host copy is let go
        if (FAILED(hr)) return Fail(" FAILED [upload]", hr);
        TexMetadata info = cur.GetMetadata();
        const auto step = [&]() { cur = std::move(next); next = DeviceScratchImage(); info = cur.GetMetadata(); };
        if (IsPlanar(info.format))          // texassemble.cpp:1587-1600
        {
            hr = ConvertToSinglePlane(dev, cur, next); if (FAILED(hr)) return Fail(" FAILED [converttosingleplane]", hr);
            step();
        }
        if (IsCompressed(info.format))
        {
            hr = Decompress(dev, cur, DXGI_FORMAT_UNKNOWN, next); if (FAILED(hr)) return Fail(" FAILED [decompress]", hr);
            step();
        }
        if (info.mipLevels > 1 && o.stripMips)
        {
            hr = CopyTopLevels(dev, cur, next); if (FAILED(hr)) return Fail(" FAILED [copy to single level]", hr);
            step();
        }
        if (o.demulAlpha && HasAlpha(info.format) && info.format != DXGI_FORMAT_A8_UNORM)
        {
            if (info.GetAlphaMode() == TEX_ALPHA_MODE_STRAIGHT) std::printf("\nWARNING: Image is already using straight alpha\n");
            else if (!info.IsPMAlpha()) std::printf("\nWARNING: Image is not using premultipled alpha\n");
            else
            {
                hr = PremultiplyAlpha(dev, cur, TEX_PMALPHA_FLAGS(TEX_PMALPHA_REVERSE | o.srgb), next); if (FAILED(hr)) return Fail(" FAILED [demultiply alpha]", hr);
                step();
            }
        }
        if (!width) width = info.width;
        if (!height) height = info.height;
        size_t targetWidth = width, targetHeight = height;
        if (o.command == CMD_FROM_MIPS || o.command == CMD_CUBE_FROM_MIPS)
        {
            const size_t faces = o.command == CMD_FROM_MIPS ? 1 : 6;
            if (!index)
            {
                if (!mipLevels) mipLevels = inputs.size() / faces;
                if (!CalculateMipLevels(width, height, mipLevels) || mipLevels * faces != inputs.size())
                {
                    std::printf("\nERROR: Too many input mips provided for the given dimensions of %zu x %zu.\n", width, height);
                    return 1;
                }
            }
            const size_t level = index % mipLevels;
            targetWidth >>= level; targetHeight >>= level;
            if (!targetWidth || !targetHeight)
            {
                std::printf("\nERROR: Too many input mips provided. For the dimensions of the first mip provided, only %zu input mips can be used.\n", index);
                return 1;
            }
        }
        if (info.width != targetWidth || info.height != targetHeight)
        {
            hr = Resize(dev, cur, targetWidth, targetHeight, filter, next); if (FAILED(hr)) return Fail(" FAILED [resize]", hr);
            step();
        }
        if (o.tonemap)
        {
            TexTransform t;
            t.op = TEX_TRANSFORM_TONEMAP;
            hr = TransformImage(dev, cur, t, next); if (FAILED(hr)) return Fail(" FAILED [tonemap apply]", hr);
            step();
        }
        if (format == DXGI_FORMAT_UNKNOWN) format = info.format;
        else if (info.format != format && !IsCompressed(format))
        {
            hr = Convert(dev, cur, format, TEX_FILTER_FLAGS(o.filter | o.filterOpts | o.srgb), TEX_THRESHOLD_DEFAULT, next); if (FAILED(hr)) return Fail(" FAILED [convert]", hr);
            step();
        }
        resident[index] = std::move(cur);
    }

    // --- Create result (texassemble.cpp:2037-2780) ---
    DeviceScratchImage result;
    HRESULT hr = S_OK;
    if (IsCrossOut(o.command)) hr = AssembleCross(dev, KindOf(o.command), resident[0], result);
    else if (IsCubeFrom(o.command))
    {
        const CrossLayout* l = GetCrossLayout(KindOf(o.command));
        if (width % l->cols || height % l->rows) std::printf("\nWARNING: %s expects %zu:%zu aspect ratio\n", o.commandName.c_str(), l->cols, l->rows);
        hr = CubeFromCross(dev, KindOf(o.command), resident[0], result);
    }
    else if (o.command == CMD_ARRAY_STRIP) hr = AssembleStrip(dev, resident[0], result);
    else if (o.command == CMD_MERGE)
    {
        if (resident.size() < 2) { std::printf("\nERROR: Need at least 2 images to assemble\n\n"); return 1; }
        hr = MergeImages(dev, resident[0], resident[1], TEX_FILTER_FLAGS(o.filter | o.filterOpts | o.srgb), o.permute, o.zero, o.one, result);
    }
    else if (o.command == CMD_FROM_MIPS || o.command == CMD_CUBE_FROM_MIPS)
    {
        TexMetadata m;
        m.width = width; m.height = height; m.depth = 1; m.mipLevels = mipLevels; m.format = format; m.dimension = TEX_DIMENSION_TEXTURE2D;
        m.arraySize = o.command == CMD_FROM_MIPS ? 1 : 6;
        if (o.command == CMD_CUBE_FROM_MIPS) m.miscFlags |= TEX_MISC_TEXTURECUBE;
        hr = result.Initialize(dev, m);
        if (SUCCEEDED(hr))
        {
            std::vector<Image> src, dst;
            for (size_t i = 0; i < resident.size(); ++i)
            {
                src.push_back(*resident[i].GetImage(0, 0, 0));
                dst.push_back(*result.GetImage(i % mipLevels, i / mipLevels, 0));
            }
            hr = CopyImages(dev, src.data(), dst.data(), src.size());
        }
    }
    else
    {
        std::vector<Image> all;
        for (const DeviceScratchImage& r : resident)
            for (size_t item = 0; item < r.GetMetadata().arraySize; ++item) all.push_back(*r.GetImage(0, item, 0));
        for (const Image& im : all)
            if (im.width != all[0].width || im.height != all[0].height || im.format != all[0].format) { std::printf("\nERROR: the images differ in size or format after conversion\n"); return 1; }
        if (o.command == CMD_VOLUME) hr = StackVolume(dev, all.data(), all.size(), result);
        else hr = StackArray(dev, all.data(), all.size(), o.command == CMD_CUBE || o.command == CMD_CUBEARRAY, result);
    }
    if (FAILED(hr)) return Fail("FAILED building result image", hr);

    std::printf("\nWriting %s ", o.output.c_str());
    PrintInfo(result.GetMetadata());
    std::printf("\n");
    std::fflush(stdout);
    struct stat st;
    if (!o.overwrite && stat(o.output.c_str(), &st) == 0) { std::printf("\nERROR: Output file already exists, use -y to overwrite\n"); return 1; }
    // the one download, by the resident writers (tool_files.h: Save)
    hr = Save(dev, FileTypeOf(o.output), result, result.GetMetadata(), o.dx10 ? DDS_FLAGS(DDS_FLAGS_FORCE_DX10_EXT | DDS_FLAGS_FORCE_DX10_EXT_MISC2) : DDS_FLAGS_NONE,
              nullptr, o.output.c_str());
    if (FAILED(hr)) return Fail(" FAILED", hr);
    return 0;
}
}

int main(int argc, char** argv)
{
    Options o;
    const int parsed = Parse(argc, argv, o);
    if (parsed) return parsed == 2 ? 0 : 1;
    if (!o.nologo) std::printf("dxtexassemble: DirectXTex texture assembler on MI355X (gfx950)\n\n");
    std::vector<std::unique_ptr<SourceFile>> inputs;
    if (LoadInputs(o, inputs)) return 1;
    Device dev;
    const HRESULT hr = dev.Create(o.gpu);
    if (FAILED(hr)) { std::printf("\nno usable gfx950 device %d (%08X): this tool has no CPU path\n", o.gpu, static_cast<unsigned int>(hr)); return 1; }
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = Run(dev, o, inputs);
    if (o.timing && !rc) std::printf("\n Processing time: %f seconds\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return rc;
}
