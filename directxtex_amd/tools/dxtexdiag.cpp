// dxtexdiag: texdiag's analyze, compare and diff commands (Texdiag/texdiag.cpp) on the MI355X host layer. DDS, HDR, TGA, PNG, JPEG and OpenEXR in.
//
//   dxtexdiag analyze [options] <files>            per image: minimum, average, maximum, variance, std dev, luminance, FP specials; BC files
//                                                  also get the block-mode histogram (texdiag's print layout, :681-695, :795-856)
//   dxtexdiag compare [options] <a> <b>            "Result: mse (r g b a) PSNR x dB" with 10 * log10(3 / (r + g + b)); when both files hold
//                                                  the same number of mips, items and slices, every image and the minimum / average / maximum
//   dxtexdiag diff [options] <a> <b> -o <out.dds|.tga|.hdr|.png|.jpg|.exr>     the difference map of the first images
//
//   -f <format>   diff: format of the map (default B8G8R8A8_UNORM)     -c <hex>   diff: colour 0xRRGGBB for texels over the threshold (masked to 24 bits)
//   -t <float>    diff: threshold (default 0.25)                        -if <filter>  image filter for diff's conversions
//   -o <file>     diff: output file, required (there is no BMP writer, texdiag's default)   -y  overwrite   -l  lower-case output name
//   -dword -badtails -permissive -ignoremips -xlum   DDS reader flags    -nologo    -gpu <n>
//   -timing       a last line with the bytes moved between host and device, as dxtexconv -timing counts them
//   Not here: dumpbc (prints one block on the CPU) and dumpdds / info (dxtexconv -info).
#include "tool_files.h"

#include <algorithm>
#include <cctype>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

struct Options
{
    std::string command, output;
    std::vector<std::string> files;
    uint32_t format = DXGI_FORMAT_B8G8R8A8_UNORM, filter = TEX_FILTER_DEFAULT, ddsRead = DDS_FLAGS_NONE, diffColor = 0;
    float threshold = 0.25f;
    bool overwrite = false, lower = false, nologo = false, timing = false;
    int gpu = 0;
};

// the types this tool reads, and diff writes: all but the portable pixmaps. Any other input is read as a .dds.
bool Takes(FileType t) { return t != FileType::UNKNOWN && t != FileType::PPM && t != FileType::PFM && t != FileType::PHM; }
FileType InputType(const std::string& file) { const FileType t = FileTypeOf(file); return Takes(t) ? t : FileType::DDS; }

int usage()
{
    std::fprintf(stderr, "usage: dxtexdiag analyze [options] <files>\n"
                         "       dxtexdiag compare [options] <file1> <file2>\n"
                         "       dxtexdiag diff [options] <file1> <file2> -o <out.dds | out.tga | out.hdr | out.png | out.jpg>\n"
                         "options: -f <format> -if <filter> -c <hex colour> -t <threshold> -o <file> -y -l -nologo -timing -gpu <n>\n"
                         "         -dword -badtails -permissive -ignoremips -xlum\n");
    return 1;
}

bool Parse(int argc, char** argv, Options& o)
{
    if (argc < 2) return false;
    o.command = argv[1];
    if (o.command != "analyze" && o.command != "compare" && o.command != "diff")
    {
        std::fprintf(stderr, "unknown command '%s' (analyze, compare, diff)\n", argv[1]);
        return false;
    }
    for (int i = 2; i < argc; ++i)
    {
        const std::string a = argv[i];
        if (a.empty() || a[0] != '-') { o.files.push_back(a); continue; }
        const auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : nullptr; };
        const auto value = [&](const char*& v) { v = next(); if (!v) std::fprintf(stderr, "%s wants a value\n", a.c_str()); return v != nullptr; };
        const char* v = nullptr;
        if (a == "-f" || a == "--format")
        {
            if (!value(v)) return false;
            if (!lookup(kFormats, v, o.format)) { std::fprintf(stderr, "invalid value specified with -f (%s)\n", v); return false; }
        }
        else if (a == "-if" || a == "--image-filter")
        {
            if (!value(v)) return false;
            if (!lookup(kFilters, v, o.filter)) { std::fprintf(stderr, "invalid value specified with -if (%s)\n", v); return false; }
        }
        else if (a == "-c" || a == "--diff-color")
        {
            if (!value(v)) return false;
            char* end = nullptr;
            const unsigned long c = std::strtoul(v, &end, 16);
            if (end == v || *end) { std::fprintf(stderr, "invalid value specified with -c (%s)\n", v); return false; }
            o.diffColor = uint32_t(c) & 0xFFFFFFu;
        }
        else if (a == "-t" || a == "--threshold")
        {
            if (!value(v)) return false;
            char* end = nullptr;
            o.threshold = std::strtof(v, &end);
            if (end == v || *end) { std::fprintf(stderr, "invalid value specified with -t (%s)\n", v); return false; }
        }
        else if (a == "-o") { if (!value(v)) return false; o.output = v; }
        else if (a == "-gpu") { if (!value(v)) return false; o.gpu = std::atoi(v); }
        else if (a == "-y" || a == "--overwrite") o.overwrite = true;
        else if (a == "-l" || a == "--to-lowercase") o.lower = true;
        else if (a == "-nologo") o.nologo = true;
        else if (a == "-timing") o.timing = true;
        else if (a == "-dword") o.ddsRead |= DDS_FLAGS_LEGACY_DWORD;
        else if (a == "-badtails") o.ddsRead |= DDS_FLAGS_BAD_DXTN_TAILS;
        else if (a == "-permissive") o.ddsRead |= DDS_FLAGS_PERMISSIVE;
        else if (a == "-ignoremips") o.ddsRead |= DDS_FLAGS_IGNORE_MIPS;
        else if (a == "-xlum") o.ddsRead |= DDS_FLAGS_EXPAND_LUMINANCE;
        else { std::fprintf(stderr, "unknown option %s\n", a.c_str()); return false; }
    }
    if (o.command == "analyze" && o.files.empty()) { std::fprintf(stderr, "analyze wants at least one file\n"); return false; }
    if (o.command != "analyze" && o.files.size() != 2) { std::fprintf(stderr, "%s wants exactly two files\n", o.command.c_str()); return false; }
    if (o.command == "diff")
    {
        if (o.output.empty()) { std::fprintf(stderr, "diff wants -o <out.dds | out.tga | out.hdr | out.png | out.jpg>\n"); return false; }
        if (o.lower) std::transform(o.output.begin(), o.output.end(), o.output.begin(), [](unsigned char c) { return char(std::tolower(c)); });
        if (!Takes(FileTypeOf(o.output)))
        {
            std::fprintf(stderr, "the output file must be .dds, .tga or .hdr, or .png or .jpg\n");
            return false;
        }
        struct stat st;
        if (!o.overwrite && stat(o.output.c_str(), &st) == 0) { std::fprintf(stderr, "output file %s already exists, use -y to overwrite\n", o.output.c_str()); return false; }
    }
    return true;
}

// Every file goes up once, at the bytes a texel it has on disk, and becomes the texture on the device (tool_files.h: SourceFile); the readers'
// flags are texdiag's (texdiag.cpp:599-608). A planar file becomes its single-plane form there, as texdiag's loader makes it
// (texdiag.cpp:3959-3972).
HRESULT Load(Device& dev, const Options& o, const std::string& file, TexMetadata& info, DeviceScratchImage& resident)
{
    LoadFlags flags;
    flags.dds = DDS_FLAGS(o.ddsRead);
    HRESULT hr = tool::Load(dev, file.c_str(), InputType(file), flags, info, resident);
    if (FAILED(hr) || !IsPlanar(info.format)) return hr;
    DeviceScratchImage single;
    hr = ConvertToSinglePlane(dev, resident, single);
    if (FAILED(hr)) return hr;
    resident = std::move(single);
    info.format = resident.GetMetadata().format;
    return S_OK;
}

// One file of compare / diff, resident. ComputeMSE and Difference take image 0 of it; compare's loop over every image takes the others.
struct Side
{
    TexMetadata info;
    DeviceScratchImage resident;
    size_t count = 0;          // images in the file

    HRESULT Open(Device& dev, const Options& o, const std::string& file)
    {
        const HRESULT hr = Load(dev, o, file, info, resident);
        count = resident.GetImageCount();
        return hr;
    }
    // for compare's loop: a block-compressed texture is decompressed once, not once per pair (ComputeMSE would, to the same floats)
    HRESULT Expand(Device& dev)
    {
        if (!IsCompressed(resident.GetMetadata().format)) return S_OK;
        DeviceScratchImage floats;
        const HRESULT hr = Decompress(dev, resident, DXGI_FORMAT_R32G32B32A32_FLOAT, floats);
        if (SUCCEEDED(hr)) resident = std::move(floats);
        return hr;
    }
};

void Print(const AnalyzeData& d)
{
    std::printf("\t  Minimum - (%f %f %f %f)\n", d.imageMin[0], d.imageMin[1], d.imageMin[2], d.imageMin[3]);
    std::printf("\t  Average - (%f %f %f %f)\n", d.imageAvg[0], d.imageAvg[1], d.imageAvg[2], d.imageAvg[3]);
    std::printf("\t  Maximum - (%f %f %f %f)\n", d.imageMax[0], d.imageMax[1], d.imageMax[2], d.imageMax[3]);
    std::printf("\t Variance - (%f %f %f %f)\n", d.imageVariance[0], d.imageVariance[1], d.imageVariance[2], d.imageVariance[3]);
    std::printf("\t  Std Dev - (%f %f %f %f)\n", d.imageStdDev[0], d.imageStdDev[1], d.imageStdDev[2], d.imageStdDev[3]);
    std::printf("\tLuminance - %f (maximum)\n", d.luminance);
    if (d.specials[0] || d.specials[1] || d.specials[2] || d.specials[3])
        std::printf("     FP specials - (%llu %llu %llu %llu)\n", (unsigned long long)d.specials[0], (unsigned long long)d.specials[1],
                    (unsigned long long)d.specials[2], (unsigned long long)d.specials[3]);
}

void Print(const AnalyzeBCData& d, DXGI_FORMAT fmt)
{
    const auto n = [&](size_t i) { return (unsigned long long)d.blockHist[i]; };
    std::printf("\t        Compression - %s\n\t       Total blocks - %llu\n", FormatName(fmt), (unsigned long long)d.blocks);
    switch (fmt)
    {
    case DXGI_FORMAT_BC1_UNORM: case DXGI_FORMAT_BC1_UNORM_SRGB:
        std::printf("\t     4 color blocks - %llu\n\t     3 color blocks - %llu\n", n(0), n(1)); break;
    case DXGI_FORMAT_BC3_UNORM: case DXGI_FORMAT_BC3_UNORM_SRGB:
        std::printf("\t     8 alpha blocks - %llu\n\t     6 alpha blocks - %llu\n", n(0), n(1)); break;
    case DXGI_FORMAT_BC4_UNORM: case DXGI_FORMAT_BC4_SNORM:
        std::printf("\t     8 red blocks - %llu\n\t     6 red blocks - %llu\n", n(0), n(1)); break;
    case DXGI_FORMAT_BC5_UNORM: case DXGI_FORMAT_BC5_SNORM:
        std::printf("\t     8 red blocks - %llu\n\t     6 red blocks - %llu\n\t   8 green blocks - %llu\n\t   6 green blocks - %llu\n", n(0), n(1), n(2), n(3)); break;
    case DXGI_FORMAT_BC6H_UF16: case DXGI_FORMAT_BC6H_SF16:
        for (size_t j = 1; j <= 14; ++j) if (d.blockHist[j]) std::printf("\t     Mode %02zu blocks - %llu\n", j, n(j));
        if (d.blockHist[0]) std::printf("\tReserved mode blcks - %llu\n", n(0));
        break;
    case DXGI_FORMAT_BC7_UNORM: case DXGI_FORMAT_BC7_UNORM_SRGB:
        for (size_t j = 0; j <= 7; ++j) if (d.blockHist[j]) std::printf("\t     Mode %02zu blocks - %llu\n", j, n(j));
        if (d.blockHist[8]) std::printf("\tReserved mode blcks - %llu\n", n(8));
        break;
    default: break;
    }
}

int RunAnalyze(Device& dev, const Options& o)
{
    for (const std::string& file : o.files)
    {
        TexMetadata info;
        // the whole file goes up once; every image is analysed on the device, the figures come back in one copy
        DeviceScratchImage resident;
        HRESULT hr = Load(dev, o, file, info, resident);
        if (FAILED(hr)) return Fail((" FAILED loading " + file).c_str(), hr);
        std::printf("%s\n", file.c_str());
        const size_t n = resident.GetImageCount();
        std::vector<AnalyzeData> data(n);
        std::vector<AnalyzeBCData> bc(IsCompressed(info.format) ? n : 0);
        hr = Analyze(dev, resident, data.data());
        if (FAILED(hr)) return Fail("ERROR: Failed analyzing the images", hr);
        if (!bc.empty()) { hr = AnalyzeBC(dev, resident, bc.data()); if (FAILED(hr)) return Fail("ERROR: Failed analyzing the BC images", hr); }
        const auto one = [&](size_t mip, size_t item, size_t slice) -> bool
        {
            const size_t idx = info.ComputeIndex(mip, item, slice);
            if (idx >= n) return false;
            Print(data[idx]);
            if (!bc.empty()) Print(bc[idx], info.format);
            std::printf("\n");
            return true;
        };
        if (info.depth > 1)
        {
            std::printf("Results by mip (%3zu) and slice (%3zu)\n\n", info.mipLevels, info.depth);
            size_t depth = info.depth;
            for (size_t mip = 0; mip < info.mipLevels; ++mip)
            {
                for (size_t slice = 0; slice < depth; ++slice)
                {
                    std::printf("Result slice %3zu, mip %3zu:\n", slice, mip);
                    if (!one(mip, 0, slice)) { std::printf("ERROR: Unexpected error at slice %3zu, mip %3zu\n", slice, mip); return 1; }
                }
                if (depth > 1) depth >>= 1;
            }
        }
        else
        {
            std::printf("Results by item (%3zu) and mip (%3zu)\n\n", info.arraySize, info.mipLevels);
            for (size_t item = 0; item < info.arraySize; ++item)
                for (size_t mip = 0; mip < info.mipLevels; ++mip)
                {
                    if (info.arraySize > 1 || info.mipLevels > 1) std::printf("Result item %3zu, mip %3zu:\n", item, mip);
                    if (!one(mip, item, 0)) { std::printf("ERROR: Unexpected error at item %3zu, mip %3zu\n", item, mip); return 1; }
                }
        }
    }
    return 0;
}

double Psnr(const float* v) { return 10.0 * std::log10(3.0 / (double(v[0]) + double(v[1]) + double(v[2]))); }

int RunCompare(Device& dev, const Options& o)
{
    Side side1, side2;
    HRESULT hr = side1.Open(dev, o, o.files[0]);
    if (FAILED(hr)) return Fail((" FAILED loading " + o.files[0]).c_str(), hr);
    hr = side2.Open(dev, o, o.files[1]);
    if (FAILED(hr)) return Fail((" FAILED loading " + o.files[1]).c_str(), hr);
    const TexMetadata& info1 = side1.info; const TexMetadata& info2 = side2.info;
    if (info1.width != info2.width || info1.height != info2.height) { std::printf("ERROR: Can only compare images of the same width & height\n"); return 1; }
    if ((info1.depth == 1 && info1.arraySize == 1 && info1.mipLevels == 1) || info1.depth != info2.depth || info1.arraySize != info2.arraySize ||
        info1.mipLevels != info2.mipLevels || side1.count != side2.count)
    {
        // first images (a .tga has no other, so this is where one ends up)
        if (side1.count > 1 || side2.count > 1) std::printf("WARNING: ignoring all images but first one in each file\n");
        float mse = 0, mseV[4] = {};
        hr = ComputeMSE(dev, side1.resident, side2.resident, mse, mseV, CMSE_DEFAULT);
        if (FAILED(hr)) return Fail("Failed comparing images", hr);
        std::printf("Result: %f (%f %f %f %f) PSNR %f dB\n", mse, mseV[0], mseV[1], mseV[2], mseV[3], Psnr(mseV));
        return 0;
    }
    hr = side1.Expand(dev);
    if (SUCCEEDED(hr)) hr = side2.Expand(dev);
    if (FAILED(hr)) return Fail("Failed comparing images", hr);
    float minMse = FLT_MAX, minV[4] = { FLT_MAX, FLT_MAX, FLT_MAX, FLT_MAX }, maxMse = -FLT_MAX, maxV[4] = { -FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX };
    double sumMse = 0, sumV[4] = { 0, 0, 0, 0 };
    size_t total = 0;
    const auto pair = [&](size_t a, size_t b, size_t mip, size_t item, size_t slice) -> bool
    {
        if (!side1.resident.GetImage(mip, item, slice) || !side2.resident.GetImage(mip, item, slice)) { std::printf("ERROR: Unexpected mismatch at [%3zu,%3zu]\n", a, b); return false; }
        float mse = 0, mseV[4] = {};
        const HRESULT h = ComputeMSE(dev, side1.resident, info1.ComputeIndex(mip, item, slice), side2.resident, info2.ComputeIndex(mip, item, slice), mse, mseV, CMSE_DEFAULT);
        if (FAILED(h)) { std::printf("Failed comparing images at [%3zu,%3zu] (%08X)\n", a, b, static_cast<unsigned int>(h)); return false; }
        minMse = std::min(minMse, mse); maxMse = std::max(maxMse, mse); sumMse += double(mse);
        for (int c = 0; c < 4; ++c) { minV[c] = std::min(minV[c], mseV[c]); maxV[c] = std::max(maxV[c], mseV[c]); sumV[c] += double(mseV[c]); }
        ++total;
        std::printf("[%3zu,%3zu]: %f (%f %f %f %f) PSNR %f dB\n", a, b, mse, mseV[0], mseV[1], mseV[2], mseV[3], Psnr(mseV));
        return true;
    };
    if (info1.depth > 1)
    {
        std::printf("Results by mip (%3zu) and slice (%3zu)\n\n", info1.mipLevels, info1.depth);
        size_t depth = info1.depth;
        for (size_t mip = 0; mip < info1.mipLevels; ++mip)
        {
            for (size_t slice = 0; slice < depth; ++slice) if (!pair(mip, slice, mip, 0, slice)) return 1;
            if (depth > 1) depth >>= 1;
        }
    }
    else
    {
        std::printf("Results by item (%3zu) and mip (%3zu)\n\n", info1.arraySize, info1.mipLevels);
        for (size_t item = 0; item < info1.arraySize; ++item)
            for (size_t mip = 0; mip < info1.mipLevels; ++mip) if (!pair(item, mip, mip, item, 0)) return 1;
    }
    if (!total) { std::printf("ERROR: No images found\n"); return 1; }
    std::printf("\n    Minimum MSE: %f (%f %f %f %f) PSNR %f dB\n", minMse, minV[0], minV[1], minV[2], minV[3], Psnr(minV));
    const float avgV[4] = { float(sumV[0] / double(total)), float(sumV[1] / double(total)), float(sumV[2] / double(total)), float(sumV[3] / double(total)) };
    std::printf("    Average MSE: %f (%f %f %f %f) PSNR %f dB\n", sumMse / double(total), avgV[0], avgV[1], avgV[2], avgV[3], Psnr(avgV));
    std::printf("    Maximum MSE: %f (%f %f %f %f) PSNR %f dB\n", maxMse, maxV[0], maxV[1], maxV[2], maxV[3], Psnr(maxV));
    return 0;
}

int RunDiff(Device& dev, const Options& o)
{
    Side side1, side2;
    HRESULT hr = side1.Open(dev, o, o.files[0]);
    if (FAILED(hr)) return Fail((" FAILED loading " + o.files[0]).c_str(), hr);
    hr = side2.Open(dev, o, o.files[1]);
    if (FAILED(hr)) return Fail((" FAILED loading " + o.files[1]).c_str(), hr);
    if (side1.info.width != side2.info.width || side1.info.height != side2.info.height) { std::printf("ERROR: Can only compare images of the same width & height\n"); return 1; }
    if (side1.count > 1 || side2.count > 1) std::printf("WARNING: ignoring all images but first one in each file\n");
    DeviceScratchImage map;
    hr = Difference(dev, side1.resident, side2.resident, TEX_FILTER_FLAGS(o.filter), DXGI_FORMAT(o.format), o.diffColor, o.threshold, map);
    if (FAILED(hr)) return Fail("Failed diffing images", hr);
    // the map comes back as the file's rows the resident saver makes on the device, a .dds straight behind its header (tool_files.h: Save)
    hr = Save(dev, FileTypeOf(o.output), map, map.GetMetadata(), DDS_FLAGS_NONE, nullptr, o.output.c_str());
    if (FAILED(hr)) return Fail(" FAILED writing the difference", hr);
    std::printf("Difference %s\n", o.output.c_str());
    return 0;
}
}

int main(int argc, char** argv)
{
    Options o;
    if (!Parse(argc, argv, o)) return usage();
    if (!o.nologo) std::printf("dxtexdiag: DirectXTex diagnostics on MI355X (gfx950)\n");
    Device dev;
    const HRESULT hr = dev.Create(o.gpu);
    if (FAILED(hr)) { std::fprintf(stderr, "no usable gfx950 device %d (%08X): this tool has no CPU path\n", o.gpu, static_cast<unsigned int>(hr)); return 1; }
    const int rc = o.command == "analyze" ? RunAnalyze(dev, o) : o.command == "compare" ? RunCompare(dev, o) : RunDiff(dev, o);
    if (o.timing)
    {
        uint64_t up = 0, down = 0;
        GetTransferBytes(dev, up, down);
        std::printf("  host -> device %llu bytes, device -> host %llu bytes\n", (unsigned long long)up, (unsigned long long)down);
    }
    return rc;
}
