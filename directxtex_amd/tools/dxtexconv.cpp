// dxtexconv - a texconv-style batch converter on top of the MI355X host layer (DirectXTexAMD.h): DDS in, DDS out, every
// image-processing step on the GPU. The pipeline and its order are the reference tool's (Texconv/texconv.cpp): load (:2077-2090)
// -> decompress (:2325-2480) -> undo premultiplied alpha (:2482-2530) -> flip (:2533-2574) -> resize (:2577-2640) -> swizzle (:2645-2694) -> colour
// rotation (:2696-2964) -> tone map (:2966-3044) -> normal map (:3047-3098) or convert (:3100-3140) -> colour key (:3134-3191) -> invert Y (:3193-3240) -> reconstruct Z
// (:3242-3301) -> mipmaps (:3302-3460) -> alpha-coverage preservation (:3462-3500) -> premultiply alpha (:3502-3545) -> compress
// (:3547-3735) -> alpha mode (:3738-3766) -> save (:3858-3878). Option names are texconv's; what has no GPU implementation here (-dxt5nm /
// -dxt5rxgb, WIC codecs, dithered conversion) is refused, not approximated.
//
//   dxtexconv [options] -o <out.dds | output directory> <in.dds | in.hdr | in.tga | in.ppm | in.pfm | in.phm | in.png | in.jpg | in.exr | in.tif>...
//                          (-ft hdr | tga | ppm | pfm | png | exr | tif: Radiance / TGA / portable pixmap / PNG / OpenEXR / TIFF output of level 0)
//                          (-ft png, -ft exr, -ft tif: <out> is a directory or a .png / .exr / .tif name)
//     -w <n> -h <n>        target size                         -pow2             fit to a power of two (keeps the aspect ratio)
//     -m <n>               mip levels, 0 = full chain           -fl <9.1 .. 12.2> feature level: largest texture side allowed
//     -f <format>          DXGI format name or number           -if <filter>      POINT LINEAR CUBIC FANT BOX TRIANGLE
//     -wrap -mirror        addressing of the filters            -srgb -srgbi -srgbo   sRGB on both sides / input / output
//     -pmalpha -alpha      to / from premultiplied alpha        -keepcoverage <ref>   keep alpha-test coverage in the mips
//     -at <threshold>      alpha threshold (BC1, 1-bit alpha)   -bc <q|x|d|u>...  BC7 quick / 3 subsets, dither, uniform weights
//     -x2bias              *2 - 1 on conversions to / from SNORM -sepalpha        resize / mip alpha separately (alpha mode custom)
//     -nmap <l|r|g|b|a>[m|u|v][i][o]   height map -> normal map (channel; mirror both / u / v; invert sign; occlusion in alpha)
//     -nmapamp <weight>    normal-map amplitude, default 1 (needs -nmap first)
//     -swizzle <mask>      1-4 of rgbaxyzw01, the last repeated (e.g. bgr1, rrrg)    -tonemap   Reinhard tone map to LDR (maximum over all images)
//     -c <hex-RGB>         colour key: texels near it become transparent (formats with alpha)    -inverty   g = 1 - g    -reconstructz   z from x, y
//                          texconv's long names work too: --swizzle --tonemap --color-key --invert-y --reconstruct-z
//     --rotate-color <op>  709toHDR10 HDR10to709 709to2020 2020to709 P3D65toHDR10 P3D65to2020 709toP3D65 P3D65to709 (either case): the HDR
//                          colour rotation; HDR10to709 and P3D65to709 convert to R16G16B16A16_FLOAT first, as texconv does
//     --paper-white-nits <n>   the level of linear 1.0 for the HDR10 operations, in (0, 10000], default 200
//                          only under texconv's long names (with one or two dashes): its short -rotatecolor and -nits stay refused
//     --horizontal-flip --vertical-flip   mirror the whole texture (every item, mip and slice) left-right / top-bottom, after the
//                          un-premultiply and before the resize; under the long names only: the short -hflip and -vflip stay refused
//     -dword -badtails -permissive -ignoremips -xlum            DDS reader tolerances (DDS_FLAGS)
//     -dx10 -dx9           force the 'DX10' header (+ alpha mode) / a Direct3D 9 file        -tga20   TGA output with the 2.0 extension area
//     -px <s> -sx <s> -l   output name prefix / suffix, lower case    -y   overwrite    -info (print what the files hold, no GPU)    -timing -nologo -gpu <n> | -gpus <a,b,...> (files dealt out over the GPUs)
//     -overlap <n>         workers (contexts) per GPU, default 2: the transfers and file codecs of one file overlap the kernels of another
#include "tool_files.h"

#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <sys/stat.h>
#include <atomic>
#include <thread>
#include <vector>

using namespace tool;

namespace
{
// texconv's short names for the block formats it has one for (texconv.cpp:420-440); the other tools refuse them
const Name kBlockAliases[] = { { "BC4", 80 }, { "BC5", 83 }, { "BC6H", 95 }, { "BC7", 98 } };
const Name kFilters[] = {
    { "POINT", TEX_FILTER_POINT }, { "LINEAR", TEX_FILTER_LINEAR }, { "CUBIC", TEX_FILTER_CUBIC }, { "BOX", TEX_FILTER_BOX }, { "FANT", TEX_FILTER_BOX },
    { "TRIANGLE", TEX_FILTER_TRIANGLE },
    { "POINT_WRAP", TEX_FILTER_POINT | TEX_FILTER_WRAP }, { "LINEAR_WRAP", TEX_FILTER_LINEAR | TEX_FILTER_WRAP }, { "CUBIC_WRAP", TEX_FILTER_CUBIC | TEX_FILTER_WRAP },
    { "TRIANGLE_WRAP", TEX_FILTER_TRIANGLE | TEX_FILTER_WRAP }, { "LINEAR_MIRROR", TEX_FILTER_LINEAR | TEX_FILTER_MIRROR }, { "CUBIC_MIRROR", TEX_FILTER_CUBIC | TEX_FILTER_MIRROR },
};
const Name kFeatureLevels[] = {         // largest 2D texture side (texconv.cpp:880-905)
    { "9.1", 2048 }, { "9.2", 2048 }, { "9.3", 4096 }, { "10.0", 8192 }, { "10.1", 8192 }, { "11.0", 16384 }, { "11.1", 16384 }, { "12.0", 16384 }, { "12.1", 16384 }, { "12.2", 16384 },
};
const Name kRotations[] = {           // g_pRotateColor (texconv.cpp:543-554)
    { "709to2020", TEX_ROTATE_709_TO_2020 }, { "2020to709", TEX_ROTATE_2020_TO_709 }, { "709toHDR10", TEX_ROTATE_709_TO_HDR10 },
    { "HDR10to709", TEX_ROTATE_HDR10_TO_709 }, { "P3D65to2020", TEX_ROTATE_P3D65_TO_2020 }, { "P3D65toHDR10", TEX_ROTATE_P3D65_TO_HDR10 },
    { "709toP3D65", TEX_ROTATE_709_TO_P3D65 }, { "P3D65to709", TEX_ROTATE_P3D65_TO_709 },
};
constexpr uint32_t TEX_FILTER_SEPARATE_ALPHA = 0x100;

struct Options
{
    size_t width = 0, height = 0, mipLevels = 0, maxSize = 16384;          // mipLevels 0: keep a chain the input has, else build the full one
    bool pow2 = false, pmalpha = false, demul = false, dx10 = false, dx9 = false, sepalpha = false, lower = false, overwrite = false,
         timing = false, nologo = false, ignoreSrgb = false, tga20 = false, info = false;
    FileType outType = FileType::DDS;   // -ft
    uint32_t format = 0, filter = 0, filterOpts = 0, srgb = 0, convert = 0, compress = 0, ddsRead = DDS_FLAGS_ALLOW_LARGE_FILES;
    float alphaThreshold = TEX_THRESHOLD_DEFAULT, keepCoverage = 0.f;
    bool nmap = false;                  // -nmap: ComputeNormalMap replaces the convert step
    uint32_t nmapFlags = 0;             // CNMAP_FLAGS
    float nmapAmplitude = 1.f;
    TexTransform swizzle;               // -swizzle: runs unless it is the identity
    bool tonemap = false, colorKey = false, invertY = false, reconstructZ = false;
    uint32_t colorKeyValue = 0;         // -c: 0x00RRGGBB
    uint32_t rotateColor = 0;           // --rotate-color: TEX_ROTATE_COLOR, 0 = none
    float paperWhiteNits = 200.f;       // --paper-white-nits
    bool hflip = false, vflip = false;  // --horizontal-flip, --vertical-flip
    std::vector<int> gpus;              // one worker (own Device, own host thread) per entry; input i goes to worker i mod n
    size_t overlap = 2;                 // workers per listed GPU: file k + 1 is read, decoded and uploaded while file k's kernels run
    std::string prefix, suffix, out;
    std::vector<std::string> inputs;

    // the readers' flags are texconv's (texconv.cpp:2192-2217): -ignoresrgb keeps a .png's sRGB chunk and gAMA from choosing the format and
    // makes a colour .jpg linear and keeps a .tif's Exif colour space from choosing the format; a .png headed for a BGR format is decoded as one (the load only: -info reports the file)
    LoadFlags ReadFlags(bool load) const
    {
        return { DDS_FLAGS(ddsRead), TGA_FLAGS_NONE, PNG_FLAGS((load ? PngBgrFor(format) : PNG_FLAGS_NONE) | (ignoreSrgb ? PNG_FLAGS_IGNORE_SRGB : PNG_FLAGS_NONE)),
                 ignoreSrgb ? JPEG_FLAGS_DEFAULT_LINEAR : JPEG_FLAGS_NONE, ignoreSrgb ? TIFF_FLAGS_IGNORE_SRGB : TIFF_FLAGS_NONE };
    }
};

// the types this tool writes: every one with a -ft name but JPEG
bool Writes(FileType t) { return t != FileType::UNKNOWN && t != FileType::PHM && t != FileType::JPEG; }
// an extension this tool does not know is read as a .dds
FileType InputType(const std::string& file) { const FileType t = FileTypeOf(file); return t == FileType::UNKNOWN ? FileType::DDS : t; }

bool ispow2(size_t x) { return x && !(x & (x - 1)); }

// FitPowerOf2 (texconv.cpp:1019-1057): the larger side snaps down to a power of two, the other takes the power of two that keeps
// the aspect ratio best
void FitPowerOf2(size_t origx, size_t origy, size_t& targetx, size_t& targety, size_t maxsize)
{
    const float aspect = float(origx) / float(origy);
    size_t& major = (origx > origy) ? targetx : targety;
    size_t& minor = (origx > origy) ? targety : targetx;
    size_t m;
    for (m = maxsize; m > 1; m >>= 1) if (m <= major) break;
    major = m;
    float best = 3.402823466e+38f;
    for (size_t o = maxsize; o > 0; o >>= 1)
    {
        const float score = std::fabs(((origx > origy) ? float(m) / float(o) : float(o) / float(m)) - aspect);
        if (score < best) { best = score; minor = o; }
    }
}

int usage()
{
    std::fprintf(stderr, "usage: dxtexconv [-w W] [-h H] [-pow2] [-fl LEVEL] [-m N] [-f FORMAT] [-if FILTER] [-wrap] [-mirror] [-srgb|-srgbi|-srgbo]\n"
                         "                 [-pmalpha|-alpha] [-keepcoverage REF] [-at T] [-bc qxdu] [-x2bias] [-sepalpha] [-nmap <l|r|g|b|a>[m|u|v][i][o]] [-nmapamp W]\n"
                         "                 [-swizzle MASK] [-tonemap] [-c RRGGBB] [-inverty] [-reconstructz]\n"
                         "                 [--rotate-color 709toHDR10|HDR10to709|709to2020|2020to709|P3D65toHDR10|P3D65to2020|709toP3D65|P3D65to709] [--paper-white-nits N]\n"
                         "                 [--horizontal-flip] [--vertical-flip]\n"
                         "                 [-dword] [-badtails] [-permissive]\n"
                         "                 [-ignoremips] [-xlum] [-dx10|-dx9] [-px S] [-sx S] [-l] [-y] [-timing] [-nologo] [-gpu N | -gpus A,B,...] [-overlap N]\n"
                         "                 [-ft dds|hdr|tga|ppm|pfm|png|exr|tif] [-ignoresrgb] -o <out | dir> <in.dds | in.hdr | in.tga | in.ppm | in.pfm | in.phm | in.png | in.jpg | in.exr | in.tif>...\n");
    return 1;
}

bool Parse(int argc, char** argv, Options& o)
{
    for (int i = 1; i < argc; ++i)
    {
        std::string a = argv[i];
        if (a.size() > 2 && a[0] == '-' && a[1] == '-') a.erase(0, 1);          // --long-form spelled like the short one
        bool missing = false;
        auto next = [&]() -> const char* { if (i + 1 < argc) return argv[++i]; missing = true; return ""; };
        if (a == "-w") o.width = std::strtoull(next(), nullptr, 10);
        else if (a == "-h") o.height = std::strtoull(next(), nullptr, 10);
        else if (a == "-m") o.mipLevels = std::strtoull(next(), nullptr, 10);
        else if (a == "-f") { const char* v = next(); if (!lookup(kFormats, v, o.format, true) && !lookup(kBlockAliases, v, o.format)) { std::fprintf(stderr, "unknown format\n"); return false; } }
        else if (a == "-if") { if (!lookup(kFilters, next(), o.filter, true)) { std::fprintf(stderr, "unknown filter (dithered filters have no GPU path)\n"); return false; } }
        else if (a == "-fl") { uint32_t v; if (!lookup(kFeatureLevels, next(), v)) { std::fprintf(stderr, "unknown feature level\n"); return false; } o.maxSize = v; }
        else if (a == "-bc")
        {
            for (const char* p = next(); *p; ++p)
                switch (*p)
                {
                case 'q': o.compress |= TEX_COMPRESS_BC7_QUICK; break;
                case 'x': o.compress |= TEX_COMPRESS_BC7_USE_3SUBSETS; break;
                case 'd': o.compress |= TEX_COMPRESS_DITHER; break;
                case 'u': o.compress |= TEX_COMPRESS_UNIFORM; break;
                default: std::fprintf(stderr, "unknown -bc flag %c\n", *p); return false;
                }
        }
        else if (a == "-srgb") o.srgb |= TEX_FILTER_SRGB;
        else if (a == "-srgbi") o.srgb |= TEX_FILTER_SRGB_IN;
        else if (a == "-srgbo") o.srgb |= TEX_FILTER_SRGB_OUT;
        else if (a == "-wrap") { if (o.filterOpts & TEX_FILTER_MIRROR) { std::fprintf(stderr, "-wrap and -mirror exclude each other\n"); return false; } o.filterOpts |= TEX_FILTER_WRAP; }
        else if (a == "-mirror") { if (o.filterOpts & TEX_FILTER_WRAP) { std::fprintf(stderr, "-wrap and -mirror exclude each other\n"); return false; } o.filterOpts |= TEX_FILTER_MIRROR; }
        else if (a == "-sepalpha") { o.sepalpha = true; o.filterOpts |= TEX_FILTER_SEPARATE_ALPHA; }
        else if (a == "-x2bias") o.convert |= TEX_FILTER_FLOAT_X2BIAS;
        else if (a == "-nmap" || a == "-normal-map")
        {
            // texconv.cpp:1638-1693: the first channel letter found in the order l r g b a; m, or u / v; i; o
            const std::string v = next();
            const auto has = [&](char c) { return v.find(c) != std::string::npos; };
            uint32_t f = CNMAP_DEFAULT;
            if (has('l')) f |= CNMAP_CHANNEL_LUMINANCE;
            else if (has('r')) f |= CNMAP_CHANNEL_RED;
            else if (has('g')) f |= CNMAP_CHANNEL_GREEN;
            else if (has('b')) f |= CNMAP_CHANNEL_BLUE;
            else if (has('a')) f |= CNMAP_CHANNEL_ALPHA;
            else if (!missing) { std::fprintf(stderr, "invalid value for -nmap (%s): missing l, r, g, b or a\n", v.c_str()); return false; }
            if (has('m')) f |= CNMAP_MIRROR;
            else { if (has('u')) f |= CNMAP_MIRROR_U; if (has('v')) f |= CNMAP_MIRROR_V; }
            if (has('i')) f |= CNMAP_INVERT_SIGN;
            if (has('o')) f |= CNMAP_COMPUTE_OCCLUSION;
            o.nmap = true; o.nmapFlags = f;
        }
        else if (a == "-nmapamp" || a == "-normal-map-amplitude")
        {
            // texconv.cpp:1695-1713
            if (!o.nmap) { std::fprintf(stderr, "-nmapamp requires -nmap\n"); return false; }
            const char* v = next();
            char* end = nullptr;
            o.nmapAmplitude = std::strtof(v, &end);
            if (!missing && end == v) { std::fprintf(stderr, "invalid value for -nmapamp (%s)\n", v); return false; }
            if (o.nmapAmplitude < 0.f) { std::fprintf(stderr, "normal map amplitude must be positive (%s)\n", v); return false; }
        }
        else if (a == "-swizzle")
        {
            // texconv.cpp:1919-1931
            const char* v = next();
            if (missing) { std::fprintf(stderr, "option %s needs a value\n", a.c_str()); return false; }
            if (!*v || std::strlen(v) > 4) { std::fprintf(stderr, "Invalid value specified with -swizzle (%s)\n", v); return false; }
            if (!ParseSwizzleMask(v, o.swizzle)) { std::fprintf(stderr, "-swizzle requires a 1 to 4 character mask composed of these letters: r, g, b, a, x, y, w, z, 0, 1\n"); return false; }
        }
        else if (a == "-c" || a == "-color-key")
        {
            // texconv.cpp:1825-1834: swscanf "%x", then & 0xFFFFFF
            const char* v = next();
            unsigned int key = 0;
            if (missing || std::sscanf(v, "%x", &key) != 1) { std::fprintf(stderr, "Invalid value specified with -c (%s)\n", v); return false; }
            o.colorKey = true; o.colorKeyValue = key & 0xFFFFFFu;
        }
        else if (a == "-rotate-color")
        {
            // texconv.cpp:1545-1553 (LookupByName: either case); the short -rotatecolor is not accepted
            const char* v = next();
            if (missing) { std::fprintf(stderr, "option %s needs a value\n", a.c_str()); return false; }
            if (!lookup(kRotations, v, o.rotateColor)) { std::fprintf(stderr, "Invalid value specified with -rotatecolor (%s)\n", v); return false; }
        }
        else if (a == "-paper-white-nits")
        {
            // texconv.cpp:1891-1903; the short -nits is not accepted
            const char* v = next();
            if (missing) { std::fprintf(stderr, "option %s needs a value\n", a.c_str()); return false; }
            if (std::sscanf(v, "%f", &o.paperWhiteNits) != 1) { std::fprintf(stderr, "Invalid value specified with -nits (%s)\n", v); return false; }
            if (!(o.paperWhiteNits > 0.f && o.paperWhiteNits <= 10000.f)) { std::fprintf(stderr, "-nits (%s) parameter must be between 0 and 10000\n", v); return false; }
        }
        else if (a == "-horizontal-flip") o.hflip = true;           // texconv.cpp:289, :318; the short -hflip and -vflip are not accepted
        else if (a == "-vertical-flip") o.vflip = true;
        else if (a == "-tonemap") o.tonemap = true;
        else if (a == "-inverty" || a == "-invert-y") o.invertY = true;
        else if (a == "-reconstructz" || a == "-reconstruct-z") o.reconstructZ = true;
        else if (a == "-pow2") o.pow2 = true;
        else if (a == "-pmalpha") o.pmalpha = true;
        else if (a == "-alpha") o.demul = true;
        else if (a == "-keepcoverage") { o.keepCoverage = float(std::atof(next())); if (!(o.keepCoverage >= 0.f && o.keepCoverage <= 1.f)) { std::fprintf(stderr, "-keepcoverage wants a value in [0, 1]\n"); return false; } }
        else if (a == "-at") { o.alphaThreshold = float(std::atof(next())); if (!(o.alphaThreshold >= 0.f)) { std::fprintf(stderr, "-at wants a non-negative value\n"); return false; } }
        else if (a == "-aw") next();                                              // the DirectCompute encoder's alpha weight: no meaning here
        else if (a == "-dword") o.ddsRead |= DDS_FLAGS_LEGACY_DWORD;
        else if (a == "-badtails") o.ddsRead |= DDS_FLAGS_BAD_DXTN_TAILS;
        else if (a == "-permissive") o.ddsRead |= DDS_FLAGS_PERMISSIVE;
        else if (a == "-ignoremips") o.ddsRead |= DDS_FLAGS_IGNORE_MIPS;
        else if (a == "-xlum") o.ddsRead |= DDS_FLAGS_EXPAND_LUMINANCE;
        else if (a == "-tga20") o.tga20 = true;
        else if (a == "-ignoresrgb") o.ignoreSrgb = true;          // texconv's OPT_IGNORE_SRGB_METADATA: a .png's sRGB chunk and gAMA do not choose the format; a colour .jpg is linear
        else if (a == "-info") o.info = true;
        else if (a == "-dx10") o.dx10 = true;
        else if (a == "-dx9") o.dx9 = true;
        else if (a == "-px") o.prefix = next();
        else if (a == "-sx") o.suffix = next();
        else if (a == "-l") o.lower = true;
        else if (a == "-y") o.overwrite = true;
        else if (a == "-timing") o.timing = true;
        else if (a == "-nologo") o.nologo = true;
        else if (a == "-gpu") o.gpus.assign(1, std::atoi(next()));
        else if (a == "-gpus")
        {
            // "0,1,2,3": the files are dealt out over these GPUs, one host thread and one context each (contexts share nothing)
            o.gpus.clear();
            for (const char* p = next(); *p;)
            {
                char* end = nullptr;
                const long g = std::strtol(p, &end, 10);
                if (end == p || g < 0) { std::fprintf(stderr, "-gpus wants a comma-separated list of device ordinals\n"); return false; }
                o.gpus.push_back(int(g));
                p = (*end == ',') ? end + 1 : end;
                if (*end && *end != ',') { std::fprintf(stderr, "-gpus wants a comma-separated list of device ordinals\n"); return false; }
            }
            if (o.gpus.empty()) { std::fprintf(stderr, "-gpus wants a comma-separated list of device ordinals\n"); return false; }
        }
        else if (a == "-overlap") { o.overlap = std::strtoull(next(), nullptr, 10); if (o.overlap < 1 || o.overlap > 8) { std::fprintf(stderr, "-overlap wants 1 .. 8 workers per GPU\n"); return false; } }
        else if (a == "-o") o.out = next();
        else if (a == "-ft")
        {
            const char* ft = next();
            o.outType = FileTypeOfFt(ft);
            if (o.outType == FileType::JPEG) { std::fprintf(stderr, "-ft %s: JPEG output is not written yet (the reader is; the writer is the next step)\n", ft); return false; }
            if (o.outType == FileType::UNKNOWN) { std::fprintf(stderr, "output file types: dds, hdr, tga, ppm, pfm, png\n"); return false; }
        }
        else if (a == "-r" || a == "-nogpu" || a == "-singleproc") { }            // nothing to switch here
        else if (a[0] == '-') { std::fprintf(stderr, "unknown or unsupported option %s\n", a.c_str()); return false; }
        else o.inputs.push_back(argv[i]);
        if (missing) { std::fprintf(stderr, "option %s needs a value\n", a.c_str()); return false; }
    }
    if (o.pmalpha && o.demul) { std::fprintf(stderr, "-pmalpha and -alpha exclude each other\n"); return false; }
    if (o.dx10 && o.dx9) { std::fprintf(stderr, "-dx10 and -dx9 exclude each other\n"); return false; }
    // -ft png: -o names a directory or a .png file. A name that ends in another type's extension would receive a PNG under that name, which no
    // reader that goes by the extension opens. -ft exr and -ft tif likewise; the other types are not checked.
    const FileType named = FileTypeOf(o.out);
    if ((o.outType == FileType::PNG || o.outType == FileType::EXR || o.outType == FileType::TIFF) && Writes(named) && named != o.outType) { std::fprintf(stderr, "-ft %s writes a %s: -o %s names a %s file\n", ExtensionOf(o.outType) + 1, ExtensionOf(o.outType), o.out.c_str(), ExtensionOf(named)); return false; }
    if (named == FileType::JPEG) { std::fprintf(stderr, "-o %s: JPEG output is not written yet\n", o.out.c_str()); return false; }
    if (o.gpus.empty()) o.gpus.assign(1, 0);
    if (o.info) return !o.inputs.empty();
    return !o.inputs.empty() && !o.out.empty();
}

// <out> names a file when it ends in the extension of a type this tool writes and there is one input; otherwise a directory that receives
// <px><name><sx> and the output type's extension
std::string OutputName(const Options& o, const std::string& input)
{
    if (o.inputs.size() == 1 && Writes(FileTypeOf(o.out)) && o.prefix.empty() && o.suffix.empty()) return o.out;
    std::string base = input.substr(input.find_last_of('/') == std::string::npos ? 0 : input.find_last_of('/') + 1);
    if (base.find_last_of('.') != std::string::npos) base.erase(base.find_last_of('.'));
    std::string name = o.prefix + base + o.suffix + ExtensionOf(o.outType);
    if (o.lower) std::transform(name.begin(), name.end(), name.begin(), [](unsigned char c) { return char(std::tolower(c)); });
    return o.out + "/" + name;
}

struct StepFailed { const char* what; HRESULT hr; };

// PremultiplyAlpha checks the texture's alpha mode (DirectXTexPMAlpha.cpp:283-284); the tool tracks it in `info`, which must be what the
// resident image carries
HRESULT PremultiplyAlphaWithMode(Device& dev, const DeviceScratchImage& image, const TexMetadata& info, TEX_PMALPHA_FLAGS flags, DeviceScratchImage& result)
{
    if (image.GetMetadata().miscFlags2 != info.miscFlags2) return E_FAIL;
    return PremultiplyAlpha(dev, image, flags, result);
}

// One file through the pipeline; throws StepFailed. The texture is uploaded ONCE after the file has been decoded, every step runs on the
// device-resident copy (DeviceScratchImage in, DeviceScratchImage out: the steps queue their kernels on the Device's stream back to back),
// and the final images come back ONCE for the file writer: two PCIe transfers per file whatever the number of steps, where the
// ScratchImage -> ScratchImage calls of the reference tool's sequence would be one round trip per step.
void ConvertOne(Device& dev, const Options& o, const std::string& inFile, const std::string& outFile)
{
    auto check = [](const char* what, HRESULT hr) { if (FAILED(hr)) throw StepFailed{ what, hr }; };
    const TEX_FILTER_FLAGS filter = TEX_FILTER_FLAGS(o.filter | o.filterOpts);
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t up0 = 0, down0 = 0;
    GetTransferBytes(dev, up0, down0);

    TexMetadata info;
    // the file goes up at the bytes a texel it has on disk and becomes the image's texels on the device (tool_files.h: SourceFile)
    DeviceScratchImage image;
    check("load", Load(dev, inFile.c_str(), InputType(inFile), o.ReadFlags(true), info, image));
    std::printf("reading %s (%zux%zu", inFile.c_str(), info.width, info.height);
    if (info.dimension == TEX_DIMENSION_TEXTURE3D) std::printf("x%zu", info.depth);
    std::printf(", %zu mips, %zu items, format %u)\n", info.mipLevels, info.arraySize, unsigned(info.format));
    size_t tMips = (!o.mipLevels && info.mipLevels > 1) ? info.mipLevels : o.mipLevels;           // texconv.cpp:2270

    // --- the one upload has happened: the file's texels as the file has them
    auto keep = [&](DeviceScratchImage& t)         // a step produced t: it becomes the image, metadata keeps its alpha mode
    {
        const uint32_t misc2 = info.miscFlags2;
        image = std::move(t); info = image.GetMetadata(); info.miscFlags2 = misc2;
    };

    // --- planar (texconv.cpp:2277-2312): NV12 / P010 / P016 / NV11 become their single-plane forms on the device, before anything else
    if (IsPlanar(info.format))
    {
        DeviceScratchImage t;
        check("converttosingleplane", ConvertToSinglePlane(dev, image, t));
        keep(t);
    }
    const DXGI_FORMAT tformat = o.format ? DXGI_FORMAT(o.format) : info.format;

    // --- decompress (texconv.cpp:2325-2480). The compressed original is kept on the device: if no step below changes the texels and the
    // target is its format, it is written back as it is instead of being encoded again.
    DeviceScratchImage dcimage;
    bool haveOriginal = false;
    if (IsCompressed(info.format))
    {
        // texconv.cpp:2394-2448: BC4 / BC5 decode to four channels where a later step reads or writes the ones they lack
        const TexTransform& sw = o.swizzle;
        const bool swz123 = sw.swizzle[1] != 1 || sw.swizzle[2] != 2 || sw.swizzle[3] != 3 || sw.zero[1] || sw.zero[2] || sw.zero[3] || sw.one[1] || sw.one[2] || sw.one[3];
        const bool swz23 = sw.swizzle[2] != 2 || sw.swizzle[3] != 3 || sw.zero[2] || sw.zero[3] || sw.one[2] || sw.one[3];
        DXGI_FORMAT formatDecompress = DXGI_FORMAT_UNKNOWN;
        switch (info.format)
        {
        case DXGI_FORMAT_BC4_SNORM: if (o.invertY || o.reconstructZ || swz123) formatDecompress = DXGI_FORMAT_R8G8B8A8_SNORM; break;
        case DXGI_FORMAT_BC5_SNORM: if (o.reconstructZ || swz23) formatDecompress = DXGI_FORMAT_R8G8B8A8_SNORM; break;
        case DXGI_FORMAT_BC4_UNORM: if (o.invertY || o.reconstructZ || swz123) formatDecompress = DXGI_FORMAT_R8G8B8A8_UNORM; break;
        case DXGI_FORMAT_BC5_UNORM: if (o.reconstructZ || swz23) formatDecompress = DXGI_FORMAT_R8G8B8A8_UNORM; break;
        default: break;
        }
        DeviceScratchImage t;
        check("decompress", Decompress(dev, image, formatDecompress, t));
        dcimage = std::move(image); haveOriginal = true;
        keep(t);
    }

    // --- undo premultiplied alpha
    if (o.demul && HasAlpha(info.format) && info.format != DXGI_FORMAT_A8_UNORM)
    {
        if (info.GetAlphaMode() == TEX_ALPHA_MODE_STRAIGHT) std::printf("WARNING: image is already using straight alpha\n");
        else if (!info.IsPMAlpha()) std::printf("WARNING: image is not using premultiplied alpha\n");
        else
        {
            DeviceScratchImage t;
            // the alpha mode lives in the tool's metadata: the resident image carries the file's, which the step checks (DirectXTexPMAlpha.cpp:283-284)
            check("demultiply alpha", PremultiplyAlphaWithMode(dev, image, info, TEX_PMALPHA_FLAGS(TEX_PMALPHA_REVERSE | o.srgb), t));
            info.miscFlags2 = t.GetMetadata().miscFlags2;
            image = std::move(t);
            haveOriginal = false;
        }
    }

    // --- flip (texconv.cpp:2533-2574): every item, mip and slice of the texture; ends any hand-through of the blocks, as cimage.reset() there
    if (o.hflip || o.vflip)
    {
        DeviceScratchImage t;
        check("fliprotate", FlipRotate(dev, image, TEX_FR_FLAGS((o.hflip ? TEX_FR_FLIP_HORIZONTAL : 0u) | (o.vflip ? TEX_FR_FLIP_VERTICAL : 0u)), t));
        keep(t);
        haveOriginal = false;
    }

    // --- resize: level 0 of every item / slice; the result has one level (DirectXTexResize.cpp:942-1103)
    size_t tw = o.width ? o.width : info.width, th = o.height ? o.height : info.height;
    if (tw > o.maxSize) { if (!o.width) tw = o.maxSize; else std::printf("WARNING: width exceeds the feature level's %zu\n", o.maxSize); }
    if (th > o.maxSize) { if (!o.height) th = o.maxSize; else std::printf("WARNING: height exceeds the feature level's %zu\n", o.maxSize); }
    if (o.pow2) FitPowerOf2(info.width, info.height, tw, th, o.maxSize);
    if (tw != info.width || th != info.height)
    {
        DeviceScratchImage t;
        check("resize", Resize(dev, image, tw, th, filter, t));
        keep(t);
        haveOriginal = false;
        if (tMips > 0)
        {
            size_t maxMips = 0;
            if (info.depth > 1) CalculateMipLevels3D(info.width, info.height, info.depth, maxMips); else CalculateMipLevels(info.width, info.height, maxMips);
            tMips = std::min(tMips, maxMips);
        }
    }

    // --- per-texel transforms on the resident image (TransformImage with texconv's lambdas); each one ends any hand-through of the blocks
    auto transform = [&](const char* what, const TexTransform& t)
    {
        DeviceScratchImage r;
        check(what, TransformImage(dev, image, t, r));
        keep(r);
        haveOriginal = false;
    };
    auto simple = [](TEX_TRANSFORM_OP op, uint32_t key = 0) { TexTransform t; t.op = op; t.colorKey = key; return t; };
    if (!IsIdentitySwizzle(o.swizzle)) transform("swizzle", o.swizzle);

    // --- colour rotation (texconv.cpp:2696-2964). HDR10to709 and P3D65to709 first convert to R16G16B16A16_FLOAT with the pipeline's flags
    // and threshold (:2699-2733); `tformat` was fixed before (:2314), so without -f the convert step below returns to the input's format
    if (o.rotateColor)
    {
        if (o.rotateColor == TEX_ROTATE_HDR10_TO_709 || o.rotateColor == TEX_ROTATE_P3D65_TO_709)
        {
            // (an input that already is R16G16B16A16_FLOAT fails here with E_INVALIDARG, as it does in texconv: Convert refuses the same format)
            DeviceScratchImage t;
            check("convert", Convert(dev, image, DXGI_FORMAT_R16G16B16A16_FLOAT, TEX_FILTER_FLAGS(filter | o.srgb | o.convert), o.alphaThreshold, t));
            keep(t);
        }
        DeviceScratchImage r;
        check("rotate color apply", RotateColor(dev, image, TEX_ROTATE_COLOR(o.rotateColor), o.paperWhiteNits, r));
        keep(r);
        haveOriginal = false;
    }
    if (o.tonemap) transform("tonemap", simple(TEX_TRANSFORM_TONEMAP));

    // --- normal map (texconv.cpp:3047-3098), in place of the convert step; a compressed target gets texconv's intermediate format
    if (o.nmap)
    {
        DXGI_FORMAT nmfmt = tformat;
        if (IsCompressed(tformat))
        {
            const bool wide = BitsPerColor(info.format) > 8;
            if (tformat == DXGI_FORMAT_BC4_SNORM || tformat == DXGI_FORMAT_BC5_SNORM) nmfmt = wide ? DXGI_FORMAT_R16G16B16A16_SNORM : DXGI_FORMAT_R8G8B8A8_SNORM;
            else if (tformat == DXGI_FORMAT_BC6H_SF16 || tformat == DXGI_FORMAT_BC6H_UF16) nmfmt = DXGI_FORMAT_R32G32B32_FLOAT;
            else nmfmt = wide ? DXGI_FORMAT_R16G16B16A16_UNORM : DXGI_FORMAT_R8G8B8A8_UNORM;
        }
        DeviceScratchImage t;
        check("normalmap", ComputeNormalMap(dev, image, CNMAP_FLAGS(o.nmapFlags), o.nmapAmplitude, nmfmt, t));
        keep(t);
        haveOriginal = false;
    }
    // --- convert to the uncompressed target format
    else if (!IsCompressed(tformat) && tformat != info.format)
    {
        DeviceScratchImage t;
        check("convert", Convert(dev, image, tformat, TEX_FILTER_FLAGS(filter | o.srgb | o.convert), o.alphaThreshold, t));
        keep(t);
        haveOriginal = false;
    }

    if (o.colorKey && HasAlpha(info.format)) transform("colorkey", simple(TEX_TRANSFORM_COLOR_KEY, o.colorKeyValue));
    if (o.invertY) transform("inverty", simple(TEX_TRANSFORM_INVERT_Y));
    if (o.reconstructZ) transform("reconstructz", simple(TEX_TRANSFORM_RECONSTRUCT_Z));

    // --- mipmaps
    const bool keepCoverage = o.keepCoverage > 0.f && HasAlpha(info.format) && !IsAlphaAllOpaque(dev, image);
    TEX_FILTER_FLAGS filter3D = filter;
    if (!ispow2(info.width) || !ispow2(info.height) || !ispow2(info.depth))
    {
        if (!tMips || info.mipLevels != 1) std::printf("WARNING: not a power-of-two texture with mips\n");
        if (info.dimension == TEX_DIMENSION_TEXTURE3D) filter3D = TEX_FILTER_FLAGS(TEX_FILTER_TRIANGLE | o.filterOpts);      // the only correct one for such volumes (:3317-3321)
    }
    if ((!tMips || info.mipLevels != tMips || keepCoverage) && info.mipLevels != 1)
    {
        // generation starts from a single level: strip the existing chain
        DeviceScratchImage t;
        check("copy to single level", CopyTopLevels(dev, image, t));
        keep(t);
        if (haveOriginal && tMips == 1)
        {
            // only trimming mips off a compressed texture: its top level stays the encoder's original (:3378-3412)
            DeviceScratchImage dc;
            check("copy compressed to single level", CopyTopLevels(dev, dcimage, dc));
            dcimage = std::move(dc);
        }
        else haveOriginal = false;
    }
    if ((!tMips || info.mipLevels != tMips) && (info.width > 1 || info.height > 1 || info.depth > 1))
    {
        DeviceScratchImage t;
        if (info.dimension == TEX_DIMENSION_TEXTURE3D) check("mipmaps", GenerateMipMaps3D(dev, image, filter3D, tMips, t));
        else check("mipmaps", GenerateMipMaps(dev, image, filter, tMips, t));
        keep(t);
        haveOriginal = false;
    }

    // --- keep the alpha-test coverage of level 0 in the smaller levels
    if (keepCoverage && info.mipLevels != 1)
    {
        DeviceScratchImage t;
        check("keepcoverage", ScaleMipMapsAlphaForCoverage(dev, image, o.keepCoverage, t));
        image = std::move(t);
        haveOriginal = false;
    }

    // --- premultiplied alpha
    if (o.pmalpha && HasAlpha(info.format) && info.format != DXGI_FORMAT_A8_UNORM)
    {
        if (info.IsPMAlpha()) std::printf("WARNING: image is already using premultiplied alpha\n");
        else
        {
            DeviceScratchImage t;
            check("premultiply alpha", PremultiplyAlphaWithMode(dev, image, info, TEX_PMALPHA_FLAGS(TEX_PMALPHA_DEFAULT | o.srgb), t));
            info.miscFlags2 = t.GetMetadata().miscFlags2;
            image = std::move(t);
            haveOriginal = false;
        }
    }

    // --- compress
    bool handThrough = false;
    if (IsCompressed(tformat))
    {
        if (haveOriginal && dcimage.GetMetadata().format == tformat)
        {
            // nothing touched the texels and the input already has the target format: hand its blocks through (:3566-3574)
            handThrough = true;
            const uint32_t misc2 = info.miscFlags2;
            info = dcimage.GetMetadata(); info.miscFlags2 = misc2;
            image = std::move(dcimage);
        }
        else
        {
            if ((info.width % 4) || (info.height % 4)) std::printf("WARNING: block-compressed texture whose size is not a multiple of 4\n");
            DeviceScratchImage t;
            check("compress", Compress(dev, image, tformat, TEX_COMPRESS_FLAGS(o.compress | o.srgb), o.alphaThreshold, t));
            keep(t);
        }
    }

    // --- alpha mode (texconv.cpp:3738-3766): a reduction on the device, compressed results decoded there
    if (HasAlpha(info.format) && info.format != DXGI_FORMAT_A8_UNORM)
    {
        if (IsAlphaAllOpaque(dev, image)) info.SetAlphaMode(TEX_ALPHA_MODE_OPAQUE);
        else if (info.IsPMAlpha()) { }
        else if (o.sepalpha) info.SetAlphaMode(TEX_ALPHA_MODE_CUSTOM);
        else if (info.GetAlphaMode() == TEX_ALPHA_MODE_UNKNOWN) info.SetAlphaMode(TEX_ALPHA_MODE_STRAIGHT);
    }
    else info.SetAlphaMode(TEX_ALPHA_MODE_UNKNOWN);

    // --- save
    if (!o.overwrite)
    {
        struct stat st;
        if (::stat(outFile.c_str(), &st) == 0) { std::printf("skipping %s: it exists (use -y to overwrite)\n", outFile.c_str()); return; }
    }
    // --- the one download, by the resident writers (tool_files.h: Save). A .dds takes every image; the other types take level 0 of the first
    // item, like texconv's non-DDS codecs. -tga20: with the TGA 2.0 extension area
    uint32_t ddsFlags = DDS_FLAGS_NONE;
    if (o.dx10) ddsFlags |= DDS_FLAGS_FORCE_DX10_EXT | DDS_FLAGS_FORCE_DX10_EXT_MISC2;
    else if (o.dx9) ddsFlags |= DDS_FLAGS_FORCE_DX9_LEGACY;
    const TexMetadata* tga20 = o.tga20 ? &info : nullptr;
    if (o.outType != FileType::DDS && handThrough)
    {
        // blocks handed through: the host codec's answer
        ScratchImage result;
        check("download", image.Download(result));
        const Image& first = result.GetImages()[0];
        switch (o.outType)
        {
        case FileType::HDR: check("save", SaveToHDRFile(first, outFile.c_str())); break;
        case FileType::TGA: check("save", SaveToTGAFile(first, TGA_FLAGS_NONE, outFile.c_str(), tga20)); break;
        case FileType::PPM: check("save", SaveToPortablePixMapFile(first, outFile.c_str())); break;
        case FileType::PFM: check("save", SaveToPortablePixMapHDRFile(first, outFile.c_str())); break;
        case FileType::PNG: check("save", SaveToPNGFile(first, PNG_FLAGS_NONE, outFile.c_str())); break;
        case FileType::EXR: check("save", SaveToEXRFile(first, outFile.c_str())); break;
        case FileType::TIFF: check("save", SaveToTIFFFile(first, TIFF_FLAGS_NONE, outFile.c_str())); break;
        default: check("save", HRESULT_E_NOT_SUPPORTED);          // -ft takes no other type
        }
    }
    else check("save", Save(dev, o.outType, image, info, DDS_FLAGS(ddsFlags), tga20, outFile.c_str()));
    image.Release();
    std::printf("writing %s (%zux%zu", outFile.c_str(), info.width, info.height);
    if (info.dimension == TEX_DIMENSION_TEXTURE3D) std::printf("x%zu", info.depth);
    std::printf(", %zu mips, %zu items, format %u)\n", info.mipLevels, info.arraySize, unsigned(info.format));
    if (o.timing)
    {
        uint64_t up = 0, down = 0;
        GetTransferBytes(dev, up, down);
        std::printf("  %s: %.3f ms, host -> device %llu bytes, device -> host %llu bytes\n", inFile.c_str(),
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), (unsigned long long)(up - up0), (unsigned long long)(down - down0));
    }
}
}

// -info: what a file holds (the header only; no GPU involved) - the "info" command of the reference's texdiag in one line per file
int PrintInfo(const Options& o)
{
    int failures = 0;
    for (const std::string& f : o.inputs)
    {
        TexMetadata m;
        const HRESULT hr = GetMetadata(f.c_str(), InputType(f), o.ReadFlags(false), m);
        if (FAILED(hr)) { std::printf("%s: FAILED (%08X)\n", f.c_str(), unsigned(hr)); ++failures; continue; }
        const char* name = FormatName(m.format, "");
        static const char* const alpha[] = { "unknown", "straight", "premultiplied", "opaque", "custom" };
        size_t images = 0, bytes = 0;
        for (size_t level = 0, w = m.width, h = m.height, d = m.depth; level < m.mipLevels; ++level)
        {
            size_t rp = 0, sp = 0;
            if (SUCCEEDED(ComputePitch(m.format, w, h, rp, sp))) bytes += sp * d * (m.dimension == TEX_DIMENSION_TEXTURE3D ? 1 : m.arraySize);
            images += d * (m.dimension == TEX_DIMENSION_TEXTURE3D ? 1 : m.arraySize);
            if (w > 1) w >>= 1;
            if (h > 1) h >>= 1;
            if (d > 1) d >>= 1;
        }
        std::printf("%s: %zux%zu", f.c_str(), m.width, m.height);
        if (m.dimension == TEX_DIMENSION_TEXTURE3D) std::printf("x%zu", m.depth);
        std::printf(" %s mips %zu items %zu format %u %s bpp %zu alpha %s%s images %zu bytes %zu%s\n",
                    m.dimension == TEX_DIMENSION_TEXTURE1D ? "1D" : m.dimension == TEX_DIMENSION_TEXTURE3D ? "3D" : (m.IsCubemap() ? "cube" : "2D"),
                    m.mipLevels, m.arraySize, unsigned(m.format), name, BitsPerPixel(m.format), alpha[std::min<uint32_t>(m.GetAlphaMode(), 4)],
                    IsSRGB(m.format) ? " sRGB" : "", images, bytes, IsSupportedOnDevice(m.format) ? "" : " (container only: no GPU path for this format)");
    }
    return failures ? 1 : 0;
}

int main(int argc, char** argv)
{
    Options o;
    if (!Parse(argc, argv, o)) return usage();
    if (o.info) return PrintInfo(o);
    if (!o.nologo) std::printf("dxtexconv: DirectXTex pipeline on MI355X (gfx950)\n");

    // Image-per-GPU sharding: files are independent, so worker k takes inputs k, k + n, k + 2n, ... on its own
    // Device; no data moves between GPUs. With one GPU this is a plain loop on the calling thread.
    std::atomic<int> failures{ 0 };
    auto work = [&](size_t k, size_t n)
    {
        Device dev;
        if (FAILED(dev.Create(o.gpus[k]))) { std::fprintf(stderr, "no gfx950 device %d (this tool has no CPU path)\n", o.gpus[k]); failures += int((o.inputs.size() - k + n - 1) / n); return; }
        for (size_t i = k; i < o.inputs.size(); i += n)
        {
            try { ConvertOne(dev, o, o.inputs[i], OutputName(o, o.inputs[i])); }
            catch (const StepFailed& f)
            {
                std::fprintf(stderr, "FAILED [%s] (%08X) %s: %s\n", f.what, unsigned(f.hr), o.inputs[i].c_str(), dev.LastError());
                ++failures;                               // like texconv: report, go on with the next file, exit code 1
            }
        }
    };
    // Two (-overlap n) workers per GPU, each with its own Device: while one worker's kernels run, the other reads, decodes and uploads its next
    // file (or downloads and writes its last one), so the PCIe transfers and the file codecs of file k + 1 overlap the kernels of file k.
    if (o.overlap > 1 && o.inputs.size() > o.gpus.size())
    {
        std::vector<int> expanded;
        for (size_t r = 0; r < o.overlap; ++r) expanded.insert(expanded.end(), o.gpus.begin(), o.gpus.end());
        o.gpus = expanded;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const size_t workers = std::min(o.gpus.size(), o.inputs.size());
    if (workers <= 1) work(0, 1);
    else
    {
        std::vector<std::thread> pool;
        for (size_t k = 0; k < workers; ++k) pool.emplace_back(work, k, workers);
        for (std::thread& t : pool) t.join();
    }
    if (o.timing) std::printf("processing time: %.3f seconds\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    return failures.load() ? 1 : 0;
}
