// What the codec test programs under tests/cpp share (hdr_rgbe_, tga_, dds_, pnm_, png_, jpeg_, jpeg_write_, exr_ and tiff_host_test and
// dds_device_test): files in and out, the exact-size copy a loader is handed, the transfer and kernel-mark window around one resident call,
// what a failed resident load must leave, the seeded damaged copies, and the frame of the time_ commands. Nothing of any one codec: the
// sanitizer builds compile one codec's source each. Plain functions with internal linkage; a program uses the ones it needs.
#pragma once
#include "../../directxtex_amd/host/DirectXTexAMD.h"
#include "../../include/dxtex_amd.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <sstream>
#include <string>
#include <vector>

#pragma GCC diagnostic push
#pragma GCC diagnostic ignored "-Wunused-function"

using namespace DirectXTexAMD;

static bool read_file(const std::string& path, std::vector<uint8_t>& buf)
{
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    buf.clear();
    uint8_t chunk[65536];
    size_t n;
    while ((n = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + n);
    std::fclose(f);
    return true;
}

static bool write_file(const std::string& path, const void* p, size_t bytes)
{
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || std::fwrite(p, 1, bytes, f) == bytes;
    return (std::fclose(f) == 0) && ok;
}

// the non-empty lines of a list file; each program parses its own fields out of them
static std::vector<std::string> read_lines(const char* path)
{
    std::vector<std::string> lines;
    std::ifstream in(path);
    for (std::string line; std::getline(in, line);) if (!line.empty()) lines.push_back(line);
    return lines;
}

static bool same_metadata(const TexMetadata& a, const TexMetadata& b)
{
    return a.width == b.width && a.height == b.height && a.depth == b.depth && a.arraySize == b.arraySize && a.mipLevels == b.mipLevels &&
           a.miscFlags == b.miscFlags && a.miscFlags2 == b.miscFlags2 && a.format == b.format && a.dimension == b.dimension;
}

// the texels of two images of one format and size, row by row: their pitches may differ
static bool same_texels(const Image& a, const Image& b)
{
    size_t rp = 0, sp = 0;
    if (a.format != b.format || a.width != b.width || a.height != b.height || FAILED(ComputePitch(a.format, a.width, a.height, rp, sp))) return false;
    for (size_t y = 0; y < a.height; ++y) if (std::memcmp(a.pixels + y * a.rowPitch, b.pixels + y * b.rowPitch, rp)) return false;
    return true;
}

// <in.bin> <width> <height> <format> <rowPitch> of a command line as an image over px
static bool image_arg(char** a, std::vector<uint8_t>& px, Image& src)
{
    if (!read_file(a[0], px)) return false;
    src.width = size_t(std::atoll(a[1])); src.height = size_t(std::atoll(a[2])); src.format = DXGI_FORMAT(std::atoi(a[3]));
    src.rowPitch = size_t(std::atoll(a[4])); src.slicePitch = src.rowPitch * src.height; src.pixels = px.data();
    return px.size() >= src.slicePitch;
}

// an exact-size copy on the heap: a read past the file's last byte is a read past an allocation. p is never null; a program that hands
// a loader nullptr for an empty file says so itself
struct Exact
{
    uint8_t* p = nullptr; size_t n = 0;
    Exact(const uint8_t* s, size_t bytes) : n(bytes) { p = static_cast<uint8_t*>(std::malloc(n ? n : 1)); if (n) std::memcpy(p, s, n); }
    Exact(const Exact&) = delete;
    Exact& operator=(const Exact&) = delete;
    ~Exact() { std::free(p); }
};

// whether a failed resident load left its result empty
static bool released(const DeviceScratchImage& image)
{
    return image.GetImageCount() == 0 && image.GetPixels() == nullptr && image.GetImages() == nullptr;
}

// The bytes moved and the kernels launched around one resident call: opens on construction, end() closes it
struct Window
{
    struct Mark { unsigned launches = 0; float ms = 0; };
    Device& dev;
    uint64_t up0 = 0, down0 = 0;
    uint64_t up = 0, down = 0;          // host -> device and device -> host, once end() has run

    explicit Window(Device& d) : dev(d) { GetTransferBytes(dev, up0, down0); dxtex_ctx_profile_begin(dev.Get()); }

    // per prefix, the launches and milliseconds of the kernels whose mark starts with it; 999 launches each where the profile could not be read
    std::vector<Mark> end(std::initializer_list<const char*> prefixes = {})
    {
        std::vector<Mark> marks(prefixes.size());
        char names[4096] = {};
        float ms[64]; uint32_t launches[64]; size_t count = 0;
        if (dxtex_ctx_profile_end(dev.Get(), names, sizeof(names), ms, launches, 64, &count) != DXTEX_S_OK) for (Mark& m : marks) m.launches = 999;
        else
        {
            std::istringstream ss(names);
            std::string name;
            for (size_t i = 0; i < count && std::getline(ss, name); ++i)
            {
                size_t k = 0;
                for (const char* prefix : prefixes) { if (name.rfind(prefix, 0) == 0) { marks[k].launches += launches[i]; marks[k].ms += ms[i]; } ++k; }
            }
        }
        GetTransferBytes(dev, up, down);
        up -= up0; down -= down0;
        return marks;
    }
};

// Seeded damaged copies of a file through load(p, n, hr), the program's pair of loaders, which returns false where they left something
// behind or disagree: `cases` copies with one to four bytes changed each, or with `truncations` every proper prefix, none of which may
// load. Prints "fuzz|truncations <loaded> <refused>".
template<class Load>
static int damaged_copies(const char* file, bool truncations, uint64_t seed, size_t cases, Load&& load)
{
    std::vector<uint8_t> data;
    if (!read_file(file, data) || data.empty()) return 1;
    size_t loaded = 0, refused = 0;
    uint64_t s = seed * 6364136223846793005ull + 1442695040888963407ull;
    auto next = [&] { s = s * 6364136223846793005ull + 1442695040888963407ull; return uint32_t(s >> 33); };
    if (truncations) cases = data.size();
    for (size_t i = 0; i < cases; ++i)
    {
        std::vector<uint8_t> copy(data.begin(), truncations ? data.begin() + i : data.end());
        if (!truncations)
            for (uint32_t k = 1 + next() % 4; k; --k)
            {
                const size_t at = next() % copy.size();
                const uint32_t how = next() % 3;
                copy[at] = how == 0 ? uint8_t(next()) : how == 1 ? uint8_t(copy[at] ^ (1u << (next() % 8))) : (next() & 1 ? 0xFF : 0x00);
            }
        const Exact exact(copy.data(), copy.size());
        HRESULT hr;
        if (!load(exact.p, exact.n, hr)) return 1;
        if (truncations && SUCCEEDED(hr)) { std::fprintf(stderr, "a prefix of %zu bytes loaded\n", i); return 1; }
        if (SUCCEEDED(hr)) ++loaded; else ++refused;
    }
    std::printf("%s %zu %zu\n", truncations ? "truncations" : "fuzz", loaded, refused);
    return 0;
}

template<class F>
static double timed_ms(F&& f)
{
    const auto t0 = std::chrono::steady_clock::now();
    f();
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The time_ commands: the resident path and the same build's host path, alternating, `runs` times each after one unmeasured run each.
// resident() and host() return their milliseconds; tail(extra) runs after both, may append fields to the line and returns whether every
// step of the run succeeded.
template<class Resident, class Host, class Tail>
static int time_runs(Device& dev, int runs, Resident&& resident, Host&& host, Tail&& tail)
{
    for (int i = -1; i < runs; ++i)
    {
        uint64_t up0, down0, up1, down1, up2, down2;
        GetTransferBytes(dev, up0, down0);
        const double a = resident();
        GetTransferBytes(dev, up1, down1);
        const double b = host();
        GetTransferBytes(dev, up2, down2);
        std::string extra;
        if (!tail(extra)) { std::fprintf(stderr, "a step failed\n"); return 1; }
        if (i >= 0) std::printf("run %d resident %.3f ms up %llu down %llu host %.3f ms up %llu down %llu%s\n", i, a, (unsigned long long)(up1 - up0), (unsigned long long)(down1 - down0),
                                b, (unsigned long long)(up2 - up1), (unsigned long long)(down2 - down1), extra.c_str());
    }
    return 0;
}

#pragma GCC diagnostic pop
