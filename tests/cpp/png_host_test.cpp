// The PNG codec through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_png_cpu.py (the first three commands, which
// need no device; also built with sanitizers as png_host_test_asan) and tests/test_png_host_gpu.py (the next two).
//
//   png_host_test load_many <list>
//       <list> holds one "<PNG_FLAGS> <file path>" per line. Each file goes through LoadFromPNGMemoryRaw, the host LoadFromPNGMemory and
//       GetMetadataFromPNGMemory; one line per file: "<index> <raw hresult hex> <host hresult hex> <metadata hresult hex>" and, where it
//       loaded, " ok <width> <height> <format> <depth> <arraySize> <mipLevels> <miscFlags> <miscFlags2> <dimension> <kind> <raw flags>
//       <palette count> <row bytes> <rows bytes> <offset> <bytes>", the image's tight rows being <bytes> bytes at <offset> of <list>.out
//   png_host_test save <in.bin> <width> <height> <format> <rowPitch> <PNG_FLAGS> <out>
//       SaveToPNGMemory of the pixels -> <out>; prints "hr <hresult hex>"
//   png_host_test errors <file>
//       the null-argument and missing-file answers of the file forms; prints one "name hresult" per line
//   png_host_test device_load_many <list>
//       the same list through the host loader and through its resident form; one line per file: "<index> <resident hresult hex> <host
//       hresult hex>", then " ok <width> <height> <format> <rows bytes> <bytes host -> device> <bytes device -> host> <metadata equal>
//       <pixels equal> <png kernel launches>", or " released" / " held" for whether a failure left the result empty
//   png_host_test device_save <in.bin> <width> <height> <format> <rowPitch> <PNG_FLAGS> <out>
//       the image goes up, the resident saver writes <out> and the host one <out>.host from the same pixels; prints "hr <resident hresult
//       hex> <host hresult hex> <bytes host -> device> <bytes device -> host>" counted around the resident save alone
//   png_host_test time_raw <file> <runs> | time_load <file> <runs> | time_save <file> <runs>
//       for tools/png_bench.py: the byte-serial half alone (no device); wall time and bytes moved of the resident path beside the same
//       build's host path, one line per run
#include "codec_host_test.h"

struct Line { PNG_FLAGS flags; std::string path; };
static std::vector<Line> read_list(const char* path)
{
    std::vector<Line> lines;
    for (const std::string& line : read_lines(path))
    {
        const size_t sp = line.find(' ');
        if (sp != std::string::npos) lines.push_back({ PNG_FLAGS(std::strtoul(line.substr(0, sp).c_str(), nullptr, 0)), line.substr(sp + 1) });
    }
    return lines;
}

static int load_many(const char* list)
{
    const std::vector<Line> files = read_list(list);
    std::vector<uint8_t> data;
    PNGRawImage raw; ScratchImage image;          // one object each for every file: a failure must leave it empty whatever it held before
    FILE* out = std::fopen((std::string(list) + ".out").c_str(), "wb");
    if (!out) return 1;
    size_t offset = 0;
    for (size_t i = 0; i < files.size(); ++i)
    {
        const std::string& path = files[i].path;
        if (!read_file(path, data)) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); return 1; }
        const Exact exact(data.data(), data.size());
        TexMetadata rawMd, md, only;
        const HRESULT rawHr = LoadFromPNGMemoryRaw(exact.p, exact.n, files[i].flags, &rawMd, raw);
        const HRESULT hr = LoadFromPNGMemory(exact.p, exact.n, files[i].flags, &md, image);
        const HRESULT metaHr = GetMetadataFromPNGMemory(exact.p, exact.n, files[i].flags, only);
        if (FAILED(rawHr) && (raw.rows || raw.storage.GetBufferPointer())) { std::fprintf(stderr, "%s: the raw image was not released\n", path.c_str()); return 1; }
        if (FAILED(hr) && (image.GetImageCount() || image.GetPixels())) { std::fprintf(stderr, "%s: the image was not released\n", path.c_str()); return 1; }
        if (FAILED(rawHr) || FAILED(hr)) { std::printf("%zu %08x %08x %08x\n", i, unsigned(rawHr), unsigned(hr), unsigned(metaHr)); continue; }
        if (FAILED(metaHr) || !same_metadata(rawMd, md) || !same_metadata(md, only)) { std::fprintf(stderr, "%s: the metadata differ\n", path.c_str()); return 1; }
        if (raw.rows != raw.storage.GetBufferPointer() || raw.rowsBytes != raw.rowBytes * md.height || raw.storage.GetBufferSize() != raw.rowsBytes)
        { std::fprintf(stderr, "%s: the rows are not the storage\n", path.c_str()); return 1; }
        const Image* img = image.GetImage(0, 0, 0);
        size_t rp = 0, sp = 0;
        if (!img || FAILED(ComputePitch(md.format, md.width, md.height, rp, sp))) return 1;
        for (size_t y = 0; y < md.height; ++y) if (std::fwrite(img->pixels + y * img->rowPitch, 1, rp, out) != rp) return 1;
        std::printf("%zu %08x %08x %08x ok %zu %zu %u %zu %zu %zu %u %u %u %u %u %u %zu %zu %zu %zu\n", i, unsigned(rawHr), unsigned(hr), unsigned(metaHr), md.width, md.height,
                    unsigned(md.format), md.depth, md.arraySize, md.mipLevels, unsigned(md.miscFlags), unsigned(md.miscFlags2), unsigned(md.dimension), raw.kind, raw.flags,
                    raw.paletteCount, raw.rowBytes, raw.rowsBytes, offset, rp * md.height);
        offset += rp * md.height;
    }
    return std::fclose(out) == 0 ? 0 : 1;
}

static int save(char** a)
{
    std::vector<uint8_t> px; Image src;
    if (!image_arg(a, px, src)) return 1;
    Blob blob;
    const HRESULT hr = SaveToPNGMemory(src, PNG_FLAGS(std::strtoul(a[5], nullptr, 0)), blob);
    if (FAILED(hr) && blob.GetBufferPointer()) { std::fprintf(stderr, "the blob was not released\n"); return 1; }
    if (SUCCEEDED(hr) && !write_file(a[6], blob.GetBufferPointer(), blob.GetBufferSize())) return 1;
    std::printf("hr %08x\n", unsigned(hr));
    return 0;
}

static int errors(const char* file)
{
    TexMetadata md; ScratchImage image; PNGRawImage raw; Blob blob;
    const std::string missing = std::string(file) + ".is-not-there";
    uint8_t px[4] = {};
    Image one; one.width = one.height = 1; one.format = DXGI_FORMAT_R8G8B8A8_UNORM; one.rowPitch = one.slicePitch = 4; one.pixels = px;
    std::printf("metadata_null %08x\n", unsigned(GetMetadataFromPNGFile(nullptr, PNG_FLAGS_NONE, md)));
    std::printf("load_null %08x\n", unsigned(LoadFromPNGFile(nullptr, PNG_FLAGS_NONE, &md, image)));
    std::printf("raw_null %08x\n", unsigned(LoadFromPNGFileRaw(nullptr, PNG_FLAGS_NONE, &md, raw)));
    std::printf("memory_null %08x\n", unsigned(LoadFromPNGMemory(nullptr, 64, PNG_FLAGS_NONE, &md, image)));
    std::printf("save_null %08x\n", unsigned(SaveToPNGFile(one, PNG_FLAGS_NONE, nullptr)));
    std::printf("metadata_missing %08x\n", unsigned(GetMetadataFromPNGFile(missing.c_str(), PNG_FLAGS_NONE, md)));
    std::printf("load_missing %08x\n", unsigned(LoadFromPNGFile(missing.c_str(), PNG_FLAGS_NONE, &md, image)));
    std::printf("raw_missing %08x\n", unsigned(LoadFromPNGFileRaw(missing.c_str(), PNG_FLAGS_NONE, &md, raw)));
    std::printf("load_file %08x\n", unsigned(LoadFromPNGFile(file, PNG_FLAGS_NONE, &md, image)));
    std::printf("metadata_file %08x\n", unsigned(GetMetadataFromPNGFile(file, PNG_FLAGS_NONE, md)));
    return 0;
}

static int device_load_many(const char* list)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    const std::vector<Line> files = read_list(list);
    std::vector<uint8_t> data;
    DeviceScratchImage image;
    for (size_t i = 0; i < files.size(); ++i)
    {
        if (!read_file(files[i].path, data)) { std::fprintf(stderr, "cannot read %s\n", files[i].path.c_str()); return 1; }
        TexMetadata hostMd, rawMd; ScratchImage host; PNGRawImage raw;
        const uint8_t none = 0;
        const uint8_t* source = data.empty() ? &none : data.data();          // an empty file is a size of zero, not a null pointer
        const HRESULT hostHr = LoadFromPNGMemory(source, data.size(), files[i].flags, &hostMd, host);
        (void)LoadFromPNGMemoryRaw(source, data.size(), files[i].flags, &rawMd, raw);
        Window window(dev);
        TexMetadata md;
        const HRESULT hr = LoadFromPNGMemory(dev, source, data.size(), files[i].flags, &md, image);
        const unsigned launches = window.end({ "png_" })[0].launches;
        if (FAILED(hr)) { std::printf("%zu %08x %08x %s\n", i, unsigned(hr), unsigned(hostHr), released(image) ? "released" : "held"); continue; }
        ScratchImage back;
        if (FAILED(image.Download(back))) { std::fprintf(stderr, "%s: download failed\n", files[i].path.c_str()); return 1; }
        const bool metaEqual = SUCCEEDED(hostHr) && same_metadata(md, hostMd);
        const bool pixelsEqual = SUCCEEDED(hostHr) && back.GetPixelsSize() == host.GetPixelsSize() && !std::memcmp(back.GetPixels(), host.GetPixels(), host.GetPixelsSize());
        std::printf("%zu %08x %08x ok %zu %zu %u %zu %llu %llu %d %d %u\n", i, unsigned(hr), unsigned(hostHr), md.width, md.height, unsigned(md.format), raw.rowsBytes,
                    (unsigned long long)window.up, (unsigned long long)window.down, int(metaEqual), int(pixelsEqual), launches);
    }
    return 0;
}

static int device_save(char** a)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    std::vector<uint8_t> px; Image src;
    if (!image_arg(a, px, src)) return 1;
    const PNG_FLAGS flags = PNG_FLAGS(std::strtoul(a[5], nullptr, 0));
    TexMetadata md;
    md.width = src.width; md.height = src.height; md.depth = md.arraySize = md.mipLevels = 1; md.format = src.format; md.dimension = TEX_DIMENSION_TEXTURE2D;
    DeviceScratchImage image;
    HRESULT hr = image.Upload(dev, &src, 1, md);
    if (FAILED(hr)) { std::printf("upload %08x\n", unsigned(hr)); return 1; }
    Window window(dev);
    hr = SaveToPNGFile(dev, *image.GetImage(0, 0, 0), flags, a[6]);
    window.end();
    const std::string hostOut = std::string(a[6]) + ".host";
    const HRESULT hostHr = SaveToPNGFile(src, flags, hostOut.c_str());
    std::printf("hr %08x %08x %llu %llu\n", unsigned(hr), unsigned(hostHr), (unsigned long long)window.up, (unsigned long long)window.down);
    return 0;
}

static int time_raw(const char* file, int runs)
{
    std::vector<uint8_t> data;
    if (!read_file(file, data)) return 1;
    for (int i = -1; i < runs; ++i)
    {
        PNGRawImage raw; HRESULT hr = S_OK;
        const double ms = timed_ms([&] { hr = LoadFromPNGMemoryRaw(data.data(), data.size(), PNG_FLAGS_NONE, nullptr, raw); });
        if (FAILED(hr)) return 1;
        if (i >= 0) std::printf("run %d raw %.3f ms file %zu rows %zu\n", i, ms, data.size(), raw.rowsBytes);
    }
    return 0;
}

// a file through the resident loader and through the host loader plus Upload, alternating, `runs` times each after one unmeasured run each;
// a resident image through the resident saver and through Download plus the host saver likewise
static int time_paths(const char* file, int runs, bool save)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    std::vector<uint8_t> data;
    if (!read_file(file, data)) return 1;
    DeviceScratchImage resident;
    TexMetadata md;
    if (FAILED(LoadFromPNGMemory(dev, data.data(), data.size(), PNG_FLAGS_NONE, &md, resident))) return 1;
    bool ok = true;
    if (save)
    {
        const Image& img = *resident.GetImage(0, 0, 0);
        return time_runs(dev, runs,
            [&] { return timed_ms([&] { Blob blob; ok = ok && SUCCEEDED(SaveToPNGMemory(dev, img, PNG_FLAGS_NONE, blob)); }); },
            [&] { return timed_ms([&] { Blob blob; ScratchImage host; ok = ok && SUCCEEDED(resident.Download(host)) && SUCCEEDED(SaveToPNGMemory(*host.GetImage(0, 0, 0), PNG_FLAGS_NONE, blob)); }); },
            [&](std::string&) { return ok; });
    }
    return time_runs(dev, runs,
        [&] { return timed_ms([&] { DeviceScratchImage image; ok = ok && SUCCEEDED(LoadFromPNGMemory(dev, data.data(), data.size(), PNG_FLAGS_NONE, nullptr, image)) && dxtex_ctx_synchronize(dev.Get()) == 0; }); },
        [&] { return timed_ms([&] { ScratchImage host; DeviceScratchImage image;
                                    ok = ok && SUCCEEDED(LoadFromPNGMemory(data.data(), data.size(), PNG_FLAGS_NONE, nullptr, host)) && SUCCEEDED(image.Upload(dev, host)) && dxtex_ctx_synchronize(dev.Get()) == 0; }); },
        [&](std::string&) { return ok; });
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "time_raw")) return time_raw(argv[2], std::atoi(argv[3]));
    if (argc == 4 && !std::strcmp(argv[1], "time_load")) return time_paths(argv[2], std::atoi(argv[3]), false);
    if (argc == 4 && !std::strcmp(argv[1], "time_save")) return time_paths(argv[2], std::atoi(argv[3]), true);
    if (argc == 3 && !std::strcmp(argv[1], "load_many")) return load_many(argv[2]);
    if (argc == 9 && !std::strcmp(argv[1], "save")) return save(argv + 2);
    if (argc == 3 && !std::strcmp(argv[1], "errors")) return errors(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "device_load_many")) return device_load_many(argv[2]);
    if (argc == 9 && !std::strcmp(argv[1], "device_save")) return device_save(argv + 2);
    std::fprintf(stderr, "usage: png_host_test time_raw|time_load|time_save <file> <runs> | load_many <list> | save <in.bin> <w> <h> <format> <rowPitch> <flags> <out> | errors <file> | device_load_many <list> | device_save <in.bin> <w> <h> <format> <rowPitch> <flags> <out>\n");
    return 2;
}
