// The JPEG reader through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_jpeg_cpu.py (the first two commands, which
// need no device; also built with sanitizers as jpeg_host_test_asan) and tests/test_jpeg_host_gpu.py (the third).
//
//   jpeg_host_test load_many <list>
//       <list> holds one "<JPEG_FLAGS> <file path>" per line. Each file goes through LoadFromJPEGMemoryRaw, the host LoadFromJPEGMemory and
//       GetMetadataFromJPEGMemory; one line per file: "<index> <raw hresult hex> <host hresult hex> <metadata hresult hex>" and, where it
//       loaded, " ok <width> <height> <format> <depth> <arraySize> <mipLevels> <miscFlags> <miscFlags2> <dimension> <colour> <components>
//       <coefficient count> <offset> <bytes>" and per component " <h> <v> <quant> <blocksPerRow> <blockRows> <offset>". <list>.out holds, at
//       <offset>, the image's tight rows (<bytes>), then the coefficients (2 bytes each), then the four quantiser tables (512 bytes)
//   jpeg_host_test errors <file>
//       the null-argument and missing-file answers; prints one "name hresult" per line
//   jpeg_host_test device_load_many <list>
//       the same list through the host loader and through its resident form; one line per file: "<index> <resident hresult hex> <host
//       hresult hex>", then " ok <width> <height> <format> <coefficient bytes> <bytes host -> device> <bytes device -> host> <metadata equal>
//       <pixels equal> <jpeg kernel launches>", or " released" / " held" for whether a failure left the result empty
//   jpeg_host_test time_raw <file> <runs> | time_load <file> <runs>
//       for tools/jpeg_bench.py: the byte-serial half alone (no device); wall time and bytes moved of the resident path beside the same
//       build's host path plus Upload, one line per run
#include "codec_host_test.h"

struct Line { JPEG_FLAGS flags; std::string path; };
static std::vector<Line> read_list(const char* path)
{
    std::vector<Line> lines;
    for (const std::string& line : read_lines(path))
    {
        const size_t sp = line.find(' ');
        if (sp != std::string::npos) lines.push_back({ JPEG_FLAGS(std::strtoul(line.substr(0, sp).c_str(), nullptr, 0)), line.substr(sp + 1) });
    }
    return lines;
}

static int load_many(const char* list)
{
    const std::vector<Line> files = read_list(list);
    std::vector<uint8_t> data;
    JPEGRawImage raw; ScratchImage image;          // one object each for every file: a failure must leave it empty whatever it held before
    FILE* out = std::fopen((std::string(list) + ".out").c_str(), "wb");
    if (!out) return 1;
    size_t offset = 0;
    for (size_t i = 0; i < files.size(); ++i)
    {
        const std::string& path = files[i].path;
        if (!read_file(path, data)) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); return 1; }
        const Exact exact(data.data(), data.size());
        TexMetadata rawMd, md, only;
        const HRESULT rawHr = LoadFromJPEGMemoryRaw(exact.p, exact.n, files[i].flags, &rawMd, raw);
        const HRESULT hr = LoadFromJPEGMemory(exact.p, exact.n, files[i].flags, &md, image);
        const HRESULT metaHr = GetMetadataFromJPEGMemory(exact.p, exact.n, files[i].flags, only);
        if (FAILED(rawHr) && (raw.coefficients || raw.storage.GetBufferPointer() || raw.width)) { std::fprintf(stderr, "%s: the raw image was not released\n", path.c_str()); return 1; }
        if (FAILED(hr) && (image.GetImageCount() || image.GetPixels())) { std::fprintf(stderr, "%s: the image was not released\n", path.c_str()); return 1; }
        if (FAILED(rawHr) || FAILED(hr)) { std::printf("%zu %08x %08x %08x\n", i, unsigned(rawHr), unsigned(hr), unsigned(metaHr)); continue; }
        if (FAILED(metaHr) || !same_metadata(rawMd, md) || !same_metadata(md, only)) { std::fprintf(stderr, "%s: the metadata differ\n", path.c_str()); return 1; }
        if (raw.coefficients != reinterpret_cast<const int16_t*>(raw.storage.GetBufferPointer()) || raw.storage.GetBufferSize() != raw.coefficientCount * 2)
        { std::fprintf(stderr, "%s: the coefficients are not the storage\n", path.c_str()); return 1; }
        const Image* img = image.GetImage(0, 0, 0);
        size_t rp = 0, sp = 0;
        if (!img || FAILED(ComputePitch(md.format, md.width, md.height, rp, sp))) return 1;
        for (size_t y = 0; y < md.height; ++y) if (std::fwrite(img->pixels + y * img->rowPitch, 1, rp, out) != rp) return 1;
        if (std::fwrite(raw.coefficients, 2, raw.coefficientCount, out) != raw.coefficientCount || std::fwrite(raw.quant, 1, sizeof(raw.quant), out) != sizeof(raw.quant)) return 1;
        std::printf("%zu %08x %08x %08x ok %zu %zu %u %zu %zu %zu %u %u %u %u %u %zu %zu %zu", i, unsigned(rawHr), unsigned(hr), unsigned(metaHr), md.width, md.height,
                    unsigned(md.format), md.depth, md.arraySize, md.mipLevels, unsigned(md.miscFlags), unsigned(md.miscFlags2), unsigned(md.dimension), raw.colour, raw.components,
                    raw.coefficientCount, offset, rp * md.height);
        for (uint32_t c = 0; c < raw.components; ++c)
            std::printf(" %u %u %u %u %u %zu", raw.component[c].h, raw.component[c].v, raw.component[c].quant, raw.component[c].blocksPerRow, raw.component[c].blockRows, raw.component[c].offset);
        std::printf("\n");
        offset += rp * md.height + raw.coefficientCount * 2 + sizeof(raw.quant);
    }
    return std::fclose(out) == 0 ? 0 : 1;
}

static int errors(const char* file)
{
    TexMetadata md; ScratchImage image; JPEGRawImage raw;
    const std::string missing = std::string(file) + ".is-not-there";
    std::printf("metadata_null %08x\n", unsigned(GetMetadataFromJPEGFile(nullptr, JPEG_FLAGS_NONE, md)));
    std::printf("load_null %08x\n", unsigned(LoadFromJPEGFile(nullptr, JPEG_FLAGS_NONE, &md, image)));
    std::printf("raw_null %08x\n", unsigned(LoadFromJPEGFileRaw(nullptr, JPEG_FLAGS_NONE, &md, raw)));
    std::printf("memory_null %08x\n", unsigned(LoadFromJPEGMemory(nullptr, 64, JPEG_FLAGS_NONE, &md, image)));
    std::printf("memory_raw_null %08x\n", unsigned(LoadFromJPEGMemoryRaw(nullptr, 64, JPEG_FLAGS_NONE, &md, raw)));
    std::printf("memory_metadata_null %08x\n", unsigned(GetMetadataFromJPEGMemory(nullptr, 64, JPEG_FLAGS_NONE, md)));
    std::printf("metadata_missing %08x\n", unsigned(GetMetadataFromJPEGFile(missing.c_str(), JPEG_FLAGS_NONE, md)));
    std::printf("load_missing %08x\n", unsigned(LoadFromJPEGFile(missing.c_str(), JPEG_FLAGS_NONE, &md, image)));
    std::printf("raw_missing %08x\n", unsigned(LoadFromJPEGFileRaw(missing.c_str(), JPEG_FLAGS_NONE, &md, raw)));
    std::printf("load_file %08x\n", unsigned(LoadFromJPEGFile(file, JPEG_FLAGS_NONE, &md, image)));
    std::printf("metadata_file %08x\n", unsigned(GetMetadataFromJPEGFile(file, JPEG_FLAGS_NONE, md)));
    std::printf("raw_file %08x\n", unsigned(LoadFromJPEGFileRaw(file, JPEG_FLAGS_NONE, &md, raw)));
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
        TexMetadata hostMd, rawMd; ScratchImage host; JPEGRawImage raw;
        const uint8_t none = 0;
        const uint8_t* source = data.empty() ? &none : data.data();          // an empty file is a size of zero, not a null pointer
        const HRESULT hostHr = LoadFromJPEGMemory(source, data.size(), files[i].flags, &hostMd, host);
        (void)LoadFromJPEGMemoryRaw(source, data.size(), files[i].flags, &rawMd, raw);
        Window window(dev);
        TexMetadata md;
        const HRESULT hr = LoadFromJPEGMemory(dev, source, data.size(), files[i].flags, &md, image);
        const unsigned launches = window.end({ "jpeg_" })[0].launches;
        if (FAILED(hr)) { std::printf("%zu %08x %08x %s\n", i, unsigned(hr), unsigned(hostHr), released(image) ? "released" : "held"); continue; }
        ScratchImage back;
        if (FAILED(image.Download(back))) { std::fprintf(stderr, "%s: download failed\n", files[i].path.c_str()); return 1; }
        const bool metaEqual = SUCCEEDED(hostHr) && same_metadata(md, hostMd);
        const bool pixelsEqual = SUCCEEDED(hostHr) && back.GetPixelsSize() == host.GetPixelsSize() && !std::memcmp(back.GetPixels(), host.GetPixels(), host.GetPixelsSize());
        std::printf("%zu %08x %08x ok %zu %zu %u %zu %llu %llu %d %d %u\n", i, unsigned(hr), unsigned(hostHr), md.width, md.height, unsigned(md.format), raw.coefficientCount * 2,
                    (unsigned long long)window.up, (unsigned long long)window.down, int(metaEqual), int(pixelsEqual), launches);
    }
    return 0;
}

static int time_raw(const char* file, int runs)
{
    std::vector<uint8_t> data;
    if (!read_file(file, data)) return 1;
    for (int i = -1; i < runs; ++i)
    {
        JPEGRawImage raw; HRESULT hr = S_OK;
        const double ms = timed_ms([&] { hr = LoadFromJPEGMemoryRaw(data.data(), data.size(), JPEG_FLAGS_NONE, nullptr, raw); });
        if (FAILED(hr)) return 1;
        if (i >= 0) std::printf("run %d raw %.3f ms file %zu coefficients %zu\n", i, ms, data.size(), raw.coefficientCount * 2);
    }
    return 0;
}

// a file through the resident loader and through the host loader plus Upload, alternating, `runs` times each after one unmeasured run each
static int time_load(const char* file, int runs)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    std::vector<uint8_t> data;
    if (!read_file(file, data)) return 1;
    bool ok = true;
    return time_runs(dev, runs,
        [&] { return timed_ms([&] { DeviceScratchImage image; ok = ok && SUCCEEDED(LoadFromJPEGMemory(dev, data.data(), data.size(), JPEG_FLAGS_NONE, nullptr, image)) && dxtex_ctx_synchronize(dev.Get()) == 0; }); },
        [&] { return timed_ms([&] { ScratchImage host; DeviceScratchImage image;
                                    ok = ok && SUCCEEDED(LoadFromJPEGMemory(data.data(), data.size(), JPEG_FLAGS_NONE, nullptr, host)) && SUCCEEDED(image.Upload(dev, host)) && dxtex_ctx_synchronize(dev.Get()) == 0; }); },
        [&](std::string&) { return ok; });
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "time_raw")) return time_raw(argv[2], std::atoi(argv[3]));
    if (argc == 4 && !std::strcmp(argv[1], "time_load")) return time_load(argv[2], std::atoi(argv[3]));
    if (argc == 3 && !std::strcmp(argv[1], "load_many")) return load_many(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "errors")) return errors(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "device_load_many")) return device_load_many(argv[2]);
    std::fprintf(stderr, "usage: jpeg_host_test time_raw|time_load <file> <runs> | load_many <list> | errors <file> | device_load_many <list>\n");
    return 2;
}
