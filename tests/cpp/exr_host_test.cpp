// The OpenEXR codec through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_exr_cpu.py (the first four commands,
// which need no device; also built with sanitizers as exr_host_test_asan) and tests/test_exr_host_gpu.py (the device_ ones).
//
//   exr_host_test load_many <list>
//       <list> holds one file path per line. Each file goes through LoadFromEXRMemoryRaw, the host LoadFromEXRMemory and
//       GetMetadataFromEXRMemory; one line per file: "<index> <raw hresult hex> <host hresult hex> <metadata hresult hex>" and, where it
//       loaded, " ok <width> <height> <format> <depth> <arraySize> <mipLevels> <miscFlags> <miscFlags2> <dimension> <compression>
//       <scanlineBytes> <chunk descriptors> <coded descriptors> <stream bytes> <offset R> <type R> ... <offset A> <type A>", with the
//       image's tight rows, item after item, in <path>.out
//   exr_host_test fuzz <file> <seed> <cases>
//       <cases> copies of the file with one to four bytes changed each (a seeded generator) through the Raw loader and the host loader;
//       prints "fuzz <loaded> <refused>". Every truncation: exr_host_test truncations <file> likewise over every prefix of the file.
//   exr_host_test files <file>
//       the File forms on a path: prints "load_file <hresult hex>", "metadata_file <hresult hex>" and "raw_file <hresult hex>"
//   exr_host_test save <in.bin> <width> <height> <format> <rowPitch> <out>
//       SaveToEXRMemory of the pixels -> <out>; prints "hr <hresult hex>"
//   exr_host_test device_load_many <list>
//       the same list through the host loader and through its resident form; one line per file: "<index> <resident hresult hex> <host
//       hresult hex>", then " ok <width> <height> <arraySize> <stream bytes> <bytes host -> device> <bytes device -> host> <metadata equal>
//       <pixels equal> <exr_undo launches> <exr_texels launches>", or " released" / " held" for whether a failure left the result empty
//   exr_host_test device_save <in.bin> <width> <height> <format> <rowPitch> <out>
//       the image goes up, the resident saver writes <out> and the host one <out>.host from the same pixels; prints "hr <resident hresult
//       hex> <host hresult hex> <bytes host -> device> <bytes device -> host> <exr_pack launches>" counted around the resident save alone
//   exr_host_test time_load <file> <runs> | time_save <file> <runs>
//       for tools/exr_bench.py: wall time and bytes moved of the resident path beside the same build's host path, one line per run; time_load
//       also prints the Raw loader's time alone ("raw") and the host's serial undo of the same stream ("undo")
#include "codec_host_test.h"

// both loaders on one buffer; what a failure must leave behind is checked here
static bool load_both(const uint8_t* p, size_t n, EXRRawImage& raw, ScratchImage& image, TexMetadata& rawMd, TexMetadata& md, HRESULT& rawHr, HRESULT& hr, const char* what)
{
    rawHr = LoadFromEXRMemoryRaw(p, n, &rawMd, raw);
    hr = LoadFromEXRMemory(p, n, &md, image);
    if (FAILED(rawHr) && (raw.stream || raw.chunks || raw.storage.GetBufferPointer())) { std::fprintf(stderr, "%s: the raw image was not released\n", what); return false; }
    if (FAILED(hr) && (image.GetImageCount() || image.GetPixels())) { std::fprintf(stderr, "%s: the image was not released\n", what); return false; }
    if (rawHr != hr) { std::fprintf(stderr, "%s: the loaders disagree (%08x, %08x)\n", what, unsigned(rawHr), unsigned(hr)); return false; }
    return true;
}

static int load_many(const char* list)
{
    const std::vector<std::string> files = read_lines(list);
    std::vector<uint8_t> data;
    EXRRawImage raw; ScratchImage image;          // one object each for every file: a failure must leave it empty whatever it held before
    for (size_t i = 0; i < files.size(); ++i)
    {
        if (!read_file(files[i], data)) { std::fprintf(stderr, "cannot read %s\n", files[i].c_str()); return 1; }
        const Exact exact(data.data(), data.size());
        TexMetadata rawMd, md, infoMd;
        HRESULT rawHr, hr;
        if (!load_both(exact.p, exact.n, raw, image, rawMd, md, rawHr, hr, files[i].c_str())) return 1;
        const HRESULT infoHr = GetMetadataFromEXRMemory(exact.p, exact.n, infoMd);
        if (FAILED(hr)) { std::printf("%zu %08x %08x %08x\n", i, unsigned(rawHr), unsigned(hr), unsigned(infoHr)); continue; }
        if (FAILED(infoHr) || !same_metadata(rawMd, md) || !same_metadata(md, image.GetMetadata()) || !same_metadata(md, infoMd)) { std::fprintf(stderr, "%s: the metadata differ\n", files[i].c_str()); return 1; }
        size_t rp = 0, sp = 0;
        if (FAILED(ComputePitch(md.format, md.width, md.height, rp, sp))) return 1;
        std::vector<uint8_t> tight(rp * md.height * md.arraySize);
        for (size_t item = 0; item < md.arraySize; ++item)
        {
            const Image* img = image.GetImage(0, item, 0);
            if (!img) return 1;
            for (size_t y = 0; y < md.height; ++y) std::memcpy(tight.data() + (item * md.height + y) * rp, img->pixels + y * img->rowPitch, rp);
        }
        if (!write_file(files[i] + ".out", tight.data(), tight.size())) return 1;
        size_t coded = 0;
        for (size_t c = 0; c < raw.chunkCount; ++c) coded += raw.chunks[c].coded;
        std::printf("%zu %08x %08x %08x ok %zu %zu %u %zu %zu %zu %u %u %u %u %u %zu %zu %zu", i, unsigned(rawHr), unsigned(hr), unsigned(infoHr), md.width, md.height, unsigned(md.format),
                    md.depth, md.arraySize, md.mipLevels, unsigned(md.miscFlags), unsigned(md.miscFlags2), unsigned(md.dimension), raw.compression, raw.scanlineBytes, raw.chunkCount,
                    coded, raw.streamBytes);
        for (int k = 0; k < 4; ++k) std::printf(" %u %u", raw.channel[k].offset, raw.channel[k].type);
        std::printf("\n");
    }
    return 0;
}

static int damaged(const char* file, bool truncations, uint64_t seed, size_t cases)
{
    EXRRawImage raw; ScratchImage image;
    return damaged_copies(file, truncations, seed, cases, [&](const uint8_t* p, size_t n, HRESULT& hr)
    {
        TexMetadata rawMd, md; HRESULT rawHr;
        return load_both(p, n, raw, image, rawMd, md, rawHr, hr, "a damaged copy");
    });
}

static int files(const char* file)
{
    TexMetadata md; ScratchImage image; EXRRawImage raw;
    std::printf("load_file %08x\n", unsigned(LoadFromEXRFile(file, &md, image)));
    std::printf("metadata_file %08x\n", unsigned(GetMetadataFromEXRFile(file, md)));
    std::printf("raw_file %08x\n", unsigned(LoadFromEXRFileRaw(file, &md, raw)));
    Blob blob;
    std::printf("load_null %08x\n", unsigned(LoadFromEXRMemory(nullptr, 0, &md, image)));
    std::printf("metadata_null %08x\n", unsigned(GetMetadataFromEXRMemory(nullptr, 0, md)));
    std::printf("raw_null %08x\n", unsigned(LoadFromEXRMemoryRaw(nullptr, 0, &md, raw)));
    std::printf("load_file_null %08x\n", unsigned(LoadFromEXRFile(nullptr, &md, image)));
    std::printf("save_file_null %08x\n", unsigned(SaveToEXRFile(Image(), nullptr)));
    std::printf("save_null %08x\n", unsigned(SaveToEXRMemory(Image(), blob)));
    return 0;
}

static int save(char** a)
{
    std::vector<uint8_t> px; Image src;
    if (!image_arg(a, px, src)) return 1;
    Blob blob;
    const HRESULT hr = SaveToEXRMemory(src, blob);
    if (FAILED(hr) && blob.GetBufferPointer()) { std::fprintf(stderr, "the blob was not released\n"); return 1; }
    if (SUCCEEDED(hr) && !write_file(a[5], blob.GetBufferPointer(), blob.GetBufferSize())) return 1;
    std::printf("hr %08x\n", unsigned(hr));
    return 0;
}

static int device_load_many(const char* list)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    const std::vector<std::string> files = read_lines(list);
    std::vector<uint8_t> data;
    DeviceScratchImage image;
    for (size_t i = 0; i < files.size(); ++i)
    {
        if (!read_file(files[i], data)) { std::fprintf(stderr, "cannot read %s\n", files[i].c_str()); return 1; }
        TexMetadata hostMd, rawMd; ScratchImage host; EXRRawImage raw;
        const uint8_t none = 0;
        const uint8_t* source = data.empty() ? &none : data.data();          // an empty file is a size of zero, not a null pointer
        const HRESULT hostHr = LoadFromEXRMemory(source, data.size(), &hostMd, host);
        (void)LoadFromEXRMemoryRaw(source, data.size(), &rawMd, raw);
        Window window(dev);
        TexMetadata md;
        const HRESULT hr = LoadFromEXRMemory(dev, source, data.size(), &md, image);
        const std::vector<Window::Mark> marks = window.end({ "exr_undo", "exr_texels" });
        if (FAILED(hr)) { std::printf("%zu %08x %08x %s\n", i, unsigned(hr), unsigned(hostHr), released(image) ? "released" : "held"); continue; }
        ScratchImage back;
        if (FAILED(image.Download(back))) { std::fprintf(stderr, "%s: download failed\n", files[i].c_str()); return 1; }
        const bool metaEqual = SUCCEEDED(hostHr) && same_metadata(md, hostMd) && same_metadata(image.GetMetadata(), host.GetMetadata());
        const bool pixelsEqual = SUCCEEDED(hostHr) && back.GetPixelsSize() == host.GetPixelsSize() && !std::memcmp(back.GetPixels(), host.GetPixels(), host.GetPixelsSize());
        std::printf("%zu %08x %08x ok %zu %zu %zu %zu %llu %llu %d %d %u %u\n", i, unsigned(hr), unsigned(hostHr), md.width, md.height, md.arraySize, raw.streamBytes,
                    (unsigned long long)window.up, (unsigned long long)window.down, int(metaEqual), int(pixelsEqual), marks[0].launches, marks[1].launches);
    }
    return 0;
}

static int device_save(char** a)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    std::vector<uint8_t> px; Image src;
    if (!image_arg(a, px, src)) return 1;
    TexMetadata md;
    md.width = src.width; md.height = src.height; md.depth = md.arraySize = md.mipLevels = 1; md.format = src.format; md.dimension = TEX_DIMENSION_TEXTURE2D;
    DeviceScratchImage image;
    HRESULT hr = image.Upload(dev, &src, 1, md);
    if (FAILED(hr)) { std::printf("upload %08x\n", unsigned(hr)); return 1; }
    Window window(dev);
    hr = SaveToEXRFile(dev, *image.GetImage(0, 0, 0), a[5]);
    const std::vector<Window::Mark> marks = window.end({ "exr_pack" });
    const std::string hostOut = std::string(a[5]) + ".host";
    const HRESULT hostHr = SaveToEXRFile(src, hostOut.c_str());
    std::printf("hr %08x %08x %llu %llu %u\n", unsigned(hr), unsigned(hostHr), (unsigned long long)window.up, (unsigned long long)window.down, marks[0].launches);
    return 0;
}

// tools/exr_bench.py: a file through the resident loader and through the host loader plus Upload, alternating, `runs` times each after one
// unmeasured run each; a resident image through the resident saver and through Download plus the host saver likewise
static int time_paths(const char* file, int runs, bool save)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    std::vector<uint8_t> data;
    if (!read_file(file, data)) return 1;
    DeviceScratchImage resident;
    TexMetadata md;
    if (FAILED(LoadFromEXRMemory(dev, data.data(), data.size(), &md, resident))) return 1;
    bool ok = true;
    if (save)
    {
        const Image& img = *resident.GetImage(0, 0, 0);
        return time_runs(dev, runs,
            [&] { return timed_ms([&] { Blob blob; ok = ok && SUCCEEDED(SaveToEXRMemory(dev, img, blob)); }); },
            [&] { return timed_ms([&] { Blob blob; ScratchImage host; ok = ok && SUCCEEDED(resident.Download(host)) && SUCCEEDED(SaveToEXRMemory(*host.GetImage(0, 0, 0), blob)); }); },
            [&](std::string& extra) { extra = " raw 0.000 ms undo 0.000 ms"; return ok; });
    }
    return time_runs(dev, runs,
        [&] { return timed_ms([&] { DeviceScratchImage image; ok = ok && SUCCEEDED(LoadFromEXRMemory(dev, data.data(), data.size(), nullptr, image)) && dxtex_ctx_synchronize(dev.Get()) == 0; }); },
        [&] { return timed_ms([&] { ScratchImage host; DeviceScratchImage image;
                                    ok = ok && SUCCEEDED(LoadFromEXRMemory(data.data(), data.size(), nullptr, host)) && SUCCEEDED(image.Upload(dev, host)) && dxtex_ctx_synchronize(dev.Get()) == 0; }); },
        [&](std::string& extra)
        {
            EXRRawImage raw;
            const double rawMs = timed_ms([&] { ok = ok && SUCCEEDED(LoadFromEXRMemoryRaw(data.data(), data.size(), nullptr, raw)); });
            if (!ok) return false;
            // the host's serial undo of the same stream: the delta of every coded chunk, one byte after another
            const double undoMs = timed_ms([&]
            {
                uint8_t* s = raw.storage.GetBufferPointer();
                for (size_t c = 0; c < raw.chunkCount; ++c)
                    if (raw.chunks[c].coded) { uint8_t* t = s + raw.chunks[c].offset; for (size_t k = 1; k < raw.chunks[c].bytes; ++k) t[k] = uint8_t(t[k - 1] + t[k] - 128); }
            });
            char text[64];
            std::snprintf(text, sizeof(text), " raw %.3f ms undo %.3f ms", rawMs, undoMs);
            extra = text;
            return true;
        });
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "time_load")) return time_paths(argv[2], std::atoi(argv[3]), false);
    if (argc == 4 && !std::strcmp(argv[1], "time_save")) return time_paths(argv[2], std::atoi(argv[3]), true);
    if (argc == 3 && !std::strcmp(argv[1], "load_many")) return load_many(argv[2]);
    if (argc == 5 && !std::strcmp(argv[1], "fuzz")) return damaged(argv[2], false, std::strtoull(argv[3], nullptr, 0), size_t(std::atoll(argv[4])));
    if (argc == 3 && !std::strcmp(argv[1], "truncations")) return damaged(argv[2], true, 0, 0);
    if (argc == 3 && !std::strcmp(argv[1], "files")) return files(argv[2]);
    if (argc == 8 && !std::strcmp(argv[1], "save")) return save(argv + 2);
    if (argc == 3 && !std::strcmp(argv[1], "device_load_many")) return device_load_many(argv[2]);
    if (argc == 8 && !std::strcmp(argv[1], "device_save")) return device_save(argv + 2);
    std::fprintf(stderr, "usage: exr_host_test load_many <list> | fuzz <file> <seed> <cases> | truncations <file> | files <file> | save <in.bin> <w> <h> <format> <rowPitch> <out> | "
                         "device_load_many <list> | device_save <in.bin> <w> <h> <format> <rowPitch> <out> | time_load <file> <runs> | time_save <file> <runs>\n");
    return 2;
}
