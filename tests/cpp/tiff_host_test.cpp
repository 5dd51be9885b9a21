// The TIFF codec through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_tiff_cpu.py (the first five commands,
// which need no device; also built with sanitizers as tiff_host_test_asan) and tests/test_tiff_host_gpu.py (the device_ ones).
//
//   tiff_host_test load_many <list> <flags>
//       <list> holds one file path per line. Each file goes through LoadFromTIFFMemoryRaw, the host LoadFromTIFFMemory and
//       GetMetadataFromTIFFMemory with TIFF_FLAGS <flags>; one line per file: "<index> <raw hresult hex> <host hresult hex> <metadata
//       hresult hex>" and, where it loaded, " ok <width> <height> <format> <miscFlags2> <compression> <kind> <predictor> <bigEndian>
//       <planar> <whiteIsZero> <opaque> <segment descriptors> <stream bytes>", with the image's tight rows in <path>.out
//   tiff_host_test fuzz <file> <seed> <cases>
//       <cases> copies of the file with one to four bytes changed each (a seeded generator) through the Raw loader and the host loader;
//       prints "fuzz <loaded> <refused>". Every truncation: tiff_host_test truncations <file> likewise over every prefix of the file.
//   tiff_host_test files <file>
//       the File forms on a path and the null arguments: one "<name> <hresult hex>" a line
//   tiff_host_test save <in.bin> <width> <height> <format> <rowPitch> <flags> <out>
//       SaveToTIFFMemory of the pixels -> <out>; prints "hr <hresult hex>"
//   tiff_host_test device_load_many <list> <flags>
//       the same list through the host loader and through its resident form; one line per file: "<index> <resident hresult hex> <host
//       hresult hex>", then " ok <width> <height> <stream bytes> <bytes host -> device> <bytes device -> host> <metadata equal> <pixels
//       equal> <tiff_undo launches> <tiff_texels launches>", or " released" / " held" for whether a failure left the result empty
//   tiff_host_test device_save <in.bin> <width> <height> <format> <rowPitch> <flags> <out>
//       the image goes up, the resident saver writes <out> and the host one <out>.host from the same pixels; prints "hr <resident hresult
//       hex> <host hresult hex> <bytes host -> device> <bytes device -> host> <tiff_pack launches>" counted around the resident save alone
//   tiff_host_test time_load <file> <runs>
//       for tools/tiff_bench.py: wall time and bytes moved of the resident load beside the same build's host load plus Upload, one line per
//       run, with the Raw loader's time alone ("raw"), the host's serial undo of the same stream ("undo") and the device's kernels ("undo_gpu",
//       "texels_gpu", from the context's profile)
#include "codec_host_test.h"
#include "../../directxtex_amd/csrc/dxtex_tiff.h"

// both loaders on one buffer; what a failure must leave behind is checked here
static bool load_both(const uint8_t* p, size_t n, TIFF_FLAGS flags, TIFFRawImage& raw, ScratchImage& image, TexMetadata& rawMd, TexMetadata& md, HRESULT& rawHr, HRESULT& hr, const char* what)
{
    rawHr = LoadFromTIFFMemoryRaw(p, n, flags, &rawMd, raw);
    hr = LoadFromTIFFMemory(p, n, flags, &md, image);
    if (FAILED(rawHr) && (raw.stream || raw.segments || raw.storage.GetBufferPointer())) { std::fprintf(stderr, "%s: the raw image was not released\n", what); return false; }
    if (FAILED(hr) && (image.GetImageCount() || image.GetPixels())) { std::fprintf(stderr, "%s: the image was not released\n", what); return false; }
    if (rawHr != hr) { std::fprintf(stderr, "%s: the loaders disagree (%08x, %08x)\n", what, unsigned(rawHr), unsigned(hr)); return false; }
    return true;
}

static int load_many(const char* list, TIFF_FLAGS flags)
{
    const std::vector<std::string> files = read_lines(list);
    std::vector<uint8_t> data;
    TIFFRawImage raw; ScratchImage image;          // one object each for every file: a failure must leave it empty whatever it held before
    for (size_t i = 0; i < files.size(); ++i)
    {
        if (!read_file(files[i], data)) { std::fprintf(stderr, "cannot read %s\n", files[i].c_str()); return 1; }
        const Exact exact(data.data(), data.size());
        TexMetadata rawMd, md, infoMd;
        HRESULT rawHr, hr;
        if (!load_both(exact.p, exact.n, flags, raw, image, rawMd, md, rawHr, hr, files[i].c_str())) return 1;
        const HRESULT infoHr = GetMetadataFromTIFFMemory(exact.p, exact.n, flags, infoMd);
        if (FAILED(hr)) { std::printf("%zu %08x %08x %08x\n", i, unsigned(rawHr), unsigned(hr), unsigned(infoHr)); continue; }
        if (FAILED(infoHr) || !same_metadata(rawMd, md) || !same_metadata(md, image.GetMetadata()) || !same_metadata(md, infoMd)) { std::fprintf(stderr, "%s: the metadata differ\n", files[i].c_str()); return 1; }
        size_t rp = 0, sp = 0;
        if (FAILED(ComputePitch(md.format, md.width, md.height, rp, sp))) return 1;
        std::vector<uint8_t> tight(rp * md.height);
        const Image* img = image.GetImage(0, 0, 0);
        if (!img) return 1;
        for (size_t y = 0; y < md.height; ++y) std::memcpy(tight.data() + y * rp, img->pixels + y * img->rowPitch, rp);
        if (!write_file(files[i] + ".out", tight.data(), tight.size())) return 1;
        const TIFFRawImage::Layout& l = raw.layout;
        std::printf("%zu %08x %08x %08x ok %zu %zu %u %u %u %u %u %u %u %u %u %zu %zu\n", i, unsigned(rawHr), unsigned(hr), unsigned(infoHr), md.width, md.height, unsigned(md.format),
                    unsigned(md.miscFlags2), raw.compression, l.kind, l.predictor, l.bigEndian, l.planar, l.whiteIsZero, l.opaque, raw.segmentCount, raw.streamBytes);
    }
    return 0;
}

static int damaged(const char* file, bool truncations, uint64_t seed, size_t cases)
{
    TIFFRawImage raw; ScratchImage image;
    return damaged_copies(file, truncations, seed, cases, [&](const uint8_t* p, size_t n, HRESULT& hr)
    {
        TexMetadata rawMd, md; HRESULT rawHr;
        return load_both(p, n, TIFF_FLAGS_NONE, raw, image, rawMd, md, rawHr, hr, "a damaged copy");
    });
}

static int files(const char* file)
{
    TexMetadata md; ScratchImage image; TIFFRawImage raw;
    std::printf("load_file %08x\n", unsigned(LoadFromTIFFFile(file, TIFF_FLAGS_NONE, &md, image)));
    std::printf("metadata_file %08x\n", unsigned(GetMetadataFromTIFFFile(file, TIFF_FLAGS_NONE, md)));
    std::printf("raw_file %08x\n", unsigned(LoadFromTIFFFileRaw(file, TIFF_FLAGS_NONE, &md, raw)));
    Blob blob;
    std::printf("load_null %08x\n", unsigned(LoadFromTIFFMemory(nullptr, 0, TIFF_FLAGS_NONE, &md, image)));
    std::printf("metadata_null %08x\n", unsigned(GetMetadataFromTIFFMemory(nullptr, 0, TIFF_FLAGS_NONE, md)));
    std::printf("raw_null %08x\n", unsigned(LoadFromTIFFMemoryRaw(nullptr, 0, TIFF_FLAGS_NONE, &md, raw)));
    std::printf("load_file_null %08x\n", unsigned(LoadFromTIFFFile(nullptr, TIFF_FLAGS_NONE, &md, image)));
    std::printf("save_file_null %08x\n", unsigned(SaveToTIFFFile(Image(), TIFF_FLAGS_NONE, nullptr)));
    std::printf("save_null %08x\n", unsigned(SaveToTIFFMemory(Image(), TIFF_FLAGS_NONE, blob)));
    return 0;
}

static int save(char** a)
{
    std::vector<uint8_t> px; Image src;
    if (!image_arg(a, px, src)) return 1;
    Blob blob;
    const HRESULT hr = SaveToTIFFMemory(src, TIFF_FLAGS(std::atoi(a[5])), blob);
    if (FAILED(hr) && blob.GetBufferPointer()) { std::fprintf(stderr, "the blob was not released\n"); return 1; }
    if (SUCCEEDED(hr) && !write_file(a[6], blob.GetBufferPointer(), blob.GetBufferSize())) return 1;
    std::printf("hr %08x\n", unsigned(hr));
    return 0;
}

static int device_load_many(const char* list, TIFF_FLAGS flags)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    const std::vector<std::string> files = read_lines(list);
    std::vector<uint8_t> data;
    DeviceScratchImage image;
    for (size_t i = 0; i < files.size(); ++i)
    {
        if (!read_file(files[i], data)) { std::fprintf(stderr, "cannot read %s\n", files[i].c_str()); return 1; }
        TexMetadata hostMd, rawMd; ScratchImage host; TIFFRawImage raw;
        const uint8_t none = 0;
        const uint8_t* source = data.empty() ? &none : data.data();          // an empty file is a size of zero, not a null pointer
        const HRESULT hostHr = LoadFromTIFFMemory(source, data.size(), flags, &hostMd, host);
        (void)LoadFromTIFFMemoryRaw(source, data.size(), flags, &rawMd, raw);
        Window window(dev);
        TexMetadata md;
        const HRESULT hr = LoadFromTIFFMemory(dev, source, data.size(), flags, &md, image);
        const std::vector<Window::Mark> marks = window.end({ "tiff_undo", "tiff_texels" });
        if (FAILED(hr)) { std::printf("%zu %08x %08x %s\n", i, unsigned(hr), unsigned(hostHr), released(image) ? "released" : "held"); continue; }
        ScratchImage back;
        if (FAILED(image.Download(back))) { std::fprintf(stderr, "%s: download failed\n", files[i].c_str()); return 1; }
        const bool metaEqual = SUCCEEDED(hostHr) && same_metadata(md, hostMd) && same_metadata(image.GetMetadata(), host.GetMetadata());
        const bool pixelsEqual = SUCCEEDED(hostHr) && back.GetImageCount() == 1 && host.GetImageCount() == 1 && same_texels(*back.GetImage(0, 0, 0), *host.GetImage(0, 0, 0));
        std::printf("%zu %08x %08x ok %zu %zu %zu %llu %llu %d %d %u %u\n", i, unsigned(hr), unsigned(hostHr), md.width, md.height, raw.streamBytes,
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
    const TIFF_FLAGS flags = TIFF_FLAGS(std::atoi(a[5]));
    TexMetadata md;
    md.width = src.width; md.height = src.height; md.depth = md.arraySize = md.mipLevels = 1; md.format = src.format; md.dimension = TEX_DIMENSION_TEXTURE2D;
    DeviceScratchImage image;
    HRESULT hr = image.Upload(dev, &src, 1, md);
    if (FAILED(hr)) { std::printf("upload %08x\n", unsigned(hr)); return 1; }
    Window window(dev);
    hr = SaveToTIFFFile(dev, *image.GetImage(0, 0, 0), flags, a[6]);
    const std::vector<Window::Mark> marks = window.end({ "tiff_pack" });
    const std::string hostOut = std::string(a[6]) + ".host";
    const HRESULT hostHr = SaveToTIFFFile(src, flags, hostOut.c_str());
    std::printf("hr %08x %08x %llu %llu %u\n", unsigned(hr), unsigned(hostHr), (unsigned long long)window.up, (unsigned long long)window.down, marks[0].launches);
    return 0;
}

static int time_load(const char* file, int runs)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    std::vector<uint8_t> data;
    if (!read_file(file, data)) return 1;
    bool ok = true;
    std::vector<Window::Mark> marks;
    return time_runs(dev, runs,
        [&]
        {
            Window window(dev);          // the kernels' own milliseconds, read outside the timed call
            const double ms = timed_ms([&] { DeviceScratchImage image; ok = ok && SUCCEEDED(LoadFromTIFFMemory(dev, data.data(), data.size(), TIFF_FLAGS_NONE, nullptr, image)) && dxtex_ctx_synchronize(dev.Get()) == 0; });
            marks = window.end({ "tiff_undo", "tiff_texels" });
            return ms;
        },
        [&] { return timed_ms([&] { ScratchImage host; DeviceScratchImage image;
                                    ok = ok && SUCCEEDED(LoadFromTIFFMemory(data.data(), data.size(), TIFF_FLAGS_NONE, nullptr, host)) && SUCCEEDED(image.Upload(dev, host)) && dxtex_ctx_synchronize(dev.Get()) == 0; }); },
        [&](std::string& extra)
        {
            TIFFRawImage raw;
            const double rawMs = timed_ms([&] { ok = ok && SUCCEEDED(LoadFromTIFFMemoryRaw(data.data(), data.size(), TIFF_FLAGS_NONE, nullptr, raw)); });
            if (!ok) return false;
            // the host's serial undo of the same stream
            const double undoMs = timed_ms([&]
            {
                const dxtex::TiffLayout l{ raw.layout.width, raw.layout.height, raw.layout.bits, raw.layout.samples, raw.layout.kind, raw.layout.predictor, raw.layout.bigEndian, raw.layout.planar,
                                           raw.layout.whiteIsZero, raw.layout.opaque };
                for (size_t c = 0; c < raw.segmentCount; ++c)
                {
                    const TIFFRawImage::Segment& s = raw.segments[c];
                    dxtex::tiff_undo_segment_serial(raw.storage.GetBufferPointer(), dxtex::TiffSegment{ s.offset, s.firstRow, s.rows, s.firstCol, s.cols, s.rowBytes, s.plane }, l);
                }
            });
            char text[128];
            std::snprintf(text, sizeof(text), " raw %.3f ms undo %.3f ms undo_gpu %.4f ms texels_gpu %.4f ms", rawMs, undoMs, marks[0].ms, marks[1].ms);
            extra = text;
            return true;
        });
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "time_load")) return time_load(argv[2], std::atoi(argv[3]));
    if (argc == 4 && !std::strcmp(argv[1], "load_many")) return load_many(argv[2], TIFF_FLAGS(std::atoi(argv[3])));
    if (argc == 5 && !std::strcmp(argv[1], "fuzz")) return damaged(argv[2], false, std::strtoull(argv[3], nullptr, 0), size_t(std::atoll(argv[4])));
    if (argc == 3 && !std::strcmp(argv[1], "truncations")) return damaged(argv[2], true, 0, 0);
    if (argc == 3 && !std::strcmp(argv[1], "files")) return files(argv[2]);
    if (argc == 9 && !std::strcmp(argv[1], "save")) return save(argv + 2);
    if (argc == 4 && !std::strcmp(argv[1], "device_load_many")) return device_load_many(argv[2], TIFF_FLAGS(std::atoi(argv[3])));
    if (argc == 9 && !std::strcmp(argv[1], "device_save")) return device_save(argv + 2);
    std::fprintf(stderr, "usage: tiff_host_test load_many <list> <flags> | fuzz <file> <seed> <cases> | truncations <file> | files <file> | save <in.bin> <w> <h> <format> <rowPitch> <flags> <out> | "
                         "device_load_many <list> <flags> | device_save <in.bin> <w> <h> <format> <rowPitch> <flags> <out> | time_load <file> <runs>\n");
    return 2;
}
