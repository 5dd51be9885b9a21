// The portable pixmap codec through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_pnm_cpu.py (the first two
// commands, which need no device; also built with sanitizers as pnm_host_test_asan) and tests/test_pnm_host_gpu.py (the other two).
//
//   pnm_host_test load_many <list>
//       <list> holds one file path per line. Each file goes through LoadFromPortablePixMapMemoryRaw and through the host
//       LoadFromPortablePixMapMemory; one line per file: "<index> <raw hresult hex> <host hresult hex>" and, where it loaded, " ok <width>
//       <height> <format> <depth> <arraySize> <mipLevels> <miscFlags> <miscFlags2> <dimension> <kind> <maxval> <big endian> <ascii>
//       <payload offset> <payload bytes>", with the image's tight rows in <path>.out
//   pnm_host_test save <in.bin> <width> <height> <format> <rowPitch> <hdr 0|1> <out>
//       SaveToPortablePixMapMemory (hdr: SaveToPortablePixMapHDRMemory) of the pixels -> <out>; prints "hr <hresult hex>"
//   pnm_host_test device_load_many <list>
//       the same list through the host loader and through its resident form; one line per file: "<index> <resident hresult hex> <host
//       hresult hex>", then " ok <width> <height> <format> <payload bytes> <ascii> <bytes host -> device> <bytes device -> host> <metadata
//       equal> <pixels equal>", or " released" / " held" for whether a failure left the result empty
//   pnm_host_test device_save <in.bin> <width> <height> <format> <rowPitch> <hdr 0|1> <out>
//       the image goes up, the resident saver writes <out> and the host one <out>.host from the same pixels; prints "hr <resident hresult
//       hex> <host hresult hex> <bytes host -> device> <bytes device -> host>" counted around the resident save alone
//   pnm_host_test time_load <file> <runs> | time_save <file> <runs> <hdr 0|1>
//       for tools/pnm_bench.py: wall time and bytes moved of the resident path beside the same build's host path, one line per run
#include "codec_host_test.h"

static int load_many(const char* list)
{
    const std::vector<std::string> files = read_lines(list);
    std::vector<uint8_t> data;
    PNMRawImage raw; ScratchImage image;          // one object each for every file: a failure must leave it empty whatever it held before
    for (size_t i = 0; i < files.size(); ++i)
    {
        if (!read_file(files[i], data)) { std::fprintf(stderr, "cannot read %s\n", files[i].c_str()); return 1; }
        const Exact exact(data.data(), data.size());
        TexMetadata rawMd, md;
        const HRESULT rawHr = LoadFromPortablePixMapMemoryRaw(exact.p, exact.n, &rawMd, raw);
        const HRESULT hr = LoadFromPortablePixMapMemory(exact.p, exact.n, &md, image);
        if (FAILED(rawHr) && (raw.payload || raw.storage.GetBufferPointer())) { std::fprintf(stderr, "%s: the raw image was not released\n", files[i].c_str()); return 1; }
        if (FAILED(hr) && (image.GetImageCount() || image.GetPixels())) { std::fprintf(stderr, "%s: the image was not released\n", files[i].c_str()); return 1; }
        if (FAILED(rawHr) || FAILED(hr)) { std::printf("%zu %08x %08x\n", i, unsigned(rawHr), unsigned(hr)); continue; }
        if (!same_metadata(rawMd, md) || !same_metadata(md, image.GetMetadata())) { std::fprintf(stderr, "%s: the metadata differ\n", files[i].c_str()); return 1; }
        const bool inside = raw.payload >= exact.p && raw.payload + raw.payloadBytes <= exact.p + exact.n;
        if (inside == raw.ascii || (inside && raw.payload != exact.p + raw.payloadOffset)) { std::fprintf(stderr, "%s: payload neither in the file nor decoded\n", files[i].c_str()); return 1; }
        const Image* img = image.GetImage(0, 0, 0);
        size_t rp = 0, sp = 0;
        if (!img || FAILED(ComputePitch(md.format, md.width, md.height, rp, sp))) return 1;
        std::vector<uint8_t> tight(rp * md.height);
        for (size_t y = 0; y < md.height; ++y) std::memcpy(tight.data() + y * rp, img->pixels + y * img->rowPitch, rp);
        if (!write_file(files[i] + ".out", tight.data(), tight.size())) return 1;
        std::printf("%zu %08x %08x ok %zu %zu %u %zu %zu %zu %u %u %u %u %u %d %d %zu %zu\n", i, unsigned(rawHr), unsigned(hr), md.width, md.height, unsigned(md.format),
                    md.depth, md.arraySize, md.mipLevels, unsigned(md.miscFlags), unsigned(md.miscFlags2), unsigned(md.dimension), raw.kind, raw.maxval,
                    int(raw.bigEndian), int(raw.ascii), raw.payloadOffset, raw.payloadBytes);
    }
    return 0;
}

static int save(char** a)
{
    std::vector<uint8_t> px; Image src;
    if (!image_arg(a, px, src)) return 1;
    Blob blob;
    const HRESULT hr = std::atoi(a[5]) ? SaveToPortablePixMapHDRMemory(src, blob) : SaveToPortablePixMapMemory(src, blob);
    if (FAILED(hr) && blob.GetBufferPointer()) { std::fprintf(stderr, "the blob was not released\n"); return 1; }
    if (SUCCEEDED(hr) && !write_file(a[6], blob.GetBufferPointer(), blob.GetBufferSize())) return 1;
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
        TexMetadata hostMd, rawMd; ScratchImage host; PNMRawImage raw;
        const uint8_t none = 0;
        const uint8_t* source = data.empty() ? &none : data.data();          // an empty file is a size of zero, not a null pointer
        const HRESULT hostHr = LoadFromPortablePixMapMemory(source, data.size(), &hostMd, host);
        (void)LoadFromPortablePixMapMemoryRaw(source, data.size(), &rawMd, raw);
        Window window(dev);
        TexMetadata md;
        const HRESULT hr = LoadFromPortablePixMapMemory(dev, source, data.size(), &md, image);
        window.end();
        if (FAILED(hr)) { std::printf("%zu %08x %08x %s\n", i, unsigned(hr), unsigned(hostHr), released(image) ? "released" : "held"); continue; }
        ScratchImage back;
        if (FAILED(image.Download(back))) { std::fprintf(stderr, "%s: download failed\n", files[i].c_str()); return 1; }
        const bool metaEqual = SUCCEEDED(hostHr) && same_metadata(md, hostMd) && same_metadata(image.GetMetadata(), host.GetMetadata());
        const bool pixelsEqual = SUCCEEDED(hostHr) && back.GetPixelsSize() == host.GetPixelsSize() && !std::memcmp(back.GetPixels(), host.GetPixels(), host.GetPixelsSize());
        std::printf("%zu %08x %08x ok %zu %zu %u %zu %d %llu %llu %d %d\n", i, unsigned(hr), unsigned(hostHr), md.width, md.height, unsigned(md.format), raw.payloadBytes, int(raw.ascii),
                    (unsigned long long)window.up, (unsigned long long)window.down, int(metaEqual), int(pixelsEqual));
    }
    return 0;
}

static int device_save(char** a)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    std::vector<uint8_t> px; Image src;
    if (!image_arg(a, px, src)) return 1;
    const bool hdr = std::atoi(a[5]) != 0;
    TexMetadata md;
    md.width = src.width; md.height = src.height; md.depth = md.arraySize = md.mipLevels = 1; md.format = src.format; md.dimension = TEX_DIMENSION_TEXTURE2D;
    DeviceScratchImage image;
    HRESULT hr = image.Upload(dev, &src, 1, md);
    if (FAILED(hr)) { std::printf("upload %08x\n", unsigned(hr)); return 1; }
    Window window(dev);
    hr = hdr ? SaveToPortablePixMapHDRFile(dev, *image.GetImage(0, 0, 0), a[6]) : SaveToPortablePixMapFile(dev, *image.GetImage(0, 0, 0), a[6]);
    window.end();
    const std::string hostOut = std::string(a[6]) + ".host";
    const HRESULT hostHr = hdr ? SaveToPortablePixMapHDRFile(src, hostOut.c_str()) : SaveToPortablePixMapFile(src, hostOut.c_str());
    std::printf("hr %08x %08x %llu %llu\n", unsigned(hr), unsigned(hostHr), (unsigned long long)window.up, (unsigned long long)window.down);
    return 0;
}

// tools/pnm_bench.py: a file through the resident loader and through the host loader plus Upload, alternating, `runs` times each after one
// unmeasured run each; a resident image through the resident saver and through Download plus the host saver likewise
static int time_paths(const char* file, int runs, bool saveHdr, bool save)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    std::vector<uint8_t> data;
    if (!read_file(file, data)) return 1;
    DeviceScratchImage resident;
    TexMetadata md;
    if (FAILED(LoadFromPortablePixMapMemory(dev, data.data(), data.size(), &md, resident))) return 1;
    bool ok = true;
    if (save)
    {
        const Image& img = *resident.GetImage(0, 0, 0);
        return time_runs(dev, runs,
            [&] { return timed_ms([&] { Blob blob; ok = ok && SUCCEEDED(saveHdr ? SaveToPortablePixMapHDRMemory(dev, img, blob) : SaveToPortablePixMapMemory(dev, img, blob)); }); },
            [&] { return timed_ms([&] { Blob blob; ScratchImage host;
                                        ok = ok && SUCCEEDED(resident.Download(host)) && SUCCEEDED(saveHdr ? SaveToPortablePixMapHDRMemory(*host.GetImage(0, 0, 0), blob) : SaveToPortablePixMapMemory(*host.GetImage(0, 0, 0), blob)); }); },
            [&](std::string&) { return ok; });
    }
    return time_runs(dev, runs,
        [&] { return timed_ms([&] { DeviceScratchImage image; ok = ok && SUCCEEDED(LoadFromPortablePixMapMemory(dev, data.data(), data.size(), nullptr, image)) && dxtex_ctx_synchronize(dev.Get()) == 0; }); },
        [&] { return timed_ms([&] { ScratchImage host; DeviceScratchImage image;
                                    ok = ok && SUCCEEDED(LoadFromPortablePixMapMemory(data.data(), data.size(), nullptr, host)) && SUCCEEDED(image.Upload(dev, host)) && dxtex_ctx_synchronize(dev.Get()) == 0; }); },
        [&](std::string&) { return ok; });
}

int main(int argc, char** argv)
{
    if (argc == 4 && !std::strcmp(argv[1], "time_load")) return time_paths(argv[2], std::atoi(argv[3]), false, false);
    if (argc == 5 && !std::strcmp(argv[1], "time_save")) return time_paths(argv[2], std::atoi(argv[3]), std::atoi(argv[4]) != 0, true);
    if (argc == 3 && !std::strcmp(argv[1], "load_many")) return load_many(argv[2]);
    if (argc == 9 && !std::strcmp(argv[1], "save")) return save(argv + 2);
    if (argc == 3 && !std::strcmp(argv[1], "device_load_many")) return device_load_many(argv[2]);
    if (argc == 9 && !std::strcmp(argv[1], "device_save")) return device_save(argv + 2);
    std::fprintf(stderr, "usage: pnm_host_test time_load <file> <runs> | time_save <file> <runs> <hdr> | load_many <list> | save <in.bin> <w> <h> <format> <rowPitch> <hdr> <out> | device_load_many <list> | device_save <in.bin> <w> <h> <format> <rowPitch> <hdr> <out>\n");
    return 2;
}
