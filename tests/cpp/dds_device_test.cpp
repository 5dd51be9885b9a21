// The .dds codec's resident loaders and writers against the host forms, for tests/test_dds_host_gpu.py and tests/test_dds_tools_gpu.py.
//
//   dds_device_test load_many <list>
//       one file per line: "<path> <DDS_FLAGS>". The host LoadFromDDSMemory and LoadFromDDSMemory(Device&) + Download on the same bytes.
//       Prints "<index> <hr> <host hr> fail <released|held>" or
//       "<index> <hr> <host hr> ok <metadata equal 0/1> <pixels equal 0/1> <bytes up> <bytes down> <dds kernel launches>"; the counts cover
//       the load alone. One DeviceScratchImage serves every file.
//   dds_device_test save_many <list>
//       "<path> <DDS_FLAGS of the load> <DDS_FLAGS of the save>": the file through the host loader, saved by the host writer and, after an
//       Upload, by SaveToDDSMemory(Device&); then the resident writer's blob through the resident loader and back. Prints
//       "<index> <hr> <host hr> <blobs equal 0/1> <bytes up> <bytes down of the save> <round trip equal 0/1> <blob bytes>".
//   dds_device_test host_load <in.dds> <DDS_FLAGS> <out.bin>   the host loader's pixels (what a tool's input must equal)
//   dds_device_test host_save <in.dds> <DDS_FLAGS of the load> <DDS_FLAGS of the save> <out.dds>   load + save, host forms
//   dds_device_test time_save24 <in.dds> <out.dds> <runs>   for profiles/dds.md: a B8G8R8X8 file to a 24-bit file, file to file, the resident
//       loader and writer against the host loader + Upload + Download + host writer; prints the milliseconds of each run, alternating
#include "codec_host_test.h"

static bool same_pixels(const ScratchImage& a, const ScratchImage& b)
{
    return a.GetPixelsSize() == b.GetPixelsSize() && a.GetPixels() && b.GetPixels() && !std::memcmp(a.GetPixels(), b.GetPixels(), a.GetPixelsSize());
}

struct Line { std::string path; unsigned long a = 0, b = 0; };
static std::vector<Line> read_list(const char* list)
{
    std::vector<Line> lines;
    for (const std::string& text : read_lines(list))
    {
        std::istringstream ss(text);
        Line l;
        if (ss >> l.path >> l.a) { ss >> l.b; lines.push_back(l); }
    }
    return lines;
}

static int load_many(const char* list)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    const std::vector<Line> files = read_list(list);
    DeviceScratchImage image;
    for (size_t i = 0; i < files.size(); ++i)
    {
        std::vector<uint8_t> data;
        if (!read_file(files[i].path, data)) { std::fprintf(stderr, "cannot read %s\n", files[i].path.c_str()); return 1; }
        const DDS_FLAGS flags = DDS_FLAGS(files[i].a);
        TexMetadata hostMd; ScratchImage host;
        const HRESULT hostHr = LoadFromDDSMemory(data.data(), data.size(), flags, &hostMd, host);
        Window window(dev);
        TexMetadata md;
        const HRESULT hr = LoadFromDDSMemory(dev, data.data(), data.size(), flags, &md, image);
        const unsigned launches = window.end({ "dds_" })[0].launches;
        if (FAILED(hr)) { std::printf("%zu %08x %08x fail %s\n", i, unsigned(hr), unsigned(hostHr), released(image) ? "released" : "held"); continue; }
        ScratchImage back;
        if (FAILED(image.Download(back))) { std::fprintf(stderr, "%s: download failed\n", files[i].path.c_str()); return 1; }
        const bool metaEqual = SUCCEEDED(hostHr) && same_metadata(md, hostMd) && same_metadata(image.GetMetadata(), host.GetMetadata());
        std::printf("%zu %08x %08x ok %d %d %llu %llu %u\n", i, unsigned(hr), unsigned(hostHr), int(metaEqual), int(SUCCEEDED(hostHr) && same_pixels(back, host)),
                    (unsigned long long)window.up, (unsigned long long)window.down, launches);
    }
    return 0;
}

static int save_many(const char* list)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    const std::vector<Line> files = read_list(list);
    for (size_t i = 0; i < files.size(); ++i)
    {
        TexMetadata md; ScratchImage host;
        if (FAILED(LoadFromDDSFile(files[i].path.c_str(), DDS_FLAGS(files[i].a), &md, host))) { std::fprintf(stderr, "cannot load %s\n", files[i].path.c_str()); return 1; }
        const DDS_FLAGS flags = DDS_FLAGS(files[i].b);
        Blob hostBlob, blob;
        const HRESULT hostHr = SaveToDDSMemory(host.GetImages(), host.GetImageCount(), md, flags, hostBlob);
        DeviceScratchImage image;
        if (FAILED(image.Upload(dev, host))) { std::fprintf(stderr, "%s: upload failed\n", files[i].path.c_str()); return 1; }
        Window window(dev);
        const HRESULT hr = SaveToDDSMemory(dev, image.GetImages(), image.GetImageCount(), md, flags, blob);
        window.end();
        const bool equal = SUCCEEDED(hr) && SUCCEEDED(hostHr) && blob.GetBufferSize() == hostBlob.GetBufferSize() &&
                           !std::memcmp(blob.GetBufferPointer(), hostBlob.GetBufferPointer(), blob.GetBufferSize());
        bool roundTrip = false;
        if (SUCCEEDED(hr))
        {
            DeviceScratchImage again; ScratchImage back; TexMetadata md2;
            roundTrip = SUCCEEDED(LoadFromDDSMemory(dev, blob.GetBufferPointer(), blob.GetBufferSize(), DDS_FLAGS(files[i].a), &md2, again)) && SUCCEEDED(again.Download(back)) &&
                        same_pixels(back, host) && md2.format == md.format;
        }
        std::printf("%zu %08x %08x %d %llu %llu %d %zu\n", i, unsigned(hr), unsigned(hostHr), int(equal), (unsigned long long)window.up, (unsigned long long)window.down, int(roundTrip), blob.GetBufferSize());
    }
    return 0;
}

static int host_load(char** a)
{
    TexMetadata md; ScratchImage host;
    const HRESULT hr = LoadFromDDSFile(a[0], DDS_FLAGS(std::strtoul(a[1], nullptr, 0)), &md, host);
    std::printf("%08x\n", unsigned(hr));
    return SUCCEEDED(hr) && write_file(a[2], host.GetPixels(), host.GetPixelsSize()) ? 0 : 1;
}

static int host_save(char** a)
{
    TexMetadata md; ScratchImage host;
    HRESULT hr = LoadFromDDSFile(a[0], DDS_FLAGS(std::strtoul(a[1], nullptr, 0)), &md, host);
    if (SUCCEEDED(hr)) hr = SaveToDDSFile(host.GetImages(), host.GetImageCount(), md, DDS_FLAGS(std::strtoul(a[2], nullptr, 0)), a[3]);
    std::printf("%08x\n", unsigned(hr));
    return SUCCEEDED(hr) ? 0 : 1;
}

static int time_save24(char** a)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    const int runs = std::atoi(a[2]);
    for (int r = -1; r < runs; ++r)          // run -1 warms up and is not printed
        for (int resident = 0; resident < 2; ++resident)
        {
            const auto t0 = std::chrono::steady_clock::now();
            TexMetadata md; DeviceScratchImage image; ScratchImage host, back;
            HRESULT hr;
            if (resident)
            {
                hr = LoadFromDDSFile(dev, a[0], DDS_FLAGS_NONE, &md, image);
                if (SUCCEEDED(hr)) hr = SaveToDDSFile(dev, image.GetImages(), image.GetImageCount(), md, DDS_FLAGS_FORCE_24BPP_RGB, a[1]);
            }
            else
            {
                hr = LoadFromDDSFile(a[0], DDS_FLAGS_NONE, &md, host);
                if (SUCCEEDED(hr)) hr = image.Upload(dev, host);
                if (SUCCEEDED(hr)) hr = image.Download(back);
                if (SUCCEEDED(hr)) hr = SaveToDDSFile(back.GetImages(), back.GetImageCount(), md, DDS_FLAGS_FORCE_24BPP_RGB, a[1]);
            }
            if (FAILED(hr)) { std::fprintf(stderr, "%s failed %08x\n", resident ? "resident" : "host", unsigned(hr)); return 1; }
            if (r >= 0) std::printf("%s %.3f\n", resident ? "resident" : "host", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 5 && !std::strcmp(argv[1], "time_save24")) return time_save24(argv + 2);
    if (argc == 3 && !std::strcmp(argv[1], "load_many")) return load_many(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "save_many")) return save_many(argv[2]);
    if (argc == 5 && !std::strcmp(argv[1], "host_load")) return host_load(argv + 2);
    if (argc == 6 && !std::strcmp(argv[1], "host_save")) return host_save(argv + 2);
    std::fprintf(stderr, "usage: dds_device_test load_many <list> | save_many <list> | host_load <in> <flags> <out> | host_save <in> <load flags> <save flags> <out>\n");
    return 2;
}
