// The JPEG writer through the C++ host layer (directxtex_amd/host/DirectXTexAMD.h), for tests/test_jpeg_write_cpu.py (the first four
// commands, which need no device; also built with sanitizers as jpeg_write_host_test_asan) and tests/test_jpeg_write_host_gpu.py (the fifth).
//
//   jpeg_write_host_test save_many <list>
//       <list> holds one "<format> <width> <height> <pitch> <pixels file>" per line. Each image goes through the host SaveToJPEGMemory; one
//       line per image, "<index> <hresult hex> <bytes>", and the file as <list>.<index>.jpg where it was written
//   jpeg_write_host_test resave_many <list>
//       <list> holds one .jpg path per line. Each goes through LoadFromJPEGMemoryRaw and SaveJPEGRaw; "<index> <load hresult hex> <save
//       hresult hex> <bytes>" and <list>.<index>.jpg
//   jpeg_write_host_test errors <directory>
//       the refusals; prints one "name hresult" per line
//   jpeg_write_host_test sweep
//       every size from 1x1 to 17x17 as grey, RGBA on a padded pitch and BGRX through the host saver, the host loader and the raw pair:
//       the file loads at its size and format, and its coefficients written again are its bytes. Prints "sweep ok <files>"
//   jpeg_write_host_test device_save_many <list>
//       save_many's list through the resident SaveToJPEGMemory and the host one: "<index> <resident hresult hex> <host hresult hex>", then
//       " ok <coefficient bytes> <bytes host -> device> <bytes device -> host> <bytes equal> <jpeg kernel launches>" and the resident file
//       as <list>.<index>.jpg, or " empty" / " held" for whether a failure left the blob empty
//   jpeg_write_host_test time_save <width> <height> <format> <runs>
//       for tools/jpeg_bench.py: wall time and bytes moved of the resident saver beside Download plus the same build's host saver, and the
//       byte-serial half alone, one line per run
#include "codec_host_test.h"

struct Line { unsigned format; size_t width, height, pitch; std::string path; };
static std::vector<Line> read_list(const char* path)
{
    std::vector<Line> lines;
    for (const std::string& line : read_lines(path))
    {
        std::istringstream ss(line);
        Line l;
        if (!(ss >> l.format >> l.width >> l.height >> l.pitch)) continue;
        std::getline(ss >> std::ws, l.path);
        lines.push_back(l);
    }
    return lines;
}

static Image image_of(const Line& l, uint8_t* pixels) { return Image{ l.width, l.height, DXGI_FORMAT(l.format), l.pitch, l.pitch * l.height, pixels }; }

static std::string numbered(const char* list, size_t i) { return std::string(list) + "." + std::to_string(i) + ".jpg"; }

static int save_many(const char* list)
{
    const std::vector<Line> lines = read_list(list);
    std::vector<uint8_t> data;
    Blob blob;          // one for every image: a failure must leave it empty whatever it held before
    for (size_t i = 0; i < lines.size(); ++i)
    {
        if (!read_file(lines[i].path, data)) { std::fprintf(stderr, "cannot read %s\n", lines[i].path.c_str()); return 1; }
        const Exact exact(data.data(), data.size());
        const HRESULT hr = SaveToJPEGMemory(image_of(lines[i], exact.p), JPEG_FLAGS_NONE, blob);
        if (FAILED(hr) && (blob.GetBufferPointer() || blob.GetBufferSize())) { std::fprintf(stderr, "%zu: the blob was not released\n", i); return 1; }
        if (SUCCEEDED(hr) && !write_file(numbered(list, i), blob.GetBufferPointer(), blob.GetBufferSize())) return 1;
        std::printf("%zu %08x %zu\n", i, unsigned(hr), blob.GetBufferSize());
    }
    return 0;
}

static int resave_many(const char* list)
{
    const std::vector<std::string> files = read_lines(list);
    std::vector<uint8_t> data;
    Blob blob; JPEGRawImage raw;
    for (size_t i = 0; i < files.size(); ++i)
    {
        if (!read_file(files[i], data)) { std::fprintf(stderr, "cannot read %s\n", files[i].c_str()); return 1; }
        const Exact exact(data.data(), data.size());
        const HRESULT loadHr = LoadFromJPEGMemoryRaw(exact.p, exact.n, JPEG_FLAGS_NONE, nullptr, raw);
        const HRESULT hr = SUCCEEDED(loadHr) ? SaveJPEGRaw(raw, blob) : loadHr;
        if (SUCCEEDED(hr) && !write_file(numbered(list, i), blob.GetBufferPointer(), blob.GetBufferSize())) return 1;
        std::printf("%zu %08x %08x %zu\n", i, unsigned(loadHr), unsigned(hr), blob.GetBufferSize());
    }
    return 0;
}

// a raw frame of one grey 8 x 8 block with quantiser table 0 all ones
static void one_block(JPEGRawImage& raw, int16_t dc, int16_t ac)
{
    raw.Release();
    raw.storage.Initialize(64 * sizeof(int16_t));
    int16_t* c = reinterpret_cast<int16_t*>(raw.storage.GetBufferPointer());
    std::memset(c, 0, 64 * sizeof(int16_t));
    c[0] = dc; c[1] = ac;
    raw.width = raw.height = 8; raw.components = 1; raw.colour = DXTEX_JPEG_GREY;
    raw.component[0].h = raw.component[0].v = 1; raw.component[0].blocksPerRow = raw.component[0].blockRows = 1;
    for (uint16_t& q : raw.quant[0]) q = 1;
    raw.coefficients = c; raw.coefficientCount = 64;
}

static int errors(const char* directory)
{
    std::vector<uint8_t> px(16 * 16 * 16, 0x40);
    const auto image = [&](DXGI_FORMAT f, size_t w, size_t h, size_t pitch) { return Image{ w, h, f, pitch, pitch * h, px.data() }; };
    const std::string path = std::string(directory) + "/x.jpg";
    Blob blob;
    // a call that must fail and leave the blob, which held something before, empty
    const auto refused = [&](const char* name, auto&& call)
    {
        blob.Initialize(16);
        const HRESULT hr = call();
        std::printf("%s %08x held %d\n", name, unsigned(hr), (blob.GetBufferPointer() || blob.GetBufferSize()) ? 1 : 0);
    };
    std::printf("file_null %08x\n", unsigned(SaveToJPEGFile(image(DXGI_FORMAT_R8_UNORM, 8, 8, 8), JPEG_FLAGS_NONE, nullptr)));
    std::printf("file_null_bad_format %08x\n", unsigned(SaveToJPEGFile(image(DXGI_FORMAT_R16_UNORM, 8, 8, 16), JPEG_FLAGS_NONE, nullptr)));
    const DXGI_FORMAT others[] = { DXGI_FORMAT_R16_UNORM, DXGI_FORMAT_R8G8_UNORM, DXGI_FORMAT_R16G16B16A16_UNORM, DXGI_FORMAT_R32G32B32A32_FLOAT, DXGI_FORMAT_R8G8B8A8_SNORM,
                                    DXGI_FORMAT_R8G8B8A8_UINT, DXGI_FORMAT_R10G10B10A2_UNORM, DXGI_FORMAT_A8_UNORM, DXGI_FORMAT_BC1_UNORM, DXGI_FORMAT_B5G6R5_UNORM };
    for (const DXGI_FORMAT f : others)
    {
        refused(("format_" + std::to_string(unsigned(f))).c_str(), [&] { return SaveToJPEGMemory(image(f, 8, 8, 128), JPEG_FLAGS_NONE, blob); });
        std::printf("file_format_%u %08x\n", unsigned(f), unsigned(SaveToJPEGFile(image(f, 8, 8, 128), JPEG_FLAGS_NONE, path.c_str())));
    }
    Image none = image(DXGI_FORMAT_R8_UNORM, 8, 8, 8); none.pixels = nullptr;
    refused("pixels_null", [&] { return SaveToJPEGMemory(none, JPEG_FLAGS_NONE, blob); });
    refused("width_0", [&] { return SaveToJPEGMemory(image(DXGI_FORMAT_R8_UNORM, 0, 8, 8), JPEG_FLAGS_NONE, blob); });
    refused("width_65536", [&] { return SaveToJPEGMemory(image(DXGI_FORMAT_R8_UNORM, 65536, 1, 65536), JPEG_FLAGS_NONE, blob); });
    refused("pitch_short", [&] { return SaveToJPEGMemory(image(DXGI_FORMAT_R8G8B8A8_UNORM, 8, 8, 31), JPEG_FLAGS_NONE, blob); });
    JPEGRawImage raw;
    one_block(raw, 1016, 1016);
    std::printf("raw_ok %08x\n", unsigned(SaveJPEGRaw(raw, blob)));
    one_block(raw, 2047, 1023);
    std::printf("raw_dc_2047_ac_1023 %08x\n", unsigned(SaveJPEGRaw(raw, blob)));
    one_block(raw, 2048, 0);
    refused("raw_dc_2048", [&] { return SaveJPEGRaw(raw, blob); });
    one_block(raw, 0, 1024);
    refused("raw_ac_1024", [&] { return SaveJPEGRaw(raw, blob); });
    one_block(raw, 0, -1024);
    refused("raw_ac_minus_1024", [&] { return SaveJPEGRaw(raw, blob); });
    one_block(raw, 0, 0); raw.quant[0][63] = 0;
    refused("raw_quant_0", [&] { return SaveJPEGRaw(raw, blob); });
    one_block(raw, 0, 0); raw.component[0].blocksPerRow = 2;
    refused("raw_blocks", [&] { return SaveJPEGRaw(raw, blob); });
    one_block(raw, 0, 0); raw.coefficientCount = 63;
    refused("raw_short", [&] { return SaveJPEGRaw(raw, blob); });
    one_block(raw, 0, 0); raw.colour = DXTEX_JPEG_RGB; raw.components = 3;
    refused("raw_rgb", [&] { return SaveJPEGRaw(raw, blob); });
    one_block(raw, 0, 0); raw.coefficients = nullptr;
    refused("raw_null", [&] { return SaveJPEGRaw(raw, blob); });
    // a 16-bit table: DQT with 16-bit entries and SOF1, which the reader takes back
    one_block(raw, 3, -2); raw.quant[0][5] = 300;
    HRESULT hr = SaveJPEGRaw(raw, blob);
    JPEGRawImage again;
    const HRESULT back = SUCCEEDED(hr) ? LoadFromJPEGMemoryRaw(blob.GetBufferPointer(), blob.GetBufferSize(), JPEG_FLAGS_NONE, nullptr, again) : hr;
    const bool same = SUCCEEDED(back) && again.quant[0][5] == 300 && again.coefficientCount == 64 && !std::memcmp(again.coefficients, raw.coefficients, 128);
    std::printf("raw_wide_table %08x %08x same %d sof %02x\n", unsigned(hr), unsigned(back), int(same), SUCCEEDED(hr) ? unsigned(blob.GetBufferPointer()[2 + 18 + 2 + 129 + 3]) : 0u);
    hr = SaveToJPEGFile(image(DXGI_FORMAT_B8G8R8X8_UNORM, 9, 7, 64), JPEG_FLAGS_NONE, path.c_str());
    TexMetadata md;
    const HRESULT read = GetMetadataFromJPEGFile(path.c_str(), JPEG_FLAGS_NONE, md);
    std::printf("file_ok %08x %08x %zu %zu %u\n", unsigned(hr), unsigned(read), md.width, md.height, unsigned(md.format));
    return 0;
}

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 24; }

static int sweep()
{
    size_t files = 0;
    uint32_t seed = 1;
    Blob blob, again; ScratchImage loaded; JPEGRawImage raw;
    for (size_t h = 1; h <= 17; ++h)
        for (size_t w = 1; w <= 17; ++w)
        {
            struct Kind { DXGI_FORMAT format; size_t texel, pad; DXGI_FORMAT loads; } const kinds[] = {
                { DXGI_FORMAT_R8_UNORM, 1, 0, DXGI_FORMAT_R8_UNORM }, { DXGI_FORMAT_R8G8B8A8_UNORM, 4, 5, DXGI_FORMAT_R8G8B8A8_UNORM_SRGB }, { DXGI_FORMAT_B8G8R8X8_UNORM_SRGB, 4, 0, DXGI_FORMAT_R8G8B8A8_UNORM_SRGB } };
            for (const Kind& k : kinds)
            {
                const size_t pitch = w * k.texel + k.pad;
                std::vector<uint8_t> px(pitch * (h - 1) + w * k.texel);          // the last row ends with its last texel
                for (uint8_t& b : px) b = uint8_t(lcg(seed));
                const Exact exact(px.data(), px.size());
                HRESULT hr = SaveToJPEGMemory(Image{ w, h, k.format, pitch, pitch * h, exact.p }, JPEG_FLAGS_NONE, blob);
                if (FAILED(hr)) { std::fprintf(stderr, "%zux%zu format %u: save %08x\n", w, h, unsigned(k.format), unsigned(hr)); return 1; }
                const Exact file(blob.GetBufferPointer(), blob.GetBufferSize());
                TexMetadata md;
                hr = LoadFromJPEGMemory(file.p, file.n, JPEG_FLAGS_NONE, &md, loaded);
                if (FAILED(hr) || md.width != w || md.height != h || md.format != k.loads) { std::fprintf(stderr, "%zux%zu format %u: load %08x\n", w, h, unsigned(k.format), unsigned(hr)); return 1; }
                hr = LoadFromJPEGMemoryRaw(file.p, file.n, JPEG_FLAGS_NONE, nullptr, raw);
                if (SUCCEEDED(hr)) hr = SaveJPEGRaw(raw, again);
                if (FAILED(hr) || again.GetBufferSize() != file.n || std::memcmp(again.GetBufferPointer(), file.p, file.n))
                { std::fprintf(stderr, "%zux%zu format %u: the coefficients written again are not the file (%08x)\n", w, h, unsigned(k.format), unsigned(hr)); return 1; }
                ++files;
            }
        }
    std::printf("sweep ok %zu\n", files);
    return 0;
}

// the image of a line on the device, through a ScratchImage of its format
static HRESULT upload(Device& dev, const Line& l, const uint8_t* pixels, size_t rowBytes, DeviceScratchImage& resident)
{
    ScratchImage host;
    HRESULT hr = host.Initialize2D(DXGI_FORMAT(l.format), l.width, l.height, 1, 1);
    if (FAILED(hr)) return hr;
    const Image* img = host.GetImage(0, 0, 0);
    if (!img) return E_POINTER;
    for (size_t y = 0; y < l.height; ++y) std::memcpy(img->pixels + y * img->rowPitch, pixels + y * l.pitch, rowBytes < img->rowPitch ? rowBytes : img->rowPitch);
    return resident.Upload(dev, host);
}

static int device_save_many(const char* list)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    const std::vector<Line> lines = read_list(list);
    std::vector<uint8_t> data;
    Blob blob, host;
    for (size_t i = 0; i < lines.size(); ++i)
    {
        const Line& l = lines[i];
        if (!read_file(l.path, data)) { std::fprintf(stderr, "cannot read %s\n", l.path.c_str()); return 1; }
        const HRESULT hostHr = SaveToJPEGMemory(image_of(l, data.data()), JPEG_FLAGS_NONE, host);
        size_t rowPitch = 0, slicePitch = 0;
        DeviceScratchImage resident;
        if (FAILED(ComputePitch(DXGI_FORMAT(l.format), l.width, l.height, rowPitch, slicePitch)) || FAILED(upload(dev, l, data.data(), rowPitch, resident)))
        { std::fprintf(stderr, "%zu: upload failed\n", i); return 1; }
        const Image* img = resident.GetImage(0, 0, 0);
        if (!img) return 1;
        blob.Initialize(16);          // a failure must leave it empty whatever it held before
        Window window(dev);
        const HRESULT hr = SaveToJPEGMemory(dev, *img, JPEG_FLAGS_NONE, blob);
        const unsigned launches = window.end({ "jpeg_" })[0].launches;
        if (FAILED(hr))
        {
            std::printf("%zu %08x %08x %s\n", i, unsigned(hr), unsigned(hostHr), (blob.GetBufferPointer() || blob.GetBufferSize()) ? "held" : "empty");
            continue;
        }
        JPEGRawImage raw;
        if (FAILED(LoadFromJPEGMemoryRaw(blob.GetBufferPointer(), blob.GetBufferSize(), JPEG_FLAGS_NONE, nullptr, raw))) { std::fprintf(stderr, "%zu: the file does not load\n", i); return 1; }
        if (!write_file(numbered(list, i), blob.GetBufferPointer(), blob.GetBufferSize())) return 1;
        const bool equal = SUCCEEDED(hostHr) && blob.GetBufferSize() == host.GetBufferSize() && !std::memcmp(blob.GetBufferPointer(), host.GetBufferPointer(), host.GetBufferSize());
        std::printf("%zu %08x %08x ok %zu %llu %llu %d %u\n", i, unsigned(hr), unsigned(hostHr), raw.coefficientCount * 2, (unsigned long long)window.up, (unsigned long long)window.down,
                    int(equal), launches);
    }
    return 0;
}

// a gradient with noise through the resident saver and through Download plus the host saver, alternating, `runs` times each after one
// unmeasured run each; then the byte-serial half alone on the file's own coefficients
static int time_save(size_t width, size_t height, unsigned format, int runs)
{
    Device dev;
    if (FAILED(dev.Create(0))) { std::fprintf(stderr, "no device\n"); return 1; }
    ScratchImage host;
    if (FAILED(host.Initialize2D(DXGI_FORMAT(format), width, height, 1, 1))) return 1;
    const Image* img = host.GetImage(0, 0, 0);
    uint32_t seed = 7;
    const size_t texel = format == unsigned(DXGI_FORMAT_R8_UNORM) ? 1 : 4;
    for (size_t y = 0; y < height; ++y)
        for (size_t x = 0; x < width * texel; ++x) img->pixels[y * img->rowPitch + x] = uint8_t((x * 255 / (width * texel) + y * 255 / height) / 2 + lcg(seed) / 8);
    DeviceScratchImage resident;
    if (FAILED(resident.Upload(dev, host))) return 1;
    const Image* dimg = resident.GetImage(0, 0, 0);
    if (!dimg) { std::fprintf(stderr, "a step failed\n"); return 1; }
    bool ok = true;
    Blob a, b;
    const int failed = time_runs(dev, runs,
        [&] { return timed_ms([&] { ok = ok && SUCCEEDED(SaveToJPEGMemory(dev, *dimg, JPEG_FLAGS_NONE, a)); }); },
        [&] { return timed_ms([&] { ScratchImage back; ok = ok && SUCCEEDED(resident.Download(back)) && SUCCEEDED(SaveToJPEGMemory(*back.GetImage(0, 0, 0), JPEG_FLAGS_NONE, b)); }); },
        [&](std::string& extra)
        {
            extra = " file " + std::to_string(a.GetBufferSize());
            return ok && a.GetBufferSize() == b.GetBufferSize() && !std::memcmp(a.GetBufferPointer(), b.GetBufferPointer(), a.GetBufferSize());
        });
    if (failed) return failed;
    JPEGRawImage raw;
    if (FAILED(LoadFromJPEGMemoryRaw(a.GetBufferPointer(), a.GetBufferSize(), JPEG_FLAGS_NONE, nullptr, raw))) return 1;
    for (int i = -1; i < runs; ++i)
    {
        HRESULT hr = S_OK;
        const double ms = timed_ms([&] { hr = SaveJPEGRaw(raw, b); });
        if (FAILED(hr)) return 1;
        if (i >= 0) std::printf("run %d raw %.3f ms file %zu coefficients %zu\n", i, ms, b.GetBufferSize(), raw.coefficientCount * 2);
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 6 && !std::strcmp(argv[1], "time_save")) return time_save(size_t(std::atoll(argv[2])), size_t(std::atoll(argv[3])), unsigned(std::atoi(argv[4])), std::atoi(argv[5]));
    if (argc == 3 && !std::strcmp(argv[1], "save_many")) return save_many(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "resave_many")) return resave_many(argv[2]);
    if (argc == 3 && !std::strcmp(argv[1], "errors")) return errors(argv[2]);
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) return sweep();
    if (argc == 3 && !std::strcmp(argv[1], "device_save_many")) return device_save_many(argv[2]);
    std::fprintf(stderr, "usage: jpeg_write_host_test save_many|resave_many|device_save_many <list> | errors <directory> | sweep | time_save <width> <height> <format> <runs>\n");
    return 2;
}
