// The .dds codec's byte-serial half on the host, for tests/test_dds_raw_cpu.py. No device.
//
//   dds_host_test raw_many <list>
//       one file per line: "<path> <DDS_FLAGS>". Runs LoadFromDDSMemoryRaw and LoadFromDDSMemoryEx on an exact-size copy of the file and
//       prints, per file, "<index> <hr of Raw> <hr of Ex> fail <released 0/1>" or
//       "<index> <hr> <hr> ok <width height depth format arraySize mipLevels miscFlags miscFlags2 dimension> <op> <opaque> <paletted>
//        <direct> <payload's offset in the file> <payloadBytes> <same 0/1> <offset:rowPitch:slicePitch of every image>";
//       same = Raw's metadata is Ex's, Ex's image count is Raw's, and Raw's palette is the file's. One DDSRawImage serves every file: a
//       failure must leave it empty whatever it held before.
#include "codec_host_test.h"

static int raw_many(const char* list)
{
    std::ifstream in(list);
    DDSRawImage raw;
    size_t index = 0;
    for (std::string line; std::getline(in, line); ++index)
    {
        std::istringstream ss(line);
        std::string path; unsigned long flags = 0;
        if (!(ss >> path >> flags)) return 2;
        std::vector<uint8_t> data;
        if (!read_file(path, data)) { std::fprintf(stderr, "cannot read %s\n", path.c_str()); return 1; }
        const Exact exact(data.data(), data.size());
        const uint8_t* p = exact.n ? exact.p : nullptr;
        const HRESULT hr = LoadFromDDSMemoryRaw(p, exact.n, DDS_FLAGS(flags), nullptr, raw);
        TexMetadata md; ScratchImage image;
        const HRESULT hrEx = LoadFromDDSMemoryEx(p, exact.n, DDS_FLAGS(flags), &md, nullptr, image);
        if (FAILED(hr))
        {
            const bool released = !raw.payload && !raw.payloadBytes && raw.images.empty() && !raw.storage.GetBufferPointer();
            std::printf("%zu %08x %08x fail %d\n", index, unsigned(hr), unsigned(hrEx), int(released));
            continue;
        }
        const TexMetadata& m = raw.metadata;
        const size_t at = size_t(raw.payload - p);
        bool same = SUCCEEDED(hrEx) && same_metadata(m, md) && image.GetImageCount() == raw.images.size() && raw.payload >= p && at + raw.payloadBytes <= exact.n;
        if (same && raw.paletted) same = at >= sizeof(raw.palette) && !std::memcmp(raw.palette, raw.payload - sizeof(raw.palette), sizeof(raw.palette));
        std::printf("%zu %08x %08x ok %zu %zu %zu %u %zu %zu %u %u %u %u %d %d %d %zu %zu %d", index, unsigned(hr), unsigned(hrEx), m.width, m.height, m.depth, unsigned(m.format),
                    m.arraySize, m.mipLevels, unsigned(m.miscFlags), unsigned(m.miscFlags2), unsigned(m.dimension), raw.op, int(raw.opaque), int(raw.paletted), int(raw.direct),
                    at, raw.payloadBytes, int(same));
        for (const DDSRawImage::Source& s : raw.images) std::printf(" %zu:%zu:%zu", s.offset, s.rowPitch, s.slicePitch);
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "raw_many")) return raw_many(argv[2]);
    std::fprintf(stderr, "usage: dds_host_test raw_many <list>\n");
    return 2;
}
