// Host-only driver for DirectXTexAMD_Assemble.cpp (tests/test_assemble_cpu.py): prints the face layout tables as JSON and checks the
// argument handling that needs no device. Without arguments it creates no Device, so it runs anywhere - also as a stand-alone
// AddressSanitizer / UBSan build. `assemble_host_test gpu` (tests/test_assemble_host_gpu.py) runs the steps on device 0: six seeded faces
// into every layout and back byte for byte with a zero background, the strip, the stacks, MergeImages and the host-pointer CopyRectangle.
#include "../../directxtex_amd/host/DirectXTexAMD.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace DirectXTexAMD;

#define CHECK(COND) do { if (!(COND)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #COND); return 1; } } while (0)

static int RunGpu()
{
    Device device;
    CHECK(SUCCEEDED(device.Create(0)));
    const size_t W = 16, H = 16;
    ScratchImage faces;
    CHECK(SUCCEEDED(faces.Initialize2D(DXGI_FORMAT_R8G8B8A8_UNORM, W, H, 6, 1)));
    uint32_t seed = 12345u;
    for (size_t i = 0; i < faces.GetPixelsSize(); ++i) { seed = seed * 1664525u + 1013904223u; faces.GetPixels()[i] = uint8_t((seed >> 24) | 1u); }     // never 0: the background is
    DeviceScratchImage dfaces;
    CHECK(SUCCEEDED(dfaces.Upload(device, faces)));
    for (uint32_t k = 0; k < CROSS_KIND_COUNT; ++k)
    {
        const CrossLayout* l = GetCrossLayout(CROSS_KIND(k));
        DeviceScratchImage dcross, dcube;
        ScratchImage cross, cube;
        CHECK(SUCCEEDED(AssembleCross(device, CROSS_KIND(k), dfaces, dcross)));
        CHECK(SUCCEEDED(CubeFromCross(device, CROSS_KIND(k), dcross, dcube)));
        CHECK(SUCCEEDED(dcross.Download(cross)) && SUCCEEDED(dcube.Download(cube)));
        CHECK(cube.GetMetadata().IsCubemap() && cube.GetMetadata().arraySize == 6 && cube.GetPixelsSize() == faces.GetPixelsSize());
        CHECK(std::memcmp(cube.GetPixels(), faces.GetPixels(), faces.GetPixelsSize()) == 0);
        const Image* c = cross.GetImage(0, 0, 0);
        CHECK(c->width == W * l->cols && c->height == H * l->rows);
        size_t nonzero = 0;
        for (size_t y = 0; y < c->height; ++y) for (size_t x = 0; x < c->width * 4; ++x) nonzero += c->pixels[y * c->rowPitch + x] != 0;
        CHECK(nonzero == 6 * W * H * 4);                // the faces and nothing else
    }
    {
        DeviceScratchImage dstrip, darray, dvolume;
        ScratchImage strip, array, volume;
        CHECK(SUCCEEDED(AssembleStrip(device, dfaces, dstrip)) && SUCCEEDED(dstrip.Download(strip)));
        CHECK(strip.GetMetadata().height == 6 * H && std::memcmp(strip.GetPixels(), faces.GetPixels(), faces.GetPixelsSize()) == 0);
        std::vector<DeviceScratchImage> singles(6);
        std::vector<Image> ptrs;
        for (size_t i = 0; i < 6; ++i)
        {
            TexMetadata m = faces.GetMetadata(); m.arraySize = 1;
            CHECK(SUCCEEDED(singles[i].Upload(device, faces.GetImage(0, i, 0), 1, m)));
            ptrs.push_back(*singles[i].GetImage(0, 0, 0));
        }
        CHECK(SUCCEEDED(StackArray(device, ptrs.data(), 6, true, darray)) && SUCCEEDED(darray.Download(array)));
        CHECK(array.GetMetadata().IsCubemap() && std::memcmp(array.GetPixels(), faces.GetPixels(), faces.GetPixelsSize()) == 0);
        CHECK(StackArray(device, ptrs.data(), 5, true, darray) == E_INVALIDARG);
        CHECK(SUCCEEDED(StackVolume(device, ptrs.data(), 6, dvolume)) && SUCCEEDED(dvolume.Download(volume)));
        CHECK(volume.GetMetadata().depth == 6 && volume.GetMetadata().IsVolumemap() && std::memcmp(volume.GetPixels(), faces.GetPixels(), faces.GetPixelsSize()) == 0);
        // the DeviceScratchImage overload of CopyRectangle: a 5 x 3 piece of face 1 into face 0 of the array
        CHECK(SUCCEEDED(CopyRectangle(device, dfaces, 0, 1, 0, Rect(1, 1, 5, 3), darray, 0, 0, 0, TEX_FILTER_DEFAULT, 2, 4)) && SUCCEEDED(darray.Download(array)));
        for (size_t y = 0; y < H; ++y) for (size_t x = 0; x < W; ++x)
        {
            const bool in = x >= 2 && x < 7 && y >= 4 && y < 7;
            const Image* want = in ? faces.GetImage(0, 1, 0) : faces.GetImage(0, 0, 0);
            const size_t sx = in ? x - 1 : x, sy = in ? y - 3 : y;
            CHECK(std::memcmp(array.GetImage(0, 0, 0)->pixels + y * W * 4 + x * 4, want->pixels + sy * W * 4 + sx * 4, 4) == 0);
        }
    }
    {
        // host images: CopyRectangle moves the rectangle only; MergeImages converts image 2 to float and takes its red as alpha
        ScratchImage dst, merged;
        CHECK(SUCCEEDED(dst.Initialize2D(DXGI_FORMAT_R8G8B8A8_UNORM, 40, 30, 1, 1)));
        uint64_t up = 0, down = 0;
        GetTransferBytes(device, up, down, true);
        CHECK(SUCCEEDED(CopyRectangle(device, *faces.GetImage(0, 2, 0), Rect(3, 2, 9, 7), *dst.GetImage(0, 0, 0), TEX_FILTER_DEFAULT, 11, 5)));
        GetTransferBytes(device, up, down);
        CHECK(up == 9 * 7 * 4 && down == 9 * 7 * 4);
        for (size_t y = 0; y < 30; ++y) for (size_t x = 0; x < 40; ++x)
        {
            const bool in = x >= 11 && x < 20 && y >= 5 && y < 12;
            uint8_t want[4] = { 0, 0, 0, 0 };
            if (in) std::memcpy(want, faces.GetImage(0, 2, 0)->pixels + (y - 3) * W * 4 + (x - 8) * 4, 4);
            CHECK(std::memcmp(dst.GetPixels() + y * 160 + x * 4, want, 4) == 0);
        }
        const uint32_t permute[4] = { 0, 1, 2, 4 };
        const bool no[4] = { false, false, false, false };
        CHECK(SUCCEEDED(MergeImages(device, *faces.GetImage(0, 0, 0), *faces.GetImage(0, 1, 0), TEX_FILTER_DEFAULT, permute, no, no, merged)));
        const uint8_t* a = faces.GetImage(0, 0, 0)->pixels;
        const uint8_t* b = faces.GetImage(0, 1, 0)->pixels;
        for (size_t i = 0; i < W * H; ++i)       // 8-bit UNORM survives the trip through float exactly
            CHECK(merged.GetPixels()[4 * i] == a[4 * i] && merged.GetPixels()[4 * i + 1] == a[4 * i + 1] && merged.GetPixels()[4 * i + 2] == a[4 * i + 2] &&
                  merged.GetPixels()[4 * i + 3] == b[4 * i]);
    }
    std::printf("assemble_host_test gpu OK\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "gpu") == 0) return RunGpu();
    int bad = 0;
    Device none;                    // never created: every entry point must refuse it before touching anything
    DeviceScratchImage empty, out;
    Image image;
    const uint32_t permute[4] = { 0, 1, 2, 4 };
    const bool no[4] = { false, false, false, false };
    ScratchImage merged;
    bad += CopyRectangle(none, image, Rect(0, 0, 1, 1), image, TEX_FILTER_DEFAULT, 0, 0) != E_POINTER;
    bad += CopyRectangle(none, empty, 0, 0, 0, Rect(0, 0, 1, 1), empty, 0, 0, 0, TEX_FILTER_DEFAULT, 0, 0) != E_POINTER;
    bad += MergeImages(none, image, image, TEX_FILTER_DEFAULT, permute, no, no, merged) != E_POINTER;
    bad += AssembleCross(none, CROSS_H_CROSS, empty, out) != E_POINTER;
    bad += CubeFromCross(none, CROSS_V_CROSS, empty, out) != E_POINTER;
    bad += AssembleStrip(none, empty, out) != E_POINTER;
    bad += StackArray(none, &image, 1, false, out) != E_POINTER;
    bad += StackVolume(none, &image, 1, out) != E_POINTER;
    bad += GetCrossLayout(CROSS_KIND_COUNT) != nullptr;
    uint32_t p[4] = { 9, 9, 9, 9 }, z[4] = { 9, 9, 9, 9 }, o[4] = { 9, 9, 9, 9 };
    bad += !ParseMergeMask("rgbB", p, z, o) || p[0] != 0 || p[1] != 1 || p[2] != 2 || p[3] != 6 || z[3] || o[3];
    bad += !ParseMergeMask("A0", p, z, o) || p[0] != 7 || p[1] != 1 || p[3] != 3 || !z[1] || !z[3] || o[2];
    bad += !ParseMergeMask("x1", p, z, o) || p[0] != 0 || !o[1] || !o[3] || z[1];
    bad += ParseMergeMask("", p, z, o) || ParseMergeMask("rq", p, z, o);
    if (bad) { std::fprintf(stderr, "%d argument checks failed\n", bad); return 1; }

    std::printf("{");
    for (uint32_t k = 0; k < CROSS_KIND_COUNT; ++k)
    {
        const CrossLayout* l = GetCrossLayout(CROSS_KIND(k));
        std::printf("%s\"%s\": {\"cols\": %zu, \"rows\": %zu, \"x\": [", k ? ", " : "", l->name, l->cols, l->rows);
        for (int i = 0; i < 6; ++i) std::printf("%s%zu", i ? ", " : "", l->x[i]);
        std::printf("], \"y\": [");
        for (int i = 0; i < 6; ++i) std::printf("%s%zu", i ? ", " : "", l->y[i]);
        std::printf("]}");
    }
    std::printf("}\n");
    return 0;
}
