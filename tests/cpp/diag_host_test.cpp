// The host layer's diagnostics (DirectXTexAMD.h: ComputeMSE with CMSE_FLAGS, Analyze, AnalyzeBC, Difference) on a GPU, driven by
// tests/test_diag_host_gpu.py. Each check prints "ok <name>" or "FAIL <name>: ..."; the exit status is the number of failures.
#include "../../directxtex_amd/host/DirectXTexAMD.h"
#include "../../include/dxtex_amd.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace DirectXTexAMD;

static int g_failed = 0;
#define CHECK(NAME, COND) do { if (COND) std::printf("ok %s\n", NAME); else { std::printf("FAIL %s: %s (line %d)\n", NAME, #COND, __LINE__); ++g_failed; } } while (0)

static bool Close(double a, double b, double rtol) { return std::fabs(a - b) <= rtol * std::fabs(b); }
static bool SameBits(const float* a, const float* b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }

static bool SameExact(const AnalyzeData& a, const AnalyzeData& b)
{
    return SameBits(a.imageMin, b.imageMin, 4) && SameBits(a.imageMax, b.imageMax, 4) && SameBits(&a.luminance, &b.luminance, 1) &&
           std::memcmp(a.specials, b.specials, sizeof(a.specials)) == 0;
}
static bool SameSums(const AnalyzeData& a, const AnalyzeData& b)
{
    for (int c = 0; c < 4; ++c)
        if (!Close(a.imageAvg[c], b.imageAvg[c], 1e-6) || !Close(a.imageVariance[c], b.imageVariance[c], 1e-6) ||
            !Close(a.imageStdDev[c], std::sqrt(a.imageVariance[c]), 1e-12)) return false;
    return true;
}

// a smooth gradient with a pseudo-random part, so that BC blocks are neither flat nor noise
static void Fill(ScratchImage& img, DXGI_FORMAT fmt, size_t w, size_t h, uint32_t seed)
{
    img.Initialize2D(fmt, w, h, 1, 1);
    const Image* im = img.GetImage(0, 0, 0);
    uint32_t s = seed * 2654435761u + 12345u;
    for (size_t y = 0; y < h; ++y)
        for (size_t x = 0; x < w; ++x)
        {
            uint8_t* p = im->pixels + y * im->rowPitch + x * 4;
            s = s * 1664525u + 1013904223u;
            p[0] = uint8_t((x * 255) / (w - 1)); p[1] = uint8_t((y * 255) / (h - 1)); p[2] = uint8_t(((x + y) * 3 + (s >> 28)) & 0xFF); p[3] = uint8_t(128 + (s >> 25));
        }
}

static size_t ImageBytes(const Image& im) { return im.rowPitch * ComputeScanlines(im.format, im.height); }

int main()
{
    std::setvbuf(stdout, nullptr, _IONBF, 0);
    Device dev;
    if (FAILED(dev.Create(0))) { std::printf("FAIL device: no gfx950 device\n"); return 1; }
    uint64_t up = 0, down = 0;
    const size_t W = 64, H = 48;
    ScratchImage base, chain, bc7, bc1;
    Fill(base, DXGI_FORMAT_R8G8B8A8_UNORM, W, H, 1);
    const Image& rgba = *base.GetImage(0, 0, 0);

    // ---- Analyze of a BC7 chain == Analyze of its Decompress to RGBA32F ----
    {
        CHECK("mips", SUCCEEDED(GenerateMipMaps(dev, rgba, TEX_FILTER_LINEAR, 0, chain)));
        CHECK("bc7", SUCCEEDED(Compress(dev, chain.GetImages(), chain.GetImageCount(), chain.GetMetadata(), DXGI_FORMAT_BC7_UNORM, TEX_COMPRESS_BC7_QUICK, 0.5f, bc7)));
        const size_t n = bc7.GetImageCount();
        CHECK("bc7 chain has mips", n == 7 && bc7.GetMetadata().mipLevels == 7);
        if (g_failed) { std::printf("%d failed (setup)\n", g_failed); return g_failed; }      // everything below indexes the chain
        std::vector<AnalyzeData> got(n), want(n);
        GetTransferBytes(dev, up, down, true);
        CHECK("analyze bc7 chain", SUCCEEDED(Analyze(dev, bc7.GetImages(), n, bc7.GetMetadata(), got.data())));
        GetTransferBytes(dev, up, down, true);
        size_t payload = 0;
        for (size_t i = 0; i < n; ++i) payload += ImageBytes(bc7.GetImages()[i]);
        CHECK("analyze: one upload of the payload, one read-back of the figures", up == payload && down == n * 136);
        ScratchImage dec;
        CHECK("decompress", SUCCEEDED(Decompress(dev, bc7.GetImages(), n, bc7.GetMetadata(), DXGI_FORMAT_R32G32B32A32_FLOAT, dec)));
        if (g_failed) { std::printf("%d failed (setup)\n", g_failed); return g_failed; }
        CHECK("analyze decompressed chain", SUCCEEDED(Analyze(dev, dec.GetImages(), dec.GetImageCount(), dec.GetMetadata(), want.data())));
        bool exact = dec.GetImageCount() == n, sums = true;
        for (size_t i = 0; i < n && exact; ++i) { exact = SameExact(got[i], want[i]); sums = sums && SameSums(got[i], want[i]); }
        CHECK("analyze bc7 == analyze of its decompress (exact fields)", exact);
        CHECK("analyze bc7 == analyze of its decompress (avg, variance)", sums);
        AnalyzeData one;
        CHECK("analyze single image", SUCCEEDED(Analyze(dev, *bc7.GetImage(2, 0, 0), one)) && SameExact(one, want[2]) && SameSums(one, want[2]));
        CHECK("analyze plausible", want[0].imageMin[0] >= 0.0f && want[0].imageMax[0] <= 1.0f && want[0].imageMax[0] > 0.9f && want[0].luminance > 0.5f);

        // AnalyzeBC: host image, resident chain
        std::vector<AnalyzeBCData> hist(n);
        DeviceScratchImage resident;
        CHECK("upload bc7", SUCCEEDED(resident.Upload(dev, bc7)));
        CHECK("analyze_bc resident", SUCCEEDED(AnalyzeBC(dev, resident, hist.data())));
        AnalyzeBCData h0;
        CHECK("analyze_bc host", SUCCEEDED(AnalyzeBC(dev, *bc7.GetImage(0, 0, 0), h0)) && std::memcmp(&h0, &hist[0], sizeof(h0)) == 0);
        uint64_t total = 0;
        for (int b = 0; b < 15; ++b) total += h0.blockHist[b];
        CHECK("analyze_bc counts every block once", h0.blocks == (W / 4) * (H / 4) && total == h0.blocks && hist[6].blocks == 1);
        // the encoder writes its mode as the lowest set bit: count modes on the CPU
        uint64_t cpu[9] = {};
        const Image* top = bc7.GetImage(0, 0, 0);
        for (size_t by = 0; by < H / 4; ++by)
            for (size_t bx = 0; bx < W / 4; ++bx)
            {
                const uint8_t b0 = top->pixels[by * top->rowPitch + bx * 16];
                int m = 8;
                for (int k = 0; k < 8; ++k) if (b0 & (1 << k)) { m = k; break; }
                ++cpu[m];
            }
        bool same = true;
        for (int b = 0; b < 9; ++b) same = same && cpu[b] == h0.blockHist[b];
        CHECK("analyze_bc == CPU count of the mode bits", same);
        std::vector<AnalyzeData> res(n);
        CHECK("analyze resident", SUCCEEDED(Analyze(dev, resident, res.data())) && SameExact(res[0], want[0]) && SameExact(res[6], want[6]));
        AnalyzeBCData bad;
        CHECK("analyze_bc rejects uncompressed", AnalyzeBC(dev, rgba, bad) == HRESULT_E_NOT_SUPPORTED);
    }

    // ---- ComputeMSE with flags, one side compressed ----
    {
        CHECK("bc1", SUCCEEDED(Compress(dev, rgba, DXGI_FORMAT_BC1_UNORM, TEX_COMPRESS_DEFAULT, 0.5f, bc1)));
        if (!bc1.GetImage(0, 0, 0)) { std::printf("%d failed (setup)\n", g_failed); return g_failed ? g_failed : 1; }
        const Image& c = *bc1.GetImage(0, 0, 0);
        ScratchImage dec;
        CHECK("decompress bc1", SUCCEEDED(Decompress(dev, c, DXGI_FORMAT_R32G32B32A32_FLOAT, dec)));
        if (g_failed || !dec.GetImage(0, 0, 0)) { std::printf("%d failed (setup)\n", g_failed); return g_failed ? g_failed : 1; }
        const Image& f = *dec.GetImage(0, 0, 0);
        const CMSE_FLAGS flags = CMSE_IGNORE_GREEN | CMSE_IMAGE1_X2_BIAS | CMSE_IMAGE2_X2_BIAS;
        float mse = 0, v[4] = {}, mse2 = 0, v2[4] = {};
        GetTransferBytes(dev, up, down, true);
        CHECK("mse flags, compressed image 2", SUCCEEDED(ComputeMSE(dev, rgba, c, mse, v, flags)));
        GetTransferBytes(dev, up, down, true);
        CHECK("mse: one upload per input, 32 bytes back", up == ImageBytes(rgba) + ImageBytes(c) && down == 32);
        // the same on the CPU from the decompressed floats
        double sum[4] = {};
        for (size_t y = 0; y < H; ++y)
            for (size_t x = 0; x < W; ++x)
            {
                const uint8_t* p = rgba.pixels + y * rgba.rowPitch + x * 4;
                const float* q = reinterpret_cast<const float*>(f.pixels + y * f.rowPitch) + x * 4;
                for (int k = 0; k < 4; ++k)
                {
                    const float a = float(p[k]) * (1.0f / 255.0f) * 2.0f + -1.0f, b = q[k] * 2.0f + -1.0f;
                    const double d = (k == 1) ? 0.0 : double(a) - double(b);
                    sum[k] += d * d;
                }
            }
        bool ok = v[1] == 0.0f && mse > 0.0f;
        for (int k = 0; k < 4; ++k) ok = ok && Close(v[k], float(sum[k] / double(W * H)), 2e-6);
        CHECK("mse flags == CPU restatement on the decompressed floats", ok);
        CHECK("mse flags, compressed image 1", SUCCEEDED(ComputeMSE(dev, c, rgba, mse2, v2, CMSE_IGNORE_GREEN | CMSE_IMAGE1_X2_BIAS | CMSE_IMAGE2_X2_BIAS)) &&
              Close(mse2, mse, 1e-6));
        DeviceScratchImage d1, d2;
        CHECK("upload pair", SUCCEEDED(d1.Upload(dev, base)) && SUCCEEDED(d2.Upload(dev, bc1)));
        CHECK("mse resident", SUCCEEDED(ComputeMSE(dev, d1, d2, mse2, v2, flags)) && Close(mse2, mse, 1e-6) && Close(v2[0], v[0], 1e-6));
        float m5 = 0, m6 = 0, v5[4], v6[4];
        CHECK("mse default flags close to the five-argument form", SUCCEEDED(ComputeMSE(dev, rgba, f, m5, v5)) && SUCCEEDED(ComputeMSE(dev, rgba, f, m6, v6, CMSE_DEFAULT)) &&
              Close(m6, m5, 1e-5));
        ScratchImage small;
        Fill(small, DXGI_FORMAT_R8G8B8A8_UNORM, 32, 48, 2);
        CHECK("mse size mismatch", ComputeMSE(dev, rgba, *small.GetImage(0, 0, 0), mse, v, CMSE_DEFAULT) == E_INVALIDARG);
    }

    // ---- Difference: _SRGB image 2, B8G8R8A8_UNORM out, against Convert -> difference -> Convert done step by step ----
    {
        ScratchImage other, result, floatB, map, want;
        Fill(other, DXGI_FORMAT_R8G8B8A8_UNORM_SRGB, W, H, 7);
        const Image& srgb = *other.GetImage(0, 0, 0);
        for (size_t y = 0; y < H; ++y)          // half the image far from image 1, half near
            for (size_t x = 0; x < W / 2; ++x) { uint8_t* p = srgb.pixels + y * srgb.rowPitch + x * 4; p[0] ^= 0x80; p[1] ^= 0x80; p[2] ^= 0x80; }
        const uint32_t color = 0xFF00FF; const float threshold = 0.25f;
        GetTransferBytes(dev, up, down, true);
        CHECK("difference", SUCCEEDED(Difference(dev, rgba, srgb, TEX_FILTER_DEFAULT, DXGI_FORMAT_B8G8R8A8_UNORM, color, threshold, result)));
        GetTransferBytes(dev, up, down, true);
        CHECK("difference: one upload per input, one download of the map", up == ImageBytes(rgba) + ImageBytes(srgb) && down == result.GetPixelsSize());
        CHECK("difference format", result.GetMetadata().format == DXGI_FORMAT_B8G8R8A8_UNORM && result.GetMetadata().width == W && result.GetMetadata().height == H);
        CHECK("convert image 2", SUCCEEDED(Convert(dev, srgb, DXGI_FORMAT_R32G32B32A32_FLOAT, TEX_FILTER_DEFAULT, TEX_THRESHOLD_DEFAULT, floatB)));
        if (g_failed || !floatB.GetImage(0, 0, 0) || !result.GetPixels()) { std::printf("%d failed (setup)\n", g_failed); return g_failed ? g_failed : 1; }
        map.Initialize2D(DXGI_FORMAT_R8G8B8A8_UNORM, W, H, 1, 1);
        const Image& fb = *floatB.GetImage(0, 0, 0);
        const Image& mp = *map.GetImage(0, 0, 0);
        const dxtex_image va = { rgba.width, rgba.height, int32_t(rgba.format), rgba.rowPitch, rgba.slicePitch, rgba.pixels };
        const dxtex_image vb = { fb.width, fb.height, int32_t(fb.format), fb.rowPitch, fb.slicePitch, fb.pixels };
        const dxtex_image vd = { mp.width, mp.height, int32_t(mp.format), mp.rowPitch, mp.slicePitch, mp.pixels };
        CHECK("difference step", SUCCEEDED(dxtex_difference(dev.Get(), &va, &vb, &vd, color, threshold)));
        CHECK("convert map", SUCCEEDED(Convert(dev, mp, DXGI_FORMAT_B8G8R8A8_UNORM, TEX_FILTER_DEFAULT, TEX_THRESHOLD_DEFAULT, want)));
        CHECK("difference == Convert -> difference -> Convert", want.GetPixels() && want.GetPixelsSize() == result.GetPixelsSize() &&
              std::memcmp(want.GetPixels(), result.GetPixels(), result.GetPixelsSize()) == 0);
        size_t coloured = 0, plain = 0;
        for (size_t i = 0; i < W * H; ++i)
        {
            const uint8_t* p = result.GetPixels() + i * 4;
            if (p[0] == 255 && p[1] == 0 && p[2] == 255 && p[3] == 255) ++coloured; else ++plain;
        }
        CHECK("difference takes both branches", coloured > W * H / 8 && plain > W * H / 8);
        // image 2 is linearised, image 1 is not: an identical sRGB pair differs
        ScratchImage same;
        CHECK("difference of an image with itself", SUCCEEDED(Difference(dev, rgba, rgba, TEX_FILTER_DEFAULT, DXGI_FORMAT_R8G8B8A8_UNORM, 0, threshold, same)));
        bool zero = same.GetPixels() != nullptr;
        for (size_t i = 0; same.GetPixels() && i < W * H && zero; ++i) zero = same.GetPixels()[i * 4] == 0 && same.GetPixels()[i * 4 + 3] == 255;
        CHECK("difference of an image with itself is zero with alpha 1", zero);
        // resident overload and a compressed image 1 (the map is made in R32G32B32A32_FLOAT)
        DeviceScratchImage d1, d2, dres;
        ScratchImage back, fromBc;
        CHECK("upload pair 2", SUCCEEDED(d1.Upload(dev, base)) && SUCCEEDED(d2.Upload(dev, other)));
        CHECK("difference resident", SUCCEEDED(Difference(dev, d1, d2, TEX_FILTER_DEFAULT, DXGI_FORMAT_B8G8R8A8_UNORM, color, threshold, dres)) &&
              SUCCEEDED(dres.Download(back)) && back.GetPixelsSize() == result.GetPixelsSize() &&
              std::memcmp(back.GetPixels(), result.GetPixels(), result.GetPixelsSize()) == 0);
        CHECK("difference compressed image 1", SUCCEEDED(Difference(dev, *bc1.GetImage(0, 0, 0), rgba, TEX_FILTER_DEFAULT, DXGI_FORMAT_R32G32B32A32_FLOAT, 0, threshold, fromBc)) &&
              fromBc.GetMetadata().format == DXGI_FORMAT_R32G32B32A32_FLOAT);
        const float* d = reinterpret_cast<const float*>(fromBc.GetPixels());
        bool small = fromBc.GetPixels() != nullptr;
        for (size_t i = 0; small && i < W * H; ++i) small = d[i * 4] >= 0.0f && d[i * 4] < 0.2f && d[i * 4 + 3] == 1.0f;
        CHECK("difference of BC1 against its source is small", small);
        ScratchImage tiny;
        Fill(tiny, DXGI_FORMAT_R8G8B8A8_UNORM, 32, 48, 3);
        CHECK("difference size mismatch", Difference(dev, rgba, *tiny.GetImage(0, 0, 0), TEX_FILTER_DEFAULT, DXGI_FORMAT_R8G8B8A8_UNORM, 0, threshold, same) == E_FAIL);
    }
    std::printf("%d failed\n", g_failed);
    return g_failed;
}
