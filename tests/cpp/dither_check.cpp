// Host run of dxtex_dither.h (the per-texel steps and the speculate-and-merge scheme of the GPU's error-diffusion kernel) on an
// R32G32B32A32_FLOAT image whose conversion to the destination is the identity, for tests/test_dither_cpu.py:
//   dither_check <in.f32> <width> <height> <dst format> <segment length | 0> <out.bin>
// segment length 0 runs the plain serial chain: StoreScanlineDither's loop as written (DirectXTexConvert.cpp:4049-4127 and the
// STORE_SCANLINE body), with its own (width + 2)-entry error buffer and index / delta arithmetic; any other length runs
// dither_row_segmented and the error slots of dither_slot. Prints "rerun <texels>". The output has a tight row pitch.
#include "dxtex_dither.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dxtex;

int main(int argc, char** argv)
{
    if (argc != 7) { std::fprintf(stderr, "usage: dither_check in.f32 width height dstFormat segLen out.bin\n"); return 2; }
    const uint32_t w = uint32_t(std::atoi(argv[2])), h = uint32_t(std::atoi(argv[3]));
    const int fmt = std::atoi(argv[4]);
    const uint32_t segLen = uint32_t(std::atoi(argv[5]));
    const DitherSpec s = dither_spec(fmt);
    if (!s.valid || !w || !h) { std::fprintf(stderr, "format %d has no dithered store\n", fmt); return 2; }
    std::vector<float> src(size_t(w) * h * 4);
    FILE* f = std::fopen(argv[1], "rb");
    if (!f || std::fread(src.data(), sizeof(float), src.size(), f) != src.size()) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::fclose(f);
    const size_t pitch = size_t(w) * s.bytes;
    std::vector<uint8_t> out(pitch * h, 0);
    const float threshold = 0.5f;
    uint64_t rerun = 0;
    const F4 zero = { { 0.0f, 0.0f, 0.0f, 0.0f } };
    if (segLen == 0)
    {
        std::vector<F4> errors(w + 2, zero), row(w);
        for (uint32_t y = 0; y < h; ++y)
        {
            for (uint32_t i = 0; i < w; ++i)
                for (int c = 0; c < 4; ++c) row[i].v[c] = src[(size_t(y) * w + i) * 4 + c] + errors[i + 1].v[c];
            for (auto& e : errors) e = zero;
            F4 vError = zero;
            for (uint32_t i = 0; i < w; ++i)
            {
                const ptrdiff_t index = (y & 1) ? ptrdiff_t(w - i - 1) : ptrdiff_t(i);
                const ptrdiff_t delta = (y & 1) ? -2 : 0;
                const F4 pre = dither_pre(s, row[index].v[0], row[index].v[1], row[index].v[2], row[index].v[3]);
                F4 e;
                dither_write(out.data() + y * pitch, uint32_t(index), s.bytes, dither_diffuse(s, pre, vError, e, threshold));
                for (int c = 0; c < 4; ++c)
                {
                    errors[index - delta].v[c] = 0.1875f * e.v[c] + errors[index - delta].v[c];
                    errors[index + 1].v[c] = 0.3125f * e.v[c] + errors[index + 1].v[c];
                    errors[index + 2 + delta].v[c] = 0.0625f * e.v[c] + errors[index + 2 + delta].v[c];
                }
                vError = dither_next_state(e);
            }
        }
    }
    else
    {
        std::vector<F4> slot(w, zero), pre(w), err(w), in(w), pending(w);
        for (uint32_t y = 0; y < h; ++y)
        {
            const bool odd = (y & 1) != 0;
            for (uint32_t x = 0; x < w; ++x)
            {
                float v[4];
                for (int c = 0; c < 4; ++c) v[c] = src[(size_t(y) * w + x) * 4 + c] + slot[x].v[c];
                pre[odd ? w - 1 - x : x] = dither_pre(s, v[0], v[1], v[2], v[3]);
            }
            uint8_t* drow = out.data() + y * pitch;
            rerun += dither_row_segmented(s, pre.data(), err.data(), w, segLen, in.data(), pending.data(), threshold,
                                          [&](uint32_t p, uint64_t word) { dither_write(drow, odd ? w - 1 - p : p, s.bytes, word); });
            for (uint32_t x = 0; x < w; ++x) slot[x] = dither_slot(err.data(), odd ? w - 1 - x : x, w);
        }
    }
    f = std::fopen(argv[6], "wb");
    if (!f || std::fwrite(out.data(), 1, out.size(), f) != out.size()) { std::fprintf(stderr, "cannot write %s\n", argv[6]); return 2; }
    std::fclose(f);
    std::printf("rerun %llu\n", (unsigned long long)rerun);
    return 0;
}
