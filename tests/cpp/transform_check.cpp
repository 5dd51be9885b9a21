// Host build of dxtex_transform.h (texconv's per-texel TransformImage ops) for tests/test_transform_cpu.py, which compares it bit for bit
// with the numpy restatement in tests/transform_ref.py. Also runs the host layer's ParseSwizzleMask.
//
//   transform_check apply <op> <s0> <s1> <s2> <s3> <zeroMask> <oneMask> <colorKey hex> <unorm> <maxBits hex> <in.f32> <out.f32>
//       every float4 of in.f32 through xf_apply<op> (tone map: M = m * m with m = the float of maxBits), written to out.f32
//   transform_check maxlum <in.f32>        the tone map's running maximum over the float4s of in.f32, as hex bits
//   transform_check mask <MASK>            ParseSwizzleMask: "s0 s1 s2 s3 z0 z1 z2 z3 o0 o1 o2 o3", or "bad"
#include "dxtex_transform.h"
#include "../../directxtex_amd/host/DirectXTexAMD.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dxtex;

static std::vector<float> read_floats(const char* path)
{
    std::vector<float> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) return v;
    float x;
    while (std::fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

template<uint32_t OP>
static void run(std::vector<float>& px, const XformArgs& a, float M)
{
    for (size_t i = 0; i + 3 < px.size(); i += 4)
    {
        float c[4] = { px[i], px[i + 1], px[i + 2], px[i + 3] };
        xf_apply<OP>(c, a, M);
        for (int k = 0; k < 4; ++k) px[i + k] = c[k];
    }
}

int main(int argc, char** argv)
{
    if (argc == 3 && !std::strcmp(argv[1], "mask"))
    {
        DirectXTexAMD::TexTransform t;
        if (!DirectXTexAMD::ParseSwizzleMask(argv[2], t)) { std::printf("bad\n"); return 0; }
        std::printf("%u %u %u %u %u %u %u %u %u %u %u %u\n", t.swizzle[0], t.swizzle[1], t.swizzle[2], t.swizzle[3], t.zero[0], t.zero[1], t.zero[2], t.zero[3],
                    t.one[0], t.one[1], t.one[2], t.one[3]);
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "maxlum"))
    {
        const std::vector<float> px = read_floats(argv[2]);
        uint32_t m = 0;
        for (size_t i = 0; i + 3 < px.size(); i += 4) { const uint32_t b = xf_lum_bits(px[i], px[i + 1], px[i + 2]); if (b > m) m = b; }
        std::printf("%08x\n", m);
        return 0;
    }
    if (argc != 14 || std::strcmp(argv[1], "apply")) { std::fprintf(stderr, "usage: see the header of transform_check.cpp\n"); return 2; }
    const uint32_t op = uint32_t(std::strtoul(argv[2], nullptr, 10));
    XformArgs a = {};
    for (int k = 0; k < 4; ++k) a.swz[k] = uint32_t(std::strtoul(argv[3 + k], nullptr, 10));
    a.zero = uint32_t(std::strtoul(argv[7], nullptr, 10));
    a.one = uint32_t(std::strtoul(argv[8], nullptr, 10));
    xf_color_key_value(uint32_t(std::strtoul(argv[9], nullptr, 16)), a.key);
    a.unorm = std::atoi(argv[10]);
    const float m = xf_float(uint32_t(std::strtoul(argv[11], nullptr, 16)));
    const float M = m * m;
    std::vector<float> px = read_floats(argv[12]);
    switch (op)
    {
    case XFORM_SWIZZLE: run<XFORM_SWIZZLE>(px, a, M); break;
    case XFORM_TONEMAP: run<XFORM_TONEMAP>(px, a, M); break;
    case XFORM_COLOR_KEY: run<XFORM_COLOR_KEY>(px, a, M); break;
    case XFORM_INVERT_Y: run<XFORM_INVERT_Y>(px, a, M); break;
    case XFORM_RECONSTRUCT_Z: run<XFORM_RECONSTRUCT_Z>(px, a, M); break;
    default: return 2;
    }
    FILE* f = std::fopen(argv[13], "wb");
    if (!f || std::fwrite(px.data(), sizeof(float), px.size(), f) != px.size()) return 1;
    std::fclose(f);
    return 0;
}
