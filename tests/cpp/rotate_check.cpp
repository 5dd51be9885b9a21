// Host build of dxtex_rotate.h (texconv's HDR colour rotation) for tests/test_rotate_cpu.py, which compares it bit for bit with the numpy
// restatement in tests/rotate_ref.py.
//
//   rotate_check <rotate 1..8> <nits> <in.f32> <out.f32>
//       every float4 of in.f32 through rc_apply<curve of the operation> with the operation's matrix, written to out.f32 (alpha is moved)
#include "dxtex_rotate.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace dxtex;

template<int CURVE>
static void run(std::vector<float>& px, const RotateArgs& a)
{
    for (size_t i = 0; i + 3 < px.size(); i += 4)
    {
        float c[4] = { px[i], px[i + 1], px[i + 2], px[i + 3] };
        rc_apply<CURVE>(c, a);
        for (int k = 0; k < 3; ++k) px[i + k] = c[k];
    }
}

int main(int argc, char** argv)
{
    if (argc != 5) { std::fprintf(stderr, "usage: rotate_check <rotate 1..8> <nits> <in.f32> <out.f32>\n"); return 2; }
    RotateArgs a = {};
    int curve = 0;
    const float nits = std::strtof(argv[2], nullptr);
    if (!rotate_resolve(uint32_t(std::strtoul(argv[1], nullptr, 10)), nits, a, curve) || !rotate_nits_valid(nits)) return 2;
    std::vector<float> px;
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) return 1;
    float x;
    while (std::fread(&x, sizeof(x), 1, f) == 1) px.push_back(x);
    std::fclose(f);
    if (curve == ROTATE_CURVE_NONE) run<ROTATE_CURVE_NONE>(px, a);
    else if (curve == ROTATE_CURVE_TO_ST2084) run<ROTATE_CURVE_TO_ST2084>(px, a);
    else run<ROTATE_CURVE_FROM_ST2084>(px, a);
    f = std::fopen(argv[4], "wb");
    if (!f || std::fwrite(px.data(), sizeof(float), px.size(), f) != px.size()) return 1;
    std::fclose(f);
    return 0;
}
