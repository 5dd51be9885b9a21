// TEST INFRASTRUCTURE (tests/test_bc7_solid_cpu.py builds and runs it where the reference's sources are present): the property
// bc7_pre_kernel's election of one-colour subsets rests on, held against the reference's own D3DX_BC7::OptimizeOne, compiled in
// place with its private members exposed as tools/bc7_debug.cpp does.
//
// For a subset of n identical texels that starts from a given pair of quantised endpoints, OptimizeOne ends on the same endpoints
// whatever n is. Inputs: random (RGBA8 value, mode in {0, 1, 2, 3, 7}, start pair); half of the start pairs are the value itself,
// half the value moved by up to +-8 per channel and endpoint; both go through Quantize and FixEndpointPBits as Refine's do
// (:3428-3436), and the starting error is MapColors' over the n copies. For every subset size n that occurs in the mode's
// partition table the optimised endpoints are compared with those of the smallest size (3 texels with two subsets, 2 with three).
#define private public
#define protected public
#include "BC6HBC7.cpp"
#undef private
#undef protected

#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

static uint8_t moved(uint8_t v, int amp)
{
    const int d = amp ? int(rnd() % uint32_t(2 * amp + 1)) - amp : 0;
    const int r = int(v) + d;
    return uint8_t(r < 0 ? 0 : r > 255 ? 255 : r);
}

int main(int argc, char** argv)
{
    const int ninputs = argc > 1 ? atoi(argv[1]) : 20000;
    if (argc > 2) g_rng = uint32_t(strtoul(argv[2], nullptr, 0));
    static const int modes[5] = { 0, 1, 2, 3, 7 };

    // the subset sizes of the two- and the three-subset shapes (mode 0 sees the first 16 three-subset shapes only; all 64 is a superset)
    bool occurs[3][17] = {};
    for (int parts = 1; parts <= 2; ++parts)
        for (int s = 0; s < 64; ++s)
        {
            int n[3] = { 0, 0, 0 };
            for (int i = 0; i < 16; ++i) ++n[g_aPartitionTable[parts][s][i]];
            for (int p = 0; p <= parts; ++p) occurs[parts][n[p]] = true;
        }
    for (int parts = 1; parts <= 2; ++parts)
    {
        printf("subset sizes with %d subsets:", parts + 1);
        for (int n = 1; n <= 16; ++n) if (occurs[parts][n]) printf(" %d", n);
        printf("\n");
    }

    alignas(16) HDRColorA dummy[16] = {};
    D3DX_BC7 obj;
    long mismatches = 0, runs = 0, movedByTheSearch = 0;
    for (int t = 0; t < ninputs; ++t)
    {
        const int mode = modes[rnd() % 5];
        const int parts = D3DX_BC7::ms_aInfo[mode].uPartitions;
        LDRColorA v(uint8_t(rnd()), uint8_t(rnd()), uint8_t(rnd()), (rnd() & 1) ? uint8_t(255) : uint8_t(rnd()));
        const int amp = (t & 1) ? 8 : 0;
        LDREndPntPair start;
        for (int ch = 0; ch < 4; ++ch) { start.A[ch] = moved(v[ch], amp); start.B[ch] = moved(v[ch], amp); }

        D3DX_BC7::EncodeParams EP(dummy);
        EP.uMode = uint8_t(mode);
        LDREndPntPair q[3], org[3];
        for (int p = 0; p < 3; ++p)
        {
            q[p].A = D3DX_BC7::Quantize(start.A, D3DX_BC7::ms_aInfo[mode].RGBAPrecWithP);
            q[p].B = D3DX_BC7::Quantize(start.B, D3DX_BC7::ms_aInfo[mode].RGBAPrecWithP);
        }
        obj.FixEndpointPBits(&EP, q, org);

        LDRColorA colors[16];
        for (int i = 0; i < 16; ++i) colors[i] = v;
        LDREndPntPair base; bool haveBase = false;
        for (int n = 1; n <= 16; ++n)
        {
            if (!occurs[parts][n]) continue;
            const float orgErr = obj.MapColors(&EP, colors, size_t(n), 0, org[0], FLT_MAX);
            LDREndPntPair opt;
            obj.OptimizeOne(&EP, colors, size_t(n), 0, orgErr, org[0], opt);
            ++runs;
            if (!haveBase)
            {
                base = opt; haveBase = true;
                if (memcmp(&opt, &org[0], sizeof(opt)) != 0) ++movedByTheSearch;
                continue;
            }
            if (memcmp(&opt, &base, sizeof(opt)) != 0)
            {
                if (++mismatches <= 10)
                    printf("MISMATCH mode %d value %02x%02x%02x%02x start A %02x%02x%02x%02x B %02x%02x%02x%02x: %d texels end on A %02x%02x%02x%02x B %02x%02x%02x%02x, "
                           "the smallest subset on A %02x%02x%02x%02x B %02x%02x%02x%02x\n", mode, v.r, v.g, v.b, v.a,
                           org[0].A.r, org[0].A.g, org[0].A.b, org[0].A.a, org[0].B.r, org[0].B.g, org[0].B.b, org[0].B.a, n,
                           opt.A.r, opt.A.g, opt.A.b, opt.A.a, opt.B.r, opt.B.g, opt.B.b, opt.B.a,
                           base.A.r, base.A.g, base.A.b, base.A.a, base.B.r, base.B.g, base.B.b, base.B.a);
            }
        }
    }
    printf("%d inputs, %ld searches, %ld inputs whose search moved the endpoints: %ld mismatches\n", ninputs, runs, movedByTheSearch, mismatches);
    return mismatches ? 1 : 0;
}
