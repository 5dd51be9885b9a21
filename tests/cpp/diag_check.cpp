// Host build of dxtex_diag.h for the CPU suite (tests/test_diag_cpu.py): the rules diag.hip's kernels apply per texel and per block,
// run on files of raw values so that numpy can compare them bit for bit with tests/diag_ref.py.
//
//   diag_check texel IN.f32 OUT.u32                 rows of 4 floats -> rows of (dg_lum_bits, dg_key r, g, b, a)
//   diag_check minmax IN.u32 OUT.f32                rows of (maxKey, minKeyInv) cells -> rows of (dg_max_of, dg_min_of)
//   diag_check diff COLOR THRESHOLD A.f32 B.f32 OUT.f32   dg_difference per row of 4 floats (COLOR in hex, THRESHOLD as float bits in hex)
//   diag_check mse SRGB BIAS IN.f32 OUT.f32         dg_mse_prepare per row of 4 floats
//   diag_check bc FORMAT IN.bin OUT.i32             16-byte records (a block's head, zero padded) -> rows of (bin0, bin1)
//   diag_check modes                                prints "byte bc6h_bin bc7_bin" for all 256 values of byte 0
#include "dxtex_diag.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace dxtex;

template<class T>
static std::vector<T> read_all(const char* path)
{
    std::vector<T> v;
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    v.resize(size_t(n) / sizeof(T));
    if (!v.empty() && fread(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "short read of %s\n", path); exit(2); }
    fclose(f);
    return v;
}

template<class T>
static void write_all(const char* path, const std::vector<T>& v)
{
    FILE* f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), f);
    fclose(f);
}

int main(int argc, char** argv)
{
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "texel" && argc == 4)
    {
        const std::vector<float> in = read_all<float>(argv[2]);
        std::vector<uint32_t> out;
        for (size_t i = 0; i + 4 <= in.size(); i += 4)
        {
            out.push_back(dg_lum_bits(in[i], in[i + 1], in[i + 2]));
            for (int c = 0; c < 4; ++c) out.push_back(dg_key(in[i + c]));
        }
        write_all(argv[3], out);
        return 0;
    }
    if (cmd == "minmax" && argc == 4)
    {
        const std::vector<uint32_t> in = read_all<uint32_t>(argv[2]);
        std::vector<float> out;
        for (size_t i = 0; i + 2 <= in.size(); i += 2) { out.push_back(dg_max_of(in[i])); out.push_back(dg_min_of(in[i + 1])); }
        write_all(argv[3], out);
        return 0;
    }
    if (cmd == "diff" && argc == 7)
    {
        const uint32_t color = uint32_t(strtoul(argv[2], nullptr, 16));
        const float threshold = dg_float(uint32_t(strtoul(argv[3], nullptr, 16)));
        const std::vector<float> a = read_all<float>(argv[4]), b = read_all<float>(argv[5]);
        std::vector<float> out(a.size());
        float key[4];
        dg_diff_color(color, key);
        for (size_t i = 0; i + 4 <= a.size(); i += 4)
        {
            float c[4] = { a[i], a[i + 1], a[i + 2], a[i + 3] };
            const float d[4] = { b[i], b[i + 1], b[i + 2], b[i + 3] };
            dg_difference(c, d, color, key, threshold);
            memcpy(&out[i], c, sizeof(c));
        }
        write_all(argv[6], out);
        return 0;
    }
    if (cmd == "mse" && argc == 6)
    {
        const bool srgb = atoi(argv[2]) != 0, bias = atoi(argv[3]) != 0;
        std::vector<float> v = read_all<float>(argv[4]);
        for (size_t i = 0; i + 4 <= v.size(); i += 4)
        {
            float c[4] = { v[i], v[i + 1], v[i + 2], v[i + 3] };
            dg_mse_prepare(c, srgb, bias);
            memcpy(&v[i], c, sizeof(c));
        }
        write_all(argv[5], v);
        return 0;
    }
    if (cmd == "bc" && argc == 5)
    {
        const int format = atoi(argv[2]);
        const std::vector<uint8_t> in = read_all<uint8_t>(argv[3]);
        std::vector<int32_t> out;
        for (size_t i = 0; i + 16 <= in.size(); i += 16)
        {
            int b0, b1;
            dg_bc_bins(format, &in[i], b0, b1);
            out.push_back(b0); out.push_back(b1);
        }
        write_all(argv[4], out);
        return 0;
    }
    if (cmd == "modes")
    {
        for (uint32_t b = 0; b < 256; ++b) printf("%u %d %d\n", b, dg_bc6h_bin(b), dg_bc7_bin(b));
        return 0;
    }
    fprintf(stderr, "usage: diag_check texel|minmax|diff|mse|bc|modes ... (see the head of tests/cpp/diag_check.cpp)\n");
    return 1;
}
