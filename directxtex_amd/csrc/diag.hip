// texdiag's diagnostics on the GPU, gfx950:
//
//   Analyze      (Texdiag/texdiag.cpp:698-787)        analyze_kernel, analyze_var_kernel
//   ComputeMSE_  (DirectXTexMisc.cpp:27-176)          mse_flags_kernel (every CMSE_FLAGS bit; mse_kernel in scanline.hip stays the plain form)
//   AnalyzeBC    (Texdiag/texdiag.cpp:906-1226)       bc_hist_kernel
//   Difference   (Texdiag/texdiag.cpp:1285-1309)      difference_kernel
//
// Three reductions and one per-texel map, all bound by memory bandwidth. The reductions share one shape: a workgroup strides over rows
// (grid y) and over the quads or texels of a row (grid x), every lane keeps its own partial result, a wave combines its lanes with
// shuffles, the four waves of a workgroup meet in LDS, and the workgroup issues one global atomic per quantity. Sums are fp64 (their
// last bits depend on the order the workgroups arrive in); minimum, maximum, luminance and the counts are integers and exact.
// Formats of DXTEX_QUAD_FORMATS are read four texels at a time through 16-byte loads when the image's pointer and pitch allow it.
// The per-texel rules are in dxtex_diag.h.
#include "dxtex_kernels.h"
#include "dxtex_store.h"
#include "dxtex_quad.h"
#include "dxtex_diag.h"
#include <algorithm>

namespace dxtex
{
namespace
{
// ---- reading an image ------------------------------------------------------------------------------------------------------------------
// The four texels of the quad at p (qb = quad_bytes(format), never 0 here). load_texel sees the format as a compile-time constant and
// a register image of the quad, as in convert_quad_kernel.
__device__ __forceinline__ void load_quad_texels(const uint8_t* p, int format, uint32_t qb, Texel (&t)[4])
{
    uint32_t q[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) q[k] = 0u;
    load_quad<16>(q, p, qb);
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) { t[k].r = t[k].g = t[k].b = 0.0f; t[k].a = 1.0f; }
    switch (format)
    {
#define DXTEX_QCASE(F, QB) case F: { _Pragma("unroll") for (uint32_t k = 0; k < 4u; ++k) t[k] = load_texel(reinterpret_cast<const uint8_t*>(q), k, F); } break;
        DXTEX_QUAD_FORMATS(DXTEX_QCASE)
#undef DXTEX_QCASE
    default: break;
    }
}

// f(texel) for every texel of v that this lane owns. qb = the bytes of a quad when v may be read in quads (its format is a quad format,
// pixels and rowPitch are multiples of 16), else 0. The width / 4 whole quads of a row go four texels a lane; the up to three texels
// after them - or the whole row when qb is 0 - go one texel a lane.
template<class F>
__device__ __forceinline__ void for_each_texel(const ImgView& v, uint32_t qb, F&& f)
{
    const uint32_t quads = qb ? v.width / 4u : 0u;
    const uint32_t lane = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    for (uint32_t y = blockIdx.y; y < v.height; y += gridDim.y)
    {
        const uint8_t* row = v.pixels + uint64_t(y) * v.rowPitch;
        for (uint32_t q = lane; q < quads; q += step)
        {
            Texel t[4];
            load_quad_texels(row + uint64_t(q) * qb, v.format, qb, t);
#pragma unroll
            for (int k = 0; k < 4; ++k) f(t[k]);
        }
        for (uint64_t x = uint64_t(quads) * 4u + lane; x < v.width; x += step) f(load_texel(row, uint32_t(x), v.format));
    }
}

// ---- combining lanes ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, uint32_t(__shfl_xor(int(v), o)));
    return v;
}

// ---- Analyze -------------------------------------------------------------------------------------------------------------------------------
// Pass 1: per channel the maximum of dg_key(v) and of ~dg_key(v) over the values that are not NaN (dxtex_diag.h), the fp64 sum of every
// value and the number of values that are not finite; the maximum of dg_lum_bits over the texels.
__global__ void __launch_bounds__(256) analyze_kernel(ImgView src, uint32_t qb, AnalyzeAcc* acc)
{
    __shared__ uint32_t sMax[4][4], sMin[4][4], sLum[4];
    __shared__ double sSum[4][4];
    __shared__ unsigned long long sSpec[4][4];
    uint32_t maxKey[4] = { 0u, 0u, 0u, 0u }, minInv[4] = { 0u, 0u, 0u, 0u }, lum = 0u;
    double sum[4] = { 0.0, 0.0, 0.0, 0.0 };
    unsigned long long spec[4] = { 0ull, 0ull, 0ull, 0ull };
    for_each_texel(src, qb, [&](const Texel& t)
    {
        const float c[4] = { t.r, t.g, t.b, t.a };
        lum = max(lum, dg_lum_bits(t.r, t.g, t.b));
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            if (!dg_nan(c[k])) { const uint32_t key = dg_key(c[k]); maxKey[k] = max(maxKey[k], key); minInv[k] = max(minInv[k], ~key); }
            if (!dg_finite(c[k])) ++spec[k];
            sum[k] += double(c[k]);
        }
    });
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    lum = wave_max(lum);
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        maxKey[k] = wave_max(maxKey[k]); minInv[k] = wave_max(minInv[k]);
        sum[k] = wave_sum(sum[k]); spec[k] = wave_sum(spec[k]);
    }
    if (lane == 0)
    {
        sLum[wave] = lum;
#pragma unroll
        for (int k = 0; k < 4; ++k) { sMax[wave][k] = maxKey[k]; sMin[wave][k] = minInv[k]; sSum[wave][k] = sum[k]; sSpec[wave][k] = spec[k]; }
    }
    __syncthreads();
    const uint32_t k = threadIdx.x;
    if (k < 4u)
    {
        const uint32_t mx = max(max(sMax[0][k], sMax[1][k]), max(sMax[2][k], sMax[3][k]));
        const uint32_t mn = max(max(sMin[0][k], sMin[1][k]), max(sMin[2][k], sMin[3][k]));
        const unsigned long long sp = sSpec[0][k] + sSpec[1][k] + sSpec[2][k] + sSpec[3][k];
        if (mx) atomicMax(&acc->maxKey[k], mx);
        if (mn) atomicMax(&acc->minKeyInv[k], mn);
        if (sp) atomicAdd(&acc->specials[k], sp);
        atomicAdd(&acc->sum[k], sSum[0][k] + sSum[1][k] + sSum[2][k] + sSum[3][k]);
    }
    if (k == 4u)
    {
        const uint32_t l = max(max(sLum[0], sLum[1]), max(sLum[2], sLum[3]));
        if (l) atomicMax(&acc->lumBits, l);
    }
}

// Pass 2: sum of (v - avgf)^2 with avgf = float(sum / N) from pass 1's cell (the stream orders the passes): the subtraction in fp32 as
// the reference does it, the square and the sum in fp64.
__global__ void __launch_bounds__(256) analyze_var_kernel(ImgView src, uint32_t qb, AnalyzeAcc* acc)
{
    __shared__ double sSum[4][4];
    const double n = double(src.width) * double(src.height);
    const float avg[4] = { float(acc->sum[0] / n), float(acc->sum[1] / n), float(acc->sum[2] / n), float(acc->sum[3] / n) };
    double sum[4] = { 0.0, 0.0, 0.0, 0.0 };
    for_each_texel(src, qb, [&](const Texel& t)
    {
        const float d[4] = { t.r - avg[0], t.g - avg[1], t.b - avg[2], t.a - avg[3] };
#pragma unroll
        for (int k = 0; k < 4; ++k) sum[k] += double(d[k]) * double(d[k]);
    });
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < 4; ++k) sum[k] = wave_sum(sum[k]);
    if (lane == 0) { sSum[wave][0] = sum[0]; sSum[wave][1] = sum[1]; sSum[wave][2] = sum[2]; sSum[wave][3] = sum[3]; }
    __syncthreads();
    if (threadIdx.x < 4u)
        atomicAdd(&acc->variance[threadIdx.x], sSum[0][threadIdx.x] + sSum[1][threadIdx.x] + sSum[2][threadIdx.x] + sSum[3][threadIdx.x]);
}

// ---- ComputeMSE with flags --------------------------------------------------------------------------------------------------------------
// flags = the caller's CMSE_FLAGS with the bits the formats imply already or-ed in. qa / qb: both non-zero (quads on both sides) or both 0.
__global__ void __launch_bounds__(256) mse_flags_kernel(ImgView a, ImgView b, uint32_t qa, uint32_t qb, uint32_t flags, double* out)
{
    __shared__ double part[4][4];
    double s[4] = { 0.0, 0.0, 0.0, 0.0 };
    const bool srgbA = (flags & DG_CMSE_IMAGE1_SRGB) != 0, srgbB = (flags & DG_CMSE_IMAGE2_SRGB) != 0;
    const bool biasA = (flags & DG_CMSE_IMAGE1_X2_BIAS) != 0, biasB = (flags & DG_CMSE_IMAGE2_X2_BIAS) != 0;
    const auto texel = [&](const Texel& p, const Texel& q)
    {
        float u[4] = { p.r, p.g, p.b, p.a }, v[4] = { q.r, q.g, q.b, q.a };
        dg_mse_prepare(u, srgbA, biasA);
        dg_mse_prepare(v, srgbB, biasB);
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            const float d = (flags & (DG_CMSE_IGNORE_RED << k)) ? 0.0f : u[k] - v[k];
            s[k] += double(d) * double(d);
        }
    };
    const uint32_t quads = qa ? a.width / 4u : 0u;
    const uint32_t lane0 = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    for (uint32_t y = blockIdx.y; y < a.height; y += gridDim.y)
    {
        const uint8_t* rowA = a.pixels + uint64_t(y) * a.rowPitch;
        const uint8_t* rowB = b.pixels + uint64_t(y) * b.rowPitch;
        for (uint32_t q = lane0; q < quads; q += step)
        {
            Texel ta[4], tb[4];
            load_quad_texels(rowA + uint64_t(q) * qa, a.format, qa, ta);
            load_quad_texels(rowB + uint64_t(q) * qb, b.format, qb, tb);
#pragma unroll
            for (int k = 0; k < 4; ++k) texel(ta[k], tb[k]);
        }
        for (uint64_t x = uint64_t(quads) * 4u + lane0; x < a.width; x += step)
            texel(load_texel(rowA, uint32_t(x), a.format), load_texel(rowB, uint32_t(x), b.format));
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
    if (lane == 0) { part[wave][0] = s[0]; part[wave][1] = s[1]; part[wave][2] = s[2]; part[wave][3] = s[3]; }
    __syncthreads();
    if (threadIdx.x < 4u)
        atomicAdd(&out[threadIdx.x], part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// ---- AnalyzeBC ---------------------------------------------------------------------------------------------------------------------------
// A block per lane, a histogram per workgroup in LDS, then one atomic per bin that the workgroup touched. The classifier reads a few
// bytes of the head of each block with byte loads, so any pointer and pitch will do.
__global__ void __launch_bounds__(256) bc_hist_kernel(ImgView src, uint32_t blocksX, uint32_t blocksY, uint32_t blockBytes, unsigned long long* hist)
{
    __shared__ uint32_t bins[kBcHistBins];
    if (threadIdx.x < kBcHistBins) bins[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t by = blockIdx.y; by < blocksY; by += gridDim.y)
    {
        const uint8_t* row = src.pixels + uint64_t(by) * src.rowPitch;
        for (uint32_t bx = blockIdx.x * 256u + threadIdx.x; bx < blocksX; bx += gridDim.x * 256u)
        {
            int b0, b1;
            dg_bc_bins(src.format, row + uint64_t(bx) * blockBytes, b0, b1);
            if (b0 >= 0) atomicAdd(&bins[b0], 1u);
            if (b1 >= 0) atomicAdd(&bins[b1], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kBcHistBins && bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)bins[threadIdx.x]);
}

// ---- Difference --------------------------------------------------------------------------------------------------------------------------
// dst = the difference map of a (any loadable format) and b (R32G32B32A32_FLOAT), stored as dst.format. qb = the bytes of a quad of
// a.format when a, b and dst may all be accessed in quads and dst.format == a.format, else 0.
__global__ void __launch_bounds__(256) difference_kernel(ImgView a, ImgView b, ImgView dst, uint32_t qb, uint32_t diffColor, float threshold)
{
    float color[4];
    dg_diff_color(diffColor, color);
    const auto texel = [&](Texel t, const float4& o)
    {
        float c[4] = { t.r, t.g, t.b, t.a };
        const float d[4] = { o.x, o.y, o.z, o.w };
        dg_difference(c, d, diffColor, color, threshold);
        return Texel{ c[0], c[1], c[2], c[3] };
    };
    const uint32_t quads = qb ? a.width / 4u : 0u;
    const uint32_t lane0 = blockIdx.x * 256u + threadIdx.x, step = gridDim.x * 256u;
    for (uint32_t y = blockIdx.y; y < a.height; y += gridDim.y)
    {
        const uint8_t* rowA = a.pixels + uint64_t(y) * a.rowPitch;
        const float4* rowB = reinterpret_cast<const float4*>(b.pixels + uint64_t(y) * b.rowPitch);
        uint8_t* rowD = dst.pixels + uint64_t(y) * dst.rowPitch;
        for (uint32_t q = lane0; q < quads; q += step)
        {
            Texel t[4];
            load_quad_texels(rowA + uint64_t(q) * qb, a.format, qb, t);
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = texel(t[k], rowB[uint64_t(q) * 4u + k]);
            uint32_t out[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) out[k] = 0u;
            switch (dst.format)
            {
#define DXTEX_QCASE(F, QB) case F: { _Pragma("unroll") for (uint32_t k = 0; k < 4u; ++k) store_texel(reinterpret_cast<uint8_t*>(out), k, F, t[k]); } break;
                DXTEX_QUAD_FORMATS(DXTEX_QCASE)
#undef DXTEX_QCASE
            default: break;
            }
            store_quad<16>(rowD + uint64_t(q) * qb, out, qb);
        }
        for (uint64_t x = uint64_t(quads) * 4u + lane0; x < a.width; x += step)
            store_texel(rowD, uint32_t(x), dst.format, texel(load_texel(rowA, uint32_t(x), a.format), rowB[x]));
    }
}

// qb for a view: the bytes of a quad when the format is a quad format and every row starts on a 16-byte boundary
uint32_t view_quad_bytes(const ImgView& v)
{
    const uint32_t qb = quad_bytes(v.format);
    return (qb && ((reinterpret_cast<uintptr_t>(v.pixels) | v.rowPitch) & 15u) == 0) ? qb : 0u;
}

// About 1024 workgroups (four per compute unit): every workgroup ends in a handful of atomics on the same few words, which the memory
// system serialises, so their number - not the streaming - is what a finer grid pays for (profiles/diag.md has the figures).
// `units` = what a lane takes per step in x (quads, texels or blocks).
dim3 reduce_grid(uint32_t units, uint32_t rows)
{
    const uint32_t gx = std::min<uint32_t>((std::max<uint32_t>(units, 1u) + 255u) / 256u, 64u);
    return dim3(gx, std::min<uint32_t>(rows, std::max<uint32_t>(1u, 1024u / gx)));
}
} // namespace

#define DXTEX_MARK(NAME) do { if (marks) marks->mark(NAME); } while (0)

hipError_t launch_analyze(const ImgView& src, AnalyzeAcc* acc, hipStream_t stream, KernelMarks* marks)
{
    if (!src.width || !src.height) return hipSuccess;
    const uint32_t qb = view_quad_bytes(src);
    const dim3 grid = reduce_grid(qb ? std::max<uint32_t>(src.width / 4u, src.width % 4u) : src.width, src.height);
    DXTEX_MARK("analyze");
    hipLaunchKernelGGL(analyze_kernel, grid, dim3(256), 0, stream, src, qb, acc);
    DXTEX_MARK("analyze_var");
    hipLaunchKernelGGL(analyze_var_kernel, grid, dim3(256), 0, stream, src, qb, acc);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_mse_flags(const ImgView& a, const ImgView& b, uint32_t flags, double* out4, hipStream_t stream, KernelMarks* marks)
{
    hipError_t e = hipMemsetAsync(out4, 0, 4 * sizeof(double), stream);
    if (e != hipSuccess) return e;
    if (!a.width || !a.height) return hipSuccess;
    flags |= dg_mse_format_flags(a.format, false) | dg_mse_format_flags(b.format, true);
    uint32_t qa = view_quad_bytes(a), qb = view_quad_bytes(b);
    if (!qa || !qb) qa = qb = 0u;
    const dim3 grid = reduce_grid(qa ? std::max<uint32_t>(a.width / 4u, a.width % 4u) : a.width, a.height);
    DXTEX_MARK("mse_flags");
    hipLaunchKernelGGL(mse_flags_kernel, grid, dim3(256), 0, stream, a, b, qa, qb, flags, out4);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_bc_hist(const ImgView& src, unsigned long long* hist, hipStream_t stream, KernelMarks* marks)
{
    const uint32_t blockBytes = dg_bc_block_bytes(src.format);
    if (!blockBytes) return hipErrorInvalidValue;
    if (!src.width || !src.height) return hipSuccess;
    const uint32_t blocksX = uint32_t((uint64_t(src.width) + 3u) / 4u), blocksY = uint32_t((uint64_t(src.height) + 3u) / 4u);
    DXTEX_MARK("bc_hist");
    hipLaunchKernelGGL(bc_hist_kernel, reduce_grid(blocksX, blocksY), dim3(256), 0, stream, src, blocksX, blocksY, blockBytes, hist);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_difference(const ImgView& a, const ImgView& b, const ImgView& dst, uint32_t diffColor, float threshold, hipStream_t stream,
                             KernelMarks* marks)
{
    if (!a.width || !a.height) return hipSuccess;
    if (b.format != FMT_R32G32B32A32_FLOAT || ((reinterpret_cast<uintptr_t>(b.pixels) | b.rowPitch) & 15u)) return hipErrorInvalidValue;
    uint32_t qb = view_quad_bytes(a);
    if (dst.format != a.format || view_quad_bytes(dst) != qb) qb = 0u;
    const uint32_t units = qb ? std::max<uint32_t>(a.width / 4u, a.width % 4u) : a.width;
    // a map, not a reduction: about 8192 workgroups, as launch_transform and convert_quad launch
    const uint32_t gx = std::min<uint32_t>((units + 255u) / 256u, 64u);
    const dim3 grid(gx, std::min<uint32_t>(a.height, std::max<uint32_t>(1u, 8192u / gx)));
    DXTEX_MARK("difference");
    hipLaunchKernelGGL(difference_kernel, grid, dim3(256), 0, stream, a, b, dst, qb, diffColor, threshold);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
#undef DXTEX_MARK
} // namespace dxtex
