// Scanline-layer kernels for gfx950: Convert, Resize / GenerateMipMaps filters, ComputeMSE.
//
//   reference                                                             here
//   ConvertCustom (DirectXTexConvert.cpp:4804-4913), no-dither and         convert_kernel / convert_quad_kernel
//     ordered-dither branches (StoreScanlineDither without an error buffer)
//   ConvertCustom's error-diffusion branch (:4820-4852)                   convert_diffuse_kernel (one workgroup per image)
//   Resize{Point,Box,Linear,Cubic,Triangle}Filter (DirectXTexResize.cpp:255-803) and
//   Generate2DMips{Point,Box,Linear,Cubic,Triangle}Filter (DirectXTexMipmaps.cpp:907-1602)   resize_*_kernel
//   ComputeMSE_ (DirectXTexMisc.cpp:27-176)                                mse_kernel
//   ComputeNMap (DirectXTexNormalMaps.cpp:77-240)                          nmap_kernel
//   TransformImage / EvaluateImage (DirectXTexMisc.cpp:179-263) with       transform_kernel<op>, tonemap_max_kernel
//     texconv's swizzle / tone-map / colour-key / invert-Y / reconstruct-Z lambdas
//   CopyRectangle (DirectXTexMisc.cpp:275-381)                             copy_rect_kernel (a batch of rectangles per launch)
//   texassemble's merge lambda (Texassemble/texassemble.cpp:2236-2268)     merge_kernel
//
// The reference walks scanlines through a float4 row buffer (LoadScanline -> filter -> StoreScanline). Here every
// lane owns one destination texel and reads the source texels it needs straight from HBM/L2 with LoadScanline's
// per-texel arithmetic; nothing is staged, so a level costs one read of the source footprint (the 2x2 / 4x4
// neighbourhoods of adjacent lanes overlap in L1/L2) and one coalesced write of the destination. The per-texel
// fp32 expressions are evaluated in exactly the reference's order (compile with -ffp-contract=off), so results are
// bit-identical for the non-sRGB formats; sRGB goes through powf and is within 1 ulp per step.
#include "../../include/dxtex_amd.h"
#include "dxtex_kernels.h"
#include "dxtex_store.h"
#include "dxtex_plan.h"
#include "dxtex_quad.h"
#include "dxtex_formats.h"
#include "cubic_filter.h"
#include "dxtex_nmap.h"
#include "dxtex_transform.h"
#include "dxtex_copyrect.h"
#include <algorithm>

namespace dxtex
{
namespace
{
struct ResizeArgs
{
    ImgView src, dst;
    int srgbIn, srgbOut;    // LoadScanlineLinear / StoreScanlineLinear convert sRGB <-> linear around the filter
    int wrapU, wrapV, mirrorU, mirrorV;
    int mipAlias;           // Generate2DMipsBoxFilter: rows / columns alias when the source is 1 high / 1 wide
    ImgView stale;          // ... and what its never-refreshed fourth row pointer still sees (see resize_box_kernel)
    // triangle filter tables (device memory): per destination row / column a run of (source index, weight)
    const uint32_t* triOfsX; const uint2* triX;
    const uint32_t* triOfsY; const uint2* triY;
};

__device__ __forceinline__ Texel load_linear(const ImgView& v, uint32_t x, uint32_t y, int srgb)
{
    Texel t = load_texel(v.pixels + uint64_t(y) * v.rowPitch, x, v.format);
    if (srgb) { t.r = srgb_to_linear1(t.r); t.g = srgb_to_linear1(t.g); t.b = srgb_to_linear1(t.b); }
    return t;
}

__device__ __forceinline__ void store_linear(const ImgView& v, uint32_t x, uint32_t y, int srgb, Texel t)
{
    if (srgb) { t.r = linear_to_srgb1(t.r); t.g = linear_to_srgb1(t.g); t.b = linear_to_srgb1(t.b); }
    store_texel(v.pixels + uint64_t(y) * v.rowPitch, x, v.format, t);
}

// XMLoadUByteN4 of one channel of a packed RGBA8 texel: byte * (1/255), as load_texel does. The RGBA8 fast paths below must unpack
// with exactly this expression to keep the general kernels' bits.
__device__ __forceinline__ float unorm8(uint32_t w, uint32_t shift) { return float((w >> shift) & 0xFFu) * (1.0f / 255.0f); }
__device__ __forceinline__ Texel unpack_rgba8(uint32_t w) { Texel t; t.r = unorm8(w, 0); t.g = unorm8(w, 8); t.b = unorm8(w, 16); t.a = unorm8(w, 24); return t; }

// ---- Convert -------------------------------------------------------------------------------------------------------------
// Rows are the grid's y dimension, which HIP limits to 65535: taller images wrap (grid_rows() caps the launch, the kernels stride).
__host__ __device__ inline uint32_t grid_rows(uint32_t height) { return height < 65535u ? height : 65535u; }

// The converted texel to the destination: StoreScanline, StoreScanlineDither's ordered branch, or StoreScanline after the zero error
// row of the diffusion branch (:4073-4092: v + 0.0f, which turns -0.0f into +0.0f) for a format without a dithered store. DITHER is a
// template argument so that the undithered kernels stay the code they were (a run-time mode word cost them 7-15 %).
template<bool DITHER>
__device__ __forceinline__ void store_converted(uint8_t* row, uint32_t idx, int format, Texel t, float threshold, int dither, uint32_t x, uint32_t y, uint32_t z)
{
    if constexpr (!DITHER) { store_texel(row, idx, format, t, threshold); return; }
    if (dither == CONVERT_DITHER_ORDERED) { store_texel_dither(row, idx, format, t, threshold, x, y, z); return; }
    if (dither == CONVERT_DITHER_ZERO_ERROR) { t.r = t.r + 0.0f; t.g = t.g + 0.0f; t.b = t.b + 0.0f; t.a = t.a + 0.0f; }
    store_texel(row, idx, format, t, threshold);
}

template<bool DITHER>
__global__ void __launch_bounds__(256) convert_kernel(ImgView src, ImgView dst, ConvertPlan plan, float threshold, int dither, uint32_t z)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= src.width) return;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
    {
        const Texel t = load_texel(src.pixels + uint64_t(y) * src.rowPitch, x, src.format);
        store_converted<DITHER>(dst.pixels + uint64_t(y) * dst.rowPitch, x, dst.format, apply_plan(t, plan), threshold, dither, x, y, z);
    }
}

// Formats whose element holds several texels (FC_GROUP: R8G8_B8G8, G8R8_G8B8, YUY2, Y210, Y216, R1): every operation that writes
// one produces R32G32B32A32_FLOAT rows first - exactly the XMVECTOR row the reference hands to StoreScanline - and this kernel
// stores them, an element per lane.
__global__ void __launch_bounds__(256) pack_group_kernel(ImgView rows, ImgView dst)
{
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    const uint32_t per = group_texels(dst.format);
    if (uint64_t(g) * per >= dst.width) return;
    const uint32_t n = min(per, dst.width - g * per);
    for (uint32_t y = blockIdx.y; y < dst.height; y += gridDim.y)
    {
        const float4* in = reinterpret_cast<const float4*>(rows.pixels + uint64_t(y) * rows.rowPitch) + uint64_t(g) * per;
        Texel t[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k)
        {
            t[k].r = t[k].g = t[k].b = t[k].a = 0.0f;
            if (k < n) { const float4 v = in[k]; t[k].r = v.x; t[k].g = v.y; t[k].b = v.z; t[k].a = v.w; }
        }
        store_group(dst.pixels + uint64_t(y) * dst.rowPitch, g, dst.format, t, n);
    }
}

// Four consecutive texels of a row per lane: the source quad arrives in 1-4 sixteen-byte loads (a wavefront reads 1-4 KiB of
// consecutive bytes per instruction), is decoded / converted / encoded texel by texel with the same load_texel / apply_plan /
// store_texel as above - on a register image of the quad, every index a compile-time constant - and leaves in 1-4 sixteen-byte
// stores. Used when a texel is a whole number of dwords on both sides (>= 32 bpp) and rows are 16-byte aligned.
// (DXTEX_QUAD_FORMATS, load_quad and store_quad: dxtex_quad.h; launch_convert admits no other format)

// SQ / DQ = bytes of a source / destination quad (16, 32 or 64; 0 = taken from the arguments: the 48-byte R32G32B32 quads).
// ROWS quads (of consecutive rows, same columns) are loaded before the first is converted, so that a lane keeps 64 bytes of
// reads in flight: with one 16-byte load per lane the kernel was bound by latency x occupancy (Little's law), not by HBM.
template<int SQ, int DQ, int ROWS, bool DITHER>
__global__ void __launch_bounds__(256) convert_quad_kernel(ImgView src, ImgView dst, ConvertPlan plan, float threshold, uint32_t srcQuadBytes, uint32_t dstQuadBytes,
                                                           int dither, uint32_t z)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q * 4u >= src.width) return;
    const uint32_t sq = SQ ? uint32_t(SQ) : srcQuadBytes, dq = DQ ? uint32_t(DQ) : dstQuadBytes;
    constexpr int SW = SQ ? SQ / 4 : 16, DW = DQ ? DQ / 4 : 16;
    for (uint32_t y0 = blockIdx.y * uint32_t(ROWS); y0 < src.height; y0 += gridDim.y * uint32_t(ROWS))
    {
        uint32_t in[ROWS][SW];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
        {
#pragma unroll
            for (int k = 0; k < SW; ++k) in[r][k] = 0u;
            const uint32_t y = min(y0 + uint32_t(r), src.height - 1u);       // a short last group re-reads the last row (and does not store it)
            load_quad<SW>(in[r], src.pixels + uint64_t(y) * src.rowPitch + uint64_t(q) * sq, sq);
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
        {
            uint32_t out[DW];
#pragma unroll
            for (int k = 0; k < DW; ++k) out[k] = 0u;
            // load_texel / store_texel are called with the format as a compile-time constant (one case per whole-dword format):
            // with a run-time format their switch also holds the byte- and word-addressed formats, whose accesses would force the
            // register image of the quad into memory
            Texel tx[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) tx[k].r = tx[k].g = tx[k].b = tx[k].a = 0.0f;
            switch (src.format)
            {
#define DXTEX_QCASE(F, QB) case F: if constexpr (SQ == QB || (SQ == 0 && QB > 0)) { _Pragma("unroll") for (uint32_t k = 0; k < 4u; ++k) tx[k] = load_texel(reinterpret_cast<const uint8_t*>(in[r]), k, F); } break;
                DXTEX_QUAD_FORMATS(DXTEX_QCASE)
#undef DXTEX_QCASE
            default: break;
            }
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) tx[k] = apply_plan(tx[k], plan);
            switch (dst.format)
            {
#define DXTEX_QCASE(F, QB) case F: if constexpr (DQ == QB || (DQ == 0 && QB > 0)) { _Pragma("unroll") for (uint32_t k = 0; k < 4u; ++k) \
                store_converted<DITHER>(reinterpret_cast<uint8_t*>(out), k, F, tx[k], threshold, dither, q * 4u + k, y0 + uint32_t(r), z); } break;
                DXTEX_QUAD_FORMATS(DXTEX_QCASE)
#undef DXTEX_QCASE
            default: break;
            }
            if (y0 + uint32_t(r) < src.height)
                store_quad<DW>(dst.pixels + uint64_t(y0 + uint32_t(r)) * dst.rowPitch + uint64_t(q) * dq, out, dq);
        }
    }
}

// ---- Convert with error diffusion (ConvertCustom's TEX_FILTER_DITHER_DIFFUSION branch, :4820-4852) ---------------------------------------
// One workgroup walks the rows of one image. Per row: every lane loads, converts, adds the previous row's error slots and pre-steps texels
// (stored by processing position: even rows left to right, odd rows right to left); then the vError chain runs as segments of segLen
// positions, one per lane, first from vError = 0 and then re-run from the exact incoming state until each merges with its stored run
// (dxtex_dither.h: dither_row_segmented is the same scheme written serially); then every lane builds slots of the next row's error buffer.
// The chain reads the pre-stepped texels and reads / writes the divided errors once per step: they sit in LDS for rows of up to
// kDiffuseLdsTexels texels (2 x 64 KiB) and in device memory for wider rows (a 16384-texel row needs 256 KiB per buffer). The error
// slots and the per-segment states stay in device memory: the parallel phases touch them once per row.
constexpr uint32_t kDiffuseThreads = 1024;
constexpr uint32_t kDiffuseMinSeg = 16;         // shorter segments leave the chain's merge distance (~15-30 texels on 8-bit data) to extra rounds
constexpr uint32_t kDiffuseLdsTexels = 4096;

struct DiffuseArgs
{
    ImgView src, dst;
    ConvertPlan plan;
    DitherSpec spec;
    float threshold;
    uint32_t segLen;
    F4 *pre, *err, *slot, *in, *pending;
    unsigned long long* rerun;
};

template<bool LDS>
__global__ void __launch_bounds__(kDiffuseThreads) convert_diffuse_kernel(DiffuseArgs a)
{
    if constexpr (LDS)
    {
        __shared__ F4 rows[2 * kDiffuseLdsTexels];
        a.pre = rows; a.err = rows + kDiffuseLdsTexels;
    }
    const uint32_t n = a.src.width, L = a.segLen, nseg = (n + L - 1) / L;
    const F4 zero = { { 0.0f, 0.0f, 0.0f, 0.0f } };
    const DitherSpec& s = a.spec;
    for (uint32_t x = threadIdx.x; x < n; x += blockDim.x) a.slot[x] = zero;
    unsigned long long rerun = 0;
    for (uint32_t y = 0; y < a.src.height; ++y)
    {
        const bool odd = (y & 1u) != 0;
        const uint8_t* srow = a.src.pixels + uint64_t(y) * a.src.rowPitch;
        uint8_t* drow = a.dst.pixels + uint64_t(y) * a.dst.rowPitch;
        for (uint32_t x = threadIdx.x; x < n; x += blockDim.x)
        {
            Texel t = apply_plan(load_texel(srow, x, a.src.format), a.plan);
            const F4 e = a.slot[x];
            t.r = t.r + e.v[0]; t.g = t.g + e.v[1]; t.b = t.b + e.v[2]; t.a = t.a + e.v[3];       // :4073-4086
            a.pre[odd ? n - 1u - x : x] = dither_pre(s, t.r, t.g, t.b, t.a);
        }
        __syncthreads();
        const auto out = [&](uint32_t p, uint64_t w) { dither_write(drow, odd ? n - 1u - p : p, s.bytes, w); };
        for (uint32_t k = threadIdx.x; k < nseg; k += blockDim.x)
        {
            a.in[k] = zero;
            dither_segment(s, a.pre, a.err, k * L, min((k + 1u) * L, n), zero, false, a.threshold, out);
        }
        for (;;)
        {
            __syncthreads();
            for (uint32_t k = threadIdx.x; k < nseg; k += blockDim.x)
                if (k) a.pending[k] = dither_seg_input(a.err, k, L);
            __syncthreads();
            int changed = 0;
            for (uint32_t k = threadIdx.x; k < nseg; k += blockDim.x)
            {
                if (!k || dither_same(s, a.pending[k], a.in[k])) continue;
                a.in[k] = a.pending[k];
                rerun += dither_segment(s, a.pre, a.err, k * L, min((k + 1u) * L, n), a.in[k], true, a.threshold, out);
                changed = 1;
            }
            if (!__syncthreads_or(changed)) break;
        }
        for (uint32_t x = threadIdx.x; x < n; x += blockDim.x) a.slot[x] = dither_slot(a.err, odd ? n - 1u - x : x, n);
        __syncthreads();
    }
    if (rerun) atomicAdd(a.rerun, rerun);
}

// ---- ComputeNormalMap (DirectXTexNormalMaps.cpp:77-240) ----------------------------------------------------------------------------
// A workgroup owns kNmapThreads columns and a strip of kNmapRows rows, and walks down it with a ring of four rows of heights in LDS:
// the reference's val0 / val1 / val2 cycle plus the row being filled. Each lane turns one texel per row into a height (load_texel +
// nmap_height); lane 0 and the last lane also load the left / right halo column, so every source texel is read once per strip (plus
// the strip's two halo rows). The next row is loaded into registers before the current one is computed, so its latency overlaps the
// arithmetic and the store. Columns and rows outside the image wrap, or repeat the edge under CNMAP_MIRROR_U / _V (nmap_edge). Row -1
// under MIRROR_V is row 0: what the reference means by memcpy(row0, row1, rowPitch) (:128), which copies rowPitch bytes into a row of
// 16-byte XMVECTORs and so is defined only when the source has 16 bytes per texel and a tight pitch.
constexpr uint32_t kNmapThreads = 256, kNmapRows = 32;
struct NmapArgs { ImgView src, dst; uint32_t flags; float amplitude; int unorm; uint32_t strips; };

__device__ __forceinline__ float nmap_load(const ImgView& s, uint32_t x, uint32_t y, uint32_t flags)
{
    const Texel t = load_texel(s.pixels + uint64_t(y) * s.rowPitch, x, s.format);
    return nmap_height(t.r, t.g, t.b, t.a, flags);
}

__global__ void __launch_bounds__(kNmapThreads) nmap_kernel(NmapArgs a)
{
    __shared__ float ring[4][kNmapThreads + 2];      // slot i of a row = column x0 - 1 + i
    const uint32_t W = a.src.width, H = a.src.height, t = threadIdx.x;
    const int64_t x0 = int64_t(blockIdx.x) * kNmapThreads, x = x0 + t;
    const bool clampU = (a.flags & NMAP_MIRROR_U) != 0, clampV = (a.flags & NMAP_MIRROR_V) != 0;
    // slot t + 1 holds column x (the right halo when x == W); lane 0 adds slot 0, the last lane slot kNmapThreads + 1 if that is needed
    const bool own = x <= int64_t(W);
    const uint32_t ownCol = nmap_edge(x, W, clampU);
    const bool extra = t == 0 || (t == kNmapThreads - 1 && x0 + int64_t(kNmapThreads) <= int64_t(W));
    const uint32_t extraSlot = t == 0 ? 0u : kNmapThreads + 1u;
    const uint32_t extraCol = nmap_edge(t == 0 ? x0 - 1 : x0 + int64_t(kNmapThreads), W, clampU);
    float hv = 0.0f, he = 0.0f;
    const auto load_row = [&](int64_t r)
    {
        const uint32_t sy = nmap_edge(r, H, clampV);
        if (own) hv = nmap_load(a.src, ownCol, sy, a.flags);
        if (extra) he = nmap_load(a.src, extraCol, sy, a.flags);
    };
    const auto put_row = [&](int64_t r)      // the row loaded last into its ring slot
    {
        float* s = ring[uint32_t(r + 1) & 3u];
        if (own) s[t + 1] = hv;
        if (extra) s[extraSlot] = he;
    };
    for (uint32_t strip = blockIdx.y; strip < a.strips; strip += gridDim.y)
    {
        const uint32_t y0 = strip * kNmapRows, y1 = uint32_t(min(uint64_t(y0) + kNmapRows, uint64_t(H)));
        __syncthreads();        // the previous strip's reads of the ring are done
        load_row(int64_t(y0) - 1); put_row(int64_t(y0) - 1);
        load_row(y0); put_row(y0);
        load_row(int64_t(y0) + 1);
        for (uint32_t y = y0; y < y1; ++y)
        {
            put_row(int64_t(y) + 1);
            __syncthreads();
            if (y + 1u < y1) load_row(int64_t(y) + 2);
            if (x < int64_t(W))
            {
                const float* top = ring[y & 3u];
                const float* mid = ring[(y + 1u) & 3u];
                const float* bot = ring[(y + 2u) & 3u];
                const float h[3][3] = { { top[t], top[t + 1], top[t + 2] }, { mid[t], mid[t + 1], mid[t + 2] }, { bot[t], bot[t + 1], bot[t + 2] } };
                const NmapOut o = nmap_texel(h, a.flags, a.amplitude, a.unorm != 0);
                store_texel(a.dst.pixels + uint64_t(y) * a.dst.rowPitch, uint32_t(x), a.dst.format, Texel{ o.x, o.y, o.z, o.w });
            }
        }
    }
}

// ---- TransformImage with texconv's per-texel lambdas (DirectXTexMisc.cpp:179-263, texconv.cpp:2645-3301) --------------------------------
// LoadScanline -> op -> StoreScanline (threshold 0), a destination texel per lane, in convert_kernel's shape. The op is a template
// argument: one kernel per op, no mode word in the loop. TONEMAP reads the running maximum's bits that tonemap_max_kernel left in
// device memory, so the two passes follow each other on the stream with no host round trip.
template<uint32_t OP>
__global__ void __launch_bounds__(256) transform_kernel(ImgView src, ImgView dst, XformArgs a, const uint32_t* maxBits)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= src.width) return;
    float M = 0.0f;
    if constexpr (OP == XFORM_TONEMAP) { const float m = xf_float(*maxBits); M = m * m; }
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
    {
        const Texel t = load_texel(src.pixels + uint64_t(y) * src.rowPitch, x, src.format);
        float c[4] = { t.r, t.g, t.b, t.a };
        xf_apply<OP>(c, a, M);
        store_texel(dst.pixels + uint64_t(y) * dst.rowPitch, x, dst.format, Texel{ c[0], c[1], c[2], c[3] });
    }
}

// The tone map's maximum luminance of one image, folded into *maxBits: a wave and a workgroup maximum, then one global atomic max per
// workgroup on the float's bits (every candidate is +0 or above, where unsigned order is float order).
__global__ void __launch_bounds__(256) tonemap_max_kernel(ImgView src, uint32_t* maxBits)
{
    __shared__ uint32_t waveMax[4];
    uint32_t m = 0;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
        for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < src.width; x += gridDim.x * 256u)
        {
            const Texel t = load_texel(src.pixels + uint64_t(y) * src.rowPitch, x, src.format);
            m = max(m, xf_lum_bits(t.r, t.g, t.b));
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, uint32_t(__shfl_xor(int(m), o)));
    if ((threadIdx.x & 63u) == 0) waveMax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        m = max(max(waveMax[0], waveMax[1]), max(waveMax[2], waveMax[3]));
        if (m) atomicMax(maxBits, m);
    }
}

// ---- CopyRectangle (DirectXTexMisc.cpp:275-381) ------------------------------------------------------------------------------------
// A batch of rectangles in one launch: blockIdx.z picks the job from the argument block, blockIdx.x the 256 columns (accesses of the
// mover, texels of the converting route), blockIdx.y the first group of rows; the grid is sized for the largest job and a workgroup
// outside its own job's extent leaves at once. Both routes are pure streaming. Nothing outside the rectangle is written.
//
// The mover keeps ROWS accesses of consecutive rows in flight per lane before the first store (as convert_quad_kernel does, and for the
// same reason: one 16-byte load per lane is bound by latency, not by HBM). T is the access type of the job's `vec`.
template<typename T, int ROWS>
__device__ __forceinline__ void copy_rect_move(const CopyJob& j, uint32_t u)
{
    const uint64_t at = uint64_t(u) * sizeof(T);
    for (uint32_t y0 = blockIdx.y * uint32_t(ROWS); y0 < j.height; y0 += gridDim.y * uint32_t(ROWS))
    {
        T v[ROWS];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
        {
            const uint32_t y = min(y0 + uint32_t(r), j.height - 1u);      // a short last group re-reads the last row (and does not store it)
            v[r] = *reinterpret_cast<const T*>(j.src + uint64_t(y) * j.srcPitch + at);
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
            if (y0 + uint32_t(r) < j.height) *reinterpret_cast<T*>(j.dst + uint64_t(y0 + uint32_t(r)) * j.dstPitch + at) = v[r];
    }
}

__global__ void __launch_bounds__(256) copy_rect_kernel(CopyBatch batch)
{
    const CopyJob& j = batch.job[blockIdx.z];
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (j.vec == 0u)
    {
        // different formats: convert_kernel's texel, from texel sx + u of the source row to texel dx + u of the destination row
        if (u >= j.width) return;
        for (uint32_t y = blockIdx.y; y < j.height; y += gridDim.y)
        {
            const Texel t = load_texel(j.src + uint64_t(y) * j.srcPitch, j.sx + u, j.srcFormat);
            store_converted<false>(j.dst + uint64_t(y) * j.dstPitch, j.dx + u, j.dstFormat, apply_plan(t, j.plan), 0.0f, CONVERT_DITHER_NONE, 0u, 0u, 0u);
        }
        return;
    }
    if (u < j.width)
    {
        switch (j.vec)
        {
        case 16u: copy_rect_move<uint4, 4>(j, u); break;
        case 8u: copy_rect_move<uint2, 4>(j, u); break;
        case 4u: copy_rect_move<uint32_t, 4>(j, u); break;
        case 2u: copy_rect_move<uint16_t, 4>(j, u); break;
        default: copy_rect_move<uint8_t, 4>(j, u); break;
        }
    }
    else if (u - j.width < j.tail)
    {
        // what a row holds after its whole accesses: byte by byte, by the lanes that follow them
        const uint64_t at = uint64_t(j.width) * j.vec + (u - j.width);
        for (uint32_t y = blockIdx.y; y < j.height; y += gridDim.y) j.dst[uint64_t(y) * j.dstPitch + at] = j.src[uint64_t(y) * j.srcPitch + at];
    }
}

// ---- texassemble's merge (Texassemble/texassemble.cpp:2236-2268) --------------------------------------------------------------------
// TransformImage over image 1 with a lambda that also reads image 2 (converted to R32G32B32A32_FLOAT by the caller, as texassemble does):
// transform_kernel's shape with a second source. b's rows are read as float4 (16-byte aligned: the launcher checks).
__global__ void __launch_bounds__(256) merge_kernel(ImgView a, ImgView b, ImgView dst, MergeArgs m)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= a.width) return;
    for (uint32_t y = blockIdx.y; y < a.height; y += gridDim.y)
    {
        const Texel t = load_texel(a.pixels + uint64_t(y) * a.rowPitch, x, a.format);
        const float4 o = reinterpret_cast<const float4*>(b.pixels + uint64_t(y) * b.rowPitch)[x];
        const float ca[4] = { t.r, t.g, t.b, t.a }, cb[4] = { o.x, o.y, o.z, o.w };
        float c[4];
        merge_texel(ca, cb, m, c);
        store_texel(dst.pixels + uint64_t(y) * dst.rowPitch, x, dst.format, Texel{ c[0], c[1], c[2], c[3] });
    }
}

// ---- PremultiplyAlpha / DemultiplyAlpha (DirectXTexPMAlpha.cpp:30-205): rgb * a, or rgb / a where a > 0, in linear space ------------
__device__ __forceinline__ void pmalpha_kernel_row(ImgView src, ImgView dst, int srgbIn, int srgbOut, int reverse, const uint32_t x, const uint32_t y)
{
    if (x >= src.width) return;
    Texel t = load_linear(src, x, y, srgbIn);
    if (!reverse) { t.r = t.r * t.a; t.g = t.g * t.a; t.b = t.b * t.a; }
    else if (t.a > 0.0f) { t.r = t.r / t.a; t.g = t.g / t.a; t.b = t.b / t.a; }
    else { t.r = t.g = t.b = t.a; }     // as written (:134-141): with alpha <= 0 the select picks the undivided alpha splat, not the colour
    store_linear(dst, x, y, srgbOut, t);
}
__global__ void __launch_bounds__(256) pmalpha_kernel(ImgView src, ImgView dst, int srgbIn, int srgbOut, int reverse)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y) pmalpha_kernel_row(src, dst, srgbIn, srgbOut, reverse, x, y);        // grid_rows(): HIP caps grid.y at 65535
}

// ---- ScaleMipMapsAlphaForCoverage (DirectXTexMipmaps.cpp:143-352) ---------------------------------------------------------------------
// ScaleAlpha: alpha * scale, colour untouched.
__device__ __forceinline__ void scale_alpha_kernel_row(ImgView src, ImgView dst, float scale, const uint32_t x, const uint32_t y)
{
    if (x >= src.width) return;
    Texel t = load_texel(src.pixels + uint64_t(y) * src.rowPitch, x, src.format);
    t.a = t.a * scale;
    store_texel(dst.pixels + uint64_t(y) * dst.rowPitch, x, dst.format, t);
}
__global__ void __launch_bounds__(256) scale_alpha_kernel(ImgView src, ImgView dst, float scale)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y) scale_alpha_kernel_row(src, dst, scale, x, y);        // grid_rows(): HIP caps grid.y at 65535
}

// CalculateAlphaCoverage: every 2x2 quad of scaled, saturated alphas is sampled at 8x8 sub-positions with bilinear weights and
// the samples above alphaReference are counted. Reproduced as written, including that the running vector `v` is overwritten
// with the (splatted) sum after every sub-sample (:283), so samples 2..64 of a quad see the previous sum, not the four alphas.
__device__ __forceinline__ void alpha_coverage_kernel_row(ImgView src, float scale, float alphaReference, unsigned long long* count, const uint32_t x, const uint32_t y)
{
    uint32_t n = 0;
    if (x + 1 < src.width)
    {
        const uint8_t* row0 = src.pixels + uint64_t(y) * src.rowPitch;
        const uint8_t* row1 = row0 + src.rowPitch;
        float v[4];
        v[0] = load_texel(row0, x, src.format).a * scale; v[1] = load_texel(row1, x, src.format).a * scale;
        v[2] = load_texel(row0, x + 1, src.format).a * scale; v[3] = load_texel(row1, x + 1, src.format).a * scale;
#pragma unroll
        for (int i = 0; i < 4; ++i) { float m = (v[i] > 0.0f) ? v[i] : 0.0f; v[i] = (m < 1.0f) ? m : 1.0f; }      // XMVectorSaturate
#pragma unroll 1
        for (int sy = 0; sy < 8; ++sy)
        {
            const float fy = (float(sy) + 0.5f) / 8.0f, ify = 1.0f - fy;
#pragma unroll
            for (int sx = 0; sx < 8; ++sx)
            {
                const float fx = (float(sx) + 0.5f) / 8.0f, ifx = 1.0f - fx;
                const float s = (v[0] * (ifx * ify) + v[1] * (ifx * fy)) + (v[2] * (fx * ify) + v[3] * (fx * fy));   // XMVectorSum: (x + y) + (z + w)
                v[0] = v[1] = v[2] = v[3] = s;
                n += (s > alphaReference) ? 1u : 0u;
            }
        }
    }
    // wave total, one atomic per wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(count, static_cast<unsigned long long>(n));
}
__global__ void __launch_bounds__(256) alpha_coverage_kernel(ImgView src, float scale, float alphaReference, unsigned long long* count)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t y = blockIdx.y; y < src.height - 1u; y += gridDim.y) alpha_coverage_kernel_row(src, scale, alphaReference, count, x, y);        // grid_rows(): HIP caps grid.y at 65535
}

// ScratchImage::IsAlphaAllOpaque (DirectXTexImage.cpp:800-852): counts the texels whose alpha is below the threshold
// (XMVector4Less on the splatted alpha: a NaN alpha is not "less" and counts as opaque, as there).
__global__ void __launch_bounds__(256) alpha_below_kernel(ImgView src, float threshold, unsigned long long* count)
{
    uint32_t n = 0;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
        for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < src.width; x += gridDim.x * 256u)
            n += (load_texel(src.pixels + uint64_t(y) * src.rowPitch, x, src.format).a < threshold) ? 1u : 0u;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(count, static_cast<unsigned long long>(n));
}

// ---- point (:255-309 / :907-987): 16.16 fixed-point stepping -----------------------------------------------------------------
__device__ __forceinline__ void resize_point_kernel_row(ResizeArgs a, const uint32_t x, const uint32_t y)
{
    if (x >= a.dst.width) return;
    const uint64_t xinc = (uint64_t(a.src.width) << 16) / a.dst.width;
    const uint64_t yinc = (uint64_t(a.src.height) << 16) / a.dst.height;
    const uint32_t sx = uint32_t((uint64_t(x) * xinc) >> 16), sy = uint32_t((uint64_t(y) * yinc) >> 16);
    const Texel t = load_texel(a.src.pixels + uint64_t(sy) * a.src.rowPitch, sx, a.src.format);
    store_texel(a.dst.pixels + uint64_t(y) * a.dst.rowPitch, x, a.dst.format, t);
}
__global__ void __launch_bounds__(256) resize_point_kernel(ResizeArgs a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t y = blockIdx.y; y < a.dst.height; y += gridDim.y) resize_point_kernel_row(a, x, y);        // grid_rows(): HIP caps grid.y at 65535
}

// ---- box (filters.h:31-37): (((p0 + p1) + p2) + p3) * 0.25 with p0 = (2x, 2y), p1 = (2x, 2y+1), p2 = (2x+1, 2y), p3 = (2x+1, 2y+1)
__device__ __forceinline__ void resize_box_kernel_row(ResizeArgs a, const uint32_t x, const uint32_t y)
{
    if (x >= a.dst.width) return;
    // Generate2DMipsBoxFilter: a 1-high source reads the same row twice, a 1-wide source the same column (:1024-1033)
    const bool oneRow = a.mipAlias && a.src.height <= 1, oneCol = a.mipAlias && a.src.width <= 1;
    const uint32_t x0 = oneCol ? 0u : 2u * x, x1 = oneCol ? 0u : 2u * x + 1u;
    const uint32_t y0 = oneRow ? 0u : 2u * y, y1 = oneRow ? 0u : 2u * y + 1u;
    const Texel p0 = load_linear(a.src, x0, y0, a.srgbIn), p1 = load_linear(a.src, x0, y1, a.srgbIn);
    const Texel p2 = load_linear(a.src, x1, y0, a.srgbIn);
    // Reference quirk, reproduced: urow3 = urow1 + 1 is computed once, before the level loop (:1017), and is not
    // re-pointed when a 1-high source makes urow1 alias urow0 (:1024-1027). For W x 1 sources with W > 1 the fourth
    // tap therefore still reads the old second-row buffer: row 1 of the last level that was 2 texels high.
    const bool staleTap = oneRow && !oneCol && a.stale.pixels != nullptr;
    const Texel p3 = staleTap ? load_linear(a.stale, x1, 1u, a.srgbIn) : load_linear(a.src, x1, y1, a.srgbIn);
    Texel r;
    r.r = (((p0.r + p1.r) + p2.r) + p3.r) * 0.25f;
    r.g = (((p0.g + p1.g) + p2.g) + p3.g) * 0.25f;
    r.b = (((p0.b + p1.b) + p2.b) + p3.b) * 0.25f;
    r.a = (((p0.a + p1.a) + p2.a) + p3.a) * 0.25f;
    store_linear(a.dst, x, y, a.srgbOut, r);
}
__global__ void __launch_bounds__(256) resize_box_kernel(ResizeArgs a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t y = blockIdx.y; y < a.dst.height; y += gridDim.y) resize_box_kernel_row(a, x, y);        // grid_rows(): HIP caps grid.y at 65535
}

// The box filter of four packed RGBA8 texels, resize_box_kernel's expression per channel: (((p0 + p1) + p2) + p3) * 0.25 with p0 / p1 the
// left column's upper / lower texel and p2 / p3 the right column's.
__device__ __forceinline__ uint32_t box_rgba8(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3)
{
    uint32_t packed = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c)
    {
        const float p0 = unorm8(w0, 8 * c), p1 = unorm8(w1, 8 * c), p2 = unorm8(w2, 8 * c), p3 = unorm8(w3, 8 * c);
        packed |= store_ubn_biased((((p0 + p1) + p2) + p3) * 0.25f) << (8 * c);
    }
    return packed;
}

// Box, exactly 2:1 on RGBA8 (the upper levels of a power-of-two mip chain, where the bytes are): one lane produces two adjacent
// destination texels from one 16-byte load per source row - consecutive lanes read consecutive 16 bytes - and writes 8 bytes.
__global__ void __launch_bounds__(256) resize_box_half_rgba8_kernel(ResizeArgs a)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;              // pair of destination texels
    if (q * 2u >= a.dst.width) return;
    for (uint32_t y = blockIdx.y; y < a.dst.height; y += gridDim.y)
    {
        const uint4 t = reinterpret_cast<const uint4*>(a.src.pixels + uint64_t(2u * y) * a.src.rowPitch)[q];
        const uint4 b = reinterpret_cast<const uint4*>(a.src.pixels + uint64_t(2u * y + 1u) * a.src.rowPitch)[q];
        const uint32_t top[4] = { t.x, t.y, t.z, t.w }, bot[4] = { b.x, b.y, b.z, b.w };
        uint32_t out[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) out[k] = box_rgba8(top[2 * k], bot[2 * k], top[2 * k + 1], bot[2 * k + 1]);
        reinterpret_cast<uint2*>(a.dst.pixels + uint64_t(y) * a.dst.rowPitch)[q] = make_uint2(out[0], out[1]);
    }
}

// ---- linear (filters.h:57-104) ---------------------------------------------------------------------------------------------
struct Lin { uint32_t u0, u1; float w0, w1; };
__device__ __forceinline__ Lin linear_entry(uint32_t source, uint32_t dest, bool wrap, uint32_t u)
{
    const float scale = float(source) / float(dest);
    const float srcB = (float(u) + 0.5f) * scale + 0.5f;
    long long isrcB = (long long)srcB;
    long long isrcA = isrcB - 1;
    const float weight = 1.0f + float(isrcB) - srcB;
    if (isrcA < 0) isrcA = wrap ? (long long)source - 1 : 0;
    if ((unsigned long long)isrcB >= source) isrcB = wrap ? 0 : (long long)source - 1;
    Lin e; e.u0 = uint32_t(isrcA); e.w0 = weight; e.u1 = uint32_t(isrcB); e.w1 = 1.0f - weight;
    return e;
}

__device__ __forceinline__ void resize_linear_kernel_row(ResizeArgs a, const uint32_t x, const uint32_t y)
{
    if (x >= a.dst.width) return;
    const Lin tx = linear_entry(a.src.width, a.dst.width, a.wrapU != 0, x);
    const Lin ty = linear_entry(a.src.height, a.dst.height, a.wrapV != 0, y);
    const Texel p00 = load_linear(a.src, tx.u0, ty.u0, a.srgbIn), p01 = load_linear(a.src, tx.u1, ty.u0, a.srgbIn);
    const Texel p10 = load_linear(a.src, tx.u0, ty.u1, a.srgbIn), p11 = load_linear(a.src, tx.u1, ty.u1, a.srgbIn);
    // BILINEAR_INTERPOLATE: ((r0[u0]*wx0 + r0[u1]*wx1) * wy0) + ((r1[u0]*wx0 + r1[u1]*wx1) * wy1)
#define DXTEX_BILERP(C) (((p00.C * tx.w0 + p01.C * tx.w1) * ty.w0) + ((p10.C * tx.w0 + p11.C * tx.w1) * ty.w1))
    Texel r;
    r.r = DXTEX_BILERP(r); r.g = DXTEX_BILERP(g); r.b = DXTEX_BILERP(b); r.a = DXTEX_BILERP(a);
#undef DXTEX_BILERP
    store_linear(a.dst, x, y, a.srgbOut, r);
}
__global__ void __launch_bounds__(256) resize_linear_kernel(ResizeArgs a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t y = blockIdx.y; y < a.dst.height; y += gridDim.y) resize_linear_kernel_row(a, x, y);        // grid_rows(): HIP caps grid.y at 65535
}

// ---- cubic (filters.h:106-207) -----------------------------------------------------------------------------------------------
__device__ __forceinline__ long long bounduvw(long long u, long long maxu, bool wrap, bool mirror)
{
    if (wrap)
    {
        if (u < 0) u = maxu + u + 1;
        else if (u > maxu) u = u - maxu - 1;
    }
    else if (mirror)
    {
        if (u < 0) u = (-u) - 1;
        else if (u > maxu) u = maxu - (u - maxu - 1);
    }
    u = (u < maxu) ? u : maxu;
    u = (u > 0) ? u : 0;
    return u;
}

struct Cub { uint32_t u0, u1, u2, u3; float x; };
__device__ __forceinline__ Cub cubic_entry(uint32_t source, uint32_t dest, bool wrap, bool mirror, uint32_t u)
{
    const float scale = float(source) / float(dest);
    const float srcB = (float(u) + 0.5f) * scale - 0.5f;
    const long long maxu = (long long)source - 1;
    const long long iB = bounduvw((long long)srcB, maxu, wrap, mirror);
    Cub e;
    e.u0 = uint32_t(bounduvw(iB - 1, maxu, wrap, mirror));
    e.u1 = uint32_t(iB);
    e.u2 = uint32_t(bounduvw(iB + 1, maxu, wrap, mirror));
    e.u3 = uint32_t(bounduvw(iB + 2, maxu, wrap, mirror));
    e.x = srcB - float(iB);
    return e;
}

// CUBIC_INTERPOLATE of four texels, channel by channel
__device__ __forceinline__ Texel cubic4(float x, const Texel& p0, const Texel& p1, const Texel& p2, const Texel& p3)
{
    Texel o;
    o.r = cubic1(x, p0.r, p1.r, p2.r, p3.r); o.g = cubic1(x, p0.g, p1.g, p2.g, p3.g);
    o.b = cubic1(x, p0.b, p1.b, p2.b, p3.b); o.a = cubic1(x, p0.a, p1.a, p2.a, p3.a);
    return o;
}

// The 2-D cubic of a surface at (tx, ty): four rows through tx (cubic_row), then the column through ty (filters.h:192-207). Here the rows
// are written out, not looped over: the compiler leaves a loop over them rolled, with the array of rows indexed at run time in LDS. That
// form is the faster one for resize3d_cubic_kernel, which keeps it (128^3 RGBA8 chain: 248 us against 314 us written out), and the
// slower one for resize_cubic_kernel (1024^2 RGBA16F chain: 185 us against 123 us).
__device__ __forceinline__ Texel cubic_row(const ImgView& s, const Cub& tx, uint32_t y, int srgbIn)
{
    return cubic4(tx.x, load_linear(s, tx.u0, y, srgbIn), load_linear(s, tx.u1, y, srgbIn), load_linear(s, tx.u2, y, srgbIn), load_linear(s, tx.u3, y, srgbIn));
}
__device__ __forceinline__ Texel cubic_surface(const ImgView& s, const Cub& tx, const Cub& ty, int srgbIn)
{
    const Texel c0 = cubic_row(s, tx, ty.u0, srgbIn), c1 = cubic_row(s, tx, ty.u1, srgbIn), c2 = cubic_row(s, tx, ty.u2, srgbIn), c3 = cubic_row(s, tx, ty.u3, srgbIn);
    return cubic4(ty.x, c0, c1, c2, c3);
}

__device__ __forceinline__ void resize_cubic_kernel_row(ResizeArgs a, const uint32_t x, const uint32_t y)
{
    if (x >= a.dst.width) return;
    const Cub tx = cubic_entry(a.src.width, a.dst.width, a.wrapU != 0, a.mirrorU != 0, x);
    const Cub ty = cubic_entry(a.src.height, a.dst.height, a.wrapV != 0, a.mirrorV != 0, y);
    // RGBA8 away from the left / right border: the four taps of a row are adjacent texels, one 16-byte load instead of four
    // format-dispatched 4-byte loads
    const bool rowLoad = a.src.format == FMT_R8G8B8A8_UNORM && !a.srgbIn && tx.u1 == tx.u0 + 1u && tx.u2 == tx.u0 + 2u && tx.u3 == tx.u0 + 3u;
    Texel o;
    if (rowLoad)
    {
        const uint32_t ys[4] = { ty.u0, ty.u1, ty.u2, ty.u3 };
        Texel c[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
        {
            const uint32_t* q = reinterpret_cast<const uint32_t*>(a.src.pixels + uint64_t(ys[r]) * a.src.rowPitch) + tx.u0;
            c[r] = cubic4(tx.x, unpack_rgba8(q[0]), unpack_rgba8(q[1]), unpack_rgba8(q[2]), unpack_rgba8(q[3]));        // 4-byte aligned: the compiler merges them into one dwordx4 load
        }
        o = cubic4(ty.x, c[0], c[1], c[2], c[3]);
    }
    else o = cubic_surface(a.src, tx, ty, a.srgbIn);
    store_linear(a.dst, x, y, a.srgbOut, o);
}
__global__ void __launch_bounds__(256) resize_cubic_kernel(ResizeArgs a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t y = blockIdx.y; y < a.dst.height; y += gridDim.y) resize_cubic_kernel_row(a, x, y);        // grid_rows(): HIP caps grid.y at 65535
}

// Cubic, exactly 2:1 in both directions with clamp addressing on RGBA8 (every level of a power-of-two mip chain): srcB = 2u + 0.5, so the
// four taps are texels 2u-1 .. 2u+2 (clamped) and dx = 0.5 for every destination texel. The filter is separable in the reference too
// (CUBIC_INTERPOLATE along x for four source rows, then along y, filters.h:192-207), and neighbouring destination rows share two of their
// four source rows: a lane owns one destination column of a strip of rows and walks down it with the x-filtered values of the last four
// source rows in registers - two row passes per destination texel instead of four (plus two at the top of the strip), every source texel
// unpacked once per row pass, no LDS and no barrier (a tile in LDS held 35 KiB per workgroup and left the kernel waiting on it at four
// waves per SIMD). Same expressions, same order, same bits as resize_cubic_kernel.
__global__ void __launch_bounds__(256) resize_cubic_half_rgba8_kernel(ResizeArgs a, uint32_t stripRows)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= a.dst.width) return;
    const int64_t srcW = a.src.width, srcH = a.src.height;
    const int64_t u0 = int64_t(2) * x - 1;
    const bool inside = u0 >= 0 && u0 + 3 < srcW;
    const uint32_t i0 = uint32_t(u0 < 0 ? 0 : u0), i1 = uint32_t(u0 + 1 > srcW - 1 ? srcW - 1 : u0 + 1),
                   i2 = uint32_t(u0 + 2 > srcW - 1 ? srcW - 1 : u0 + 2), i3 = uint32_t(u0 + 3 > srcW - 1 ? srcW - 1 : u0 + 3);
    // the x-filtered texel of source row sy (clamped) at this column
    auto xpass = [&](int64_t sy) -> float4
    {
        sy = sy < 0 ? 0 : (sy > srcH - 1 ? srcH - 1 : sy);
        const uint32_t* q = reinterpret_cast<const uint32_t*>(a.src.pixels + uint64_t(sy) * a.src.rowPitch);
        uint32_t w0, w1, w2, w3;
        if (inside) { w0 = q[u0]; w1 = q[u0 + 1]; w2 = q[u0 + 2]; w3 = q[u0 + 3]; }
        else { w0 = q[i0]; w1 = q[i1]; w2 = q[i2]; w3 = q[i3]; }
        float4 c;
        c.x = cubic_half1(unorm8(w0, 0), unorm8(w1, 0), unorm8(w2, 0), unorm8(w3, 0));
        c.y = cubic_half1(unorm8(w0, 8), unorm8(w1, 8), unorm8(w2, 8), unorm8(w3, 8));
        c.z = cubic_half1(unorm8(w0, 16), unorm8(w1, 16), unorm8(w2, 16), unorm8(w3, 16));
        c.w = cubic_half1(unorm8(w0, 24), unorm8(w1, 24), unorm8(w2, 24), unorm8(w3, 24));
        return c;
    };
    // the grid's y dimension is capped at 65535 strips (HIP's limit): a taller level is covered by striding over the strips
    for (uint64_t s0 = uint64_t(blockIdx.y) * stripRows; s0 < a.dst.height; s0 += uint64_t(gridDim.y) * stripRows)
    {
    const uint32_t y0 = uint32_t(s0), y1 = uint32_t(min(s0 + stripRows, uint64_t(a.dst.height)));
    // destination row y takes source rows 2y - 1 .. 2y + 2
    float4 c0 = xpass(int64_t(2) * y0 - 1), c1 = xpass(int64_t(2) * y0), c2 = xpass(int64_t(2) * y0 + 1);
#pragma unroll 2
    for (uint32_t y = y0; y < y1; ++y)
    {
        const float4 c3 = xpass(int64_t(2) * y + 2);
        const float4 n2 = xpass(int64_t(2) * y + 3);             // row 2(y+1) + 1 of the next trip, loaded before this trip's store
        Texel o;
        o.r = cubic_half1(c0.x, c1.x, c2.x, c3.x); o.g = cubic_half1(c0.y, c1.y, c2.y, c3.y);
        o.b = cubic_half1(c0.z, c1.z, c2.z, c3.z); o.a = cubic_half1(c0.w, c1.w, c2.w, c3.w);
        reinterpret_cast<uint32_t*>(a.dst.pixels + uint64_t(y) * a.dst.rowPitch)[x] = pack_texel32(FMT_R8G8B8A8_UNORM, o);
        c0 = c2; c1 = c3; c2 = n2;
    }
    }
}

// The same filter with TWO adjacent destination texels per lane (destination width even, rows 16-byte aligned): the six source texels a
// pair needs are one 16-byte load and two neighbouring dwords, every source texel is unpacked once per pair instead of once per destination
// texel, and a wavefront reads 1 KiB runs. Same expressions in the same order as resize_cubic_half_rgba8_kernel, hence the same bits.
__global__ void __launch_bounds__(256) resize_cubic_half_rgba8_x2_kernel(ResizeArgs a, uint32_t stripRows)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;            // pair index: destination texels 2k, 2k + 1
    if (2u * k >= a.dst.width) return;
    const int64_t srcW = a.src.width, srcH = a.src.height;
    const uint32_t iL = (k == 0) ? 0u : 4u * k - 1u;               // clamp addressing: texel 4k - 1 / 4k + 4
    const uint32_t iR = uint32_t(int64_t(4) * k + 4 > srcW - 1 ? srcW - 1 : int64_t(4) * k + 4);
    struct Pair { float4 l, r; };
    auto xpass = [&](int64_t sy) -> Pair
    {
        sy = sy < 0 ? 0 : (sy > srcH - 1 ? srcH - 1 : sy);
        const uint8_t* row = a.src.pixels + uint64_t(sy) * a.src.rowPitch;
        const uint4 m = reinterpret_cast<const uint4*>(row)[k];
        const uint32_t wl = reinterpret_cast<const uint32_t*>(row)[iL], wr = reinterpret_cast<const uint32_t*>(row)[iR];
        Pair o;
#define DXTEX_ONE(S, FL, FR) { const float t0 = unorm8(wl, S), t1 = unorm8(m.x, S), t2 = unorm8(m.y, S), t3 = unorm8(m.z, S), t4 = unorm8(m.w, S), t5 = unorm8(wr, S); \
                               FL = cubic_half1(t0, t1, t2, t3); FR = cubic_half1(t2, t3, t4, t5); }
        DXTEX_ONE(0, o.l.x, o.r.x) DXTEX_ONE(8, o.l.y, o.r.y) DXTEX_ONE(16, o.l.z, o.r.z) DXTEX_ONE(24, o.l.w, o.r.w)
#undef DXTEX_ONE
        return o;
    };
    for (uint64_t s0 = uint64_t(blockIdx.y) * stripRows; s0 < a.dst.height; s0 += uint64_t(gridDim.y) * stripRows)
    {
        const uint32_t y0 = uint32_t(s0), y1 = uint32_t(min(s0 + stripRows, uint64_t(a.dst.height)));
        Pair c0 = xpass(int64_t(2) * y0 - 1), c1 = xpass(int64_t(2) * y0), c2 = xpass(int64_t(2) * y0 + 1);
#pragma unroll 2
        for (uint32_t y = y0; y < y1; ++y)
        {
            const Pair c3 = xpass(int64_t(2) * y + 2);
            const Pair n2 = xpass(int64_t(2) * y + 3);
            Texel ol, orr;
            ol.r = cubic_half1(c0.l.x, c1.l.x, c2.l.x, c3.l.x); ol.g = cubic_half1(c0.l.y, c1.l.y, c2.l.y, c3.l.y);
            ol.b = cubic_half1(c0.l.z, c1.l.z, c2.l.z, c3.l.z); ol.a = cubic_half1(c0.l.w, c1.l.w, c2.l.w, c3.l.w);
            orr.r = cubic_half1(c0.r.x, c1.r.x, c2.r.x, c3.r.x); orr.g = cubic_half1(c0.r.y, c1.r.y, c2.r.y, c3.r.y);
            orr.b = cubic_half1(c0.r.z, c1.r.z, c2.r.z, c3.r.z); orr.a = cubic_half1(c0.r.w, c1.r.w, c2.r.w, c3.r.w);
            reinterpret_cast<uint2*>(a.dst.pixels + uint64_t(y) * a.dst.rowPitch)[k] =
                make_uint2(pack_texel32(FMT_R8G8B8A8_UNORM, ol), pack_texel32(FMT_R8G8B8A8_UNORM, orr));
            c0 = c2; c1 = c3; c2 = n2;
        }
    }
}

// ---- triangle (filters.h:209-419; accumulation order of DirectXTexMipmaps.cpp:1517-1542 / DirectXTexResize.cpp:730-760) ----------
// The reference scatters every source texel into accumulation rows; the sum a destination texel receives is ordered
// by (source row, source column, row-list entry, column-list entry). The host inverts the filter lists so that a lane
// can gather its texel's contributions in that same order: acc = acc + src * (wy * wx), unfused.
__device__ __forceinline__ void resize_triangle_kernel_row(ResizeArgs a, const uint32_t x, const uint32_t y)
{
    if (x >= a.dst.width) return;
    const uint32_t yb = a.triOfsY[y], ye = a.triOfsY[y + 1];
    const uint32_t xb = a.triOfsX[x], xe = a.triOfsX[x + 1];
    Texel acc; acc.r = acc.g = acc.b = acc.a = 0.0f;
    uint32_t i = yb;
    while (i < ye)
    {
        const uint32_t sy = a.triY[i].x;
        uint32_t iEnd = i + 1;
        while (iEnd < ye && a.triY[iEnd].x == sy) ++iEnd;
        uint32_t k = xb;
        while (k < xe)
        {
            const uint32_t sx = a.triX[k].x;
            uint32_t kEnd = k + 1;
            while (kEnd < xe && a.triX[kEnd].x == sx) ++kEnd;
            const Texel p = load_linear(a.src, sx, sy, a.srgbIn);
            for (uint32_t j = i; j < iEnd; ++j)
            {
                const float wy = __uint_as_float(a.triY[j].y);
                for (uint32_t m = k; m < kEnd; ++m)
                {
                    const float w = wy * __uint_as_float(a.triX[m].y);
                    acc.r = p.r * w + acc.r; acc.g = p.g * w + acc.g; acc.b = p.b * w + acc.b; acc.a = p.a * w + acc.a;
                }
            }
            k = kEnd;
        }
        i = iEnd;
    }
    if (a.dst.format == FMT_R10G10B10A2_UNORM || a.dst.format == FMT_R10G10B10A2_UINT) acc.a = acc.a + 0.1f;       // the reference biases 2-bit alpha against accumulation error (DirectXTexMipmaps.cpp:1560-1579, DirectXTexResize.cpp:768-787)
    store_linear(a.dst, x, y, a.srgbOut, acc);
}
__global__ void __launch_bounds__(256) resize_triangle_kernel(ResizeArgs a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    for (uint32_t y = blockIdx.y; y < a.dst.height; y += gridDim.y) resize_triangle_kernel_row(a, x, y);        // grid_rows(): HIP caps grid.y at 65535
}

// ---- volume mips: Generate3DMips{Point,Box,Linear,Cubic,Triangle}Filter (DirectXTexMipmaps.cpp:1666-2826) ----------------------------
// One lane = one destination texel (x, y = blockIdx.y, z = blockIdx.z) of a level whose SOURCE has depth > 1; levels whose source
// is one slice deep take the reference's 2-D branch, i.e. the kernels above.
struct Resize3Args
{
    VolumeView src, dst;
    int srgbIn, srgbOut;
    int wrapU, wrapV, wrapW, mirrorU, mirrorV, mirrorW;
    ImgView staleU, staleV;          // box: what the never re-pointed urow3 / vrow3 still see on W x 1 x D levels (see resize3d_box_kernel)
    const uint32_t* triOfsX; const uint2* triX;
    const uint32_t* triOfsY; const uint2* triY;
    const uint32_t* triOfsZ; const uint2* triZ;
};

// ---- the tail of a mip chain in ONE workgroup --------------------------------------------------------------------------------
// The last levels of a chain are a few thousand texels each: a launch per level costs ~5 us of dispatch latency for ~1 us of
// work (ten such launches were 40 % of the 8192^2 box chain). From the first level whose source is at most kTailSide texels on a
// side, one workgroup of 1024 lanes walks the remaining levels, a workgroup barrier (with its release / acquire fences on global
// memory) between levels: level n + 1 reads what the same workgroup stored for level n, exactly as the per-level launches do.
constexpr uint32_t kTailSide = 64;
constexpr int kTailMaxLevels = 8;
struct TailArgs
{
    ResizeArgs a;                       // flags; src = the first source level
    ImgView level[kTailMaxLevels];      // the destination levels, in order
    ImgView stale[kTailMaxLevels];      // per level what launch_resize takes as `stale`: the host steps the chain's StaleTap through the tail
    int nlevels;
    uint32_t mode;                      // DXTEX_FILTER_POINT / LINEAR / BOX (resize_tail_route sends no cubic chain here)
};

__global__ void __launch_bounds__(1024) resize_tail_kernel(TailArgs t)
{
    ResizeArgs a = t.a;
    for (int l = 0; l < t.nlevels; ++l)
    {
        a.dst = t.level[l];
        a.stale = t.stale[l];
        const uint32_t n = a.dst.width * a.dst.height;
        for (uint32_t i = threadIdx.x; i < n; i += 1024u)
        {
            const uint32_t y = i / a.dst.width, x = i - y * a.dst.width;
            switch (t.mode)
            {
            case DXTEX_FILTER_POINT: resize_point_kernel_row(a, x, y); break;
            case DXTEX_FILTER_LINEAR: resize_linear_kernel_row(a, x, y); break;
            default: resize_box_kernel_row(a, x, y); break;
            }
        }
        __syncthreads();                                                     // level l is complete and visible to the whole workgroup
        a.src = a.dst;
    }
}

// The tail of a power-of-two RGBA8 cubic chain in LDS: from a source of at most 64 x 64 texels down to 1 x 1, every level an exact halving in
// both directions (clamp addressing, no sRGB). The generic tail above reads each level back from global memory - sixteen dependent taps per
// texel with nothing to hide their latency, 84 us for the six levels - and a launch per level costs ~6.6 us each. Here the source level is
// staged once, every level is produced from the previous one's packed texels in LDS (and written out), a barrier per level: the arithmetic of
// resize_cubic_half_rgba8_kernel (x-pass over four clamped taps of each of four clamped rows, then y), the same bits.
struct CubicTailArgs
{
    const uint8_t* src; uint64_t srcPitch; uint32_t srcW, srcH; int nlevels;
    uint8_t* dst[kTailMaxLevels]; uint64_t dstPitch[kTailMaxLevels];
};
template<bool CUBIC>
__global__ void __launch_bounds__(1024) resize_half_tail_rgba8_kernel(CubicTailArgs t)
{
    __shared__ uint32_t bufA[kTailSide * kTailSide], bufB[(kTailSide / 2) * (kTailSide / 2)];
    uint32_t w = t.srcW, h = t.srcH;
    for (uint32_t i = threadIdx.x; i < w * h; i += 1024u)
    {
        const uint32_t y = i / w, x = i - y * w;
        bufA[i] = reinterpret_cast<const uint32_t*>(t.src + uint64_t(y) * t.srcPitch)[x];
    }
    __syncthreads();
    uint32_t* s = bufA;
    uint32_t* d = bufB;
    for (int l = 0; l < t.nlevels; ++l)
    {
        const uint32_t dw = w >> 1, dh = h >> 1;
        for (uint32_t i = threadIdx.x; i < dw * dh; i += 1024u)
        {
            const uint32_t y = i / dw, x = i - y * dw;
            if constexpr (!CUBIC)
            {
                // the box filter of resize_box_half_rgba8_kernel over (2x, 2y), (2x, 2y + 1), (2x + 1, 2y), (2x + 1, 2y + 1)
                const uint32_t t0 = s[(2u * y) * w + 2u * x], t1 = s[(2u * y) * w + 2u * x + 1u], b0 = s[(2u * y + 1u) * w + 2u * x], b1 = s[(2u * y + 1u) * w + 2u * x + 1u];
                const uint32_t packed = box_rgba8(t0, b0, t1, b1);
                d[i] = packed;
                reinterpret_cast<uint32_t*>(t.dst[l] + uint64_t(y) * t.dstPitch[l])[x] = packed;
                continue;
            }
            const int32_t u0 = int32_t(2u * x) - 1, v0 = int32_t(2u * y) - 1;
            uint32_t xi[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { const int32_t u = u0 + k; xi[k] = uint32_t(u < 0 ? 0 : (u > int32_t(w) - 1 ? int32_t(w) - 1 : u)); }
            float4 c[4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
            {
                const int32_t v = v0 + r;
                const uint32_t* row = s + uint32_t(v < 0 ? 0 : (v > int32_t(h) - 1 ? int32_t(h) - 1 : v)) * w;
                const uint32_t w0 = row[xi[0]], w1 = row[xi[1]], w2 = row[xi[2]], w3 = row[xi[3]];
                c[r].x = cubic_half1(unorm8(w0, 0), unorm8(w1, 0), unorm8(w2, 0), unorm8(w3, 0));
                c[r].y = cubic_half1(unorm8(w0, 8), unorm8(w1, 8), unorm8(w2, 8), unorm8(w3, 8));
                c[r].z = cubic_half1(unorm8(w0, 16), unorm8(w1, 16), unorm8(w2, 16), unorm8(w3, 16));
                c[r].w = cubic_half1(unorm8(w0, 24), unorm8(w1, 24), unorm8(w2, 24), unorm8(w3, 24));
            }
            Texel o;
            o.r = cubic_half1(c[0].x, c[1].x, c[2].x, c[3].x); o.g = cubic_half1(c[0].y, c[1].y, c[2].y, c[3].y);
            o.b = cubic_half1(c[0].z, c[1].z, c[2].z, c[3].z); o.a = cubic_half1(c[0].w, c[1].w, c[2].w, c[3].w);
            const uint32_t packed = pack_texel32(FMT_R8G8B8A8_UNORM, o);
            d[i] = packed;
            reinterpret_cast<uint32_t*>(t.dst[l] + uint64_t(y) * t.dstPitch[l])[x] = packed;
        }
        __syncthreads();
        uint32_t* const tmp = s; s = d; d = tmp;          // the next level (a quarter of this one) fits where this level's source was
        w = dw; h = dh;
    }
}

// point (:1666-1813): source slice (z * zinc) >> 16, then the 2-D point filter inside it
__global__ void __launch_bounds__(256) resize3d_point_kernel(Resize3Args a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= a.dst.width) return;
    const uint64_t zinc = (uint64_t(a.src.depth) << 16) / a.dst.depth;
    const uint64_t xinc = (uint64_t(a.src.width) << 16) / a.dst.width, yinc = (uint64_t(a.src.height) << 16) / a.dst.height;
    const ImgView src = slice_of(a.src, uint32_t((uint64_t(z) * zinc) >> 16)), dst = slice_of(a.dst, z);
    const uint32_t sx = uint32_t((uint64_t(x) * xinc) >> 16), sy = uint32_t((uint64_t(y) * yinc) >> 16);
    store_texel(dst.pixels + uint64_t(y) * dst.rowPitch, x, dst.format, load_texel(src.pixels + uint64_t(sy) * src.rowPitch, sx, src.format));
}

// box (:1815-1990): AVERAGE8 over slices (2z, 2z+1) x rows x columns, summed in the macro's order, x 0.125.
__global__ void __launch_bounds__(256) resize3d_box_kernel(Resize3Args a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= a.dst.width) return;
    const bool oneRow = a.src.height <= 1, oneCol = a.src.width <= 1;
    const uint32_t za = min(2u * z, a.src.depth - 1u), zb = min(za + 1u, a.src.depth - 1u);
    const ImgView A = slice_of(a.src, za), B = slice_of(a.src, zb);
    const uint32_t x0 = oneCol ? 0u : 2u * x, x1 = oneCol ? 0u : 2u * x + 1u;
    const uint32_t y0 = oneRow ? 0u : 2u * y, y1 = oneRow ? 0u : 2u * y + 1u;
    // Reference quirk, reproduced: urow3 = urow1 + 1 and vrow3 = vrow1 + 1 are set once, before the level loop (:1849-1852); a
    // 1-high source re-points urow1 / vrow1 (:1857-1861) but not urow3 / vrow3 unless the source is also 1 wide (:1863-1869).
    // On W x 1 x D sources (W > 1) the fourth tap of either slice therefore still reads the old second-row buffers: row 1 of the
    // last two slices of the last level that was 2 texels high.
    const bool staleTap = oneRow && !oneCol && a.staleU.pixels != nullptr;
    const Texel p0 = load_linear(A, x0, y0, a.srgbIn), p1 = load_linear(A, x0, y1, a.srgbIn), p2 = load_linear(A, x1, y0, a.srgbIn);
    const Texel p3 = staleTap ? load_linear(a.staleU, x1, 1u, a.srgbIn) : load_linear(A, x1, y1, a.srgbIn);
    const Texel p4 = load_linear(B, x0, y0, a.srgbIn), p5 = load_linear(B, x0, y1, a.srgbIn), p6 = load_linear(B, x1, y0, a.srgbIn);
    const Texel p7 = staleTap ? load_linear(a.staleV, x1, 1u, a.srgbIn) : load_linear(B, x1, y1, a.srgbIn);
#define DXTEX_AVG8(C) ((((((((p0.C + p1.C) + p2.C) + p3.C) + p4.C) + p5.C) + p6.C) + p7.C) * 0.125f)
    Texel r;
    r.r = DXTEX_AVG8(r); r.g = DXTEX_AVG8(g); r.b = DXTEX_AVG8(b); r.a = DXTEX_AVG8(a);
#undef DXTEX_AVG8
    store_linear(slice_of(a.dst, z), x, y, a.srgbOut, r);
}

// linear (:1992-2188): TRILINEAR_INTERPOLATE (filters.h:106-113)
__global__ void __launch_bounds__(256) resize3d_linear_kernel(Resize3Args a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= a.dst.width) return;
    const Lin tx = linear_entry(a.src.width, a.dst.width, a.wrapU != 0, x);
    const Lin ty = linear_entry(a.src.height, a.dst.height, a.wrapV != 0, y);
    const Lin tz = linear_entry(a.src.depth, a.dst.depth, a.wrapW != 0, z);
    const ImgView A = slice_of(a.src, tz.u0), B = slice_of(a.src, tz.u1);
    const Texel a00 = load_linear(A, tx.u0, ty.u0, a.srgbIn), a01 = load_linear(A, tx.u1, ty.u0, a.srgbIn);
    const Texel a10 = load_linear(A, tx.u0, ty.u1, a.srgbIn), a11 = load_linear(A, tx.u1, ty.u1, a.srgbIn);
    const Texel b00 = load_linear(B, tx.u0, ty.u0, a.srgbIn), b01 = load_linear(B, tx.u1, ty.u0, a.srgbIn);
    const Texel b10 = load_linear(B, tx.u0, ty.u1, a.srgbIn), b11 = load_linear(B, tx.u1, ty.u1, a.srgbIn);
#define DXTEX_TRILERP(C) ((((a00.C * tx.w0 + a01.C * tx.w1) * ty.w0 + (a10.C * tx.w0 + a11.C * tx.w1) * ty.w1) * tz.w0) + \
                          (((b00.C * tx.w0 + b01.C * tx.w1) * ty.w0 + (b10.C * tx.w0 + b11.C * tx.w1) * ty.w1) * tz.w1))
    Texel r;
    r.r = DXTEX_TRILERP(r); r.g = DXTEX_TRILERP(g); r.b = DXTEX_TRILERP(b); r.a = DXTEX_TRILERP(a);
#undef DXTEX_TRILERP
    store_linear(slice_of(a.dst, z), x, y, a.srgbOut, r);
}

// cubic (:2190-2572): per source slice the 2-D cubic (rows through toX, then toY), then CUBIC_INTERPOLATE through toZ
__global__ void __launch_bounds__(256) resize3d_cubic_kernel(Resize3Args a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= a.dst.width) return;
    const Cub tx = cubic_entry(a.src.width, a.dst.width, a.wrapU != 0, a.mirrorU != 0, x);
    const Cub ty = cubic_entry(a.src.height, a.dst.height, a.wrapV != 0, a.mirrorV != 0, y);
    const Cub tz = cubic_entry(a.src.depth, a.dst.depth, a.wrapW != 0, a.mirrorW != 0, z);
    const uint32_t zs[4] = { tz.u0, tz.u1, tz.u2, tz.u3 };
    Texel d[4];
#pragma unroll 1
    for (int j = 0; j < 4; ++j)
    {
        // the rows of cubic_surface as a loop, which stays rolled: see there
        const ImgView S = slice_of(a.src, zs[j]);
        const uint32_t ys[4] = { ty.u0, ty.u1, ty.u2, ty.u3 };
        Texel c[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) c[r] = cubic_row(S, tx, ys[r], a.srgbIn);
        const Texel o = cubic4(ty.x, c[0], c[1], c[2], c[3]);
        if (j == 0) d[0] = o; else if (j == 1) d[1] = o; else if (j == 2) d[2] = o; else d[3] = o;
    }
    store_linear(slice_of(a.dst, z), x, y, a.srgbOut, cubic4(tz.x, d[0], d[1], d[2], d[3]));
}

// triangle (:2574-2826): acc = src * ((wz * wy) * wx) + acc, contributions ordered by (source slice, source row, source column,
// slice-list entry, row-list entry, column-list entry) - gathered per destination texel from the inverted lists, as in 2-D.
__global__ void __launch_bounds__(256) resize3d_triangle_kernel(Resize3Args a)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, y = blockIdx.y, z = blockIdx.z;
    if (x >= a.dst.width) return;
    const uint32_t zb = a.triOfsZ[z], ze = a.triOfsZ[z + 1];
    const uint32_t yb = a.triOfsY[y], ye = a.triOfsY[y + 1];
    const uint32_t xb = a.triOfsX[x], xe = a.triOfsX[x + 1];
    Texel acc; acc.r = acc.g = acc.b = acc.a = 0.0f;
    uint32_t h = zb;
    while (h < ze)
    {
        const uint32_t sz = a.triZ[h].x;
        uint32_t hEnd = h + 1;
        while (hEnd < ze && a.triZ[hEnd].x == sz) ++hEnd;
        const ImgView S = slice_of(a.src, sz);
        uint32_t i = yb;
        while (i < ye)
        {
            const uint32_t sy = a.triY[i].x;
            uint32_t iEnd = i + 1;
            while (iEnd < ye && a.triY[iEnd].x == sy) ++iEnd;
            uint32_t k = xb;
            while (k < xe)
            {
                const uint32_t sx = a.triX[k].x;
                uint32_t kEnd = k + 1;
                while (kEnd < xe && a.triX[kEnd].x == sx) ++kEnd;
                const Texel p = load_linear(S, sx, sy, a.srgbIn);
                for (uint32_t g = h; g < hEnd; ++g)
                {
                    const float wz = __uint_as_float(a.triZ[g].y);
                    for (uint32_t j = i; j < iEnd; ++j)
                    {
                        const float wzy = wz * __uint_as_float(a.triY[j].y);
                        for (uint32_t m = k; m < kEnd; ++m)
                        {
                            const float w = wzy * __uint_as_float(a.triX[m].y);
                            acc.r = p.r * w + acc.r; acc.g = p.g * w + acc.g; acc.b = p.b * w + acc.b; acc.a = p.a * w + acc.a;
                        }
                    }
                }
                k = kEnd;
            }
            i = iEnd;
        }
        h = hEnd;
    }
    if (a.dst.format == FMT_R10G10B10A2_UNORM || a.dst.format == FMT_R10G10B10A2_UINT) acc.a = acc.a + 0.1f;       // DirectXTexMipmaps.cpp:2767-2786
    store_linear(slice_of(a.dst, z), x, y, a.srgbOut, acc);
}

// ---- ComputeMSE: sum over texels of (v1 - v2)^2 per channel, accumulated in fp64 ----------------------------------------------
__global__ void __launch_bounds__(256) mse_kernel(ImgView a, ImgView b, int srgbA, int srgbB, int ignoreAlpha, double* out)
{
    __shared__ double part[4][4];
    double s[4] = { 0.0, 0.0, 0.0, 0.0 };
    for (uint32_t y = blockIdx.y; y < a.height; y += gridDim.y)
        for (uint32_t x = blockIdx.x * 256u + threadIdx.x; x < a.width; x += gridDim.x * 256u)
        {
            Texel p = load_texel(a.pixels + uint64_t(y) * a.rowPitch, x, a.format);
            Texel q = load_texel(b.pixels + uint64_t(y) * b.rowPitch, x, b.format);
            // XMVectorPow(v, g_Gamma22) with g_Gamma22 = { 2.2, 2.2, 2.2, 1 } (DirectXTexMisc.cpp:24): alpha keeps its value
            if (srgbA) { p.r = powf(p.r, 2.2f); p.g = powf(p.g, 2.2f); p.b = powf(p.b, 2.2f); }
            if (srgbB) { q.r = powf(q.r, 2.2f); q.g = powf(q.g, 2.2f); q.b = powf(q.b, 2.2f); }
            const float d[4] = { p.r - q.r, p.g - q.g, p.b - q.b, ignoreAlpha ? 0.0f : p.a - q.a };
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c] += double(d[c]) * double(d[c]);
        }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        for (int d = 32; d >= 1; d >>= 1) s[c] += __shfl_xor(s[c], d);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { part[wave][0] = s[0]; part[wave][1] = s[1]; part[wave][2] = s[2]; part[wave][3] = s[3]; }
    __syncthreads();
    if (threadIdx.x < 4)
        atomicAdd(&out[threadIdx.x], part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x]);
}

// the stale tap of a level that has none (the kernels test .pixels)
ImgView no_stale(int format) { return ImgView{ nullptr, 0, 0, 2, format }; }

bool srgb_linear_format(int format)
{
    return format == FMT_R8G8B8A8_UNORM_SRGB || format == FMT_B8G8R8A8_UNORM_SRGB || format == FMT_B8G8R8X8_UNORM_SRGB;
}

bool can_srgb(int format)
{
    // LoadScanlineLinear / StoreScanlineLinear: "can't treat A8, XR, Depth, SNORM, UINT, or SINT as sRGB" (:2842-2858)
    switch (format)
    {
    case FMT_R32G32B32A32_FLOAT: case FMT_R16G16B16A16_FLOAT: case FMT_R16G16B16A16_UNORM: case FMT_R32G32_FLOAT:
    case FMT_R8G8B8A8_UNORM: case FMT_R16G16_FLOAT: case FMT_R16G16_UNORM: case FMT_R32_FLOAT: case FMT_R8G8_UNORM:
    case FMT_R16_FLOAT: case FMT_R16_UNORM: case FMT_R8_UNORM: case FMT_B8G8R8A8_UNORM: case FMT_B8G8R8X8_UNORM:
    case FMT_R32G32B32_FLOAT: case FMT_R10G10B10A2_UNORM: case FMT_R11G11B10_FLOAT: case FMT_R9G9B9E5_SHAREDEXP:
    case FMT_R8G8_B8G8_UNORM: case FMT_G8R8_G8B8_UNORM: case FMT_B5G6R5_UNORM: case FMT_B5G5R5A1_UNORM: case FMT_B4G4R4A4_UNORM:
    case FMT_A4B4G4R4_UNORM:         // the whole list of :2825-2849
        return true;
    default:
        return srgb_linear_format(format);
    }
}

// (format, TEX_FILTER flags) -> what the filter kernels take: sRGB formats filter in linear space and TEX_FILTER_SRGB_IN / OUT force it
// for the other colour formats (LoadScanlineLinear / StoreScanlineLinear, :2803-2945); wrap / mirror addressing per axis.
struct FilterBits { int srgbIn, srgbOut, wrapU, wrapV, wrapW, mirrorU, mirrorV, mirrorW; };
FilterBits decode_filter(int format, uint32_t flags)
{
    const bool linear = can_srgb(format);
    FilterBits f;
    f.srgbIn = (linear && (srgb_linear_format(format) || (flags & TF_SRGB_IN))) ? 1 : 0;
    f.srgbOut = (linear && (srgb_linear_format(format) || (flags & TF_SRGB_OUT))) ? 1 : 0;
    f.wrapU = (flags & DXTEX_FILTER_WRAP_U) != 0; f.wrapV = (flags & DXTEX_FILTER_WRAP_V) != 0; f.wrapW = (flags & TF_WRAP_W) != 0;
    f.mirrorU = (flags & DXTEX_FILTER_MIRROR_U) != 0; f.mirrorV = (flags & DXTEX_FILTER_MIRROR_V) != 0; f.mirrorW = (flags & TF_MIRROR_W) != 0;
    return f;
}

// The 2-D fields of a level's arguments that do not depend on the level
ResizeArgs resize_args(int format, uint32_t filterFlags, bool mipAlias, const TriangleTables* tri)
{
    const FilterBits f = decode_filter(format, filterFlags);
    ResizeArgs a;
    a.srgbIn = f.srgbIn; a.srgbOut = f.srgbOut;
    a.wrapU = f.wrapU; a.wrapV = f.wrapV; a.mirrorU = f.mirrorU; a.mirrorV = f.mirrorV;
    a.mipAlias = mipAlias ? 1 : 0;
    a.stale = no_stale(format);
    a.triOfsX = tri ? tri->ofsX : nullptr; a.triX = tri ? reinterpret_cast<const uint2*>(tri->entX) : nullptr;
    a.triOfsY = tri ? tri->ofsY : nullptr; a.triY = tri ? reinterpret_cast<const uint2*>(tri->entY) : nullptr;
    return a;
}
} // namespace

// The launchers below name the kernel they enqueue (a string literal: dxtex_ctx_profile_end aggregates by pointer) and close the call
// with a null mark, as the BC encoders do; with marks == nullptr (not profiling) nothing is recorded.
#define DXTEX_MARK(NAME) do { if (marks) marks->mark(NAME); } while (0)

hipError_t launch_pack_group(const ImgView& rows, const ImgView& dst, hipStream_t stream, KernelMarks* marks)
{
    if (!dst.width || !dst.height) return hipSuccess;
    const uint32_t per = group_texels(dst.format), groups = (dst.width + per - 1) / per;
    DXTEX_MARK("pack_group");
    hipLaunchKernelGGL(pack_group_kernel, dim3((groups + 255) / 256, grid_rows(dst.height)), dim3(256), 0, stream, rows, dst);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_convert(const ImgView& sv, const ImgView& dv, const ConvertPlan& plan, float threshold, hipStream_t stream, int dither, uint32_t z,
                          KernelMarks* marks)
{
    const uint32_t width = sv.width, height = sv.height;
    if (!width || !height) return hipSuccess;
    const FmtInfo* in = format_info(sv.format);
    const FmtInfo* out = format_info(dv.format);
    // four texels per lane through 16-byte loads / stores where a texel is a whole number of dwords on both sides and rows are 16-byte aligned
    if (in && out && !((in->cls | out->cls) & FC_GROUP) && in->bpp >= 32 && out->bpp >= 32 && (in->bpp % 32) == 0 && (out->bpp % 32) == 0 && (width % 4u) == 0 &&
        ((reinterpret_cast<uintptr_t>(sv.pixels) | sv.rowPitch | reinterpret_cast<uintptr_t>(dv.pixels) | dv.rowPitch) & 15u) == 0)
    {
        const uint32_t quads = width / 4u;
        const uint32_t gx = (quads + 255u) / 256u;
        const uint32_t sq = uint32_t(in->bpp / 8u) * 4u, dq = uint32_t(out->bpp / 8u) * 4u;
        // row groups per workgroup column: enough workgroups to fill 256 CUs several times over, few enough that a lane streams several groups
#define DXTEX_QUAD(SQ, DQ, ROWS) do { const uint32_t groups = (height + (ROWS) - 1u) / (ROWS); \
            const uint32_t gy = std::min<uint32_t>(groups, std::max<uint32_t>(1u, 8192u / gx)); \
            if (dither) { DXTEX_MARK("convert_quad<" #SQ "," #DQ "," #ROWS ",dither>"); \
                          hipLaunchKernelGGL((convert_quad_kernel<SQ, DQ, ROWS, true>), dim3(gx, gy), dim3(256), 0, stream, sv, dv, plan, threshold, sq, dq, dither, z); } \
            else { DXTEX_MARK("convert_quad<" #SQ "," #DQ "," #ROWS ">"); \
                   hipLaunchKernelGGL((convert_quad_kernel<SQ, DQ, ROWS, false>), dim3(gx, gy), dim3(256), 0, stream, sv, dv, plan, threshold, sq, dq, dither, z); } } while (0)
        if (sq == 16u && dq == 16u) DXTEX_QUAD(16, 16, 4);
        else if (sq == 16u && dq == 32u) DXTEX_QUAD(16, 32, 4);
        else if (sq == 16u && dq == 64u) DXTEX_QUAD(16, 64, 4);
        else if (sq == 32u && dq == 16u) DXTEX_QUAD(32, 16, 2);
        else if (sq == 32u && dq == 32u) DXTEX_QUAD(32, 32, 2);
        else if (sq == 32u && dq == 64u) DXTEX_QUAD(32, 64, 2);
        else if (sq == 64u && dq == 16u) DXTEX_QUAD(64, 16, 1);
        else if (sq == 64u && dq == 32u) DXTEX_QUAD(64, 32, 1);
        else DXTEX_QUAD(0, 0, 1);
#undef DXTEX_QUAD
        DXTEX_MARK(nullptr);
        return hipGetLastError();
    }
    const dim3 grid((width + 255) / 256, grid_rows(height));
    if (dither) { DXTEX_MARK("convert<dither>"); hipLaunchKernelGGL(convert_kernel<true>, grid, dim3(256), 0, stream, sv, dv, plan, threshold, dither, z); }
    else { DXTEX_MARK("convert"); hipLaunchKernelGGL(convert_kernel<false>, grid, dim3(256), 0, stream, sv, dv, plan, threshold, dither, z); }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_normal_map(const ImgView& src, const ImgView& dst, uint32_t flags, float amplitude, bool unorm, hipStream_t stream)
{
    const uint32_t width = src.width, height = src.height;
    if (!width || !height) return hipSuccess;
    NmapArgs a;
    a.src = src; a.dst = dst;
    a.flags = flags; a.amplitude = amplitude; a.unorm = unorm ? 1 : 0;
    a.strips = uint32_t((uint64_t(height) + kNmapRows - 1u) / kNmapRows);
    hipLaunchKernelGGL(nmap_kernel, dim3(uint32_t((uint64_t(width) + kNmapThreads - 1u) / kNmapThreads), grid_rows(a.strips)), dim3(kNmapThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_transform(const ImgView& sv, const ImgView& dv, uint32_t op, const XformArgs& args, const uint32_t* maxBits, hipStream_t stream,
                            KernelMarks* marks)
{
    const uint32_t width = sv.width, height = sv.height;
    if (!width || !height) return hipSuccess;
    // about 8192 workgroups, as convert_quad launches: a workgroup walks several rows rather than one workgroup being dispatched per row
    const uint32_t gx = (width + 255) / 256;
    const dim3 grid(gx, std::min<uint32_t>(grid_rows(height), std::max<uint32_t>(1u, 8192u / gx)));
#define DXTEX_XFORM(OP, NAME) do { DXTEX_MARK(NAME); hipLaunchKernelGGL(transform_kernel<OP>, grid, dim3(256), 0, stream, sv, dv, args, maxBits); } while (0)
    switch (op)
    {
    case XFORM_SWIZZLE: DXTEX_XFORM(XFORM_SWIZZLE, "transform<swizzle>"); break;
    case XFORM_TONEMAP: DXTEX_XFORM(XFORM_TONEMAP, "transform<tonemap>"); break;
    case XFORM_COLOR_KEY: DXTEX_XFORM(XFORM_COLOR_KEY, "transform<color_key>"); break;
    case XFORM_INVERT_Y: DXTEX_XFORM(XFORM_INVERT_Y, "transform<invert_y>"); break;
    case XFORM_RECONSTRUCT_Z: DXTEX_XFORM(XFORM_RECONSTRUCT_Z, "transform<reconstruct_z>"); break;
    default: return hipErrorInvalidValue;
    }
#undef DXTEX_XFORM
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_copy_rects(const CopyJob* jobs, size_t count, hipStream_t stream, KernelMarks* marks)
{
    for (size_t first = 0; first < count; first += kCopyBatchMax)
    {
        CopyBatch batch;
        batch.count = uint32_t(std::min<size_t>(kCopyBatchMax, count - first));
        uint32_t units = 0, rows = 0;
        for (uint32_t k = 0; k < batch.count; ++k)
        {
            const CopyJob& j = jobs[first + k];
            batch.job[k] = j;
            units = std::max(units, j.width + (j.vec ? j.tail : 0u));
            rows = std::max(rows, j.vec ? (j.height + 3u) / 4u : j.height);
        }
        for (uint32_t k = batch.count; k < kCopyBatchMax; ++k) batch.job[k] = CopyJob{};
        if (!units || !rows) continue;
        // about 8192 workgroups over the batch, as convert_quad launches: a lane streams several row groups rather than one workgroup per row
        const uint32_t gx = (units + 255u) / 256u;
        const uint32_t gy = std::min<uint32_t>(grid_rows(rows), std::max<uint32_t>(1u, 8192u / (gx * batch.count)));
        DXTEX_MARK("copy_rect");
        hipLaunchKernelGGL(copy_rect_kernel, dim3(gx, gy, batch.count), dim3(256), 0, stream, batch);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    DXTEX_MARK(nullptr);
    return hipSuccess;
}

hipError_t launch_merge(const ImgView& a, const ImgView& b, const ImgView& dst, const MergeArgs& args, hipStream_t stream, KernelMarks* marks)
{
    if (!a.width || !a.height) return hipSuccess;
    if (b.format != FMT_R32G32B32A32_FLOAT || ((reinterpret_cast<uintptr_t>(b.pixels) | b.rowPitch) & 15u)) return hipErrorInvalidValue;
    const uint32_t gx = (a.width + 255) / 256;
    const dim3 grid(gx, std::min<uint32_t>(grid_rows(a.height), std::max<uint32_t>(1u, 8192u / gx)));
    DXTEX_MARK("merge");
    hipLaunchKernelGGL(merge_kernel, grid, dim3(256), 0, stream, a, b, dst, args);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_tonemap_max(const ImgView& src, uint32_t* maxBits, hipStream_t stream, KernelMarks* marks)
{
    const uint32_t width = src.width, height = src.height;
    if (!width || !height) return hipSuccess;
    // about 2048 workgroups at most, each looping over its rows: one atomic per workgroup stays far below the cost of the read
    const uint32_t gx = std::min<uint32_t>((width + 255) / 256, 8), gy = std::min<uint32_t>(height, std::max<uint32_t>(1u, 2048u / gx));
    DXTEX_MARK("tonemap_max");
    hipLaunchKernelGGL(tonemap_max_kernel, dim3(gx, gy), dim3(256), 0, stream, src, maxBits);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

size_t convert_diffuse_scratch_bytes(uint32_t width)
{
    return size_t(5) * width * sizeof(F4);      // pre, err, slot by texel; in, pending by segment (at most one per texel)
}

hipError_t launch_convert_diffuse(const ImgView& src, const ImgView& dst, const ConvertPlan& plan, float threshold, void* scratch,
                                  unsigned long long* rerun, uint32_t segLen, hipStream_t stream)
{
    const uint32_t width = src.width;
    if (!width || !src.height) return hipSuccess;
    DiffuseArgs a;
    a.spec = dither_spec(dst.format);
    if (!a.spec.valid) return hipErrorInvalidValue;
    a.src = src; a.dst = dst;
    a.plan = plan; a.threshold = threshold;
    a.segLen = segLen ? segLen : std::max<uint32_t>(kDiffuseMinSeg, (width + kDiffuseThreads - 1) / kDiffuseThreads);
    a.rerun = rerun;
    F4* f = static_cast<F4*>(scratch);
    a.pre = f; a.err = f + width; a.slot = f + 2 * size_t(width); a.in = f + 3 * size_t(width); a.pending = f + 4 * size_t(width);
    if (width <= kDiffuseLdsTexels) hipLaunchKernelGGL(convert_diffuse_kernel<true>, dim3(1), dim3(kDiffuseThreads), 0, stream, a);
    else hipLaunchKernelGGL(convert_diffuse_kernel<false>, dim3(1), dim3(kDiffuseThreads), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_resize(const ImgView& src, const ImgView& dst, uint32_t filterMode, uint32_t filterFlags, bool mipAlias,
                         const TriangleTables* tri, hipStream_t stream, const ImgView* stale, KernelMarks* marks)
{
    const uint32_t srcW = src.width, srcH = src.height, dstW = dst.width, dstH = dst.height;
    const int format = src.format;
    if (!dstW || !dstH) return hipSuccess;
    ResizeArgs a = resize_args(format, filterFlags, mipAlias, tri);
    if (stale) a.stale = *stale;
    a.src = src; a.dst = dst;
    const dim3 grid((dstW + 255) / 256, grid_rows(dstH)), block(256);
    switch (filterMode)
    {
    case DXTEX_FILTER_POINT: DXTEX_MARK("resize_point"); hipLaunchKernelGGL(resize_point_kernel, grid, block, 0, stream, a); break;
    case DXTEX_FILTER_LINEAR: DXTEX_MARK("resize_linear"); hipLaunchKernelGGL(resize_linear_kernel, grid, block, 0, stream, a); break;
    case DXTEX_FILTER_CUBIC:
        // the 2:1 RGBA8 case of a power-of-two mip chain has a separable kernel (a column strip per lane); the small levels take it too (6 us a
        // launch against 10 - 30 us of the general kernel's sixteen dependent taps)
        if (format == FMT_R8G8B8A8_UNORM && !a.srgbIn && !a.srgbOut && srcW == 2 * dstW && srcH == 2 * dstH &&
            !a.wrapU && !a.wrapV && !a.mirrorU && !a.mirrorV && (src.rowPitch % 4) == 0 && (dst.rowPitch % 4) == 0 &&
            (reinterpret_cast<uintptr_t>(src.pixels) % 4) == 0 && (reinterpret_cast<uintptr_t>(dst.pixels) % 4) == 0)
        {
            // rows per lane: long strips amortise the two extra row passes at their top; short ones keep a small level spread over the chip
            // (at least ~4096 wavefronts while that leaves 4 rows or more per strip)
            uint32_t strip = 32;
            // two destination texels per lane where the rows allow 16-byte loads and 8-byte stores (every level of a power-of-two chain down to 2 texels)
#if !defined(DXTEX_CUBIC_X2)
#define DXTEX_CUBIC_X2 1               // 0: every level through the one-texel-per-lane kernel (A/B builds)
#endif
            const bool pairs = DXTEX_CUBIC_X2 && (dstW % 2) == 0 && (src.rowPitch % 16) == 0 && (dst.rowPitch % 8) == 0 && (reinterpret_cast<uintptr_t>(src.pixels) % 16) == 0 &&
                               (reinterpret_cast<uintptr_t>(dst.pixels) % 8) == 0;
            const uint32_t lanesX = pairs ? dstW / 2 : dstW;
            while (strip > 4 && uint64_t((lanesX + 63) / 64) * ((dstH + strip - 1) / strip) < 4096) strip >>= 1;
            if (pairs)
            {
                DXTEX_MARK("resize_cubic_half_rgba8_x2");
                hipLaunchKernelGGL(resize_cubic_half_rgba8_x2_kernel, dim3((lanesX + 255) / 256, grid_rows((dstH + strip - 1) / strip)), block, 0, stream, a, strip);
            }
            else
            {
                DXTEX_MARK("resize_cubic_half_rgba8");
                hipLaunchKernelGGL(resize_cubic_half_rgba8_kernel, dim3((dstW + 255) / 256, grid_rows((dstH + strip - 1) / strip)), block, 0, stream, a, strip);
            }
        }
        else
        {
            DXTEX_MARK("resize_cubic");
            hipLaunchKernelGGL(resize_cubic_kernel, grid, block, 0, stream, a);
        }
        break;
    case DXTEX_FILTER_BOX:
        if (format == FMT_R8G8B8A8_UNORM && !a.srgbIn && !a.srgbOut && srcW == 2 * dstW && srcH == 2 * dstH && (dstW % 2) == 0 && dstW >= 256 &&
            (src.rowPitch % 16) == 0 && (dst.rowPitch % 8) == 0 && (reinterpret_cast<uintptr_t>(src.pixels) % 16) == 0 && (reinterpret_cast<uintptr_t>(dst.pixels) % 8) == 0)
        {
            DXTEX_MARK("resize_box_half_rgba8");
            hipLaunchKernelGGL(resize_box_half_rgba8_kernel, dim3((dstW / 2 + 255) / 256, grid_rows(dstH)), block, 0, stream, a);
        }
        else
        {
            DXTEX_MARK("resize_box");
            hipLaunchKernelGGL(resize_box_kernel, grid, block, 0, stream, a);
        }
        break;
    case DXTEX_FILTER_TRIANGLE: DXTEX_MARK("resize_triangle"); hipLaunchKernelGGL(resize_triangle_kernel, grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

TailRoute resize_tail_route(const ImgView* levels, int nlevels, uint32_t filterMode, uint32_t filterFlags)
{
    // at least two levels to write (one is a plain launch), all of them in one argument block, from a source that 1024 lanes cover in a few trips
    if (nlevels < 3 || nlevels - 1 > kTailMaxLevels || levels[0].width > kTailSide || levels[0].height > kTailSide) return TailRoute::None;
    const FmtInfo* info = format_info(levels[0].format);
    if (!info || (info->cls & FC_GROUP)) return TailRoute::None;           // grouped formats are stored from float rows, level by level
    // the LDS tail of a power-of-two RGBA8 box / cubic chain: clamp addressing, no sRGB, dword access, every level halves both sides exactly
    bool halving = (filterMode == DXTEX_FILTER_CUBIC || filterMode == DXTEX_FILTER_BOX) && levels[0].format == FMT_R8G8B8A8_UNORM && !(filterFlags & TF_SRGB_WRAP_MIRROR);
    for (int k = 0; halving && k < nlevels; ++k)
    {
        halving = (levels[k].rowPitch % 4) == 0 && (reinterpret_cast<uintptr_t>(levels[k].pixels) % 4) == 0;
        if (k) halving = halving && levels[k].width * 2u == levels[k - 1].width && levels[k].height * 2u == levels[k - 1].height;
    }
    if (halving) return TailRoute::HalvingLds;
    // measured (8192^2 chain, rocprofv3): the box tail takes 15.8 us in one workgroup against 6 launches x 3.2 us; the cubic tail 84 us
    // against 6 x 7 us (sixteen dependent-latency taps per texel and no other workgroup to hide them) - so cubic keeps its launches
    const bool generic = filterMode == DXTEX_FILTER_POINT || filterMode == DXTEX_FILTER_LINEAR || filterMode == DXTEX_FILTER_BOX;
    return generic ? TailRoute::Generic : TailRoute::None;
}

hipError_t launch_resize_tail(const ImgView* levels, int nlevels, uint32_t filterMode, uint32_t filterFlags,
                              const ImgView* twoHigh, hipStream_t stream, KernelMarks* marks)
{
    const int format = levels[0].format;
    switch (resize_tail_route(levels, nlevels, filterMode, filterFlags))
    {
    case TailRoute::HalvingLds:
    {
        CubicTailArgs c;
        c.src = levels[0].pixels; c.srcPitch = levels[0].rowPitch; c.srcW = levels[0].width; c.srcH = levels[0].height; c.nlevels = nlevels - 1;
        for (int k = 0; k < kTailMaxLevels; ++k) { const ImgView& d = levels[k + 1 < nlevels ? k + 1 : 1]; c.dst[k] = d.pixels; c.dstPitch[k] = d.rowPitch; }
        if (filterMode == DXTEX_FILTER_CUBIC) { DXTEX_MARK("resize_half_tail_rgba8<cubic>"); hipLaunchKernelGGL(resize_half_tail_rgba8_kernel<true>, dim3(1), dim3(1024), 0, stream, c); }
        else { DXTEX_MARK("resize_half_tail_rgba8<box>"); hipLaunchKernelGGL(resize_half_tail_rgba8_kernel<false>, dim3(1), dim3(1024), 0, stream, c); }
        break;
    }
    case TailRoute::Generic:
    {
        TailArgs t;
        t.a = resize_args(format, filterFlags, true, nullptr);
        t.a.src = levels[0];
        t.a.dst = levels[0];
        t.nlevels = nlevels - 1;
        StaleTap<ImgView> tap{ twoHigh ? *twoHigh : no_stale(format) };
        for (int k = 0; k < kTailMaxLevels; ++k)
        {
            const bool used = k + 1 < nlevels;                  // level k + 1 is filtered from level k; unused slots repeat the first level
            t.level[k] = levels[used ? k + 1 : 1];
            t.stale[k] = (used && tap.step(levels[k], filterMode == DXTEX_FILTER_BOX)) ? tap.twoHigh : no_stale(format);
        }
        t.mode = filterMode;
        DXTEX_MARK("resize_tail");
        hipLaunchKernelGGL(resize_tail_kernel, dim3(1), dim3(1024), 0, stream, t);
        break;
    }
    default: return hipErrorInvalidValue;
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_pmalpha(const ImgView& src, const ImgView& dst, uint32_t pmFlags, hipStream_t stream, KernelMarks* marks)
{
    const int format = src.format;
    if (!src.width || !src.height) return hipSuccess;
    // TEX_PMALPHA_IGNORE_SRGB: plain Load/StoreScanline; otherwise the *Linear wrappers with the SRGB_IN/OUT bits (:68-112), which are TEX_FILTER's
    const FilterBits f = (pmFlags & DXTEX_PMALPHA_IGNORE_SRGB) ? FilterBits{} : decode_filter(format, pmFlags & (TF_SRGB_IN | TF_SRGB_OUT));
    DXTEX_MARK("pmalpha");
    hipLaunchKernelGGL(pmalpha_kernel, dim3((src.width + 255) / 256, grid_rows(src.height)), dim3(256), 0, stream, src, dst,
                       f.srgbIn, f.srgbOut, (pmFlags & DXTEX_PMALPHA_REVERSE) ? 1 : 0);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_scale_alpha(const ImgView& src, const ImgView& dst, float scale, hipStream_t stream, KernelMarks* marks)
{
    if (!src.width || !src.height) return hipSuccess;
    DXTEX_MARK("scale_alpha");
    hipLaunchKernelGGL(scale_alpha_kernel, dim3((src.width + 255) / 256, grid_rows(src.height)), dim3(256), 0, stream, src, dst, scale);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_alpha_coverage(const ImgView& src, float scale, float alphaReference, unsigned long long* count, hipStream_t stream, KernelMarks* marks)
{
    hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned long long), stream);
    if (e != hipSuccess) return e;
    if (src.width < 2 || src.height < 2) return hipSuccess;
    DXTEX_MARK("alpha_coverage");
    hipLaunchKernelGGL(alpha_coverage_kernel, dim3((src.width - 1 + 255) / 256, grid_rows(src.height - 1)), dim3(256), 0, stream,
                       src, scale, alphaReference, count);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_alpha_below(const ImgView& src, float threshold, unsigned long long* count, hipStream_t stream, KernelMarks* marks)
{
    if (!src.width || !src.height) return hipSuccess;
    const uint32_t gx = std::min<uint32_t>((src.width + 255) / 256, 64), gy = std::min<uint32_t>(src.height, 2048);
    DXTEX_MARK("alpha_below");
    hipLaunchKernelGGL(alpha_below_kernel, dim3(gx, gy), dim3(256), 0, stream, src, threshold, count);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_resize3d(const VolumeView& src, const VolumeView& dst, uint32_t filterMode, uint32_t filterFlags, const TriangleTables3* tri,
                           hipStream_t stream, const ImgView* staleU, const ImgView* staleV, KernelMarks* marks)
{
    if (!dst.width || !dst.height || !dst.depth) return hipSuccess;
    Resize3Args a;
    a.src = src; a.dst = dst;
    const int format = src.format;
    const FilterBits f = decode_filter(format, filterFlags);
    a.srgbIn = f.srgbIn; a.srgbOut = f.srgbOut;
    a.wrapU = f.wrapU; a.wrapV = f.wrapV; a.wrapW = f.wrapW; a.mirrorU = f.mirrorU; a.mirrorV = f.mirrorV; a.mirrorW = f.mirrorW;
    a.staleU = staleU ? *staleU : no_stale(format);
    a.staleV = staleV ? *staleV : no_stale(format);
    a.triOfsX = tri ? tri->ofsX : nullptr; a.triX = tri ? reinterpret_cast<const uint2*>(tri->entX) : nullptr;
    a.triOfsY = tri ? tri->ofsY : nullptr; a.triY = tri ? reinterpret_cast<const uint2*>(tri->entY) : nullptr;
    a.triOfsZ = tri ? tri->ofsZ : nullptr; a.triZ = tri ? reinterpret_cast<const uint2*>(tri->entZ) : nullptr;
    const dim3 grid((dst.width + 255) / 256, dst.height, dst.depth), block(256);
    switch (filterMode)
    {
    case DXTEX_FILTER_POINT: DXTEX_MARK("resize3d_point"); hipLaunchKernelGGL(resize3d_point_kernel, grid, block, 0, stream, a); break;
    case DXTEX_FILTER_LINEAR: DXTEX_MARK("resize3d_linear"); hipLaunchKernelGGL(resize3d_linear_kernel, grid, block, 0, stream, a); break;
    case DXTEX_FILTER_CUBIC: DXTEX_MARK("resize3d_cubic"); hipLaunchKernelGGL(resize3d_cubic_kernel, grid, block, 0, stream, a); break;
    case DXTEX_FILTER_BOX: DXTEX_MARK("resize3d_box"); hipLaunchKernelGGL(resize3d_box_kernel, grid, block, 0, stream, a); break;
    case DXTEX_FILTER_TRIANGLE: DXTEX_MARK("resize3d_triangle"); hipLaunchKernelGGL(resize3d_triangle_kernel, grid, block, 0, stream, a); break;
    default: return hipErrorInvalidValue;
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_mse(const ImgView& a, const ImgView& b, double* out4, hipStream_t stream, KernelMarks* marks)
{
    const uint32_t width = a.width, height = a.height;
    const int aFormat = a.format, bFormat = b.format;
    hipError_t e = hipMemsetAsync(out4, 0, 4 * sizeof(double), stream);
    if (e != hipSuccess) return e;
    if (!width || !height) return hipSuccess;
    const bool ignoreAlpha = aFormat == FMT_B8G8R8X8_UNORM || aFormat == FMT_B8G8R8X8_UNORM_SRGB || bFormat == FMT_B8G8R8X8_UNORM || bFormat == FMT_B8G8R8X8_UNORM_SRGB;
    const uint32_t gx = std::min<uint32_t>((width + 255) / 256, 64), gy = std::min<uint32_t>(height, 1024);
    DXTEX_MARK("mse");
    hipLaunchKernelGGL(mse_kernel, dim3(gx, gy), dim3(256), 0, stream, a, b, srgb_linear_format(aFormat) ? 1 : 0, srgb_linear_format(bFormat) ? 1 : 0,
                       ignoreAlpha ? 1 : 0, out4);
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
#undef DXTEX_MARK
} // namespace dxtex
