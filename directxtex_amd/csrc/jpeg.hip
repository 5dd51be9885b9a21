// JPEG samples on gfx950 (dxtex_jpeg.h holds the rules): everything a .jpg needs behind the host's Huffman walk, so that a file crosses PCIe
// as its quantised coefficients and the integer arithmetic that is independent per block and per texel runs here. Two kernels on the
// caller's stream, nothing between them on the host:
//   jpeg_idct_kernel    every 8 x 8 block of every component in one launch: coefficient * quantiser entry, jidctint.c's two passes, the
//                       range limit. A grey frame is this kernel alone: its samples go straight into the R8_UNORM image through its pitch,
//                       cropped to width and height. A colour frame's samples go into block-padded uint8 planes in memory of the context.
//   jpeg_colour_kernel  per texel of the image: the three samples at it - chroma through jdsample.c's fancy filters, never written out at
//                       full size - jdcolor.c's transform, the clamp, alpha 0xff, one store.
//
// jpeg_idct_kernel: one lane a block, 256 blocks a workgroup. A lane loads its block's 64 coefficients as eight 16-byte accesses (a whole
// 128-byte line to itself; from a base that is no multiple of 16, 2-byte reads), dequantises them with the quantiser tables, which arrive by
// value in the kernel's arguments and are held in LDS, keeps the 64-word workspace in registers through both passes - every index is a
// constant once unrolled - and stores each row's 8 samples as one 8-byte access where the row is whole and aligned (always so in a plane).
// The other mapping - eight lanes a block, lane j loading row j, the 8 x 8 transposes between the passes through LDS - was built and measured
// beside this one, alternating, three runs each at 4096 x 4096: it read a block as one coalesced 128-byte access but took 0.0244 against
// 0.0233 ms for 4:2:0, 0.0408 against 0.0358 ms for 4:4:4 and 0.0182 against 0.0173 ms for grey (profiles/jpeg.md), with three barriers and
// 9 KiB of LDS that this one does not need. It offered eight times the lanes for a small image, whose kernel is a few microseconds either way.
//
// jpeg_colour_kernel: 256 lanes, x across, rows strided over gridDim.y (dxtex_stream.h's grid). Two routes:
//   wide    a lane takes four texels and stores them as one dwordx4; the luma samples are one dword.
//           THE RULE: width is a multiple of 4, and the image's base and row pitch are multiples of 16.
//   narrow  everything else: a lane takes one texel, stored as a dword where base and pitch are multiples of 4, else byte by byte.
//
// Every coefficient read lies inside the frame's blocks, every plane access inside the planes' padded rows, and every image write inside
// its row's `width` texels: a lane stores only where its block, row or first texel lies inside.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_jpeg.h"

namespace dxtex
{
namespace
{
struct IdctArgs
{
    uint16_t quant[4][64];
    uint32_t first[4];              // the first block of each component in the launch's numbering; first[components] = all of them
    uint32_t blocksPerRow[3], quantOf[3];
    uint8_t* out[3];                // grey: the image; colour: the component's plane
    uint64_t pitch[3];
    uint32_t width, height;         // grey: the crop; colour: unused (the planes are whole blocks)
    uint32_t components;
};

template<bool ALIGNED>
__global__ void __launch_bounds__(256) jpeg_idct_kernel(const int16_t* coefficients, IdctArgs a)
{
    __shared__ uint16_t quant[4 * 64];
    quant[threadIdx.x] = a.quant[threadIdx.x >> 6][threadIdx.x & 63u];
    __syncthreads();
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.first[a.components]) return;
    const uint32_t c = a.components > 1u ? uint32_t(g >= a.first[1]) + uint32_t(g >= a.first[2]) : 0u;
    const int16_t* blk = coefficients + uint64_t(g) * 64u;
    const uint16_t* q = quant + a.quantOf[c] * 64u;
    int32_t ws[64];
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r)
    {
        if constexpr (ALIGNED)
        {
            const uint4 t = reinterpret_cast<const uint4*>(blk)[r];
            const uint32_t d[4] = { t.x, t.y, t.z, t.w };
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) { ws[r * 8 + 2 * k] = jpeg_dequant(int16_t(d[k] & 0xFFFFu), q[r * 8 + 2 * k]); ws[r * 8 + 2 * k + 1] = jpeg_dequant(int16_t(d[k] >> 16), q[r * 8 + 2 * k + 1]); }
        }
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) ws[r * 8 + k] = jpeg_dequant(blk[r * 8 + k], q[r * 8 + k]);
        }
    }
#pragma unroll
    for (uint32_t col = 0; col < 8; ++col)
    {
        int32_t in[8], out[8];
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) in[r] = ws[r * 8 + col];
        jpeg_idct_pass(in, out, 11);
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) ws[r * 8 + col] = out[r];
    }
    const uint32_t local = g - a.first[c], bx = local % a.blocksPerRow[c], by = local / a.blocksPerRow[c];
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r)
    {
        int32_t in[8], out[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) in[k] = ws[r * 8 + k];
        jpeg_idct_pass(in, out, 18);
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) { lo |= jpeg_range_limit(out[k]) << (8u * k); hi |= jpeg_range_limit(out[4 + k]) << (8u * k); }
        const uint32_t x = bx * 8u, y = by * 8u + r;
        uint8_t* d = a.out[c] + uint64_t(y) * a.pitch[c] + x;
        if (a.components > 1u) { *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi); continue; }
        if (y >= a.height || x >= a.width) continue;
        const uint32_t n = a.width - x < 8u ? a.width - x : 8u;
        if (n == 8u && multiple_of(d, 0, 8u)) { *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi); continue; }
        const uint64_t both = uint64_t(lo) | (uint64_t(hi) << 32);
        for (uint32_t k = 0; k < n; ++k) d[k] = uint8_t(both >> (8u * k));
    }
}

struct ColourArgs
{
    JpegPlane plane[3];
    int colour;
};

template<bool WIDE>
__global__ void __launch_bounds__(256) jpeg_colour_kernel(ColourArgs a, ImgView dst, bool dwords)
{
    constexpr uint32_t G = WIDE ? 4u : 1u;
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * G;
    if (x >= dst.width) return;
    for (uint32_t y = blockIdx.y; y < dst.height; y += gridDim.y)
    {
        uint8_t* d = dst.pixels + uint64_t(y) * dst.rowPitch + uint64_t(x) * 4u;
        if constexpr (WIDE)
        {
            // luma is 1 x 1 and its plane's rows start on 8 bytes: four samples are one dword
            const uint32_t luma = *reinterpret_cast<const uint32_t*>(a.plane[0].samples + uint64_t(y) * a.plane[0].pitch + x);
            uint32_t t[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                t[k] = jpeg_texel(a.colour, (luma >> (8u * k)) & 0xFFu, jpeg_upsample(a.plane[1], x + k, y), jpeg_upsample(a.plane[2], x + k, y));
            store_span<4>(d, t);
        }
        else
        {
            const uint32_t t = jpeg_texel(a.colour, jpeg_upsample(a.plane[0], x, y), jpeg_upsample(a.plane[1], x, y), jpeg_upsample(a.plane[2], x, y));
            store1<4>(d, t, dwords);
        }
    }
}

size_t plane_bytes(const JpegComponent& c) { return (size_t(c.blocksPerRow) * 8u * c.blockRows * 8u + 255u) & ~size_t(255); }
} // namespace

size_t jpeg_plane_bytes(const JpegFrame& f)
{
    size_t total = 0;
    for (uint32_t c = 0; f.components > 1u && c < f.components; ++c) total += plane_bytes(f.comp[c]);
    return total;
}

hipError_t launch_jpeg_decode(const int16_t* coefficients, const JpegFrame& f, const ImgView& dv, uint8_t* planes, hipStream_t hs, KernelMarks* marks)
{
    if (!dv.width || !dv.height) return hipSuccess;
    if (f.components != 1u && f.components != 3u) return hipErrorInvalidValue;
    if (f.components == 3u && !planes) return hipErrorInvalidValue;
    IdctArgs ia = {};
    for (uint32_t t = 0; t < 4; ++t) for (uint32_t k = 0; k < 64; ++k) ia.quant[t][k] = f.quant[t][k];
    ColourArgs ca = {};
    ca.colour = f.colour;
    uint32_t blocks = 0;
    size_t at = 0;
    for (uint32_t c = 0; c < f.components; ++c)
    {
        const JpegComponent& k = f.comp[c];
        ia.first[c] = blocks;
        blocks += k.blocksPerRow * k.blockRows;
        ia.blocksPerRow[c] = k.blocksPerRow; ia.quantOf[c] = k.quant & 3u;
        if (f.components == 1u) { ia.out[0] = dv.pixels; ia.pitch[0] = dv.rowPitch; }
        else
        {
            ia.out[c] = planes + at; ia.pitch[c] = uint64_t(k.blocksPerRow) * 8u;
            const uint32_t hmax = f.comp[0].h, vmax = f.comp[0].v;
            ca.plane[c] = JpegPlane{ planes + at, k.blocksPerRow * 8u, jpeg_downsampled(f.width, k.h, hmax), jpeg_downsampled(f.height, k.v, vmax), hmax / k.h, vmax / k.v };
            at += plane_bytes(k);
        }
    }
    for (uint32_t c = f.components; c < 4; ++c) ia.first[c] = blocks;
    ia.width = dv.width; ia.height = dv.height; ia.components = f.components;
    const dim3 grid((blocks + 255u) / 256u);
    if (multiple_of(coefficients, 0, 16u))
    {
        DXTEX_MARK("jpeg_idct");
        hipLaunchKernelGGL((jpeg_idct_kernel<true>), grid, dim3(256), 0, hs, coefficients, ia);
    }
    else
    {
        DXTEX_MARK("jpeg_idct<unaligned>");
        hipLaunchKernelGGL((jpeg_idct_kernel<false>), grid, dim3(256), 0, hs, coefficients, ia);
    }
    if (f.components == 3u)
    {
        if (dv.width % 4u == 0 && multiple_of(dv.pixels, dv.rowPitch, 16u))
        {
            DXTEX_MARK("jpeg_colour<wide>");
            hipLaunchKernelGGL((jpeg_colour_kernel<true>), stream_grid(dv.width, dv.height, 4u), dim3(256), 0, hs, ca, dv, true);
        }
        else
        {
            DXTEX_MARK("jpeg_colour<narrow>");
            hipLaunchKernelGGL((jpeg_colour_kernel<false>), stream_grid(dv.width, dv.height, 1u), dim3(256), 0, hs, ca, dv, multiple_of(dv.pixels, dv.rowPitch, 4u));
        }
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
} // namespace dxtex
