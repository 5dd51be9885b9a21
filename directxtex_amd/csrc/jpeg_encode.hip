// JPEG coefficients on gfx950 (dxtex_jpeg.h holds the rules): everything a .jpg needs in front of the host's Huffman coder, so that a resident
// image comes down as its quantised coefficients - 2 bytes a texel for grey, 3 for 4:2:0 - and never as pixels. jpeg.hip run backwards. Two
// kernels on the caller's stream, nothing between them on the host:
//   jpeg_samples_kernel  colour frames only. Reads the image once: jccolor.c's transform per texel, jcsample.c's 2 x 1 or 2 x 2 average for
//                        chroma, and jcprepct.c's edge replication out to whole MCUs, into three block-padded uint8 planes in memory of the
//                        context (jpeg_plane_bytes's layout, the reader's).
//   jpeg_fdct_kernel     every 8 x 8 block of every component in one launch: the level shift, jfdctint.c's two passes, jcdctmgr.c's
//                        quantiser, jccoefct.c's dummy blocks. A grey frame is this kernel alone: it reads the R8_UNORM image through its
//                        pitch with clamped coordinates.
//
// jpeg_samples_kernel: 256 lanes, a lane takes 8 texels across and vs rows down (vs = the luma's vertical factor) of the padded luma plane,
// rows strided over gridDim.y (dxtex_stream.h's grid). It stores each luma row's 8 samples as one 8-byte access and each chroma plane's
// 8 (1 x 1) or 4 (2 x 1, 2 x 2) samples as one 8- or 4-byte access; plane rows start on 8 bytes and a lane's samples on 4. Two routes, which
// differ in the loads alone:
//   wide    two 16-byte loads of four texels a row. THE RULE: width is a multiple of 4, and the image's base and row pitch are multiples of
//           16. A quad at or past the image's width is its last texel four times.
//   narrow  everything else: a texel at a time, as a dword where base and pitch are multiples of 4, else byte by byte, columns clamped.
// Past the chroma plane's own ceil(height / 2) rows a 2 x 2 lane repeats the plane's last row while its luma rows repeat the image's last
// row (dxtex_jpeg.h, jpeg_plane_sample): those lanes - at most 7 rows of them - read twice.
//
// jpeg_fdct_kernel: one lane a block, 256 blocks a workgroup, as jpeg_idct_kernel and for its reasons; the other mapping was not built for
// this direction. A lane loads its block as eight 8-byte accesses (grey: where the row's 8 texels lie inside the image and on 8 bytes, else
// byte by byte with clamped columns), keeps the 64-word workspace in registers through both passes, quantises with the tables, which arrive
// by value in the kernel's arguments and are held in LDS, and stores 64 int16 as eight 16-byte accesses (to a base that is no multiple of
// 16: 2-byte stores). A dummy block's lane transforms the block whose DC it takes and stores zeros behind it: no pass on the host.
//
// Every image read lies inside width x height, every plane access inside the planes' padded rows, every coefficient store inside the
// frame's blocks. The image is never written.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_jpeg.h"

namespace dxtex
{
namespace
{
struct SamplesArgs
{
    uint8_t* plane[3];
    uint32_t pitch[3];
    uint32_t paddedWidth, units;          // of the luma plane; units = its rows / vs
    uint32_t hs, vs, chromaRows;          // chromaRows = ceil(height / vs): the chroma planes' own
    bool bgr;
};

template<bool WIDE>
__global__ void __launch_bounds__(256) jpeg_samples_kernel(SamplesArgs a, ImgView src, bool dwords)
{
    const uint32_t x0 = (blockIdx.x * 256u + threadIdx.x) * 8u;
    if (x0 >= a.paddedWidth) return;
    const uint32_t lastX = src.width - 1u, lastY = src.height - 1u;
    // 8 texels of row `row` from column x0, as Y | Cb << 8 | Cr << 16
    auto load_row = [&](uint32_t row, uint32_t (&t)[8])
    {
        const uint8_t* s = src.pixels + uint64_t(row) * src.rowPitch;
        if constexpr (WIDE)
        {
#pragma unroll
            for (uint32_t q = 0; q < 2; ++q)
            {
                const uint32_t x = x0 + 4u * q;
                uint32_t w[4];
                if (x < src.width) load_span<4>(s + uint64_t(x) * 4u, w);          // width % 4 == 0: the whole quad is inside
                else w[0] = w[1] = w[2] = w[3] = *reinterpret_cast<const uint32_t*>(s + uint64_t(lastX) * 4u);
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) t[4 * q + k] = jpeg_ycc(w[k], a.bgr);
            }
        }
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k)
            {
                const uint32_t x = x0 + k < lastX ? x0 + k : lastX;
                t[k] = jpeg_ycc(load1<4>(s + uint64_t(x) * 4u, dwords), a.bgr);
            }
        }
    };
    auto store_luma = [&](uint32_t row, const uint32_t (&t)[8])
    {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) { lo |= (t[k] & 0xFFu) << (8u * k); hi |= (t[4 + k] & 0xFFu) << (8u * k); }
        *reinterpret_cast<uint2*>(a.plane[0] + uint64_t(row) * a.pitch[0] + x0) = make_uint2(lo, hi);
    };
    for (uint32_t u = blockIdx.y; u < a.units; u += gridDim.y)
    {
        const uint32_t cy = u < a.chromaRows ? u : a.chromaRows - 1u;
        const bool same = a.vs == 1u || u < a.chromaRows;          // the luma rows are the rows the chroma is averaged from
        uint32_t cb[8] = {}, cr[8] = {}, t[8];
        for (uint32_t j = 0; j < a.vs; ++j)
        {
            const uint32_t row = a.vs * cy + j;
            load_row(row < lastY ? row : lastY, t);
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) { cb[k] += (t[k] >> 8) & 0xFFu; cr[k] += t[k] >> 16; }
            if (same) store_luma(a.vs * u + j, t);
        }
        if (!same)
        {
            load_row(lastY, t);
            store_luma(2u * u, t);
            store_luma(2u * u + 1u, t);
        }
        if (a.hs == 1u)
        {
            uint32_t w[2][2] = {};
#pragma unroll
            for (uint32_t k = 0; k < 8; ++k) { w[0][k >> 2] |= cb[k] << (8u * (k & 3u)); w[1][k >> 2] |= cr[k] << (8u * (k & 3u)); }
            store_span<2>(a.plane[1] + uint64_t(u) * a.pitch[1] + x0, w[0]);
            store_span<2>(a.plane[2] + uint64_t(u) * a.pitch[2] + x0, w[1]);
        }
        else
        {
            uint32_t w[2] = {};
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
            {
                const uint32_t bias = jpeg_downsample_bias(a.vs, k);          // x0 / 2 is even: the column's parity is k's
                w[0] |= ((cb[2 * k] + cb[2 * k + 1] + bias) >> a.vs) << (8u * k);
                w[1] |= ((cr[2 * k] + cr[2 * k + 1] + bias) >> a.vs) << (8u * k);
            }
            *reinterpret_cast<uint32_t*>(a.plane[1] + uint64_t(u) * a.pitch[1] + (x0 >> 1)) = w[0];
            *reinterpret_cast<uint32_t*>(a.plane[2] + uint64_t(u) * a.pitch[2] + (x0 >> 1)) = w[1];
        }
    }
}

struct FdctArgs
{
    uint16_t quant[4][64];
    uint32_t first[4];              // the first block of each component in the launch's numbering; first[components] = all of them
    uint32_t blocksPerRow[3], quantOf[3];
    uint32_t realWidth[3], realHeight[3], h[3];          // the blocks that hold the component's own samples, and its horizontal factor
    const uint8_t* in[3];           // grey: the image; colour: the component's plane
    uint64_t pitch[3];
    uint32_t width, height;         // grey: the image's, for the clamp; colour: unused (the planes are whole blocks)
    uint32_t components;
};

template<bool ALIGNED>
__global__ void __launch_bounds__(256) jpeg_fdct_kernel(FdctArgs a, int16_t* coefficients)
{
    __shared__ uint16_t quant[4 * 64];
    quant[threadIdx.x] = a.quant[threadIdx.x >> 6][threadIdx.x & 63u];
    __syncthreads();
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= a.first[a.components]) return;
    const uint32_t c = a.components > 1u ? uint32_t(g >= a.first[1]) + uint32_t(g >= a.first[2]) : 0u;
    const uint16_t* q = quant + a.quantOf[c] * 64u;
    const uint32_t local = g - a.first[c];
    uint32_t bx = local % a.blocksPerRow[c], by = local / a.blocksPerRow[c], sx = 0, sy = 0;
    const bool dummy = jpeg_dummy_block(bx, by, a.realWidth[c], a.realHeight[c], a.h[c], sx, sy);
    if (dummy) { bx = sx; by = sy; }
    int32_t ws[64];
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r)
    {
        uint32_t x = bx * 8u, y = by * 8u + r;
        uint64_t both;
        if (a.components > 1u) { const uint2 t = *reinterpret_cast<const uint2*>(a.in[c] + uint64_t(y) * a.pitch[c] + x); both = uint64_t(t.x) | (uint64_t(t.y) << 32); }
        else
        {
            y = y < a.height ? y : a.height - 1u;
            const uint8_t* s = a.in[0] + uint64_t(y) * a.pitch[0];
            if (x + 8u <= a.width && multiple_of(s + x, 0, 8u)) { const uint2 t = *reinterpret_cast<const uint2*>(s + x); both = uint64_t(t.x) | (uint64_t(t.y) << 32); }
            else
            {
                both = 0;
                for (uint32_t k = 0; k < 8; ++k) both |= uint64_t(s[x + k < a.width ? x + k : a.width - 1u]) << (8u * k);
            }
        }
        int32_t in[8], out[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) in[k] = int32_t(uint32_t(both >> (8u * k)) & 0xFFu) - 128;
        jpeg_fdct_pass(in, out, true);
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) ws[r * 8 + k] = out[k];
    }
#pragma unroll
    for (uint32_t col = 0; col < 8; ++col)
    {
        int32_t in[8], out[8];
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) in[r] = ws[r * 8 + col];
        jpeg_fdct_pass(in, out, false);
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) ws[r * 8 + col] = uint16_t(jpeg_quantise(out[r], q[r * 8 + col]));
    }
    int16_t* blk = coefficients + uint64_t(g) * 64u;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r)
    {
        uint32_t w[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) w[k] = dummy ? 0u : uint32_t(ws[r * 8 + 2 * k]) | (uint32_t(ws[r * 8 + 2 * k + 1]) << 16);
        if (dummy && r == 0) w[0] = uint32_t(ws[0]);
        if constexpr (ALIGNED) store_span<4>(reinterpret_cast<uint8_t*>(blk + r * 8), w);
        else
        {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) { blk[r * 8 + 2 * k] = int16_t(uint16_t(w[k])); blk[r * 8 + 2 * k + 1] = int16_t(uint16_t(w[k] >> 16)); }
        }
    }
}
} // namespace

hipError_t launch_jpeg_encode(const ImgView& sv, bool bgr, const JpegFrame& f, int16_t* coefficients, uint8_t* planes, hipStream_t hs, KernelMarks* marks)
{
    if (!sv.width || !sv.height) return hipSuccess;
    if (f.components != 1u && f.components != 3u) return hipErrorInvalidValue;
    if (f.components == 3u && !planes) return hipErrorInvalidValue;
    FdctArgs fa = {};
    for (uint32_t t = 0; t < 4; ++t) for (uint32_t k = 0; k < 64; ++k) fa.quant[t][k] = f.quant[t][k];
    SamplesArgs sa = {};
    const uint32_t hmax = f.comp[0].h, vmax = f.comp[0].v;
    uint32_t blocks = 0;
    size_t at = 0;
    for (uint32_t c = 0; c < f.components; ++c)
    {
        const JpegComponent& k = f.comp[c];
        fa.first[c] = blocks;
        blocks += k.blocksPerRow * k.blockRows;
        fa.blocksPerRow[c] = k.blocksPerRow; fa.quantOf[c] = k.quant & 3u; fa.h[c] = k.h;
        fa.realWidth[c] = jpeg_real_blocks(f.width, k.h, hmax); fa.realHeight[c] = jpeg_real_blocks(f.height, k.v, vmax);
        if (f.components == 1u) { fa.in[0] = sv.pixels; fa.pitch[0] = sv.rowPitch; }
        else
        {
            fa.in[c] = planes + at; fa.pitch[c] = uint64_t(k.blocksPerRow) * 8u;
            sa.plane[c] = planes + at; sa.pitch[c] = k.blocksPerRow * 8u;
            at += (size_t(k.blocksPerRow) * 8u * k.blockRows * 8u + 255u) & ~size_t(255);          // jpeg_plane_bytes's layout
        }
    }
    for (uint32_t c = f.components; c < 4; ++c) fa.first[c] = blocks;
    fa.width = sv.width; fa.height = sv.height; fa.components = f.components;
    if (f.components == 3u)
    {
        sa.paddedWidth = f.comp[0].blocksPerRow * 8u; sa.units = f.comp[0].blockRows * 8u / vmax;
        sa.hs = hmax; sa.vs = vmax; sa.chromaRows = jpeg_downsampled(f.height, 1u, vmax); sa.bgr = bgr;
        if (sv.width % 4u == 0 && multiple_of(sv.pixels, sv.rowPitch, 16u))
        {
            DXTEX_MARK("jpeg_samples<wide>");
            hipLaunchKernelGGL((jpeg_samples_kernel<true>), stream_grid(sa.paddedWidth, sa.units, 8u), dim3(256), 0, hs, sa, sv, true);
        }
        else
        {
            DXTEX_MARK("jpeg_samples<narrow>");
            hipLaunchKernelGGL((jpeg_samples_kernel<false>), stream_grid(sa.paddedWidth, sa.units, 8u), dim3(256), 0, hs, sa, sv, multiple_of(sv.pixels, sv.rowPitch, 4u));
        }
    }
    const dim3 grid((blocks + 255u) / 256u);
    if (multiple_of(coefficients, 0, 16u))
    {
        DXTEX_MARK("jpeg_fdct");
        hipLaunchKernelGGL((jpeg_fdct_kernel<true>), grid, dim3(256), 0, hs, fa, coefficients);
    }
    else
    {
        DXTEX_MARK("jpeg_fdct<unaligned>");
        hipLaunchKernelGGL((jpeg_fdct_kernel<false>), grid, dim3(256), 0, hs, fa, coefficients);
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
} // namespace dxtex
