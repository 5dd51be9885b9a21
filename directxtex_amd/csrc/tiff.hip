// TIFF texels on gfx950 (dxtex_tiff.h holds the rules): what the .tif codec does per byte and per texel behind LZW, PackBits and inflate,
// so that a file's strips and tiles cross PCIe as they leave the decoder.
//   tiff_undo_kernel     the predictor, in place: every row of every segment is an inclusive prefix sum over 8- or 16-bit elements with a
//                        stride of S elements (predictor 3 is the 8-bit sum over the row's bytes). A workgroup takes a row; a lane takes 48
//                        bytes of it - whole pixels - and sums them per sample, the wave scans the S sums (__shfl_up), LDS carries them
//                        across the four waves, and a row longer than one tile (kTiffUndoTile) is walked tile by tile with the carry in
//                        registers. One launch; no workgroup waits on another. A big-endian 16-bit row is swapped in the same pass.
//   tiff_texels_kernel   one lane per texel of a segment: reads the samples where they lie (tiff_sample: sub-byte samples, the four byte
//                        planes of predictor 3, big-endian samples the undo did not touch), makes the texel (tiff_texel: WhiteIsZero,
//                        the palette from LDS, the alpha RGB lacks) and stores it at its place in the image; a separate plane's segment
//                        stores its one component of every texel
//   tiff_pack_kernel     the writer's BGR sources: B8G8R8A8 -> RGBA, B8G8R8X8 -> RGB at 3 bytes, tight rows
//
// Routes. tiff_undo: wide where the stream's base, every segment's offset and every rowBytes are multiples of 16 - a lane's 48 bytes move
// as three dwordx4 - narrow otherwise, byte by byte; a lane whose run crosses the row's end moves the bytes it has one by one on either
// route, so nothing outside a row is read or written. tiff_texels: wide where the image's base and pitch are multiples of the texel's
// access (its bytes; 4 for a 12-byte texel) - one store a texel or component - narrow otherwise, as bytes. tiff_pack: wide where width is a
// multiple of 4 and the image's base and pitch and the rows' base are multiples of 16 - a lane takes four texels - narrow otherwise.
// Segment descriptors come in the kernels' arguments, kTiffBatchMax a launch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "dxtex_kernels.h"
#include "dxtex_tiff.h"

namespace dxtex
{
namespace
{
struct TiffBatch { TiffSegment seg[kTiffBatchMax]; };

constexpr uint32_t kLaneDwords = kTiffUndoLaneBytes / 4u;

// the lane's run: `valid` (0..48) bytes at p, the rest zero
template<bool WIDE>
__device__ __forceinline__ void load_run(const uint8_t* p, uint32_t valid, uint32_t (&w)[kLaneDwords])
{
    if (WIDE && valid == kTiffUndoLaneBytes) { load_span<kLaneDwords>(p, w); return; }
#pragma unroll
    for (uint32_t k = 0; k < kLaneDwords; ++k)
    {
        const uint32_t rem = valid > 4u * k ? (valid - 4u * k < 4u ? valid - 4u * k : 4u) : 0u;
        w[k] = rem ? le_load32(p + 4u * k, rem) : 0u;
    }
}

template<bool WIDE>
__device__ __forceinline__ void store_run(uint8_t* p, uint32_t valid, const uint32_t (&w)[kLaneDwords])
{
    if (WIDE && valid == kTiffUndoLaneBytes) { store_span<kLaneDwords>(p, w); return; }
#pragma unroll
    for (uint32_t k = 0; k < kLaneDwords; ++k)
    {
        const uint32_t rem = valid > 4u * k ? (valid - 4u * k < 4u ? valid - 4u * k : 4u) : 0u;
        if (rem) le_store32(p + 4u * k, w[k], rem);
    }
}

// element j of the run, E bytes wide
template<uint32_t E>
__device__ __forceinline__ uint32_t element(const uint32_t (&w)[kLaneDwords], uint32_t j, bool swap)
{
    if constexpr (E == 1u) return (w[j / 4u] >> (8u * (j % 4u))) & 0xFFu;
    else { const uint32_t e = (w[j / 2u] >> (16u * (j % 2u))) & 0xFFFFu; return swap ? swap16(e) : e; }
}

// v[s] summed over the workgroup's 256 lanes for each of the S samples (total[s], in every lane); v[s] becomes this lane's exclusive
// prefix of it. lds: 4 * S words; the barriers are reached by every lane.
template<uint32_t S>
__device__ __forceinline__ void block_scan(uint32_t (&v)[S], uint32_t* lds, uint32_t (&total)[S])
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc[S];
#pragma unroll
    for (uint32_t s = 0; s < S; ++s)
    {
        inc[s] = v[s];
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1)
        {
            const uint32_t up = __shfl_up(inc[s], d, 64);
            if (lane >= d) inc[s] += up;
        }
    }
    __syncthreads();          // the previous use of lds is over
    if (lane == 63u)
    {
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) lds[wave * S + s] = inc[s];
    }
    __syncthreads();
#pragma unroll
    for (uint32_t s = 0; s < S; ++s)
    {
        uint32_t before = 0; total[s] = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) { const uint32_t t = lds[k * S + s]; total[s] += t; if (k < wave) before += t; }
        v[s] = before + inc[s] - v[s];
    }
}

// grid: x strided over the segment's rows, y = segment of the batch. E: the element's bytes, S: the stride in elements.
template<uint32_t E, uint32_t S, bool WIDE>
__global__ void __launch_bounds__(256) tiff_undo_kernel(uint8_t* stream, TiffBatch batch, bool swap)
{
    static_assert(kTiffUndoLaneBytes % (E * S) == 0, "a lane's run is whole pixels");
    constexpr uint32_t N = kTiffUndoLaneBytes / E;
    __shared__ uint32_t lds[4u * S];
    const TiffSegment seg = batch.seg[blockIdx.y];
    for (uint32_t r = blockIdx.x; r < seg.rows; r += gridDim.x)          // uniform over the workgroup, and so is the tile loop
    {
        uint8_t* row = stream + seg.offset + uint64_t(r) * seg.rowBytes;
        uint32_t carry[S];
#pragma unroll
        for (uint32_t s = 0; s < S; ++s) carry[s] = 0;
        for (uint32_t base = 0; base < seg.rowBytes; base += kTiffUndoTile)
        {
            const uint32_t left = seg.rowBytes - base, o = threadIdx.x * kTiffUndoLaneBytes;
            const uint32_t valid = o < left ? (left - o < kTiffUndoLaneBytes ? left - o : kTiffUndoLaneBytes) : 0u;
            uint8_t* p = row + base + o;          // dereferenced only for its `valid` bytes
            uint32_t w[kLaneDwords], run[S], total[S];
            load_run<WIDE>(p, valid, w);
#pragma unroll
            for (uint32_t s = 0; s < S; ++s) run[s] = 0;
#pragma unroll
            for (uint32_t j = 0; j < N; ++j) run[j % S] += element<E>(w, j, swap);
            block_scan<S>(run, lds, total);
#pragma unroll
            for (uint32_t s = 0; s < S; ++s) run[s] += carry[s];
            uint32_t out[kLaneDwords];
#pragma unroll
            for (uint32_t k = 0; k < kLaneDwords; ++k) out[k] = 0;
#pragma unroll
            for (uint32_t j = 0; j < N; ++j)
            {
                run[j % S] += element<E>(w, j, swap);
                if constexpr (E == 1u) out[j / 4u] |= (run[j % S] & 0xFFu) << (8u * (j % 4u));
                else out[j / 2u] |= (run[j % S] & 0xFFFFu) << (16u * (j % 2u));
            }
            store_run<WIDE>(p, valid, out);
#pragma unroll
            for (uint32_t s = 0; s < S; ++s) carry[s] += total[s];
        }
    }
}

// `bytes` (1, 2, 4, 8, 12 or 16) of a texel held as little-endian words: one access where WIDE (the address is a multiple of the access)
template<bool WIDE>
__device__ __forceinline__ void store_texel(uint8_t* d, const uint32_t (&t)[4], uint32_t bytes)
{
    if constexpr (WIDE)
    {
        if (bytes == 1u) *d = uint8_t(t[0]);
        else if (bytes == 2u) *reinterpret_cast<uint16_t*>(d) = uint16_t(t[0]);
        else if (bytes == 4u) *reinterpret_cast<uint32_t*>(d) = t[0];
        else if (bytes == 8u) *reinterpret_cast<uint2*>(d) = make_uint2(t[0], t[1]);
        else if (bytes == 12u) { uint32_t* q = reinterpret_cast<uint32_t*>(d); q[0] = t[0]; q[1] = t[1]; q[2] = t[2]; }
        else *reinterpret_cast<uint4*>(d) = make_uint4(t[0], t[1], t[2], t[3]);
    }
    else
    {
        for (uint32_t b = 0; b < bytes; ++b) d[b] = uint8_t(t[b >> 2] >> (8u * (b & 3u)));
    }
}

// grid: x across the segment's columns, y strided over its rows, z = segment of the batch
template<bool PAL, bool WIDE>
__global__ void __launch_bounds__(256) tiff_texels_kernel(const uint8_t* stream, TiffBatch batch, TiffLayout layout, PaletteArg<PAL> pal, ImgView dst, uint32_t imageBytes)
{
    __shared__ uint32_t lds[PAL ? 256 : 1];
    if constexpr (PAL) palette_to_lds(lds, pal);          // the whole workgroup, before any lane leaves
    const TiffSegment seg = batch.seg[blockIdx.z];
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= seg.cols) return;
    const uint32_t E = layout.bits / 8u;          // of a component; used only where planes are separate (8, 16 or 32 bits)
    for (uint32_t r = blockIdx.y; r < seg.rows; r += gridDim.y)
    {
        const uint8_t* row = stream + seg.offset + uint64_t(r) * seg.rowBytes;
        uint8_t* d = dst.pixels + uint64_t(seg.firstRow + r) * dst.rowPitch + uint64_t(seg.firstCol + x) * imageBytes;
        uint32_t t[4];
        if (layout.planar)
        {
            t[0] = tiff_plane_component(row, seg.rowBytes, layout, seg.plane, x); t[1] = t[2] = t[3] = 0;
            store_texel<WIDE>(d + seg.plane * E, t, E);
            if (seg.plane == 0u && tiff_fills_alpha(layout)) { t[0] = tiff_alpha_max(layout.bits); store_texel<WIDE>(d + 3u * E, t, E); }
        }
        else
        {
            tiff_texel(row, seg.rowBytes, layout, lds, x, t);
            store_texel<WIDE>(d, t, imageBytes);
        }
    }
}

// X: the file texel has 3 bytes (B8G8R8X8), else 4
template<bool X, bool WIDE>
__global__ void __launch_bounds__(256) tiff_pack_kernel(ImgView src, uint8_t* rows, bool imageAligned)
{
    constexpr uint32_t F = X ? 3u : 4u, G = WIDE ? 4u : 1u;
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * G;
    if (x >= src.width) return;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
    {
        const uint8_t* s = src.pixels + uint64_t(y) * src.rowPitch + uint64_t(x) * 4u;
        uint8_t* d = rows + (uint64_t(y) * src.width + x) * F;
        if constexpr (WIDE)
        {
            uint32_t in[4];
            load_span<4u>(s, in);
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) in[k] = tiff_pack_bgr(in[k]);
            if constexpr (X)
            {
                uint32_t out[3];
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) in[k] &= 0xFFFFFFu;
                pack3x4(in, out);
                store_span<3u, 4u>(d, out);
            }
            else store_span<4u>(d, in);
        }
        else
        {
            const uint32_t t = tiff_pack_bgr(load1<4u>(s, imageAligned));
            le_store32(d, t, F);
        }
    }
}

template<uint32_t E, uint32_t S>
hipError_t undo_batches(uint8_t* stream, const TiffSegment* segs, size_t count, bool swap, bool wide, hipStream_t hs, KernelMarks* marks)
{
    for (size_t first = 0; first < count; first += kTiffBatchMax)
    {
        TiffBatch batch;
        const uint32_t n = uint32_t(std::min<size_t>(count - first, kTiffBatchMax));
        uint32_t maxRows = 0;
        for (uint32_t i = 0; i < kTiffBatchMax; ++i)
        {
            batch.seg[i] = i < n ? segs[first + i] : TiffSegment{ 0, 0, 0, 0, 0, 0, 0 };
            if (!batch.seg[i].rowBytes) batch.seg[i].rows = 0;
            maxRows = std::max(maxRows, batch.seg[i].rows);
        }
        if (!maxRows) continue;
        // rows are strided over about 8192 workgroups in all
        const dim3 grid(std::min<uint32_t>(maxRows, std::max<uint32_t>(1u, 8192u / n)), n);
        if (wide)
        {
            DXTEX_MARK("tiff_undo<wide>");
            hipLaunchKernelGGL((tiff_undo_kernel<E, S, true>), grid, dim3(256), 0, hs, stream, batch, swap);
        }
        else
        {
            DXTEX_MARK("tiff_undo<narrow>");
            hipLaunchKernelGGL((tiff_undo_kernel<E, S, false>), grid, dim3(256), 0, hs, stream, batch, swap);
        }
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

template<bool PAL, bool WIDE>
hipError_t texel_batches(const uint8_t* stream, const TiffSegment* segs, size_t count, const TiffLayout& layout, const uint32_t* palette, const ImgView& dv, hipStream_t hs,
                         KernelMarks* marks)
{
    PaletteArg<PAL> pal;
    if constexpr (PAL) std::copy(palette, palette + 256, pal.word);
    const uint32_t imageBytes = tiff_kind_row(layout.kind).imageBytes;
    for (size_t first = 0; first < count; first += kTiffBatchMax)
    {
        TiffBatch batch;
        const uint32_t n = uint32_t(std::min<size_t>(count - first, kTiffBatchMax));
        uint32_t maxRows = 0, maxCols = 0;
        for (uint32_t i = 0; i < kTiffBatchMax; ++i)
        {
            batch.seg[i] = i < n ? segs[first + i] : TiffSegment{ 0, 0, 0, 0, 0, 0, 0 };
            maxRows = std::max(maxRows, batch.seg[i].rows); maxCols = std::max(maxCols, batch.seg[i].cols);
        }
        if (!maxRows || !maxCols) continue;
        const dim3 g = stream_grid(maxCols, maxRows, 1u);
        DXTEX_MARK(WIDE ? "tiff_texels<wide>" : "tiff_texels<narrow>");
        hipLaunchKernelGGL((tiff_texels_kernel<PAL, WIDE>), dim3(g.x, g.y, n), dim3(256), 0, hs, stream, batch, layout, pal, dv, imageBytes);
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

template<bool X>
hipError_t pack_bgr(const ImgView& sv, uint8_t* rows, hipStream_t hs, KernelMarks* marks)
{
    if (sv.width % 4u == 0 && multiple_of(rows, 0, 16u) && multiple_of(sv.pixels, sv.rowPitch, 16u))
    {
        DXTEX_MARK("tiff_pack<wide>");
        hipLaunchKernelGGL((tiff_pack_kernel<X, true>), stream_grid(sv.width, sv.height, 4u), dim3(256), 0, hs, sv, rows, true);
    }
    else
    {
        DXTEX_MARK("tiff_pack<narrow>");
        hipLaunchKernelGGL((tiff_pack_kernel<X, false>), stream_grid(sv.width, sv.height, 1u), dim3(256), 0, hs, sv, rows, multiple_of(sv.pixels, sv.rowPitch, 4u));
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
} // namespace

hipError_t launch_tiff_undo(uint8_t* stream, const TiffSegment* segs, size_t count, const TiffLayout& layout, hipStream_t hs, KernelMarks* marks)
{
    if (layout.predictor < 2u || !count) return hipSuccess;
    if (!tiff_predictor_fits(layout.predictor, layout.bits)) return hipErrorInvalidValue;
    bool wide = multiple_of(stream, 0, 16u);
    for (size_t i = 0; i < count && wide; ++i) wide = ((segs[i].offset | segs[i].rowBytes) & 15u) == 0;
    const uint32_t E = tiff_undo_element(layout), S = tiff_undo_stride(layout);
    const bool swap = tiff_undo_swaps(layout);
    if (E == 1u && S == 1u) return undo_batches<1u, 1u>(stream, segs, count, swap, wide, hs, marks);
    if (E == 1u && S == 3u) return undo_batches<1u, 3u>(stream, segs, count, swap, wide, hs, marks);
    if (E == 1u && S == 4u) return undo_batches<1u, 4u>(stream, segs, count, swap, wide, hs, marks);
    if (E == 2u && S == 1u) return undo_batches<2u, 1u>(stream, segs, count, swap, wide, hs, marks);
    if (E == 2u && S == 3u) return undo_batches<2u, 3u>(stream, segs, count, swap, wide, hs, marks);
    if (E == 2u && S == 4u) return undo_batches<2u, 4u>(stream, segs, count, swap, wide, hs, marks);
    return hipErrorInvalidValue;
}

hipError_t launch_tiff_texels(const uint8_t* stream, const TiffSegment* segs, size_t count, const TiffLayout& layout, const uint32_t* palette, const ImgView& dv,
                              hipStream_t hs, KernelMarks* marks)
{
    if (!count || !dv.width || !dv.height) return hipSuccess;
    const uint32_t imageBytes = tiff_kind_row(layout.kind).imageBytes;
    if (!imageBytes || (tiff_is_palette(layout.kind) && !palette)) return hipErrorInvalidValue;
    const bool wide = multiple_of(dv.pixels, dv.rowPitch, imageBytes == 12u ? 4u : imageBytes);
    if (tiff_is_palette(layout.kind))
        return wide ? texel_batches<true, true>(stream, segs, count, layout, palette, dv, hs, marks) : texel_batches<true, false>(stream, segs, count, layout, palette, dv, hs, marks);
    return wide ? texel_batches<false, true>(stream, segs, count, layout, palette, dv, hs, marks) : texel_batches<false, false>(stream, segs, count, layout, palette, dv, hs, marks);
}

hipError_t launch_tiff_pack(const ImgView& sv, uint8_t* rows, hipStream_t hs, KernelMarks* marks)
{
    if (!sv.width || !sv.height) return hipSuccess;
    const TiffSource src = tiff_pack_source(sv.format);
    if (!src.bgr) return hipErrorInvalidValue;
    return src.fileBytes == 3u ? pack_bgr<true>(sv, rows, hs, marks) : pack_bgr<false>(sv, rows, hs, marks);
}
} // namespace dxtex
