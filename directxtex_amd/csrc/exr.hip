// OpenEXR scanline texels on gfx950 (dxtex_exr.h holds the rules): what the .exr codec does per byte and per texel behind the inflater, so
// that a file's chunks cross PCIe as they leave it.
//   exr_undo_sums_kernel   launch one of two, only where a coded chunk is longer than one tile (kExrUndoTile): every tile's byte sum
//   exr_undo_kernel        the byte-wise prefix sum of every coded chunk, in place: a lane sums its run of 16 dwords, the wave scans the
//                          lanes' totals (__shfl_up), LDS carries them across the four waves, and the tiles in front of this one come in as
//                          the sums of launch one. The "- 128 i" term is an exclusive-or of the odd bytes with 0x80. No workgroup waits on
//                          another: the order between the two launches is the stream's. The two byte planes stay where they are;
//                          exr_texels addresses them (exr_plain_index).
//   exr_texels_kernel      one lane per texel: gathers R, G, B, A through the channel table from a plain or an undone chunk, converts
//                          (exr_sample_to_half), fills what is absent, and stores 8 bytes at the row's place in its item
//   exr_pack_kernel        the writer's rows: a texel of R16G16B16A16_FLOAT, R32G32B32A32_FLOAT or R32G32B32_FLOAT -> four halves into the
//                          A, B, G, R planes of its scanline (8 * width bytes a row, tight)
//
// Routes. exr_undo: wide where the stream's base and every coded chunk's offset are multiples of 16 - a lane's 64 bytes move as four
// dwordx4 - narrow otherwise, byte by byte; a lane whose run crosses the chunk's end moves the bytes it has one by one on either route, so
// nothing outside a chunk is read or written. exr_texels: the texel's 8 bytes as one store where the items' bases and pitches are
// multiples of 8, as bytes otherwise. exr_pack: wide where width is a multiple of 4, the stream's base of 8 and the image's base and
// pitch of 16 - a lane takes four texels - narrow otherwise.
// Chunk descriptors come in the kernels' arguments, kExrBatchMax a launch.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_exr.h"

namespace dxtex
{
namespace
{
struct ExrBatch { ExrChunk chunk[kExrBatchMax]; };
// undo: where tile 0 of each chunk of the batch lies in the partial sums
struct ExrSumBase { uint32_t at[kExrBatchMax]; };

constexpr uint32_t kLaneDwords = kExrUndoLaneBytes / 4u;

// the lane's run: `valid` (0..64) bytes at p, the rest zero
template<bool WIDE>
__device__ __forceinline__ void load_run(const uint8_t* p, uint32_t valid, uint32_t (&w)[kLaneDwords])
{
    if (WIDE && valid == kExrUndoLaneBytes) { load_span<kLaneDwords>(p, w); return; }
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
    if (WIDE && valid == kExrUndoLaneBytes) { store_span<kLaneDwords>(p, w); return; }
#pragma unroll
    for (uint32_t k = 0; k < kLaneDwords; ++k)
    {
        const uint32_t rem = valid > 4u * k ? (valid - 4u * k < 4u ? valid - 4u * k : 4u) : 0u;
        if (rem) le_store32(p + 4u * k, w[k], rem);
    }
}

// the sum of a dword's four bytes
__device__ __forceinline__ uint32_t byte_sum(uint32_t w) { return (w & 0xFFu) + ((w >> 8) & 0xFFu) + ((w >> 16) & 0xFFu) + (w >> 24); }

// v summed over the workgroup's 256 lanes (the answer in every lane), and this lane's exclusive prefix of it. lds: 4 words; the
// barriers are reached by every lane.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* lds, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1)
    {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    __syncthreads();          // the previous use of lds is over
    if (lane == 63u) lds[wave] = inc;
    __syncthreads();
    uint32_t before = 0; total = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) { const uint32_t s = lds[k]; total += s; if (k < wave) before += s; }
    return before + inc - v;
}

// grid: x = tile of the chunk, y = chunk of the batch
template<bool WIDE>
__global__ void __launch_bounds__(256) exr_undo_sums_kernel(const uint8_t* stream, ExrBatch batch, ExrSumBase base, uint32_t* sums)
{
    __shared__ uint32_t lds[4];
    const ExrChunk c = batch.chunk[blockIdx.y];
    const uint32_t tiles = (c.bytes + kExrUndoTile - 1u) / kExrUndoTile;
    if (!c.coded || tiles < 2u || blockIdx.x >= tiles) return;          // uniform over the workgroup
    const uint32_t o = blockIdx.x * kExrUndoTile + threadIdx.x * kExrUndoLaneBytes;
    const uint32_t valid = o < c.bytes ? (c.bytes - o < kExrUndoLaneBytes ? c.bytes - o : kExrUndoLaneBytes) : 0u;
    uint32_t w[kLaneDwords], s = 0, total;
    load_run<WIDE>(stream + c.offset + o, valid, w);
#pragma unroll
    for (uint32_t k = 0; k < kLaneDwords; ++k) s += byte_sum(w[k]);
    (void)block_scan(s, lds, total);
    if (threadIdx.x == 0) sums[base.at[blockIdx.y] + blockIdx.x] = total;
}

template<bool WIDE>
__global__ void __launch_bounds__(256) exr_undo_kernel(uint8_t* stream, ExrBatch batch, ExrSumBase base, const uint32_t* sums)
{
    __shared__ uint32_t lds[4];
    const ExrChunk c = batch.chunk[blockIdx.y];
    const uint32_t tiles = (c.bytes + kExrUndoTile - 1u) / kExrUndoTile;
    if (!c.coded || blockIdx.x >= tiles) return;          // uniform over the workgroup
    uint32_t carry = 0, total;
    if (blockIdx.x)          // uniform; `sums` is read only where launch one wrote it
    {
        uint32_t mine = 0;
        for (uint32_t t = threadIdx.x; t < blockIdx.x; t += 256u) mine += sums[base.at[blockIdx.y] + t];
        (void)block_scan(mine, lds, carry);
    }
    const uint32_t o = blockIdx.x * kExrUndoTile + threadIdx.x * kExrUndoLaneBytes;
    const uint32_t valid = o < c.bytes ? (c.bytes - o < kExrUndoLaneBytes ? c.bytes - o : kExrUndoLaneBytes) : 0u;
    uint32_t w[kLaneDwords], s = 0;
    uint8_t* p = stream + c.offset + o;
    load_run<WIDE>(p, valid, w);
#pragma unroll
    for (uint32_t k = 0; k < kLaneDwords; ++k) s += byte_sum(w[k]);
    uint32_t run = carry + block_scan(s, lds, total);
    // o is a multiple of 4, so a byte's index within the chunk is odd where its place in the dword is
#pragma unroll
    for (uint32_t k = 0; k < kLaneDwords; ++k)
    {
        const uint32_t b0 = run + (w[k] & 0xFFu), b1 = b0 + ((w[k] >> 8) & 0xFFu), b2 = b1 + ((w[k] >> 16) & 0xFFu), b3 = b2 + (w[k] >> 24);
        w[k] = ((b0 & 0xFFu) | ((b1 & 0xFFu) << 8) | ((b2 & 0xFFu) << 16) | (b3 << 24)) ^ 0x80008000u;
        run = b3;
    }
    store_run<WIDE>(p, valid, w);
}

struct ExrItems { uint8_t* pixels[kExrItemsMax]; uint64_t rowPitch[kExrItemsMax]; };

// grid: x across the row, y strided over the chunk's rows, z = chunk of the batch
__global__ void __launch_bounds__(256) exr_texels_kernel(const uint8_t* stream, ExrBatch batch, ExrLayout layout, ExrItems items, bool aligned)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= layout.width) return;
    const ExrChunk c = batch.chunk[blockIdx.z];
    const uint8_t* chunk = stream + c.offset;
    for (uint32_t r = blockIdx.y; r < c.rows; r += gridDim.y)
    {
        const uint32_t y = c.firstRow + r, item = y / layout.itemRows, row = y - item * layout.itemRows;
        const uint64_t t = exr_texel(chunk, c.coded != 0, c.bytes, r * layout.scanlineBytes, layout.channel, x);
        store1<8u>(items.pixels[item] + uint64_t(row) * items.rowPitch[item] + uint64_t(x) * 8u, t, aligned);
    }
}

template<int SRC, bool WIDE>
__global__ void __launch_bounds__(256) exr_pack_kernel(ImgView src, uint8_t* stream, bool imageAligned, bool streamAligned)
{
    constexpr uint32_t S = exr_source_bytes(SRC), G = WIDE ? 4u : 1u;
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * G;
    if (x >= src.width) return;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
    {
        const uint8_t* s = src.pixels + uint64_t(y) * src.rowPitch + uint64_t(x) * S;
        uint8_t* line = stream + uint64_t(y) * src.width * kExrFileTexelBytes;
        if constexpr (WIDE)
        {
            uint32_t in[S];
            load_span<S>(s, in);
            uint64_t t[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) t[k] = exr_pack_halves<SRC>(in + k * (S / 4u));
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c)
            {
                uint32_t out[2];
                out[0] = (uint32_t(t[0] >> (16u * c)) & 0xFFFFu) | (uint32_t(t[1] >> (16u * c)) << 16);
                out[1] = (uint32_t(t[2] >> (16u * c)) & 0xFFFFu) | (uint32_t(t[3] >> (16u * c)) << 16);
                store_span<2u>(line + (uint64_t(exr_file_plane(c)) * src.width + x) * 2u, out);
            }
        }
        else
        {
            uint32_t in[S / 4u];
#pragma unroll
            for (uint32_t i = 0; i < S / 4u; ++i) in[i] = load1<4u>(s + 4u * i, imageAligned);
            const uint64_t t = exr_pack_halves<SRC>(in);
#pragma unroll
            for (uint32_t c = 0; c < 4u; ++c) store1<2u>(line + (uint64_t(exr_file_plane(c)) * src.width + x) * 2u, uint32_t(t >> (16u * c)) & 0xFFFFu, streamAligned);
        }
    }
}

template<bool WIDE>
hipError_t undo_batches(uint8_t* stream, const ExrChunk* chunks, size_t count, uint32_t* sums, hipStream_t hs, KernelMarks* marks)
{
    uint32_t sumsUsed = 0;
    for (size_t first = 0; first < count;)
    {
        ExrBatch batch; ExrSumBase base;
        uint32_t n = 0, maxTiles = 0;
        bool split = false;
        for (; first < count && n < kExrBatchMax; ++first)
        {
            if (!chunks[first].coded) continue;
            const uint32_t tiles = (chunks[first].bytes + kExrUndoTile - 1u) / kExrUndoTile;
            batch.chunk[n] = chunks[first]; base.at[n] = sumsUsed;
            if (tiles > 1u) { split = true; sumsUsed += tiles; }
            maxTiles = tiles > maxTiles ? tiles : maxTiles;
            ++n;
        }
        if (!n || !maxTiles) continue;
        for (uint32_t i = n; i < kExrBatchMax; ++i) { batch.chunk[i] = ExrChunk{ 0, 0, 0, 0, 0 }; base.at[i] = 0; }
        if (split)
        {
            DXTEX_MARK("exr_undo_sums");
            hipLaunchKernelGGL((exr_undo_sums_kernel<WIDE>), dim3(maxTiles, n), dim3(256), 0, hs, stream, batch, base, sums);
        }
        DXTEX_MARK(WIDE ? "exr_undo<wide>" : "exr_undo<narrow>");
        hipLaunchKernelGGL((exr_undo_kernel<WIDE>), dim3(maxTiles, n), dim3(256), 0, hs, stream, batch, base, sums);
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

template<int SRC>
hipError_t pack_source(const ImgView& sv, uint8_t* stream, hipStream_t hs, KernelMarks* marks)
{
    if (sv.width % 4u == 0 && multiple_of(stream, 0, 8u) && multiple_of(sv.pixels, sv.rowPitch, 16u))
    {
        DXTEX_MARK("exr_pack<wide>");
        hipLaunchKernelGGL((exr_pack_kernel<SRC, true>), stream_grid(sv.width, sv.height, 4u), dim3(256), 0, hs, sv, stream, true, true);
    }
    else
    {
        DXTEX_MARK("exr_pack<narrow>");
        hipLaunchKernelGGL((exr_pack_kernel<SRC, false>), stream_grid(sv.width, sv.height, 1u), dim3(256), 0, hs, sv, stream,
                           multiple_of(sv.pixels, sv.rowPitch, 4u), multiple_of(stream, 0, 2u));
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
} // namespace

size_t exr_undo_sums_count(const ExrChunk* chunks, size_t count)
{
    size_t words = 0;
    for (size_t i = 0; i < count; ++i)
        if (chunks[i].coded && chunks[i].bytes > kExrUndoTile) words += (chunks[i].bytes + kExrUndoTile - 1u) / kExrUndoTile;
    return words;
}

hipError_t launch_exr_undo(uint8_t* stream, const ExrChunk* chunks, size_t count, uint32_t* sums, hipStream_t hs, KernelMarks* marks)
{
    bool wide = multiple_of(stream, 0, 16u), any = false;
    for (size_t i = 0; i < count; ++i)
        if (chunks[i].coded && chunks[i].bytes) { any = true; wide = wide && (chunks[i].offset & 15u) == 0; }
    if (!any) return hipSuccess;
    return wide ? undo_batches<true>(stream, chunks, count, sums, hs, marks) : undo_batches<false>(stream, chunks, count, sums, hs, marks);
}

hipError_t launch_exr_texels(const uint8_t* stream, const ExrChunk* chunks, size_t count, const ExrLayout& layout, const ImgView* items, size_t itemCount,
                             hipStream_t hs, KernelMarks* marks)
{
    if (!layout.width || !layout.rows || !count) return hipSuccess;
    if (!itemCount || itemCount > kExrItemsMax || !layout.itemRows || uint64_t(layout.itemRows) * itemCount < layout.rows) return hipErrorInvalidValue;
    ExrItems it;
    bool aligned = true;
    for (size_t i = 0; i < kExrItemsMax; ++i)
    {
        const ImgView& v = items[i < itemCount ? i : 0];
        it.pixels[i] = v.pixels; it.rowPitch[i] = v.rowPitch;
        aligned = aligned && multiple_of(v.pixels, v.rowPitch, 8u);
    }
    for (size_t first = 0; first < count; first += kExrBatchMax)
    {
        ExrBatch batch;
        const uint32_t n = uint32_t(count - first < kExrBatchMax ? count - first : kExrBatchMax);
        uint32_t maxRows = 0;
        for (uint32_t i = 0; i < kExrBatchMax; ++i)
        {
            batch.chunk[i] = i < n ? chunks[first + i] : ExrChunk{ 0, 0, 0, 0, 0 };
            maxRows = batch.chunk[i].rows > maxRows ? batch.chunk[i].rows : maxRows;
        }
        if (!maxRows) continue;
        const dim3 g = stream_grid(layout.width, maxRows, 1u);
        DXTEX_MARK("exr_texels");
        hipLaunchKernelGGL(exr_texels_kernel, dim3(g.x, g.y, n), dim3(256), 0, hs, stream, batch, layout, it, aligned);
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_exr_pack(const ImgView& sv, int source, uint8_t* stream, hipStream_t hs, KernelMarks* marks)
{
    if (!sv.width || !sv.height) return hipSuccess;
    switch (source)
    {
    case EXR_SRC_RGBA16F: return pack_source<EXR_SRC_RGBA16F>(sv, stream, hs, marks);
    case EXR_SRC_RGBA32F: return pack_source<EXR_SRC_RGBA32F>(sv, stream, hs, marks);
    case EXR_SRC_RGB32F: return pack_source<EXR_SRC_RGB32F>(sv, stream, hs, marks);
    default: return hipErrorInvalidValue;
    }
}
} // namespace dxtex
