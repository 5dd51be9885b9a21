// FlipRotate (DirectXTexFlipRotate.cpp) on gfx950: the eight symmetries of the rectangle as byte moves. dxtex_fliprotate.h holds the
// rule, the routes and every index; the kernels here only move what those indices name.
//
//   flip_rows_kernel       the four symmetries that keep width and height. Pure streaming, no LDS: blockIdx.z picks the job from the
//                          argument block, blockIdx.x the 256 units of a row (16 bytes on the wide form, one texel on the narrow one),
//                          blockIdx.y the first group of rows. A lane keeps kFlipRowsInFlight rows in flight before its first store.
//   flip_transpose_kernel  the four that exchange them. A workgroup owns a square destination tile: its source block goes through LDS so
//                          that both global sides have consecutive lanes on consecutive texels; no lane walks a source column in global
//                          memory. The LDS row pitch is padded (fr_tile_pitch) so that the column-order read is free of bank conflicts.
//
// The grid is sized for the largest job of the batch and a workgroup outside its own job's extent leaves at once. Only the texels of the
// destination's rows are written: never row padding, never anything outside the image.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_fliprotate.h"
#include <algorithm>
#include <vector>

namespace dxtex
{
namespace
{
// plain structs (HIP's vector types have constructors and cannot sit in a union)
struct alignas(8) FlipU2 { uint32_t x, y; };
struct alignas(4) FlipU3 { uint32_t x, y, z; };
struct alignas(16) FlipU4 { uint32_t x, y, z, w; };

// B bytes from / to global memory in pieces of A bytes (A divides B and the address)
template<typename A, uint32_t B>
struct FlipTexel
{
    static constexpr uint32_t N = B / sizeof(A);
    A v[N];
    __device__ __forceinline__ void load(const uint8_t* p)
    {
#pragma unroll
        for (uint32_t i = 0; i < N; ++i) v[i] = reinterpret_cast<const A*>(p)[i];
    }
    __device__ __forceinline__ void store(uint8_t* p) const
    {
#pragma unroll
        for (uint32_t i = 0; i < N; ++i) reinterpret_cast<A*>(p)[i] = v[i];
    }
};

// ---- rows -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void flip_rows_wide(const FlipJob& j, uint32_t u)
{
    for (uint32_t y0 = blockIdx.y * kFlipRowsInFlight; y0 < j.height; y0 += gridDim.y * kFlipRowsInFlight)
    {
        uint4 v[kFlipRowsInFlight];
        uint64_t to[kFlipRowsInFlight];
#pragma unroll
        for (uint32_t r = 0; r < kFlipRowsInFlight; ++r)
        {
            uint64_t from;
            fr_row_unit(j, u, min(y0 + r, j.height - 1u), &from, &to[r]);       // a short last group re-reads the last row (and does not store it)
            v[r] = *reinterpret_cast<const uint4*>(j.src + from);
        }
#pragma unroll
        for (uint32_t r = 0; r < kFlipRowsInFlight; ++r)
        {
            if (y0 + r >= j.height) break;
            uint32_t w[4] = { v[r].x, v[r].y, v[r].z, v[r].w };
            if (j.mirrorX) fr_reverse16(w, j.texel);
            *reinterpret_cast<uint4*>(j.dst + to[r]) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

template<typename A, uint32_t B>
__device__ __forceinline__ void flip_rows_narrow(const FlipJob& j, uint32_t u)
{
    for (uint32_t y0 = blockIdx.y * kFlipRowsInFlight; y0 < j.height; y0 += gridDim.y * kFlipRowsInFlight)
    {
        FlipTexel<A, B> v[kFlipRowsInFlight];
        uint64_t to[kFlipRowsInFlight];
#pragma unroll
        for (uint32_t r = 0; r < kFlipRowsInFlight; ++r)
        {
            uint64_t from;
            fr_row_unit(j, u, min(y0 + r, j.height - 1u), &from, &to[r]);
            v[r].load(j.src + from);
        }
#pragma unroll
        for (uint32_t r = 0; r < kFlipRowsInFlight; ++r)
            if (y0 + r < j.height) v[r].store(j.dst + to[r]);
    }
}

// the texel size picks B, the job's access width A: every A the host can choose for that B
template<uint32_t B>
__device__ __forceinline__ void flip_rows_narrow_by_access(const FlipJob& j, uint32_t u)
{
    if constexpr (B % 16u == 0) if (j.access == 16u) return flip_rows_narrow<FlipU4, B>(j, u);
    if constexpr (B % 8u == 0) if (j.access == 8u) return flip_rows_narrow<FlipU2, B>(j, u);
    if constexpr (B % 4u == 0) if (j.access == 4u) return flip_rows_narrow<uint32_t, B>(j, u);
    if constexpr (B % 2u == 0) if (j.access == 2u) return flip_rows_narrow<uint16_t, B>(j, u);
    flip_rows_narrow<uint8_t, B>(j, u);
}

__global__ void __launch_bounds__(kFlipThreads) flip_rows_kernel(FlipBatch batch)
{
    const FlipJob& j = batch.job[blockIdx.z];
    const uint32_t u = blockIdx.x * kFlipThreads + threadIdx.x;
    if (u >= fr_row_units(j)) return;
    if (j.route == FR_ROW_WIDE) return flip_rows_wide(j, u);
    switch (j.texel)
    {
    case 1u: flip_rows_narrow_by_access<1>(j, u); break;
    case 2u: flip_rows_narrow_by_access<2>(j, u); break;
    case 4u: flip_rows_narrow_by_access<4>(j, u); break;
    case 8u: flip_rows_narrow_by_access<8>(j, u); break;
    case 12u: flip_rows_narrow_by_access<12>(j, u); break;
    default: flip_rows_narrow_by_access<16>(j, u); break;
    }
}

// ---- tiles ------------------------------------------------------------------------------------------------------------------------------
// L is the texel as LDS holds it (naturally aligned there: fr_tile_pitch keeps it so), A the piece global memory is touched in.
template<typename L, typename A>
__device__ __forceinline__ void flip_tile(const FlipJob& j, uint8_t* lds)
{
    constexpr uint32_t B = sizeof(L);
    constexpr uint32_t SIDE = B <= 4u ? 64u : 32u, PASSES = SIDE / (kFlipThreads / SIDE);
    for (uint32_t by = blockIdx.y; ; by += gridDim.y)
    {
        FlipTile t;
        if (!fr_tile(j, blockIdx.x, by, &t)) return;          // uniform over the workgroup
        union { FlipTexel<A, B> g; L l; } v[PASSES];
        uint32_t at[PASSES];
        bool has[PASSES];
#pragma unroll
        for (uint32_t k = 0; k < PASSES; ++k)
        {
            uint64_t from = 0;
            has[k] = fr_tile_load(j, t, threadIdx.x, k, &from, &at[k]);
            if (has[k]) v[k].g.load(j.src + from);
        }
#pragma unroll
        for (uint32_t k = 0; k < PASSES; ++k)
            if (has[k]) *reinterpret_cast<L*>(lds + at[k]) = v[k].l;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < PASSES; ++k)
        {
            uint32_t in = 0;
            uint64_t to = 0;
            if (!fr_tile_store(j, t, threadIdx.x, k, &in, &to)) continue;
            union { FlipTexel<A, B> g; L l; } w;
            w.l = *reinterpret_cast<const L*>(lds + in);
            w.g.store(j.dst + to);
        }
        __syncthreads();                                       // the next tile overwrites the LDS this one still reads
    }
}

template<typename L>
__device__ __forceinline__ void flip_tile_by_access(const FlipJob& j, uint8_t* lds)
{
    constexpr uint32_t B = sizeof(L);
    if constexpr (B % 16u == 0) if (j.access == 16u) return flip_tile<L, FlipU4>(j, lds);
    if constexpr (B % 8u == 0) if (j.access == 8u) return flip_tile<L, FlipU2>(j, lds);
    if constexpr (B % 4u == 0) if (j.access == 4u) return flip_tile<L, uint32_t>(j, lds);
    if constexpr (B % 2u == 0) if (j.access == 2u) return flip_tile<L, uint16_t>(j, lds);
    flip_tile<L, uint8_t>(j, lds);
}

__global__ void __launch_bounds__(kFlipThreads) flip_transpose_kernel(FlipBatch batch)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kFlipTileLdsBytes];
    const FlipJob& j = batch.job[blockIdx.z];
    switch (j.texel)
    {
    case 1u: flip_tile_by_access<uint8_t>(j, lds); break;
    case 2u: flip_tile_by_access<uint16_t>(j, lds); break;
    case 4u: flip_tile_by_access<uint32_t>(j, lds); break;
    case 8u: flip_tile_by_access<FlipU2>(j, lds); break;
    case 12u: flip_tile_by_access<FlipU3>(j, lds); break;
    case 16u: flip_tile_by_access<FlipU4>(j, lds); break;
    default: break;
    }
}
} // namespace

hipError_t launch_flip_rotate(const FlipJob* jobs, size_t count, hipStream_t stream, KernelMarks* marks)
{
    // one launch per route per kFlipBatchMax jobs: the row forms share a kernel, the tiles have their own
    for (int tiles = 0; tiles < 2; ++tiles)
    {
        std::vector<FlipJob> mine;
        for (size_t i = 0; i < count; ++i)
            if ((jobs[i].route == FR_TILE) == (tiles != 0) && jobs[i].width && jobs[i].height) mine.push_back(jobs[i]);
        for (size_t first = 0; first < mine.size(); first += kFlipBatchMax)
        {
            FlipBatch batch;
            batch.count = uint32_t(std::min<size_t>(kFlipBatchMax, mine.size() - first));
            bool wide = false, narrow = false;
            for (uint32_t k = 0; k < kFlipBatchMax; ++k)
            {
                batch.job[k] = k < batch.count ? mine[first + k] : FlipJob{};
                if (k < batch.count) (batch.job[k].route == FR_ROW_WIDE ? wide : narrow) = true;
            }
            uint32_t gx = 0, gy = 0;
            fr_grid(batch, tiles != 0, &gx, &gy);
            if (!gx || !gy) continue;
            if (tiles)
            {
                if (marks) marks->mark("flip_transpose");
                hipLaunchKernelGGL(flip_transpose_kernel, dim3(gx, gy, batch.count), dim3(kFlipThreads), 0, stream, batch);
            }
            else
            {
                if (marks) marks->mark(wide && narrow ? "flip_rows<mixed>" : wide ? "flip_rows<wide>" : "flip_rows<narrow>");
                hipLaunchKernelGGL(flip_rows_kernel, dim3(gx, gy, batch.count), dim3(kFlipThreads), 0, stream, batch);
            }
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    if (marks) marks->mark(nullptr);
    return hipSuccess;
}
} // namespace dxtex
