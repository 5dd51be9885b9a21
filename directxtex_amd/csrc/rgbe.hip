// Radiance RGBE texels on gfx950 (dxtex_rgbe.h holds the arithmetic): what the .hdr codec does per texel either side of its byte-serial
// run-length coder, so that a file's texels cross PCIe as the 4 bytes they are.
//   rgbe_decode_kernel  R8G8B8A8_UINT rows of shared-exponent texels -> R32G32B32A32_FLOAT rows: 4 bytes read, 16 written per texel
//   rgbe_encode_kernel  R32G32B32A32_FLOAT, R32G32B32_FLOAT or R16G16B16A16_FLOAT rows -> RGBE rows
//
// Pure streaming: no LDS, no atomics, no cross-lane work. One texel per lane, x = blockIdx.x * 256 + threadIdx.x, rows strided over
// gridDim.y (dxtex_stream.h's grid). Two routes, by the alignment of the float side:
//   wide    its base and row pitch are multiples of the texel (16 bytes; 8 for halves): one dwordx4 (dwordx2) access per texel, lane i at
//           base + 16 * i, 1 KiB per wave instruction
//   narrow  one access per channel (dwords; 16-bit loads for halves). R32G32B32_FLOAT always goes here. Alpha is not read.
// The RGBE side is a dword per lane where its base and pitch are multiples of 4 (a tight row of a device allocation always), else four
// byte accesses. Both kernels are bound by memory: 20 bytes a texel.
//
// Every read and write of a lane lies inside its row's `width` texels: x < width, y < height.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_rgbe.h"

namespace dxtex
{
namespace
{
template<bool WIDE>
__global__ void __launch_bounds__(256) rgbe_decode_kernel(ImgView src, ImgView dst, float scale, bool dwords)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= src.width) return;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
    {
        const uint32_t v = load1<4u>(src.pixels + uint64_t(y) * src.rowPitch + uint64_t(x) * 4u, dwords);
        const uint8_t in[4] = { uint8_t(v), uint8_t(v >> 8), uint8_t(v >> 16), uint8_t(v >> 24) };
        float out[4];
        rgbe_decode(in, scale, out);
        float* d = reinterpret_cast<float*>(dst.pixels + uint64_t(y) * dst.rowPitch + uint64_t(x) * 16u);
        if constexpr (WIDE) *reinterpret_cast<float4*>(d) = make_float4(out[0], out[1], out[2], out[3]);
        else { d[0] = out[0]; d[1] = out[1]; d[2] = out[2]; d[3] = out[3]; }
    }
}

// FORMAT = the float side's: FMT_R32G32B32A32_FLOAT, FMT_R32G32B32_FLOAT (never WIDE) or FMT_R16G16B16A16_FLOAT
template<int FORMAT, bool WIDE>
__global__ void __launch_bounds__(256) rgbe_encode_kernel(ImgView src, ImgView dst, bool dwords)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= src.width) return;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
    {
        const uint8_t* row = src.pixels + uint64_t(y) * src.rowPitch;
        float r, g, b;
        if constexpr (FORMAT == FMT_R16G16B16A16_FLOAT)
        {
            uint16_t h[3];
            if constexpr (WIDE)
            {
                const uint2 v = *reinterpret_cast<const uint2*>(row + uint64_t(x) * 8u);
                h[0] = uint16_t(v.x); h[1] = uint16_t(v.x >> 16); h[2] = uint16_t(v.y);
            }
            else
            {
                const uint16_t* s = reinterpret_cast<const uint16_t*>(row + uint64_t(x) * 8u);
                h[0] = s[0]; h[1] = s[1]; h[2] = s[2];
            }
            r = rgbe_half_to_float(h[0]); g = rgbe_half_to_float(h[1]); b = rgbe_half_to_float(h[2]);
        }
        else if constexpr (WIDE)
        {
            const float4 v = *reinterpret_cast<const float4*>(row + uint64_t(x) * 16u);
            r = v.x; g = v.y; b = v.z;
        }
        else
        {
            const float* s = reinterpret_cast<const float*>(row + uint64_t(x) * (FORMAT == FMT_R32G32B32_FLOAT ? 12u : 16u));
            r = s[0]; g = s[1]; b = s[2];
        }
        uint8_t out[4];
        rgbe_encode(r, g, b, out);
        store1<4u>(dst.pixels + uint64_t(y) * dst.rowPitch + uint64_t(x) * 4u,
                   uint32_t(out[0]) | (uint32_t(out[1]) << 8) | (uint32_t(out[2]) << 16) | (uint32_t(out[3]) << 24), dwords);
    }
}
} // namespace

hipError_t launch_rgbe_decode(const ImgView& sv, const ImgView& dv, float scale, hipStream_t stream, KernelMarks* marks)
{
    if (!sv.width || !sv.height) return hipSuccess;
    if (sv.format != FMT_R8G8B8A8_UINT || dv.format != FMT_R32G32B32A32_FLOAT || sv.width != dv.width || sv.height != dv.height) return hipErrorInvalidValue;
    const dim3 grid = stream_grid(sv.width, sv.height, 1u);
    const bool dwords = multiple_of(sv.pixels, sv.rowPitch, 4u);
    if (multiple_of(dv.pixels, dv.rowPitch, 16u))
    {
        DXTEX_MARK("rgbe_decode<wide>");
        hipLaunchKernelGGL((rgbe_decode_kernel<true>), grid, dim3(256), 0, stream, sv, dv, scale, dwords);
    }
    else
    {
        DXTEX_MARK("rgbe_decode<narrow>");
        hipLaunchKernelGGL((rgbe_decode_kernel<false>), grid, dim3(256), 0, stream, sv, dv, scale, dwords);
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

hipError_t launch_rgbe_encode(const ImgView& sv, const ImgView& dv, hipStream_t stream, KernelMarks* marks)
{
    if (!sv.width || !sv.height) return hipSuccess;
    if (dv.format != FMT_R8G8B8A8_UINT || sv.width != dv.width || sv.height != dv.height) return hipErrorInvalidValue;
    const dim3 grid = stream_grid(sv.width, sv.height, 1u);
    const bool dwords = multiple_of(dv.pixels, dv.rowPitch, 4u);
#define DXTEX_RGBE_ENCODE(FORMAT, WIDE) do { DXTEX_MARK((WIDE) ? "rgbe_encode<wide>" : "rgbe_encode<narrow>"); \
        hipLaunchKernelGGL((rgbe_encode_kernel<FORMAT, WIDE>), grid, dim3(256), 0, stream, sv, dv, dwords); } while (0)
    switch (sv.format)
    {
    case FMT_R32G32B32A32_FLOAT: if (multiple_of(sv.pixels, sv.rowPitch, 16u)) DXTEX_RGBE_ENCODE(FMT_R32G32B32A32_FLOAT, true); else DXTEX_RGBE_ENCODE(FMT_R32G32B32A32_FLOAT, false); break;
    case FMT_R16G16B16A16_FLOAT: if (multiple_of(sv.pixels, sv.rowPitch, 8u)) DXTEX_RGBE_ENCODE(FMT_R16G16B16A16_FLOAT, true); else DXTEX_RGBE_ENCODE(FMT_R16G16B16A16_FLOAT, false); break;
    case FMT_R32G32B32_FLOAT: DXTEX_RGBE_ENCODE(FMT_R32G32B32_FLOAT, false); break;
    default: return hipErrorInvalidValue;
    }
#undef DXTEX_RGBE_ENCODE
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
} // namespace dxtex
