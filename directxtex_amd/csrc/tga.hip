// Truevision TGA texels on gfx950 (dxtex_tga.h holds the per-texel rules): what the .tga codec does per texel either side of its
// byte-serial header, palette and run-length packets, so that a file's texels cross PCIe as the 1, 2, 3 or 4 bytes they are.
//   tga_unpack_kernel  the texel stream in file order (tight rows of width * B bytes; the first row is the image's bottom row unless
//                      TGA_TOP_DOWN, the first texel its rightmost one if TGA_RIGHT_TO_LEFT) -> the image through its own pitch, both flips
//                      applied, and for the kinds with an alpha rule the OR of every alpha and of every alpha ^ 255 into alphaWord[0..1]
//   tga_opaque_kernel  right behind it for those kinds: reads the two ORs, leaves the loader's answer (tga_alpha_answer) in *answer and,
//                      where every alpha is zero and that is not allowed, sets them. Every other wave returns after two scalar loads.
//   tga_pack_kernel    level 0 of an image -> the file's rows: top-down, tight, B bytes a texel
//
// 256 lanes, x across, rows strided over gridDim.y (dxtex_stream.h's grid). Two routes:
//   wide    a lane takes four texels and every access is a naturally aligned dword or wider: 4 * B bytes of the stream as B dwords, 4 * D
//           bytes of the image as one dword (D = 1), dwordx2 (D = 2) or dwordx4 (D = 4). Three-byte texels: three dwords in, one dwordx4
//           out. Under TGA_RIGHT_TO_LEFT the four are reversed and the store address mirrored.
//           THE RULE: width is a multiple of 4, the stream's base is a multiple of 4 (every row and every group of four then starts on a
//           dword, whatever B), and the image's base and row pitch are multiples of 4 * D.
//   narrow  everything else - a width with a tail, a stream at an odd base, image rows off that alignment: a lane takes one texel, reads
//           its B bytes one by one and writes one D-byte word (single bytes where the image's base or pitch is no multiple of D).
// The palette arrives by value in the kernel's arguments (1 KiB, no copy, no host synchronisation) and each workgroup holds it in LDS.
// The alpha ORs: each lane accumulates over its rows, one xor-shuffle reduction per wave, the workgroup's four waves through LDS, at most
// one vector atomicOr per workgroup and word into the two dwords the launcher cleared on the stream (a workgroup whose bits the word
// already holds sends none). OR commutes, so the answer does not depend on the order of the workgroups.
//
// Every read lies inside the stream's width * height * B bytes and every write inside its row's `width` texels: a lane works only where
// x < width (wide: x + 3 < width, as width is a multiple of 4) and y < height.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_tga.h"
#include <algorithm>

namespace dxtex
{
namespace
{
// four D-byte words as one aligned access
template<uint32_t D>
__device__ __forceinline__ void store4(uint8_t* d, const uint32_t (&t)[4])
{
    if constexpr (D == 1u) *reinterpret_cast<uint32_t*>(d) = t[0] | (t[1] << 8) | (t[2] << 16) | (t[3] << 24);
    else if constexpr (D == 2u) *reinterpret_cast<uint2*>(d) = make_uint2(t[0] | (t[1] << 16), t[2] | (t[3] << 16));
    else *reinterpret_cast<uint4*>(d) = make_uint4(t[0], t[1], t[2], t[3]);
}

template<uint32_t D>
__device__ __forceinline__ void load4(const uint8_t* s, uint32_t (&t)[4])
{
    if constexpr (D == 1u) { const uint32_t v = *reinterpret_cast<const uint32_t*>(s); t[0] = v & 0xFFu; t[1] = (v >> 8) & 0xFFu; t[2] = (v >> 16) & 0xFFu; t[3] = v >> 24; }
    else if constexpr (D == 2u) { const uint2 v = *reinterpret_cast<const uint2*>(s); t[0] = v.x & 0xFFFFu; t[1] = v.x >> 16; t[2] = v.y & 0xFFFFu; t[3] = v.y >> 16; }
    else { const uint4 v = *reinterpret_cast<const uint4*>(s); t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w; }
}

__device__ __forceinline__ uint32_t wave_or(uint32_t v)          // gfx950: 64 lanes
{
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off);
    return v;
}

// dstAligned (narrow only): dst's base and pitch are multiples of its texel
template<int KIND, bool WIDE>
__global__ void __launch_bounds__(256) tga_unpack_kernel(const uint8_t* stream, uint32_t flags, ImgView dst, bool dstAligned, uint32_t* alphaWord, PaletteArg<KIND == TGA_PALETTE> pal)
{
    constexpr uint32_t B = tga_file_bytes(KIND), D = tga_image_bytes(KIND), G = WIDE ? 4u : 1u;
    __shared__ uint32_t table[KIND == TGA_PALETTE ? 256 : 1];
    if constexpr (KIND == TGA_PALETTE) palette_to_lds(table, pal);
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * G;
    const bool rightToLeft = (flags & TGA_RIGHT_TO_LEFT) != 0, topDown = (flags & TGA_TOP_DOWN) != 0;
    uint32_t orAlpha = 0, orNotAlpha = 0;
    if (x < dst.width)          // no early return: every lane of the wave takes part in the reduction below
    {
        const uint32_t dx = rightToLeft ? dst.width - G - x : x;
        for (uint32_t y = blockIdx.y; y < dst.height; y += gridDim.y)
        {
            const uint8_t* s = stream + (uint64_t(y) * dst.width + x) * B;
            uint8_t* d = dst.pixels + uint64_t(topDown ? y : dst.height - 1u - y) * dst.rowPitch + uint64_t(dx) * D;
            uint32_t alpha;
            if constexpr (WIDE)
            {
                uint32_t w[B], t[4];
                load_span<B, 4u>(s, w);
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k)
                {
                    t[k] = tga_unpack_texel(texel_of<B>(w, k), KIND, table, alpha);
                    orAlpha |= alpha; orNotAlpha |= alpha ^ 255u;
                }
                if (rightToLeft) { uint32_t v = t[0]; t[0] = t[3]; t[3] = v; v = t[1]; t[1] = t[2]; t[2] = v; }
                store4<D>(d, t);
            }
            else
            {
                store1<D>(d, tga_unpack_texel(le_load32(s, B), KIND, table, alpha), dstAligned);
                orAlpha |= alpha; orNotAlpha |= alpha ^ 255u;
            }
        }
    }
    if constexpr (tga_has_alpha_rule(KIND))
    {
        // wave, then workgroup (four waves through LDS), then at most one atomic per word from lane 0. Only a workgroup that has a bit
        // the word lacks sends its atomic: the word can gain eight bits, so after the first workgroups the rest find theirs there. Every
        // atomic queues on one address - with one per wave and no look a 4096^2 image took 0.75 ms where it streams in 0.02. Bits are
        // only ever set, so a look that misses a newer value costs an atomic, never a bit.
        __shared__ uint32_t waveOr[2][256 / 64];
        orAlpha = wave_or(orAlpha); orNotAlpha = wave_or(orNotAlpha);
        if ((threadIdx.x & 63u) == 0) { waveOr[0][threadIdx.x / 64u] = orAlpha; waveOr[1][threadIdx.x / 64u] = orNotAlpha; }
        __syncthreads();
        if (threadIdx.x == 0)
        {
            orAlpha = waveOr[0][0] | waveOr[0][1] | waveOr[0][2] | waveOr[0][3];
            orNotAlpha = waveOr[1][0] | waveOr[1][1] | waveOr[1][2] | waveOr[1][3];
            if (orAlpha & ~__hip_atomic_load(alphaWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(alphaWord, orAlpha);
            if (orNotAlpha & ~__hip_atomic_load(alphaWord + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicOr(alphaWord + 1, orNotAlpha);
        }
    }
}

// D = 2: B5G5R5A1, bit 15; D = 4: alpha is the fourth byte. One texel per lane, the alpha byte alone is touched.
template<uint32_t D>
__global__ void __launch_bounds__(256) tga_opaque_kernel(ImgView dst, const uint32_t* alphaWord, bool allowAllZero, uint32_t* answer)
{
    bool makeOpaque;
    const uint32_t a = tga_alpha_answer(alphaWord[0], alphaWord[1], allowAllZero, makeOpaque);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *answer = a;
    if (!makeOpaque) return;
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= dst.width) return;
    for (uint32_t y = blockIdx.y; y < dst.height; y += gridDim.y)
    {
        uint8_t* top = dst.pixels + uint64_t(y) * dst.rowPitch + uint64_t(x) * D + (D - 1u);
        *top = D == 2u ? uint8_t(*top | 0x80u) : uint8_t(0xFFu);
    }
}

// B = the file's bytes a texel; the image's are 4 for TGA_ROW_DROP_X, else B. aligned (narrow only): src's base and pitch are multiples
// of its texel, the stream's base of B.
template<int ROW, uint32_t B, bool WIDE>
__global__ void __launch_bounds__(256) tga_pack_kernel(ImgView src, uint8_t* stream, bool srcAligned, bool dstAligned)
{
    constexpr uint32_t D = ROW == TGA_ROW_DROP_X ? 4u : B, G = WIDE ? 4u : 1u;
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * G;
    if (x >= src.width) return;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
    {
        const uint8_t* s = src.pixels + uint64_t(y) * src.rowPitch + uint64_t(x) * D;
        uint8_t* d = stream + (uint64_t(y) * src.width + x) * B;
        if constexpr (WIDE)
        {
            uint32_t t[4];
            load4<D>(s, t);
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) t[k] = tga_pack_texel(t[k], ROW);
            if constexpr (B == 3u)
            {
                uint32_t out[3];
                pack3x4(t, out);
                store_span<3u>(d, out);
            }
            else store4<B>(d, t);
        }
        else store1<B>(d, tga_pack_texel(load1<D>(s, srcAligned), ROW), dstAligned);
    }
}

template<int KIND>
hipError_t unpack_kind(const uint8_t* stream, uint32_t flags, const uint32_t* palette, const ImgView& dv, uint32_t* alphaWord, uint32_t* answer, hipStream_t hs, KernelMarks* marks)
{
    constexpr uint32_t D = tga_image_bytes(KIND);
    PaletteArg<KIND == TGA_PALETTE> pal;
    if constexpr (KIND == TGA_PALETTE) std::copy(palette, palette + 256, pal.word);
    if constexpr (tga_has_alpha_rule(KIND))
    {
        const hipError_t e = hipMemsetAsync(alphaWord, 0, 2 * sizeof(uint32_t), hs);
        if (e != hipSuccess) return e;
    }
    const uint32_t orient = flags & (TGA_RIGHT_TO_LEFT | TGA_TOP_DOWN);
    if (dv.width % 4u == 0 && multiple_of(stream, 0, 4u) && multiple_of(dv.pixels, dv.rowPitch, 4u * D))
    {
        DXTEX_MARK("tga_unpack<wide>");
        hipLaunchKernelGGL((tga_unpack_kernel<KIND, true>), stream_grid(dv.width, dv.height, 4u), dim3(256), 0, hs, stream, orient, dv, true, alphaWord, pal);
    }
    else
    {
        DXTEX_MARK("tga_unpack<narrow>");
        hipLaunchKernelGGL((tga_unpack_kernel<KIND, false>), stream_grid(dv.width, dv.height, 1u), dim3(256), 0, hs, stream, orient, dv, multiple_of(dv.pixels, dv.rowPitch, D), alphaWord, pal);
    }
    if constexpr (tga_has_alpha_rule(KIND))
    {
        DXTEX_MARK("tga_opaque");
        hipLaunchKernelGGL((tga_opaque_kernel<D>), stream_grid(dv.width, dv.height, 1u), dim3(256), 0, hs, dv, alphaWord, (flags & TGA_ALLOW_ALL_ZERO_ALPHA) != 0, answer);
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

template<int ROW, uint32_t B>
hipError_t pack_row(const ImgView& sv, uint8_t* stream, hipStream_t hs, KernelMarks* marks)
{
    constexpr uint32_t D = ROW == TGA_ROW_DROP_X ? 4u : B;
    if (sv.width % 4u == 0 && multiple_of(stream, 0, 4u) && multiple_of(sv.pixels, sv.rowPitch, 4u * D))
    {
        DXTEX_MARK("tga_pack<wide>");
        hipLaunchKernelGGL((tga_pack_kernel<ROW, B, true>), stream_grid(sv.width, sv.height, 4u), dim3(256), 0, hs, sv, stream, true, true);
    }
    else
    {
        DXTEX_MARK("tga_pack<narrow>");
        hipLaunchKernelGGL((tga_pack_kernel<ROW, B, false>), stream_grid(sv.width, sv.height, 1u), dim3(256), 0, hs, sv, stream, multiple_of(sv.pixels, sv.rowPitch, D), multiple_of(stream, 0, B == 3u ? 1u : B));
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
} // namespace

hipError_t launch_tga_unpack(const uint8_t* stream, int kind, uint32_t flags, const uint32_t* palette, const ImgView& dv, uint32_t* alphaWord, uint32_t* answer,
                             hipStream_t hs, KernelMarks* marks)
{
    if (!dv.width || !dv.height) return hipSuccess;
    switch (kind)
    {
#define DXTEX_TGA_KIND(K) case K: return unpack_kind<K>(stream, flags, palette, dv, alphaWord, answer, hs, marks)
    DXTEX_TGA_KIND(TGA_GREY); DXTEX_TGA_KIND(TGA_5551); DXTEX_TGA_KIND(TGA_RGB_RGBA); DXTEX_TGA_KIND(TGA_RGB_BGRX);
    DXTEX_TGA_KIND(TGA_BGRA_RGBA); DXTEX_TGA_KIND(TGA_BGRA_BGRA);
#undef DXTEX_TGA_KIND
    case TGA_PALETTE: return palette ? unpack_kind<TGA_PALETTE>(stream, flags, palette, dv, alphaWord, answer, hs, marks) : hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_tga_pack(const ImgView& sv, int row, uint32_t bytesPerTexel, uint8_t* stream, hipStream_t hs, KernelMarks* marks)
{
    if (!sv.width || !sv.height) return hipSuccess;
    if (row == TGA_ROW_SWAP_RB && bytesPerTexel == 4u) return pack_row<TGA_ROW_SWAP_RB, 4u>(sv, stream, hs, marks);
    if (row == TGA_ROW_DROP_X && bytesPerTexel == 3u) return pack_row<TGA_ROW_DROP_X, 3u>(sv, stream, hs, marks);
    if (row != TGA_ROW_COPY) return hipErrorInvalidValue;
    switch (bytesPerTexel)
    {
    case 1u: return pack_row<TGA_ROW_COPY, 1u>(sv, stream, hs, marks);
    case 2u: return pack_row<TGA_ROW_COPY, 2u>(sv, stream, hs, marks);
    case 4u: return pack_row<TGA_ROW_COPY, 4u>(sv, stream, hs, marks);
    default: return hipErrorInvalidValue;
    }
}
} // namespace dxtex
