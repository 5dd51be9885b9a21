// PNG texels on gfx950 (dxtex_png.h holds the per-texel rules): what the .png codec does per texel once the host has inflated and
// unfiltered the image data, so that a file's rows cross PCIe as the 1/8 to 8 bytes a texel they are.
//   png_unpack_kernel  the unfiltered rows (tight, ceil(width * bits / 8) bytes each) -> the image through its own pitch: sub-byte grey
//                      multiplied out, palette indices looked up, grey + alpha and RGB widened to four channels, 16-bit samples swapped
//                      to little-endian, B and R exchanged under PNG_BGR
//   png_pack_kernel    level 0 of an image -> the file's rows, tight: B and R exchanged for a BGR source, X dropped, 16-bit samples
//                      swapped to big-endian
//
// 256 lanes, x across, rows strided over gridDim.y (dxtex_stream.h's grid). Two routes:
//   wide    whole-byte kinds: a lane takes four texels, 4 * B bytes of the stream and 4 * D bytes of the image, each moved as the widest
//           aligned accesses its dword count allows (dxtex_stream.h's span_align: a multiple of four dwords as dwordx4, of two as dwordx2, else single
//           dwords). RGB 8: three dwords in, one dwordx4 out. RGBA 16: two dwordx4 in and out. Grey 8 and palette 8: one dword in.
//           Sub-byte kinds: a lane takes one byte of the stream and writes its 8, 4 or 2 texels: 8 bytes of grey 1, a dwordx4 of palette 2,
//           two of palette 1.
//           THE RULE: width is a multiple of 4 (sub-byte: of the texels in a byte), and the stream's base, the image's base and the
//           image's row pitch are multiples of their side's alignment. A row of the stream is then whole groups, so with the base every
//           row and every group is aligned.
//   narrow  everything else - a width with a tail, a stream behind an odd base, image rows off that alignment: a lane takes one texel and
//           moves it byte by byte.
// Both routes call the same functions of dxtex_png.h on the same little-endian words, as the host codec does.
// The palette arrives by value in the kernel's arguments (1 KiB, no copy, no host synchronisation) with PNG_BGR already applied, and each
// workgroup holds it in LDS: 256 words, read at a data-dependent index, one word per lane.
//
// Every read lies inside the stream's height * ceil(width * bits / 8) bytes and every write inside its row's `width` texels: a lane works
// only where its first texel x < width (wide: the whole group, as width is a multiple of the group) and y < height.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_png.h"
#include <algorithm>

namespace dxtex
{
namespace
{
// BYTES bytes at byte OFF of consecutive little-endian dwords, as a little-endian word; every index is a constant once unrolled
template<uint32_t OFF, uint32_t BYTES, uint32_t N>
__device__ __forceinline__ uint64_t get_bytes(const uint32_t (&w)[N])
{
    static_assert(OFF + BYTES <= 4u * N && BYTES <= 8u, "inside the span");
    if constexpr (OFF % 4u == 0 && BYTES == 4u) return w[OFF / 4u];
    else if constexpr (OFF % 4u == 0 && BYTES == 8u) return uint64_t(w[OFF / 4u]) | (uint64_t(w[OFF / 4u + 1u]) << 32);
    else
    {
        uint64_t v = 0;
#pragma unroll
        for (uint32_t b = 0; b < BYTES; ++b) v |= uint64_t((w[(OFF + b) / 4u] >> (8u * ((OFF + b) % 4u))) & 0xFFu) << (8u * b);
        return v;
    }
}

// the reverse, ORed into dwords that start as zero
template<uint32_t OFF, uint32_t BYTES, uint32_t N>
__device__ __forceinline__ void put_bytes(uint32_t (&w)[N], uint64_t v)
{
    static_assert(OFF + BYTES <= 4u * N && BYTES <= 8u, "inside the span");
    if constexpr (OFF % 4u == 0 && BYTES == 4u) w[OFF / 4u] = uint32_t(v);
    else if constexpr (OFF % 4u == 0 && BYTES == 8u) { w[OFF / 4u] = uint32_t(v); w[OFF / 4u + 1u] = uint32_t(v >> 32); }
    else
    {
#pragma unroll
        for (uint32_t b = 0; b < BYTES; ++b) w[(OFF + b) / 4u] |= uint32_t((v >> (8u * b)) & 0xFFu) << (8u * ((OFF + b) % 4u));
    }
}

constexpr uint32_t dwords_of(uint32_t bytes) { return bytes < 4u ? 1u : bytes / 4u; }

// the group of texels a lane of the wide route takes, and the bytes it writes
template<int KIND> constexpr uint32_t wide_group() { return png_is_sub_byte(KIND) ? 8u / png_file_bits(KIND) : 4u; }
template<int KIND> constexpr uint32_t wide_image_bytes() { return wide_group<KIND>() * png_image_bytes(KIND); }
// the alignment the image side of the wide route needs: 2 bytes for grey 4's two texels, else that of its dwords
template<int KIND> constexpr uint32_t wide_image_align() { return wide_image_bytes<KIND>() < 4u ? wide_image_bytes<KIND>() : span_align<wide_image_bytes<KIND>() / 4u>(); }
template<int KIND> constexpr uint32_t wide_stream_align() { return png_is_sub_byte(KIND) ? 1u : span_align<png_file_bits(KIND) / 8u>(); }

template<int KIND, uint32_t K>
__device__ __forceinline__ void unpack_one(const uint32_t (&in)[png_file_bits(KIND) / 8u], uint32_t (&out)[png_image_bytes(KIND)], bool bgr, const uint32_t* table)
{
    constexpr uint32_t B = png_file_bits(KIND) / 8u, D = png_image_bytes(KIND);
    put_bytes<K * D, D>(out, png_texel(KIND, get_bytes<K * B, B>(in), bgr, table));
}

template<int KIND, bool WIDE>
__global__ void __launch_bounds__(256) png_unpack_kernel(const uint8_t* stream, bool bgr, ImgView dst, PaletteArg<png_is_palette(KIND)> pal)
{
    constexpr uint32_t BITS = png_file_bits(KIND), D = png_image_bytes(KIND), G = WIDE ? wide_group<KIND>() : 1u;
    __shared__ uint32_t lds[png_is_palette(KIND) ? 256 : 1];
    const uint32_t* table = nullptr;
    if constexpr (png_is_palette(KIND))
    {
        lds[threadIdx.x] = bgr ? swap_rb(pal.word[threadIdx.x]) : pal.word[threadIdx.x];          // the whole workgroup reaches the barrier
        __syncthreads();
        table = lds;
        bgr = false;
    }
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * G;
    if (x >= dst.width) return;
    const uint64_t rowBytes = png_row_bytes(KIND, dst.width);
    for (uint32_t y = blockIdx.y; y < dst.height; y += gridDim.y)
    {
        const uint8_t* row = stream + uint64_t(y) * rowBytes;
        uint8_t* d = dst.pixels + uint64_t(y) * dst.rowPitch + uint64_t(x) * D;
        if constexpr (!WIDE) png_unpack_texel(row, x, d, KIND, bgr, table);
        else if constexpr (BITS < 8u)
        {
            constexpr uint32_t W = wide_image_bytes<KIND>();
            const uint32_t byte = row[x / G];
            uint32_t out[dwords_of(W)] = {};
            if constexpr (D == 4u)
            {
#pragma unroll
                for (uint32_t j = 0; j < G; ++j) out[j] = png_sub_byte_texel(KIND, byte, j, false, table);
            }
            else
            {
#pragma unroll
                for (uint32_t j = 0; j < G; ++j) out[j / 4u] |= png_sub_byte_texel(KIND, byte, j, false, table) << (8u * (j % 4u));
            }
            if constexpr (W < 4u) *reinterpret_cast<uint16_t*>(d) = uint16_t(out[0]);
            else store_span<W / 4u>(d, out);
        }
        else
        {
            constexpr uint32_t B = BITS / 8u;
            uint32_t in[B], out[D] = {};
            load_span<B>(row + uint64_t(x) * B, in);
            unpack_one<KIND, 0>(in, out, bgr, table); unpack_one<KIND, 1>(in, out, bgr, table);
            unpack_one<KIND, 2>(in, out, bgr, table); unpack_one<KIND, 3>(in, out, bgr, table);
            store_span<D>(d, out);
        }
    }
}

template<int SRC, uint32_t K>
__device__ __forceinline__ void pack_one(const uint32_t (&in)[png_source_bytes(SRC)], uint32_t (&out)[png_source_file_bytes(SRC)])
{
    constexpr uint32_t S = png_source_bytes(SRC), F = png_source_file_bytes(SRC);
    put_bytes<K * F, F>(out, png_pack(SRC, get_bytes<K * S, S>(in)));
}

template<int SRC, bool WIDE>
__global__ void __launch_bounds__(256) png_pack_kernel(ImgView src, uint8_t* stream)
{
    constexpr uint32_t S = png_source_bytes(SRC), F = png_source_file_bytes(SRC), G = WIDE ? 4u : 1u;
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * G;
    if (x >= src.width) return;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
    {
        const uint8_t* s = src.pixels + uint64_t(y) * src.rowPitch + uint64_t(x) * S;
        uint8_t* d = stream + (uint64_t(y) * src.width + x) * F;
        if constexpr (WIDE)
        {
            uint32_t in[S], out[F] = {};
            load_span<S>(s, in);
            pack_one<SRC, 0>(in, out); pack_one<SRC, 1>(in, out); pack_one<SRC, 2>(in, out); pack_one<SRC, 3>(in, out);
            store_span<F>(d, out);
        }
        else png_pack_texel(s, d, SRC);
    }
}

template<int KIND>
hipError_t unpack_kind(const uint8_t* stream, uint32_t flags, const uint32_t* palette, const ImgView& dv, hipStream_t hs, KernelMarks* marks)
{
    const bool bgr = (flags & PNG_BGR) != 0 && png_takes_bgr(KIND);
    PaletteArg<png_is_palette(KIND)> pal;
    if constexpr (png_is_palette(KIND)) std::copy(palette, palette + 256, pal.word);
    constexpr uint32_t G = wide_group<KIND>();
    if (dv.width % G == 0 && multiple_of(stream, 0, wide_stream_align<KIND>()) && multiple_of(dv.pixels, dv.rowPitch, wide_image_align<KIND>()))
    {
        DXTEX_MARK("png_unpack<wide>");
        hipLaunchKernelGGL((png_unpack_kernel<KIND, true>), stream_grid(dv.width, dv.height, G), dim3(256), 0, hs, stream, bgr, dv, pal);
    }
    else
    {
        DXTEX_MARK("png_unpack<narrow>");
        hipLaunchKernelGGL((png_unpack_kernel<KIND, false>), stream_grid(dv.width, dv.height, 1u), dim3(256), 0, hs, stream, bgr, dv, pal);
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

template<int SRC>
hipError_t pack_source(const ImgView& sv, uint8_t* stream, hipStream_t hs, KernelMarks* marks)
{
    constexpr uint32_t S = png_source_bytes(SRC), F = png_source_file_bytes(SRC);
    if (sv.width % 4u == 0 && multiple_of(stream, 0, span_align<F>()) && multiple_of(sv.pixels, sv.rowPitch, span_align<S>()))
    {
        DXTEX_MARK("png_pack<wide>");
        hipLaunchKernelGGL((png_pack_kernel<SRC, true>), stream_grid(sv.width, sv.height, 4u), dim3(256), 0, hs, sv, stream);
    }
    else
    {
        DXTEX_MARK("png_pack<narrow>");
        hipLaunchKernelGGL((png_pack_kernel<SRC, false>), stream_grid(sv.width, sv.height, 1u), dim3(256), 0, hs, sv, stream);
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
} // namespace

hipError_t launch_png_unpack(const uint8_t* stream, int kind, uint32_t flags, const uint32_t* palette, const ImgView& dv, hipStream_t hs, KernelMarks* marks)
{
    if (!dv.width || !dv.height) return hipSuccess;
    if (kind >= 0 && kind < PNG_KINDS && png_is_palette(kind) && !palette) return hipErrorInvalidValue;
    switch (kind)
    {
#define DXTEX_PNG_KIND(K) case K: return unpack_kind<K>(stream, flags, palette, dv, hs, marks)
    DXTEX_PNG_KIND(PNG_G1); DXTEX_PNG_KIND(PNG_G2); DXTEX_PNG_KIND(PNG_G4); DXTEX_PNG_KIND(PNG_G8); DXTEX_PNG_KIND(PNG_G16);
    DXTEX_PNG_KIND(PNG_GA8); DXTEX_PNG_KIND(PNG_GA16); DXTEX_PNG_KIND(PNG_RGB8); DXTEX_PNG_KIND(PNG_RGB16); DXTEX_PNG_KIND(PNG_RGBA8);
    DXTEX_PNG_KIND(PNG_RGBA16); DXTEX_PNG_KIND(PNG_P1); DXTEX_PNG_KIND(PNG_P2); DXTEX_PNG_KIND(PNG_P4); DXTEX_PNG_KIND(PNG_P8);
#undef DXTEX_PNG_KIND
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_png_pack(const ImgView& sv, int source, uint8_t* stream, hipStream_t hs, KernelMarks* marks)
{
    if (!sv.width || !sv.height) return hipSuccess;
    switch (source)
    {
    case PNG_SRC_R8: return pack_source<PNG_SRC_R8>(sv, stream, hs, marks);
    case PNG_SRC_R16: return pack_source<PNG_SRC_R16>(sv, stream, hs, marks);
    case PNG_SRC_RGBA8: return pack_source<PNG_SRC_RGBA8>(sv, stream, hs, marks);
    case PNG_SRC_BGRA8: return pack_source<PNG_SRC_BGRA8>(sv, stream, hs, marks);
    case PNG_SRC_RGBA16: return pack_source<PNG_SRC_RGBA16>(sv, stream, hs, marks);
    case PNG_SRC_BGRX8: return pack_source<PNG_SRC_BGRX8>(sv, stream, hs, marks);
    default: return hipErrorInvalidValue;
    }
}
} // namespace dxtex
