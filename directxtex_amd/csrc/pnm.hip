// Portable pixmap texels on gfx950 (dxtex_pnm.h holds the per-texel rules): what the .ppm / .pfm / .phm codec does per texel behind its
// text header, so that a file's samples cross PCIe as the 3, 12, 4, 6 or 2 bytes a texel they are.
//   pnm_unpack_kernel  the samples in file order (tight rows of width * B bytes; a float kind's first row is the image's bottom row) -> the
//                      image through its own pitch: 3 bytes to 4 with the maxval rescale (PNM_P6), 3 elements to 4 with an alpha of one
//                      (PNM_PF, PNM_PH), a copy (PNM_Pf, PNM_Ph), the elements' bytes swapped under PNM_BIG_ENDIAN
//   pnm_pack_kernel    level 0 of an image -> the file's rows, tight: alpha dropped, B and R exchanged for a BGR source, halves widened, a
//                      float kind's rows bottom first
//
// 256 lanes, x across, rows strided over gridDim.y (dxtex_stream.h's grid). Two routes:
//   wide    a lane takes four texels: 4 * B bytes of the stream and 4 * D bytes of the image, each moved as the widest aligned accesses
//           its dword count allows (dxtex_stream.h's span_align: a multiple of four dwords as dwordx4, of two as dwordx2, else single dwords). P6: three
//           dwords in, one dwordx4 out. PF: three dwordx4 in, four out. PH: three dwordx2 in, two dwordx4 out.
//           THE RULE: width is a multiple of 4, and the stream's base, the image's base and the image's row pitch are multiples of their
//           side's span_align (stream: 4 for P6, 16 for PF and Pf, 8 for PH and Ph; image: 16, and 8 for Ph). A row of the stream is
//           width / 4 whole groups, so with the base every row and every group is aligned.
//   narrow  everything else - a width with a tail, a stream behind an odd base, image rows off that alignment: a lane takes one texel and
//           moves it element by element (single bytes where that side's base or pitch is no multiple of the element; a P6 texel's three
//           bytes always singly).
// Both routes call the same functions of dxtex_pnm.h on the same little-endian words, as the host codec does.
// The maxval table (PNM_P6 with maxval != 255 only): 256 words of 255 * i / maxval in LDS, one division per lane and workgroup. With
// maxval == 255 there is no table and no division: the word is the three bytes and 0xff.
//
// Every read lies inside the stream's width * height * B bytes and every write inside its row's `width` texels: a lane works only where
// x < width (wide: x + 3 < width, as width is a multiple of 4) and y < height.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_pnm.h"

namespace dxtex
{
namespace
{
// 16-bit element j of consecutive ones held as little-endian dwords
template<uint32_t N>
__device__ __forceinline__ uint32_t half_of(const uint32_t (&w)[N], uint32_t j) { return (w[j / 2u] >> (16u * (j & 1u))) & 0xFFFFu; }

// four file texels (B dwords) -> four image texels (D dwords)
template<int KIND>
__device__ __forceinline__ void unpack4(const uint32_t (&in)[pnm_file_bytes(KIND)], uint32_t (&out)[pnm_image_bytes(KIND)], bool bigEndian, const uint32_t* scale)
{
    if constexpr (KIND == PNM_P6)
    {
        // texel k's three bytes start at bit 24 * k of the 96. This is texel_of<3> written out without its 24-bit mask, which
        // pnm_p6_texel does not need (it ignores the top byte): with the mask the kernel came out two instructions longer and, in one of
        // two measurements, 3 to 5 % slower (profiles/stream_layer.md)
        out[0] = pnm_p6_texel(in[0], scale);
        out[1] = pnm_p6_texel((in[0] >> 24) | (in[1] << 8), scale);
        out[2] = pnm_p6_texel((in[1] >> 16) | (in[2] << 16), scale);
        out[3] = pnm_p6_texel(in[2] >> 8, scale);
    }
    else if constexpr (KIND == PNM_PF)
    {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
        {
#pragma unroll
            for (uint32_t c = 0; c < 3u; ++c) out[4 * k + c] = pnm_element(in[3 * k + c], 4u, bigEndian);
            out[4 * k + 3] = pnm_one(KIND);
        }
    }
    else if constexpr (KIND == PNM_Pf)
    {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) out[k] = pnm_element(in[k], 4u, bigEndian);
    }
    else if constexpr (KIND == PNM_PH)
    {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
        {
            out[2 * k] = pnm_element(half_of(in, 3 * k), 2u, bigEndian) | (pnm_element(half_of(in, 3 * k + 1), 2u, bigEndian) << 16);
            out[2 * k + 1] = pnm_element(half_of(in, 3 * k + 2), 2u, bigEndian) | (pnm_one(KIND) << 16);
        }
    }
    else
    {
#pragma unroll
        for (uint32_t i = 0; i < 2u; ++i) out[i] = pnm_element(in[i] & 0xFFFFu, 2u, bigEndian) | (pnm_element(in[i] >> 16, 2u, bigEndian) << 16);
    }
}

// streamAligned / imageAligned (narrow only): that side's base (and pitch) is a multiple of the element
template<int KIND, bool WIDE>
__global__ void __launch_bounds__(256) pnm_unpack_kernel(const uint8_t* stream, uint32_t maxval, bool bigEndian, ImgView dst, bool streamAligned, bool imageAligned)
{
    constexpr uint32_t B = pnm_file_bytes(KIND), D = pnm_image_bytes(KIND), E = pnm_element_bytes(KIND), G = WIDE ? 4u : 1u;
    __shared__ uint32_t table[KIND == PNM_P6 ? 256 : 1];
    const uint32_t* scale = nullptr;
    if constexpr (KIND == PNM_P6)
    {
        if (maxval != 255u)          // uniform: the barrier is reached by the whole workgroup or by none of it
        {
            table[threadIdx.x] = pnm_scale(threadIdx.x, maxval);
            __syncthreads();
            scale = table;
        }
    }
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * G;
    if (x >= dst.width) return;
    for (uint32_t y = blockIdx.y; y < dst.height; y += gridDim.y)
    {
        const uint8_t* s = stream + (uint64_t(y) * dst.width + x) * B;
        uint8_t* d = dst.pixels + uint64_t(pnm_image_row(KIND, y, dst.height)) * dst.rowPitch + uint64_t(x) * D;
        if constexpr (WIDE)
        {
            uint32_t in[B], out[D];
            load_span<B>(s, in);
            unpack4<KIND>(in, out, bigEndian, scale);
            store_span<D>(d, out);
        }
        else if constexpr (KIND == PNM_P6) store1<4u>(d, pnm_p6_texel(le_load32(s, 3u), scale), imageAligned);
        else
        {
            constexpr uint32_t n = pnm_file_elements(KIND);
#pragma unroll
            for (uint32_t c = 0; c < n; ++c) store1<E>(d + c * E, pnm_element(load1<E>(s + c * E, streamAligned), E, bigEndian), imageAligned);
            if constexpr (n == 3u) store1<E>(d + 3u * E, pnm_one(KIND), imageAligned);
        }
    }
}

// four image texels (S dwords) -> four file texels (B dwords)
template<int SRC>
__device__ __forceinline__ void pack4(const uint32_t (&in)[pnm_source_bytes(SRC)], uint32_t (&out)[pnm_file_bytes(pnm_source_kind(SRC))])
{
    if constexpr (SRC == PNM_SRC_RGBA8 || SRC == PNM_SRC_BGRA8)
    {
        uint32_t t[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) t[k] = pnm_pack_p6(in[k], SRC == PNM_SRC_BGRA8);
        pack3x4(t, out);
    }
    else if constexpr (SRC == PNM_SRC_RGBA32F)
    {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
#pragma unroll
            for (uint32_t c = 0; c < 3u; ++c) out[3 * k + c] = in[4 * k + c];
    }
    else if constexpr (SRC == PNM_SRC_RGBA16F)
    {
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k)
#pragma unroll
            for (uint32_t c = 0; c < 3u; ++c) out[3 * k + c] = pnm_half_to_float_bits(half_of(in, 4 * k + c));
    }
    else
    {
#pragma unroll
        for (uint32_t i = 0; i < pnm_source_bytes(SRC); ++i) out[i] = in[i];          // RGB32F, R32F: the flip is all there is
    }
}

template<int SRC, bool WIDE>
__global__ void __launch_bounds__(256) pnm_pack_kernel(ImgView src, uint8_t* stream, bool imageAligned, bool streamAligned)
{
    constexpr int KIND = pnm_source_kind(SRC);
    constexpr uint32_t S = pnm_source_bytes(SRC), B = pnm_file_bytes(KIND), G = WIDE ? 4u : 1u;
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * G;
    if (x >= src.width) return;
    for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
    {
        const uint8_t* s = src.pixels + uint64_t(pnm_image_row(KIND, y, src.height)) * src.rowPitch + uint64_t(x) * S;
        uint8_t* d = stream + (uint64_t(y) * src.width + x) * B;
        if constexpr (WIDE)
        {
            uint32_t in[S], out[B];
            load_span<S>(s, in);
            pack4<SRC>(in, out);
            store_span<B>(d, out);
        }
        else if constexpr (KIND == PNM_P6) le_store32(d, pnm_pack_p6(load1<4u>(s, imageAligned), SRC == PNM_SRC_BGRA8), 3u);
        else if constexpr (SRC == PNM_SRC_RGBA16F)
        {
#pragma unroll
            for (uint32_t c = 0; c < 3u; ++c) store1<4u>(d + 4u * c, pnm_half_to_float_bits(load1<2u>(s + 2u * c, imageAligned)), streamAligned);
        }
        else
        {
#pragma unroll
            for (uint32_t c = 0; c < B / 4u; ++c) store1<4u>(d + 4u * c, load1<4u>(s + 4u * c, imageAligned), streamAligned);
        }
    }
}

template<int KIND>
hipError_t unpack_kind(const uint8_t* stream, uint32_t maxval, uint32_t flags, const ImgView& dv, hipStream_t hs, KernelMarks* marks)
{
    constexpr uint32_t B = pnm_file_bytes(KIND), D = pnm_image_bytes(KIND), E = pnm_element_bytes(KIND);
    const bool bigEndian = (flags & PNM_BIG_ENDIAN) != 0;
    if (dv.width % 4u == 0 && multiple_of(stream, 0, span_align<B>()) && multiple_of(dv.pixels, dv.rowPitch, span_align<D>()))
    {
        DXTEX_MARK("pnm_unpack<wide>");
        hipLaunchKernelGGL((pnm_unpack_kernel<KIND, true>), stream_grid(dv.width, dv.height, 4u), dim3(256), 0, hs, stream, maxval, bigEndian, dv, true, true);
    }
    else
    {
        DXTEX_MARK("pnm_unpack<narrow>");
        hipLaunchKernelGGL((pnm_unpack_kernel<KIND, false>), stream_grid(dv.width, dv.height, 1u), dim3(256), 0, hs, stream, maxval, bigEndian, dv,
                           multiple_of(stream, 0, E), multiple_of(dv.pixels, dv.rowPitch, KIND == PNM_P6 ? 4u : E));
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}

template<int SRC>
hipError_t pack_source(const ImgView& sv, uint8_t* stream, hipStream_t hs, KernelMarks* marks)
{
    constexpr uint32_t S = pnm_source_bytes(SRC), B = pnm_file_bytes(pnm_source_kind(SRC));
    if (sv.width % 4u == 0 && multiple_of(stream, 0, span_align<B>()) && multiple_of(sv.pixels, sv.rowPitch, span_align<S>()))
    {
        DXTEX_MARK("pnm_pack<wide>");
        hipLaunchKernelGGL((pnm_pack_kernel<SRC, true>), stream_grid(sv.width, sv.height, 4u), dim3(256), 0, hs, sv, stream, true, true);
    }
    else
    {
        DXTEX_MARK("pnm_pack<narrow>");
        hipLaunchKernelGGL((pnm_pack_kernel<SRC, false>), stream_grid(sv.width, sv.height, 1u), dim3(256), 0, hs, sv, stream,
                           multiple_of(sv.pixels, sv.rowPitch, SRC == PNM_SRC_RGBA16F ? 2u : 4u), multiple_of(stream, 0, 4u));
    }
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
} // namespace

hipError_t launch_pnm_unpack(const uint8_t* stream, int kind, uint32_t maxval, uint32_t flags, const ImgView& dv, hipStream_t hs, KernelMarks* marks)
{
    if (!dv.width || !dv.height) return hipSuccess;
    switch (kind)
    {
    case PNM_P6: return (maxval >= 1u && maxval <= 255u) ? unpack_kind<PNM_P6>(stream, maxval, flags, dv, hs, marks) : hipErrorInvalidValue;
    case PNM_PF: return unpack_kind<PNM_PF>(stream, maxval, flags, dv, hs, marks);
    case PNM_Pf: return unpack_kind<PNM_Pf>(stream, maxval, flags, dv, hs, marks);
    case PNM_PH: return unpack_kind<PNM_PH>(stream, maxval, flags, dv, hs, marks);
    case PNM_Ph: return unpack_kind<PNM_Ph>(stream, maxval, flags, dv, hs, marks);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_pnm_pack(const ImgView& sv, int source, uint8_t* stream, hipStream_t hs, KernelMarks* marks)
{
    if (!sv.width || !sv.height) return hipSuccess;
    switch (source)
    {
    case PNM_SRC_RGBA8: return pack_source<PNM_SRC_RGBA8>(sv, stream, hs, marks);
    case PNM_SRC_BGRA8: return pack_source<PNM_SRC_BGRA8>(sv, stream, hs, marks);
    case PNM_SRC_RGBA32F: return pack_source<PNM_SRC_RGBA32F>(sv, stream, hs, marks);
    case PNM_SRC_RGB32F: return pack_source<PNM_SRC_RGB32F>(sv, stream, hs, marks);
    case PNM_SRC_RGBA16F: return pack_source<PNM_SRC_RGBA16F>(sv, stream, hs, marks);
    case PNM_SRC_R32F: return pack_source<PNM_SRC_R32F>(sv, stream, hs, marks);
    default: return hipErrorInvalidValue;
    }
}
} // namespace dxtex
