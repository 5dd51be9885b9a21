// The texel-stream layer under the file codecs (rgbe.hip, tga.hip, dds.hip, pnm.hip, png.hip, exr.hip and their dxtex_*.h): what moving a
// file's texels at their own bytes a texel needs whatever the format, once. The per-format headers hold only their enums, tables and
// texel rules and call these directly.
//
// First the pieces for host and device, which also build as plain C++ (the host codecs of host/ and the checks of tests/cpp;
// tests/cpp/stream_check.cpp checks them): the format ids (FMT_*), little-endian words at any address, the byte swaps, a texel cut out of dwords, four 3-byte
// texels as three dwords, the alignment a route asks for, and the launch grid as plain integers. Then, for the .hip files only, the
// accesses themselves: spans of dwords, one element, the palette argument, the dim3 grid and the mark macro.
#pragma once
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define DXTEX_FN __host__ __device__ inline
#else
#define DXTEX_FN inline
#endif
#include <stdint.h>

namespace dxtex
{
// Public DXGI numbering (only the formats this library names): the one list of format ids, for the kernels (dxtex_device.h includes
// this header) and for plain C++, which the codec tables of dxtex_{tga,dds,pnm,png,jpeg}.h are written over.
// host/DirectXTexAMD_Internal.h ties DirectXTexAMD.h's DXGI_FORMAT_* to it.
enum : int
{
    FMT_UNKNOWN = 0,
    FMT_R32G32B32A32_TYPELESS = 1, FMT_R32G32B32A32_FLOAT = 2, FMT_R32G32B32A32_UINT = 3, FMT_R32G32B32A32_SINT = 4,
    FMT_R32G32B32_FLOAT = 6, FMT_R32G32B32_UINT = 7, FMT_R32G32B32_SINT = 8,
    FMT_R16G16B16A16_TYPELESS = 9, FMT_R16G16B16A16_FLOAT = 10,
    FMT_R16G16B16A16_UNORM = 11, FMT_R16G16B16A16_UINT = 12,
    FMT_R16G16B16A16_SNORM = 13, FMT_R16G16B16A16_SINT = 14,
    FMT_R32G32_FLOAT = 16, FMT_R32G32_UINT = 17, FMT_R32G32_SINT = 18,
    FMT_D32_FLOAT_S8X24_UINT = 20,
    FMT_R10G10B10A2_TYPELESS = 23, FMT_R10G10B10A2_UNORM = 24, FMT_R10G10B10A2_UINT = 25,
    FMT_R11G11B10_FLOAT = 26,
    FMT_R8G8B8A8_TYPELESS = 27, FMT_R8G8B8A8_UNORM = 28,
    FMT_R8G8B8A8_UNORM_SRGB = 29, FMT_R8G8B8A8_UINT = 30,
    FMT_R8G8B8A8_SNORM = 31, FMT_R8G8B8A8_SINT = 32,
    FMT_R16G16_FLOAT = 34,
    FMT_R16G16_UNORM = 35, FMT_R16G16_UINT = 36,
    FMT_R16G16_SNORM = 37, FMT_R16G16_SINT = 38,
    FMT_D32_FLOAT = 40, FMT_R32_FLOAT = 41, FMT_R32_UINT = 42, FMT_R32_SINT = 43,
    FMT_D24_UNORM_S8_UINT = 45,
    FMT_R8G8_UNORM = 49, FMT_R8G8_UINT = 50,
    FMT_R8G8_SNORM = 51, FMT_R8G8_SINT = 52,
    FMT_R16_FLOAT = 54, FMT_D16_UNORM = 55,
    FMT_R16_UNORM = 56, FMT_R16_UINT = 57,
    FMT_R16_SNORM = 58, FMT_R16_SINT = 59,
    FMT_R8_UNORM = 61, FMT_R8_UINT = 62,
    FMT_R8_SNORM = 63, FMT_R8_SINT = 64,
    FMT_A8_UNORM = 65, FMT_R1_UNORM = 66,
    FMT_R9G9B9E5_SHAREDEXP = 67, FMT_R8G8_B8G8_UNORM = 68, FMT_G8R8_G8B8_UNORM = 69,
    FMT_BC1_UNORM = 71, FMT_BC1_UNORM_SRGB = 72,
    FMT_BC2_UNORM = 74, FMT_BC2_UNORM_SRGB = 75,
    FMT_BC3_UNORM = 77, FMT_BC3_UNORM_SRGB = 78,
    FMT_BC4_UNORM = 80, FMT_BC4_SNORM = 81,
    FMT_BC5_UNORM = 83, FMT_BC5_SNORM = 84,
    FMT_B5G6R5_UNORM = 85, FMT_B5G5R5A1_UNORM = 86,
    FMT_B8G8R8A8_UNORM = 87, FMT_B8G8R8X8_UNORM = 88, FMT_R10G10B10_XR_BIAS_A2_UNORM = 89,
    FMT_B8G8R8A8_TYPELESS = 90, FMT_B8G8R8A8_UNORM_SRGB = 91, FMT_B8G8R8X8_TYPELESS = 92, FMT_B8G8R8X8_UNORM_SRGB = 93,
    FMT_BC6H_UF16 = 95, FMT_BC6H_SF16 = 96,
    FMT_BC7_UNORM = 98, FMT_BC7_UNORM_SRGB = 99,
    FMT_AYUV = 100, FMT_Y410 = 101, FMT_Y416 = 102, FMT_YUY2 = 107, FMT_Y210 = 108, FMT_Y216 = 109,
    FMT_B4G4R4A4_UNORM = 115,
    FMT_R10G10B10_7E3_A2_FLOAT = 116, FMT_R10G10B10_6E4_A2_FLOAT = 117,       // XBOX_DXGI_FORMAT_*: the console HDR formats
    FMT_R10G10B10_SNORM_A2_UNORM = 189, FMT_R4G4_UNORM = 190,                 // XBOX_DXGI_FORMAT_*
    FMT_A4B4G4R4_UNORM = 191,
};

// 1 to 4 bytes at any address as a little-endian word, the rest zero
DXTEX_FN uint32_t le_load32(const uint8_t* s, uint32_t bytes)
{
    uint32_t t = s[0];
    if (bytes > 1) t |= uint32_t(s[1]) << 8;
    if (bytes > 2) t |= uint32_t(s[2]) << 16;
    if (bytes > 3) t |= uint32_t(s[3]) << 24;
    return t;
}

DXTEX_FN void le_store32(uint8_t* d, uint32_t t, uint32_t bytes)
{
    d[0] = uint8_t(t);
    if (bytes > 1) d[1] = uint8_t(t >> 8);
    if (bytes > 2) d[2] = uint8_t(t >> 16);
    if (bytes > 3) d[3] = uint8_t(t >> 24);
}

// 0 to 8 bytes likewise
DXTEX_FN uint64_t le_load64(const uint8_t* s, uint32_t bytes)
{
    uint64_t t = 0;
    for (uint32_t b = 0; b < bytes; ++b) t |= uint64_t(s[b]) << (8u * b);
    return t;
}

DXTEX_FN void le_store64(uint8_t* d, uint64_t t, uint32_t bytes)
{
    for (uint32_t b = 0; b < bytes; ++b) d[b] = uint8_t(t >> (8u * b));
}

// bytes 0 and 2 of a word exchanged: R and B of an 8-bit colour texel
DXTEX_FN constexpr uint32_t swap_rb(uint32_t t) { return (t & 0xFF00FF00u) | ((t & 0xFFu) << 16) | ((t >> 16) & 0xFFu); }
// the bytes of a 16-bit element (the word's upper half is ignored), of a 32-bit one, of each of four 16-bit ones
DXTEX_FN constexpr uint32_t swap16(uint32_t e) { return ((e & 0xFFu) << 8) | ((e >> 8) & 0xFFu); }
DXTEX_FN constexpr uint32_t swap32(uint32_t e) { return (e << 24) | ((e & 0xFF00u) << 8) | ((e >> 8) & 0xFF00u) | (e >> 24); }
DXTEX_FN constexpr uint64_t swap16x4(uint64_t t) { return ((t & 0x00FF00FF00FF00FFull) << 8) | ((t >> 8) & 0x00FF00FF00FF00FFull); }

// texel k of four consecutive B-byte texels held as B little-endian dwords
template<uint32_t B>
DXTEX_FN uint32_t texel_of(const uint32_t (&w)[B], uint32_t k)
{
    const uint32_t bit = k * 8u * B, i = bit / 32u, shift = bit % 32u;
    uint32_t t = w[i] >> shift;
    if (shift + 8u * B > 32u) t |= w[i + 1] << (32u - shift);
    return B == 4u ? t : t & ((1u << (8u * (B & 3u))) - 1u);
}

// the reverse for B = 3: four texels, each in the low three bytes of its word with the fourth zero, as three dwords
DXTEX_FN void pack3x4(const uint32_t (&t)[4], uint32_t (&out)[3])
{
    out[0] = t[0] | (t[1] << 24); out[1] = (t[1] >> 8) | (t[2] << 16); out[2] = (t[2] >> 16) | (t[3] << 8);
}

// what every route rule asks: an address and a pitch (0 for a tight stream) that are both multiples of `bytes`, a power of two
DXTEX_FN bool multiple_of(const void* p, uint64_t pitch, uint32_t bytes) { return ((reinterpret_cast<uintptr_t>(p) | pitch) & (bytes - 1u)) == 0; }

// The stream kernels' grid: 256 lanes of `group` texels across a row, and rows strided over about 8192 workgroups in all - enough to
// fill 256 CUs several times over, few enough that a lane streams several rows
DXTEX_FN constexpr uint32_t stream_grid_x(uint32_t width, uint32_t group) { return ((width + group - 1u) / group + 255u) / 256u; }
DXTEX_FN constexpr uint32_t stream_grid_y(uint32_t gx, uint32_t height)
{
    const uint32_t rows = height < 65535u ? height : 65535u, share = 8192u / gx > 1u ? 8192u / gx : 1u;
    return rows < share ? rows : share;
}
} // namespace dxtex

#if defined(__HIPCC__) || defined(__HIP__)
#include <type_traits>

namespace dxtex
{
// the widest access N consecutive dwords can be moved with: a multiple of four as dwordx4, of two as dwordx2, else single dwords
template<uint32_t N> constexpr uint32_t span_align() { return N % 4u == 0 ? 16u : N % 2u == 0 ? 8u : 4u; }

// N dwords at s as accesses of ALIGN bytes; s is a multiple of ALIGN. A caller whose route rule promises less than span_align<N>()
// (tga.hip and dds.hip ask 4 of a stream of fewer than four dwords) says so and gets single dwords.
template<uint32_t N, uint32_t ALIGN = span_align<N>()>
__device__ __forceinline__ void load_span(const uint8_t* s, uint32_t (&w)[N])
{
    static_assert(ALIGN == 4u || (ALIGN == 8u && N % 2u == 0) || (ALIGN == 16u && N % 4u == 0), "whole accesses");
    if constexpr (ALIGN == 16u)
    {
#pragma unroll
        for (uint32_t i = 0; i < N / 4u; ++i) { const uint4 v = reinterpret_cast<const uint4*>(s)[i]; w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
    }
    else if constexpr (ALIGN == 8u)
    {
#pragma unroll
        for (uint32_t i = 0; i < N / 2u; ++i) { const uint2 v = reinterpret_cast<const uint2*>(s)[i]; w[2 * i] = v.x; w[2 * i + 1] = v.y; }
    }
    else
    {
#pragma unroll
        for (uint32_t i = 0; i < N; ++i) w[i] = reinterpret_cast<const uint32_t*>(s)[i];
    }
}

template<uint32_t N, uint32_t ALIGN = span_align<N>()>
__device__ __forceinline__ void store_span(uint8_t* d, const uint32_t (&w)[N])
{
    static_assert(ALIGN == 4u || (ALIGN == 8u && N % 2u == 0) || (ALIGN == 16u && N % 4u == 0), "whole accesses");
    if constexpr (ALIGN == 16u)
    {
#pragma unroll
        for (uint32_t i = 0; i < N / 4u; ++i) reinterpret_cast<uint4*>(d)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
    }
    else if constexpr (ALIGN == 8u)
    {
#pragma unroll
        for (uint32_t i = 0; i < N / 2u; ++i) reinterpret_cast<uint2*>(d)[i] = make_uint2(w[2 * i], w[2 * i + 1]);
    }
    else
    {
#pragma unroll
        for (uint32_t i = 0; i < N; ++i) reinterpret_cast<uint32_t*>(d)[i] = w[i];
    }
}

// one E-byte element (1, 2, 3 or 4 bytes; stores 8 as well): one access where the address is a multiple of E, bytes otherwise
template<uint32_t E>
__device__ __forceinline__ uint32_t load1(const uint8_t* s, bool aligned)
{
    if (E == 1u || E == 3u || !aligned) return le_load32(s, E);
    if constexpr (E == 2u) return *reinterpret_cast<const uint16_t*>(s);
    else return *reinterpret_cast<const uint32_t*>(s);
}

template<uint32_t E>
__device__ __forceinline__ void store1(uint8_t* d, uint64_t t, bool aligned)
{
    if (E == 1u || E == 3u || !aligned) { if constexpr (E <= 4u) le_store32(d, uint32_t(t), E); else le_store64(d, t, E); return; }
    if constexpr (E == 2u) *reinterpret_cast<uint16_t*>(d) = uint16_t(t);
    else if constexpr (E == 4u) *reinterpret_cast<uint32_t*>(d) = uint32_t(t);
    else *reinterpret_cast<uint2*>(d) = make_uint2(uint32_t(t), uint32_t(t >> 32));
}

// A 256-word palette by value in the kernel's arguments (1 KiB, no copy, no host synchronisation), or nothing for an instantiation
// that reads none. Each workgroup of 256 lanes holds it in LDS: palette_to_lds() on a path the whole workgroup takes.
struct Palette { uint32_t word[256]; };
struct NoPalette {};
template<bool HAS> using PaletteArg = std::conditional_t<HAS, Palette, NoPalette>;

__device__ __forceinline__ void palette_to_lds(uint32_t (&lds)[256], const Palette& pal)
{
    lds[threadIdx.x] = pal.word[threadIdx.x];
    __syncthreads();
}

inline dim3 stream_grid(uint32_t width, uint32_t height, uint32_t group, uint32_t images = 1u)
{
    const uint32_t gx = stream_grid_x(width, group);
    return dim3(gx, stream_grid_y(gx, height), images);
}
} // namespace dxtex

// `marks` is the launcher's KernelMarks*, null outside a profile
#define DXTEX_MARK(NAME) do { if (marks) marks->mark(NAME); } while (0)
#endif
