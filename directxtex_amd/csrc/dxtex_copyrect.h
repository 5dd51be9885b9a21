// CopyRectangle (DirectXTexMisc.cpp:275-381) and texassemble's merge (Texassemble/texassemble.cpp:2236-2268): what the host resolves
// per job and what the kernels in scanline.hip receive. Plain data and integer arithmetic only, __host__ __device__.
//
//   same format (:321-338)       a byte mover: h rows of w * texelBytes bytes, memcpy's bytes. A texel counts BitsPerPixel / 8 bytes as
//                                the reference computes it (:303-317), which for the packed two-texel formats is the size of an ELEMENT
//                                (4 bytes for R8G8_B8G8 / G8R8_G8B8 / YUY2, 8 for Y210 / Y216): the reference's memcpy then runs past the
//                                row into the next one, and so does this one, byte for byte (the end-of-image check is the reference's)
//   different formats (:340-380) LoadScanline -> ConvertScanline(filter) -> StoreScanline: load_texel, apply_plan and store_texel with
//                                StoreScanline's default threshold, as convert_kernel runs them, with the two texel offsets added
//
// The mover's access width is the largest of 16 / 8 / 4 / 2 / 1 bytes that divides both first-row addresses and (with more than one row)
// both pitches; what is left of a row after whole accesses - a 12-byte texel under 16-byte accesses, an odd byte count - moves byte by byte.
#pragma once
#include "dxtex_store.h"
#include "dxtex_formats.h"

namespace dxtex
{
// One rectangle. Mover (vec != 0): src / dst point at the first byte of the first row, `width` = whole accesses of `vec` bytes per row,
// `tail` = bytes after them. Converting (vec == 0): src / dst point at the first row, `width` texels from texel sx / to texel dx.
struct CopyJob
{
    const uint8_t* src;
    uint8_t* dst;
    uint64_t srcPitch, dstPitch;
    uint32_t width, height;
    uint32_t sx, dx;
    int srcFormat, dstFormat;
    ConvertPlan plan;
    uint32_t vec, tail;
};

// Jobs travel in the kernel's argument block (4 KiB on this runtime): no table to upload, and a batch is ONE launch. More jobs than this
// are cut into several launches by launch_copy_rects.
constexpr uint32_t kCopyBatchMax = 32;
struct CopyBatch
{
    CopyJob job[kCopyBatchMax];
    uint32_t count;
};
static_assert(sizeof(CopyBatch) <= 3072, "the batch must fit the kernel argument block next to nothing else");

// bytes of a "texel" as CopyRectangle counts them: (BitsPerPixel(format) + 7) / 8 with the reference's BitsPerPixel
__host__ __device__ inline uint32_t copy_texel_bytes(const FmtInfo& f)
{
    return (f.cls & FC_PACKED) ? group_bytes(f.format) : (f.bpp + 7u) / 8u;
}

// the widest access (16, 8, 4, 2, 1) that every row start of both sides is aligned to
__host__ __device__ inline uint32_t copy_access_bytes(uint64_t srcAddr, uint64_t dstAddr, uint64_t srcPitch, uint64_t dstPitch, uint32_t rows)
{
    uint64_t bits = srcAddr | dstAddr;
    if (rows > 1) bits |= srcPitch | dstPitch;
    uint32_t v = 16;
    while (v > 1 && (bits & (v - 1u))) v >>= 1;
    return v;
}

// texassemble's merge: out[k] = (sel[k] < 4 ? a : b)[sel[k] & 3], then 0 where bit k of zero, then 1 where bit k of one
// (XMVectorPermute + two XMVectorSelect: channels are moved, never computed, so NaN payloads and -0 survive)
struct MergeArgs
{
    uint32_t sel[4];
    uint32_t zero, one;
};

__host__ __device__ inline void merge_texel(const float (&a)[4], const float (&b)[4], const MergeArgs& m, float (&out)[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        const uint32_t s = m.sel[k], c = s & 3u;
        const float va = c == 0 ? a[0] : c == 1 ? a[1] : c == 2 ? a[2] : a[3];
        const float vb = c == 0 ? b[0] : c == 1 ? b[1] : c == 2 ? b[2] : b[3];
        float v = s < 4u ? va : vb;
        if (m.zero & (1u << k)) v = 0.0f;
        if (m.one & (1u << k)) v = 1.0f;
        out[k] = v;
    }
}
} // namespace dxtex
