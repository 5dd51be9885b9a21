// ConvertToSinglePlane (DirectXTexConvert.cpp:4912-5077, :5411-5523): the planar video formats interleaved into their single-plane 4:2:2
// forms. What the host resolves per image, what single_plane_kernel (single_plane.hip) receives, and what ONE lane of it produces: the
// kernel and the host check (tests/cpp/plane_check.cpp) both call plane_lane(). Plain data and integer arithmetic only, __host__ __device__.
//
//   PlanarToSingle (:4912-4939)  NV12 (103), NV11 (110) -> YUY2 (107); P010 (104) -> Y210 (108); P016 (105) -> Y216 (109); nothing else
//   4:2:0 (NV12, P010, P016)     element k of destination rows 2c and 2c + 1 is (Y[row][2k], U, Y[row][2k + 1], V) with U, V the samples 2k and
//                                2k + 1 of chroma row c; the chroma plane starts at byte height * rowPitch, its rows are rowPitch apart
//   4:1:1 (NV11)                 chroma pair j of row y, at byte height * rowPitch + y * (rowPitch >> 1) + 2j, feeds elements 2j and 2j + 1
//                                of row y, whose luma is samples 4j .. 4j + 3 of luma row y
//   the end guard (:4962, :5048) `if ((sPtrUV + 1) >= sourceE) break;` with sourceE = pixels + slicePitch: a chroma pair whose second sample
//                                lies at or beyond slicePitch is not read, and neither it nor any later pair of that chroma row is written.
//                                With ComputePitch's slicePitch it never fires; with a smaller one the tail of the last rows stays as it was.
//
// plane_check() returns the reference's HRESULTs in its order (:5413-5424, :5005-5030): E_INVALIDARG for a source format that is not planar,
// E_POINTER for null pixels, NOT_SUPPORTED for a planar format PlanarToSingle does not map, E_INVALIDARG for an odd width or height
// (4:2:0) or a width that is no multiple of four (NV11). ADDED HERE, where the reference would read outside the image it was handed or has no
// destination of the caller's to get wrong: E_INVALIDARG for a source rowPitch below the row's bytes, for slicePitch < height * rowPitch, for
// an odd pointer or pitch with 16-bit samples, for a destination whose format is not PlanarToSingle(source), for a destination rowPitch
// below its row's bytes, and for read and written bytes that overlap; E_FAIL for a destination of another size.
//
// Routes, chosen per job by the host from the real addresses and pitches (as copy_access_bytes does for CopyRectangle's mover):
//   wide     a lane owns 16 destination bytes of a row - of both rows of the pair for 4:2:0, so the chroma is read once: 8 luma bytes per
//            row, 8 chroma bytes (4 for NV11), one 16-byte store per row. Taken when every row start of luma, chroma and destination is
//            aligned for those accesses.
//   element  a lane owns one destination element (4 or 8 bytes), moved sample by sample. The whole row without the alignment; otherwise the
//            elements after the whole 16-byte groups, and the elements of a group that the end guard cuts.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dxtex
{
constexpr int32_t kPlaneOk = 0, kPlaneInvalidArg = int32_t(0x80070057u), kPlanePointer = int32_t(0x80004003u), kPlaneNotSupported = int32_t(0x80070032u),
                  kPlaneFail = int32_t(0x80004005u);

// IsPlanar (DirectXTexUtil.cpp:396-429, the Direct3D 11 answer): NV12 P010 P016 420_OPAQUE NV11, the Xbox depth planes, P208 V208 V408
__host__ __device__ inline bool plane_is_planar(int f)
{
    return f == 103 || f == 104 || f == 105 || f == 106 || f == 110 || f == 118 || f == 119 || f == 120 || f == 130 || f == 131 || f == 132;
}

// PlanarToSingle (:4916-4939); 0 (DXGI_FORMAT_UNKNOWN) where there is no single-plane form
__host__ __device__ inline int plane_to_single(int f)
{
    return (f == 103 || f == 110) ? 107 : f == 104 ? 108 : f == 105 ? 109 : 0;
}

// An image as the C ABI hands it over (dxtex_image), the pixels as an address
struct PlaneImage
{
    uint64_t width, height;
    int format;
    uint64_t rowPitch, slicePitch;
    uint64_t pixels;
};

// One image. `elems` destination elements (two texels each) per row; `units` row pairs (4:2:0) or rows (NV11), one chroma row each.
struct PlaneJob
{
    const uint8_t* src;
    uint8_t* dst;
    uint64_t srcPitch, dstPitch;
    uint64_t chromaAt, chromaPitch;     // first byte of the chroma plane from src, and the distance of its rows
    uint64_t chromaBytes;               // slicePitch - chromaAt: what the end guard lets the chroma plane hold
    uint32_t elems, units;
    uint32_t sample;                    // bytes of a sample: 1 or 2
    uint32_t nv11;                      // 1: 4:1:1 (a unit is one row, a chroma pair feeds two elements), 0: 4:2:0
    uint32_t groups;                    // whole 16-byte destination groups per row on the wide route, 0 on the element route
    uint32_t pad;
};

// Jobs travel in the kernel's argument block like CopyBatch: a batch is ONE launch, more jobs are cut into several launches.
constexpr uint32_t kPlaneBatchMax = 32;
struct PlaneBatch
{
    PlaneJob job[kPlaneBatchMax];
    uint32_t count;
};
static_assert(sizeof(PlaneBatch) <= 3072, "the batch must fit the kernel argument block next to nothing else");

constexpr uint32_t kPlaneThreads = 256;

struct alignas(8) PlaneU2 { uint32_t x, y; };
struct alignas(16) PlaneU4 { uint32_t x, y, z, w; };

__host__ __device__ inline uint32_t plane_elem_bytes(const PlaneJob& j) { return 4u * j.sample; }
__host__ __device__ inline uint32_t plane_group_elems(const PlaneJob& j) { return 4u / j.sample; }                 // elements of 16 destination bytes
__host__ __device__ inline uint32_t plane_group_pairs(const PlaneJob& j) { return j.nv11 ? 2u : 4u / j.sample; }   // chroma pairs they read
// lanes of a row: the wide groups, then one per element after them
__host__ __device__ inline uint32_t plane_lanes(const PlaneJob& j) { return j.groups + (j.elems - j.groups * plane_group_elems(j)); }

// The end guard: the index of the first chroma pair of chroma row `unit` that is NOT read (the row's pair count where the guard does not fire).
// Pair k is read when its second sample ends at or before slicePitch.
__host__ __device__ inline uint32_t plane_pairs(const PlaneJob& j, uint32_t unit)
{
    const uint32_t all = j.nv11 ? j.elems / 2u : j.elems;
    const uint64_t at = uint64_t(unit) * j.chromaPitch;
    const uint64_t fit = at < j.chromaBytes ? (j.chromaBytes - at) / (2u * j.sample) : 0u;
    return fit < all ? uint32_t(fit) : all;
}

// destination elements of `unit`'s rows that are written
__host__ __device__ inline uint32_t plane_written_elems(const PlaneJob& j, uint32_t unit) { return j.nv11 ? 2u * plane_pairs(j, unit) : plane_pairs(j, unit); }

// (l0, c0, l1, c1) from the low two bytes of l and of c
__host__ __device__ inline uint32_t plane_pack8(uint32_t l, uint32_t c)
{
    return (l & 0xFFu) | ((c & 0xFFu) << 8) | ((l & 0xFF00u) << 8) | ((c & 0xFF00u) << 16);
}

template<typename T>
__host__ __device__ inline void plane_element_row(const uint8_t* luma, const uint8_t* uv, uint8_t* out)
{
    const T* l = reinterpret_cast<const T*>(luma);
    const T* c = reinterpret_cast<const T*>(uv);
    T* d = reinterpret_cast<T*>(out);
    d[0] = l[0]; d[1] = c[0]; d[2] = l[1]; d[3] = c[1];
}

// element e of the unit's rows, where the guard lets its chroma pair be read
__host__ __device__ inline void plane_element(const PlaneJob& j, uint32_t e, uint32_t unit, uint32_t pairs)
{
    const uint32_t pair = j.nv11 ? e / 2u : e;
    if (pair >= pairs) return;
    const uint8_t* uv = j.src + j.chromaAt + uint64_t(unit) * j.chromaPitch + uint64_t(pair) * 2u * j.sample;
    const uint64_t lumaAt = uint64_t(e) * 2u * j.sample, outAt = uint64_t(e) * 4u * j.sample;
    const uint32_t rows = j.nv11 ? 1u : 2u;
    for (uint32_t r = 0; r < rows; ++r)
    {
        const uint64_t y = uint64_t(unit) * rows + r;
        if (j.sample == 1u) plane_element_row<uint8_t>(j.src + y * j.srcPitch + lumaAt, uv, j.dst + y * j.dstPitch + outAt);
        else plane_element_row<uint16_t>(j.src + y * j.srcPitch + lumaAt, uv, j.dst + y * j.dstPitch + outAt);
    }
}

// What lane gx of a row's lanes produces for `unit` (a row pair of 4:2:0, a row of NV11).
__host__ __device__ inline void plane_lane(const PlaneJob& j, uint32_t gx, uint32_t unit)
{
    const uint32_t pairs = plane_pairs(j, unit);
    const uint32_t ge = plane_group_elems(j);
    if (gx >= j.groups)
    {
        const uint32_t e = j.groups * ge + (gx - j.groups);
        if (e < j.elems) plane_element(j, e, unit, pairs);
        return;
    }
    if ((uint64_t(gx) + 1u) * plane_group_pairs(j) > pairs)
    {
        // a group the end guard cuts: its elements one by one
        for (uint32_t k = 0; k < ge; ++k) plane_element(j, gx * ge + k, unit, pairs);
        return;
    }
    const uint8_t* uv = j.src + j.chromaAt + uint64_t(unit) * j.chromaPitch;
    if (j.nv11)
    {
        const PlaneU2 l = *reinterpret_cast<const PlaneU2*>(j.src + uint64_t(unit) * j.srcPitch + uint64_t(gx) * 8u);
        const uint32_t c = *reinterpret_cast<const uint32_t*>(uv + uint64_t(gx) * 4u);
        *reinterpret_cast<PlaneU4*>(j.dst + uint64_t(unit) * j.dstPitch + uint64_t(gx) * 16u) =
            PlaneU4{ plane_pack8(l.x, c), plane_pack8(l.x >> 16, c), plane_pack8(l.y, c >> 16), plane_pack8(l.y >> 16, c >> 16) };
        return;
    }
    const uint64_t y0 = uint64_t(unit) * 2u;
    const PlaneU2 l0 = *reinterpret_cast<const PlaneU2*>(j.src + y0 * j.srcPitch + uint64_t(gx) * 8u);
    const PlaneU2 l1 = *reinterpret_cast<const PlaneU2*>(j.src + (y0 + 1u) * j.srcPitch + uint64_t(gx) * 8u);
    const PlaneU2 c = *reinterpret_cast<const PlaneU2*>(uv + uint64_t(gx) * 8u);
    PlaneU4 d0, d1;
    if (j.sample == 1u)
    {
        d0 = PlaneU4{ plane_pack8(l0.x, c.x), plane_pack8(l0.x >> 16, c.x >> 16), plane_pack8(l0.y, c.y), plane_pack8(l0.y >> 16, c.y >> 16) };
        d1 = PlaneU4{ plane_pack8(l1.x, c.x), plane_pack8(l1.x >> 16, c.x >> 16), plane_pack8(l1.y, c.y), plane_pack8(l1.y >> 16, c.y >> 16) };
    }
    else
    {
        const uint32_t u0 = c.x << 16, v0 = c.x & 0xFFFF0000u, u1 = c.y << 16, v1 = c.y & 0xFFFF0000u;
        d0 = PlaneU4{ (l0.x & 0xFFFFu) | u0, (l0.x >> 16) | v0, (l0.y & 0xFFFFu) | u1, (l0.y >> 16) | v1 };
        d1 = PlaneU4{ (l1.x & 0xFFFFu) | u0, (l1.x >> 16) | v0, (l1.y & 0xFFFFu) | u1, (l1.y >> 16) | v1 };
    }
    *reinterpret_cast<PlaneU4*>(j.dst + y0 * j.dstPitch + uint64_t(gx) * 16u) = d0;
    *reinterpret_cast<PlaneU4*>(j.dst + (y0 + 1u) * j.dstPitch + uint64_t(gx) * 16u) = d1;
}

// The launch geometry of a batch: x over the lanes of the widest job, y over units (a lane strides over more), z over jobs.
__host__ __device__ inline void plane_grid(const PlaneBatch& b, uint32_t& gx, uint32_t& gy)
{
    uint32_t lanes = 0, units = 0;
    for (uint32_t k = 0; k < b.count; ++k)
    {
        const uint32_t l = plane_lanes(b.job[k]);
        lanes = l > lanes ? l : lanes;
        units = b.job[k].units > units ? b.job[k].units : units;
    }
    gx = (lanes + kPlaneThreads - 1u) / kPlaneThreads;
    // about 8192 workgroups over the batch, as copy_rect launches: a lane streams several units rather than one workgroup per row
    const uint32_t cap = gx && b.count ? 8192u / (gx * b.count) : 1u;
    gy = units < 65535u ? units : 65535u;
    if (gy > (cap ? cap : 1u)) gy = cap ? cap : 1u;
}

// The checks, in the order the header comment gives, and the resolved job. An image without texels resolves to a job without lanes.
__host__ __device__ inline int32_t plane_check(const PlaneImage& s, const PlaneImage& d, PlaneJob* out)
{
    if (!plane_is_planar(s.format)) return kPlaneInvalidArg;
    if (!s.pixels || !d.pixels) return kPlanePointer;
    const int single = plane_to_single(s.format);
    if (!single) return kPlaneNotSupported;
    if (s.width > 0xFFFFFFFFull || s.height > 0xFFFFFFFFull) return kPlaneInvalidArg;
    const bool nv11 = s.format == 110;
    if (nv11 ? (s.width % 4u) != 0 : ((s.width % 2u) != 0 || (s.height % 2u) != 0)) return kPlaneInvalidArg;
    // added here
    const uint64_t sample = s.format == 104 || s.format == 105 ? 2u : 1u;
    if (d.format != single) return kPlaneInvalidArg;
    if (d.width != s.width || d.height != s.height) return kPlaneFail;
    if (s.rowPitch < s.width * sample) return kPlaneInvalidArg;
    if (s.height && s.rowPitch > UINT64_MAX / s.height) return kPlaneInvalidArg;
    if (s.slicePitch < s.height * s.rowPitch) return kPlaneInvalidArg;
    if (sample == 2u && ((s.pixels | s.rowPitch | s.slicePitch | d.pixels | d.rowPitch) & 1u)) return kPlaneInvalidArg;
    const uint64_t dstRow = s.width * 2u * sample;
    if (d.rowPitch < dstRow) return kPlaneInvalidArg;
    if (s.height && d.rowPitch > UINT64_MAX / s.height) return kPlaneInvalidArg;
    const uint64_t written = s.height ? (s.height - 1u) * d.rowPitch + dstRow : 0u;
    if (s.pixels > UINT64_MAX - s.slicePitch || d.pixels > UINT64_MAX - written) return kPlaneInvalidArg;
    if (s.pixels < d.pixels + written && d.pixels < s.pixels + s.slicePitch) return kPlaneInvalidArg;

    PlaneJob j = {};
    j.src = reinterpret_cast<const uint8_t*>(uintptr_t(s.pixels));
    j.dst = reinterpret_cast<uint8_t*>(uintptr_t(d.pixels));
    j.srcPitch = s.rowPitch; j.dstPitch = d.rowPitch;
    j.chromaAt = s.height * s.rowPitch;
    j.chromaPitch = nv11 ? s.rowPitch >> 1 : s.rowPitch;
    j.chromaBytes = s.slicePitch - j.chromaAt;
    j.elems = uint32_t(s.width / 2u);
    j.units = uint32_t(nv11 ? s.height : s.height / 2u);
    j.sample = uint32_t(sample);
    j.nv11 = nv11 ? 1u : 0u;
    // the wide route: 8-byte luma and chroma reads (4-byte chroma reads at half the pitch for NV11), 16-byte stores
    const bool wide = ((s.pixels | s.rowPitch) & 7u) == 0 && (d.pixels & 15u) == 0 && (s.height < 2u || (d.rowPitch & 15u) == 0);
    j.groups = wide ? j.elems / plane_group_elems(j) : 0u;
    *out = j;
    return kPlaneOk;
}
} // namespace dxtex
