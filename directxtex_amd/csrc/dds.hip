// DDS texels on gfx950 (dxtex_dds.h holds the per-texel rules): what the .dds codec does per texel behind its byte-serial header, so that
// a file's payload crosses PCIe as the bytes it has on disk and a 24-bit file leaves at 3 bytes a texel.
//   dds_unpack_kernel<OP, TARGET, WIDE>  the payload, on the device as it is in the file -> the images of a resident texture, each through
//                                        its own pitch. OP = a DdsRowOp, TARGET = what the result format makes of it (dds_target).
//   dds_pack24_kernel<WIDE>              B8G8R8X8 images -> the writer's 24-bit rows (DDS_FLAGS_FORCE_24BPP_RGB) at the file's pitches
//
// One launch takes a BATCH of images (array items, mip levels, depth slices): up to kDdsBatchMax = 32 DdsImage descriptors by value in the
// kernel's arguments (1280 bytes; with the 1 KiB palette still well inside the 4 KiB of a launch), blockIdx.z picks the image. 256 lanes, x
// across, rows strided over gridDim.y; the grid is sized for the largest image of the batch and a lane outside its own image leaves at
// once. A texture with more images takes several launches on the stream, nothing between them.
//
// Two routes, chosen PER IMAGE by the launcher, which sorts a texture's images into wide launches and narrow launches (the images are
// disjoint, so their order is free) - the top levels of a 24-bit chain stay wide when its tail falls off alignment:
//   wide    a lane takes four texels and every access is a naturally aligned dword or wider: 4 * B file bytes as B dwords (B = 1, 2, 3; one
//           dwordx4 for B = 4), 4 * D image bytes as one dwordx2 (D = 2), one dwordx4 (D = 4) or two dwordx4 (D = 8, ROW_L16). ROW_COPY,
//           which works in bytes, takes 16 of them per lane: dwordx4 in and out, whatever the texel.
//           THE RULE: texels per row are a multiple of 4; the file side's address (payload + offset) and row pitch are multiples of 4
//           (of 16 for B = 4); the image's base and row pitch are multiples of min(4 * D, 16). ROW_COPY: row bytes, both addresses and
//           both pitches are multiples of 16 (a copy whose rows lie back to back on both sides counts as one long row). wide_ok() is
//           the one place that decides it.
//   narrow  everything else: a lane takes one texel, a single access where the address is a multiple of the texel's size and bytes where it
//           is not. ROW_COPY: one texel of the forced-alpha rule; a plain copy moves one aligned dword a lane where both addresses, both
//           pitches and the row's bytes are multiples of 4 (copy_words_ok(), decided per image), else one byte.
// The palette of ROW_P8 / ROW_A8P8 arrives by value in the kernel's arguments and each workgroup holds it in LDS. No atomics.
//
// Every read lies inside its image's rows x file pitch span (the launcher has checked each span against payloadBytes before anything is
// queued) and every write inside its row's `width` texels: a lane works only where x < width (wide: x + 3 < width as width is a multiple of
// 4) and y < rows. Pitch padding of an image is never written.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_dds.h"
#include <algorithm>
#include <cstdio>

namespace dxtex
{
namespace
{
struct DdsBatch { DdsImage image[kDdsBatchMax]; };

// four D-byte image texels as aligned accesses
template<uint32_t D>
__device__ __forceinline__ void store4(uint8_t* d, const uint64_t (&t)[4])
{
    if constexpr (D == 2u) *reinterpret_cast<uint2*>(d) = make_uint2(uint32_t(t[0]) | (uint32_t(t[1]) << 16), uint32_t(t[2]) | (uint32_t(t[3]) << 16));
    else if constexpr (D == 4u) *reinterpret_cast<uint4*>(d) = make_uint4(uint32_t(t[0]), uint32_t(t[1]), uint32_t(t[2]), uint32_t(t[3]));
    else
    {
        reinterpret_cast<uint4*>(d)[0] = make_uint4(uint32_t(t[0]), uint32_t(t[0] >> 32), uint32_t(t[1]), uint32_t(t[1] >> 32));
        reinterpret_cast<uint4*>(d)[1] = make_uint4(uint32_t(t[2]), uint32_t(t[2] >> 32), uint32_t(t[3]), uint32_t(t[3] >> 32));
    }
}

// a plain narrow copy moves aligned dwords where the whole image allows it: both addresses, both pitches and the row's bytes multiples of 4
__host__ __device__ __forceinline__ bool copy_words_ok(const uint8_t* src, const DdsImage& im)
{
    return ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(im.pixels) | im.filePitch | im.pitch | im.width) & 3u) == 0;
}

// `rule` is read by ROW_COPY only: its forced alpha (texelBytes 0: a plain copy). im.width counts bytes for ROW_COPY, texels otherwise.
template<int OP, int TARGET, bool WIDE>
__global__ void __launch_bounds__(256) dds_unpack_kernel(const uint8_t* payload, DdsBatch batch, uint32_t opaque, DdsOpaque rule, PaletteArg<dds_has_palette(OP)> pal)
{
    __shared__ uint32_t table[dds_has_palette(OP) ? 256 : 1];
    if constexpr (dds_has_palette(OP)) palette_to_lds(table, pal);
    const DdsImage& im = batch.image[blockIdx.z];
    const uint8_t* src = payload + im.fileOffset;
    const uint32_t lane = blockIdx.x * 256u + threadIdx.x;
    if constexpr (OP == ROW_COPY)
    {
        if constexpr (WIDE)
        {
            const uint32_t x = lane * 16u;
            if (x >= im.width) return;
            const DdsOpaque16 o = dds_opaque16_of(rule);
            for (uint32_t y = blockIdx.y; y < im.rows; y += gridDim.y)
            {
                uint4 v = *reinterpret_cast<const uint4*>(src + uint64_t(y) * im.filePitch + x);
                if (o.which & 1u) v.x = (v.x & o.keep) | o.set;
                if (o.which & 2u) v.y = (v.y & o.keep) | o.set;
                if (o.which & 4u) v.z = (v.z & o.keep) | o.set;
                if (o.which & 8u) v.w = (v.w & o.keep) | o.set;
                *reinterpret_cast<uint4*>(im.pixels + uint64_t(y) * im.pitch + x) = v;
            }
        }
        else
        {
            // one texel of the rule (whole texels only, as CopyScanline); a plain copy: one aligned dword where copy_words_ok(), else one byte
            const bool words = !rule.texelBytes && copy_words_ok(src, im);
            const uint32_t T = rule.texelBytes ? rule.texelBytes : words ? 4u : 1u, W = T < 4u ? T : 4u;
            const uint64_t x = uint64_t(lane) * T;
            if (x + T > im.width) return;
            for (uint32_t y = blockIdx.y; y < im.rows; y += gridDim.y)
            {
                const uint8_t* s = src + uint64_t(y) * im.filePitch + x;
                uint8_t* d = im.pixels + uint64_t(y) * im.pitch + x;
                if (words) { *reinterpret_cast<uint32_t*>(d) = *reinterpret_cast<const uint32_t*>(s); continue; }
                for (uint32_t i = 0; i + W < T; ++i) d[i] = s[i];
                const uint32_t v = le_load32(s + (T - W), W);
                le_store64(d + (T - W), rule.texelBytes ? dds_opaque_word(v, rule) : v, W);
            }
        }
    }
    else
    {
        constexpr uint32_t B = dds_file_bytes(OP), D = dds_image_bytes(TARGET), G = WIDE ? 4u : 1u;
        const uint32_t x = lane * G;
        if (x >= im.width) return;
        const bool srcAligned = multiple_of(src, im.filePitch, B == 3u ? 1u : B), dstAligned = multiple_of(im.pixels, im.pitch, D);
        for (uint32_t y = blockIdx.y; y < im.rows; y += gridDim.y)
        {
            const uint8_t* s = src + uint64_t(y) * im.filePitch + uint64_t(x) * B;
            uint8_t* d = im.pixels + uint64_t(y) * im.pitch + uint64_t(x) * D;
            if constexpr (WIDE)
            {
                uint32_t w[B];
                uint64_t t[4];
                load_span<B, B == 4u ? 16u : 4u>(s, w);
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) t[k] = dds_unpack_texel(texel_of<B>(w, k), OP, TARGET, opaque != 0, table);
                store4<D>(d, t);
            }
            else store1<D>(d, dds_unpack_texel(load1<B>(s, srcAligned), OP, TARGET, opaque != 0, table), dstAligned);
        }
    }
}

// batch.image: fileOffset / filePitch = where the 24-bit rows go in `out`, pixels / pitch = the B8G8R8X8 image that is read
template<bool WIDE>
__global__ void __launch_bounds__(256) dds_pack24_kernel(uint8_t* out, DdsBatch batch)
{
    const DdsImage& im = batch.image[blockIdx.z];
    const uint32_t x = (blockIdx.x * 256u + threadIdx.x) * (WIDE ? 4u : 1u);
    if (x >= im.width) return;
    uint8_t* dst = out + im.fileOffset;
    const bool srcAligned = multiple_of(im.pixels, im.pitch, 4u);
    for (uint32_t y = blockIdx.y; y < im.rows; y += gridDim.y)
    {
        const uint8_t* s = im.pixels + uint64_t(y) * im.pitch + uint64_t(x) * 4u;
        uint8_t* d = dst + uint64_t(y) * im.filePitch + uint64_t(x) * 3u;
        if constexpr (WIDE)
        {
            uint32_t t[4], o[3];
            load_span<4u>(s, t);
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) t[k] = dds_pack24_texel(t[k]);
            pack3x4(t, o);
            store_span<3u>(d, o);
        }
        else le_store64(d, dds_pack24_texel(load1<4u>(s, srcAligned)), 3u);
    }
}

// THE RULE of the wide route (see the top of the file)
template<int OP, int TARGET>
bool wide_ok(const uint8_t* payload, const DdsImage& im)
{
    if constexpr (OP == ROW_COPY) return im.width % 16u == 0 && multiple_of(payload + im.fileOffset, im.filePitch, 16u) && multiple_of(im.pixels, im.pitch, 16u);
    else
    {
        constexpr uint32_t B = dds_file_bytes(OP), D = dds_image_bytes(TARGET);
        return im.width % 4u == 0 && multiple_of(payload + im.fileOffset, im.filePitch, B == 4u ? 16u : 4u) && multiple_of(im.pixels, im.pitch, std::min(4u * D, 16u));
    }
}
inline bool pack24_wide_ok(const uint8_t* out, const DdsImage& im)
{
    return im.width % 4u == 0 && multiple_of(out + im.fileOffset, im.filePitch, 4u) && multiple_of(im.pixels, im.pitch, 16u);
}

// One batch: the grid for its largest image, over lanes of `unit` texels (bytes for ROW_COPY)
struct Pending
{
    DdsBatch batch;
    uint32_t count = 0, lanes = 0, rows = 0;
    void add(const DdsImage& im, uint32_t unit)
    {
        batch.image[count++] = im;
        lanes = std::max(lanes, uint32_t((uint64_t(im.width) + unit - 1u) / unit));
        rows = std::max(rows, im.rows);
    }
    dim3 grid() const { return stream_grid(lanes, rows, 1u, count); }
    void clear() { for (uint32_t k = 0; k < count; ++k) batch.image[k] = DdsImage{}; count = lanes = rows = 0; }
};

const char* const kOpName[ROW_OPS] = { "copy", "swizzle", "565", "5551", "4444", "abgr4", "888", "332", "8332", "p8", "a8p8", "44", "l8", "l16", "a8l8", "l6v5u5", "l8u8v8", "wuv10" };
// "dds_unpack<888,wide>": static storage, as KernelMarks keeps the pointer
struct MarkNames
{
    char name[ROW_OPS][2][40];
    MarkNames() { for (int op = 0; op < ROW_OPS; ++op) for (int w = 0; w < 2; ++w) std::snprintf(name[op][w], sizeof(name[op][w]), "dds_unpack<%s,%s>", kOpName[op], w ? "wide" : "narrow"); }
};
const MarkNames kMarkNames;
const char* mark_name(int op, bool wide) { return kMarkNames.name[op][wide ? 1 : 0]; }

// The batch, flush and route loop of both launchers: sorts a texture's images into wide and narrow batches, queues each batch as it fills
// and the two rests at the end, wide first. route(im, unit) decides one image's route and the texels (bytes) a lane takes of it, and may
// reshape the image; launch(batch, isWide) marks and queues one kernel.
template<class Route, class Launch>
hipError_t launch_batches(const DdsImage* images, size_t count, KernelMarks* marks, Route&& route, Launch&& launch)
{
    Pending wide, narrow;
    const auto flush = [&](Pending& p, bool isWide) -> hipError_t
    {
        if (!p.count) return hipSuccess;
        launch(p, isWide);
        p.clear();
        return hipGetLastError();
    };
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < count && e == hipSuccess; ++i)
    {
        DdsImage im = images[i];
        if (!im.width || !im.rows) continue;
        uint32_t unit;
        const bool isWide = route(im, unit);
        Pending& p = isWide ? wide : narrow;
        p.add(im, unit);
        if (p.count == uint32_t(kDdsBatchMax)) e = flush(p, isWide);
    }
    if (e == hipSuccess) e = flush(wide, true);
    if (e == hipSuccess) e = flush(narrow, false);
    DXTEX_MARK(nullptr);
    return e;
}

template<int OP, int TARGET>
hipError_t unpack_op(const uint8_t* payload, bool opaque, const DdsOpaque& rule, const uint32_t* palette, const DdsImage* images, size_t count, hipStream_t hs, KernelMarks* marks)
{
    PaletteArg<dds_has_palette(OP)> pal;
    if constexpr (dds_has_palette(OP)) std::copy(palette, palette + 256, pal.word);
    const uint32_t narrowUnit = OP == ROW_COPY ? std::max(1u, rule.texelBytes) : 1u, wideUnit = OP == ROW_COPY ? 16u : 4u;
    return launch_batches(images, count, marks,
        [&](DdsImage& im, uint32_t& unit)
        {
            // a copy whose rows lie back to back on both sides is one long row
            if (OP == ROW_COPY && im.filePitch == im.width && im.pitch == im.width && uint64_t(im.width) * im.rows <= 0xFFFFFFF0ull) { im.width *= im.rows; im.rows = 1; }
            const bool isWide = wide_ok<OP, TARGET>(payload, im);
            unit = isWide ? wideUnit : (OP == ROW_COPY && !rule.texelBytes && copy_words_ok(payload + im.fileOffset, im)) ? 4u : narrowUnit;
            return isWide;
        },
        [&](const Pending& p, bool isWide)
        {
            DXTEX_MARK(mark_name(OP, isWide));
            if (isWide) hipLaunchKernelGGL((dds_unpack_kernel<OP, TARGET, true>), p.grid(), dim3(256), 0, hs, payload, p.batch, opaque ? 1u : 0u, rule, pal);
            else hipLaunchKernelGGL((dds_unpack_kernel<OP, TARGET, false>), p.grid(), dim3(256), 0, hs, payload, p.batch, opaque ? 1u : 0u, rule, pal);
        });
}
} // namespace

hipError_t launch_dds_unpack(const uint8_t* payload, size_t payloadBytes, int op, int format, bool opaque, const uint32_t* palette, const DdsImage* images, size_t count,
                             hipStream_t hs, KernelMarks* marks)
{
    const int target = dds_target(op, format);
    if (target < 0 || (op == ROW_SWIZZLE && target == DDS_TO_BYTES) || (dds_has_palette(op) && !palette)) return hipErrorInvalidValue;
    const DdsOpaque rule = (op == ROW_COPY && opaque) ? dds_opaque_of(format) : DdsOpaque{ 0u, 0xffffffffu, 0u };
    const uint32_t B = op == ROW_COPY ? 1u : dds_file_bytes(op);
    for (size_t i = 0; i < count; ++i)
        if (!dds_image_in_payload(images[i], B, payloadBytes)) return hipErrorInvalidValue;          // before anything is queued
#define DXTEX_DDS_OP(OP, TARGET) if (op == OP && target == TARGET) return unpack_op<OP, TARGET>(payload, opaque, rule, palette, images, count, hs, marks)
    DXTEX_DDS_OP(ROW_COPY, DDS_TO_BYTES);
    DXTEX_DDS_OP(ROW_SWIZZLE, DDS_TO_8888); DXTEX_DDS_OP(ROW_SWIZZLE, DDS_TO_1010102); DXTEX_DDS_OP(ROW_SWIZZLE, DDS_TO_YUY2);
    DXTEX_DDS_OP(ROW_565, DDS_TO_8888); DXTEX_DDS_OP(ROW_5551, DDS_TO_8888); DXTEX_DDS_OP(ROW_4444, DDS_TO_8888); DXTEX_DDS_OP(ROW_ABGR4, DDS_TO_8888);
    DXTEX_DDS_OP(ROW_888, DDS_TO_8888); DXTEX_DDS_OP(ROW_332, DDS_TO_8888); DXTEX_DDS_OP(ROW_332, DDS_TO_565); DXTEX_DDS_OP(ROW_8332, DDS_TO_8888);
    DXTEX_DDS_OP(ROW_P8, DDS_TO_8888); DXTEX_DDS_OP(ROW_A8P8, DDS_TO_8888); DXTEX_DDS_OP(ROW_44, DDS_TO_8888); DXTEX_DDS_OP(ROW_44, DDS_TO_4444);
    DXTEX_DDS_OP(ROW_L8, DDS_TO_8888); DXTEX_DDS_OP(ROW_L16, DDS_TO_16161616); DXTEX_DDS_OP(ROW_A8L8, DDS_TO_8888); DXTEX_DDS_OP(ROW_L6V5U5, DDS_TO_8888);
    DXTEX_DDS_OP(ROW_L8U8V8, DDS_TO_8888); DXTEX_DDS_OP(ROW_WUV10, DDS_TO_1010102);
#undef DXTEX_DDS_OP
    return hipErrorInvalidValue;
}

hipError_t launch_dds_pack24(const DdsImage* images, size_t count, uint8_t* out, size_t outBytes, hipStream_t hs, KernelMarks* marks)
{
    for (size_t i = 0; i < count; ++i)
        if (!dds_image_in_payload(images[i], 3u, outBytes)) return hipErrorInvalidValue;
    return launch_batches(images, count, marks,
        [&](DdsImage& im, uint32_t& unit)
        {
            const bool isWide = pack24_wide_ok(out, im);
            unit = isWide ? 4u : 1u;
            return isWide;
        },
        [&](const Pending& p, bool isWide)
        {
            DXTEX_MARK(isWide ? "dds_pack24<wide>" : "dds_pack24<narrow>");
            if (isWide) hipLaunchKernelGGL((dds_pack24_kernel<true>), p.grid(), dim3(256), 0, hs, out, p.batch);
            else hipLaunchKernelGGL((dds_pack24_kernel<false>), p.grid(), dim3(256), 0, hs, out, p.batch);
        });
}
} // namespace dxtex
