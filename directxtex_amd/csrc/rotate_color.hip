// texconv's HDR colour rotation (Texconv/texconv.cpp:2696-2964) on gfx950: LoadScanline -> one of the eight lambdas of dxtex_rotate.h
// -> StoreScanline (threshold 0) on r, g and b; alpha is moved.
//
// Pure streaming, no LDS. The curve (none, to ST.2084, from ST.2084) is a template argument; the matrix and the paper-white level are
// kernel arguments, so the eight operations share three bodies. Two routes:
//   quad   a format of DXTEX_QUAD_FORMATS (dxtex_quad.h) with 16-byte aligned rows and pitches on both sides: four texels per lane through
//          load_quad / store_quad, decoded and encoded on a register image of the quad as convert_quad_kernel does, ROWS quads of
//          consecutive rows in flight per lane before the first store. The lanes after the last quad of a row take the 1-3 texels of a
//          width that is no multiple of four, one each, through load_texel / store_texel.
//   texel  every other format load_texel / store_texel know (and a quad format with unaligned rows): a texel per lane, transform_kernel's
//          shape. The destination may be R32G32B32A32_FLOAT rows for launch_pack_group.
// Without a curve the kernel moves bytes and does 24 fp32 operations per texel: it is bound by memory. With a curve it evaluates six
// double-precision pow() per texel and is bound by the fp64 rate (DESIGN.md section 4 has the measured times), so those bodies keep one
// quad in flight: more would only add registers.
//
// Every read and write of a lane lies inside its row's `width` texels: q < width / 4 for a quad, x < width for a texel.
#include <hip/hip_runtime.h>
#include "dxtex_kernels.h"
#include "dxtex_store.h"
#include "dxtex_quad.h"
#include "dxtex_formats.h"
#include "dxtex_rotate.h"
#include <algorithm>

namespace dxtex
{
namespace
{
template<int CURVE>
__device__ __forceinline__ Texel rotate_texel(const Texel& t, const RotateArgs& a)
{
    float c[4] = { t.r, t.g, t.b, t.a };
    rc_apply<CURVE>(c, a);
    return Texel{ c[0], c[1], c[2], t.a };
}

constexpr int kRouteTexel = -1;

// one lane of the quad route. QB = bytes of a quad (16 or 32; 0 = taken from the argument: 48 and 64); src.format == dst.format is one of
// DXTEX_QUAD_FORMATS
template<int CURVE, int QB, int ROWS>
__device__ __forceinline__ void rotate_quad_lane(const ImgView& src, const ImgView& dst, const RotateArgs& a, uint32_t quadBytes)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    const uint32_t quads = src.width / 4u;
    if (q >= quads)
    {
        // the width's tail: one texel per lane
        const uint32_t x = quads * 4u + (q - quads);
        if (x >= src.width) return;
        for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
        {
            const Texel t = load_texel(src.pixels + uint64_t(y) * src.rowPitch, x, src.format);
            store_texel(dst.pixels + uint64_t(y) * dst.rowPitch, x, dst.format, rotate_texel<CURVE>(t, a));
        }
        return;
    }
    const uint32_t qb = QB ? uint32_t(QB) : quadBytes;
    constexpr int W = QB ? QB / 4 : 16;
    for (uint32_t y0 = blockIdx.y * uint32_t(ROWS); y0 < src.height; y0 += gridDim.y * uint32_t(ROWS))
    {
        uint32_t in[ROWS][W];
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
        {
#pragma unroll
            for (int k = 0; k < W; ++k) in[r][k] = 0u;
            const uint32_t y = min(y0 + uint32_t(r), src.height - 1u);       // a short last group re-reads the last row (and does not store it)
            load_quad<W>(in[r], src.pixels + uint64_t(y) * src.rowPitch + uint64_t(q) * qb, qb);
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
        {
            uint32_t out[W];
#pragma unroll
            for (int k = 0; k < W; ++k) out[k] = 0u;
            Texel tx[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) tx[k].r = tx[k].g = tx[k].b = tx[k].a = 0.0f;
            // the format as a compile-time constant per case, as in convert_quad_kernel: the register image stays in registers
            switch (src.format)
            {
#define DXTEX_QCASE(F, FQB) case F: if constexpr (QB == FQB || (QB == 0 && FQB > 32)) { _Pragma("unroll") for (uint32_t k = 0; k < 4u; ++k) tx[k] = load_texel(reinterpret_cast<const uint8_t*>(in[r]), k, F); } break;
                DXTEX_QUAD_FORMATS(DXTEX_QCASE)
#undef DXTEX_QCASE
            default: break;
            }
#pragma unroll
            for (uint32_t k = 0; k < 4u; ++k) tx[k] = rotate_texel<CURVE>(tx[k], a);
            switch (src.format)
            {
#define DXTEX_QCASE(F, FQB) case F: if constexpr (QB == FQB || (QB == 0 && FQB > 32)) { _Pragma("unroll") for (uint32_t k = 0; k < 4u; ++k) store_texel(reinterpret_cast<uint8_t*>(out), k, F, tx[k]); } break;
                DXTEX_QUAD_FORMATS(DXTEX_QCASE)
#undef DXTEX_QCASE
            default: break;
            }
            if (y0 + uint32_t(r) < src.height)
                store_quad<W>(dst.pixels + uint64_t(y0 + uint32_t(r)) * dst.rowPitch + uint64_t(q) * qb, out, qb);
        }
    }
}

// ROUTE = kRouteTexel, or rotate_quad_lane's QB
template<int CURVE, int ROUTE, int ROWS>
__global__ void __launch_bounds__(256) rotate_color_kernel(ImgView src, ImgView dst, RotateArgs a, uint32_t quadBytes)
{
    if constexpr (ROUTE == kRouteTexel)
    {
        const uint32_t x = blockIdx.x * 256u + threadIdx.x;
        if (x >= src.width) return;
        for (uint32_t y = blockIdx.y; y < src.height; y += gridDim.y)
        {
            const Texel t = load_texel(src.pixels + uint64_t(y) * src.rowPitch, x, src.format);
            store_texel(dst.pixels + uint64_t(y) * dst.rowPitch, x, dst.format, rotate_texel<CURVE>(t, a));
        }
    }
    else rotate_quad_lane<CURVE, ROUTE, ROWS>(src, dst, a, quadBytes);
}
} // namespace

#define DXTEX_MARK(NAME) do { if (marks) marks->mark(NAME); } while (0)

hipError_t launch_rotate_color(const ImgView& sv, const ImgView& dv, int curve, const RotateArgs& args, hipStream_t stream, KernelMarks* marks)
{
    const uint32_t width = sv.width, height = sv.height;
    if (!width || !height) return hipSuccess;
    if (curve < ROTATE_CURVE_NONE || curve > ROTATE_CURVE_FROM_ST2084) return hipErrorInvalidValue;
    const uint32_t qb = sv.format == dv.format ? quad_bytes(sv.format) : 0u;
    // launch_convert's admission rule for convert_quad_kernel: 16-byte aligned rows and pitches on both sides
    if (qb && ((reinterpret_cast<uintptr_t>(sv.pixels) | sv.rowPitch | reinterpret_cast<uintptr_t>(dv.pixels) | dv.rowPitch) & 15u) == 0)
    {
        const uint32_t gx = (width / 4u + width % 4u + 255u) / 256u;
        // about 8192 workgroups: enough to fill 256 CUs several times over, few enough that a lane streams several row groups
#define DXTEX_RQUAD(CURVE, QB, ROWS, NAME) do { const uint32_t groups = (height + (ROWS) - 1u) / (ROWS); \
            const uint32_t gy = std::min<uint32_t>(std::min<uint32_t>(groups, 65535u), std::max<uint32_t>(1u, 8192u / gx)); \
            DXTEX_MARK(NAME); \
            hipLaunchKernelGGL((rotate_color_kernel<CURVE, QB, ROWS>), dim3(gx, gy), dim3(256), 0, stream, sv, dv, args, qb); } while (0)
        if (curve == ROTATE_CURVE_NONE)
        {
            if (qb == 16u) DXTEX_RQUAD(ROTATE_CURVE_NONE, 16, 4, "rotate_color<quad>");
            else if (qb == 32u) DXTEX_RQUAD(ROTATE_CURVE_NONE, 32, 2, "rotate_color<quad>");
            else DXTEX_RQUAD(ROTATE_CURVE_NONE, 0, 1, "rotate_color<quad>");
        }
        else if (curve == ROTATE_CURVE_TO_ST2084)
        {
            if (qb == 16u) DXTEX_RQUAD(ROTATE_CURVE_TO_ST2084, 16, 1, "rotate_color<quad,st2084>");
            else if (qb == 32u) DXTEX_RQUAD(ROTATE_CURVE_TO_ST2084, 32, 1, "rotate_color<quad,st2084>");
            else DXTEX_RQUAD(ROTATE_CURVE_TO_ST2084, 0, 1, "rotate_color<quad,st2084>");
        }
        else
        {
            if (qb == 16u) DXTEX_RQUAD(ROTATE_CURVE_FROM_ST2084, 16, 1, "rotate_color<quad,st2084_inverse>");
            else if (qb == 32u) DXTEX_RQUAD(ROTATE_CURVE_FROM_ST2084, 32, 1, "rotate_color<quad,st2084_inverse>");
            else DXTEX_RQUAD(ROTATE_CURVE_FROM_ST2084, 0, 1, "rotate_color<quad,st2084_inverse>");
        }
#undef DXTEX_RQUAD
        DXTEX_MARK(nullptr);
        return hipGetLastError();
    }
    const uint32_t gx = (width + 255u) / 256u;
    const dim3 grid(gx, std::min<uint32_t>(std::min<uint32_t>(height, 65535u), std::max<uint32_t>(1u, 8192u / gx)));
#define DXTEX_RTEXEL(CURVE, NAME) do { DXTEX_MARK(NAME); hipLaunchKernelGGL((rotate_color_kernel<CURVE, kRouteTexel, 1>), grid, dim3(256), 0, stream, sv, dv, args, 0u); } while (0)
    if (curve == ROTATE_CURVE_NONE) DXTEX_RTEXEL(ROTATE_CURVE_NONE, "rotate_color<texel>");
    else if (curve == ROTATE_CURVE_TO_ST2084) DXTEX_RTEXEL(ROTATE_CURVE_TO_ST2084, "rotate_color<texel,st2084>");
    else DXTEX_RTEXEL(ROTATE_CURVE_FROM_ST2084, "rotate_color<texel,st2084_inverse>");
#undef DXTEX_RTEXEL
    DXTEX_MARK(nullptr);
    return hipGetLastError();
}
} // namespace dxtex
