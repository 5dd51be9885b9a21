// C ABI of libdxtex_amd.so (include/dxtex_amd.h): context, validation with the reference's HRESULTs,
// staging for the host-pointer variants, and kernel submission. There is no CPU compute path here: every
// entry point either launches HIP kernels on gfx950 or fails.
#include "../../include/dxtex_amd.h"
#include "dxtex_formats.h"
#include "dxtex_kernels.h"
#include "dxtex_tga.h"
#include "dxtex_dds.h"
#include "dxtex_pnm.h"
#include "dxtex_png.h"
#include "dxtex_jpeg.h"
#include "dxtex_exr.h"
#include "dxtex_tiff.h"
#include "dxtex_nmap.h"
#include "dxtex_transform.h"
#include "dxtex_rotate.h"
#include "dxtex_diag.h"
#include "dxtex_plan.h"
#include "dxtex_copyrect.h"
#include "dxtex_plane.h"
#include "dxtex_fliprotate.h"
#include "dxtex_staging.h"
#include "triangle_filter.h"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

using namespace dxtex;

struct dxtex_ctx;
namespace
{
// Per-kernel device timing (dxtex_ctx_profile_*): an event before every kernel and one after the last.
struct Marks final : dxtex::KernelMarks
{
    dxtex_ctx* ctx = nullptr;
    std::vector<hipEvent_t> pool;        // reused across calls
    std::vector<const char*> names;      // names[i] labels the interval events[i] -> events[i+1]; nullptr = end of a call
    size_t used = 0;
    void mark(const char* kernelName) override;
    void reset() { names.clear(); used = 0; }
};

// A grow-only buffer of the context, device (hipMalloc) or pinned host memory (hipHostMalloc). grow() keeps an allocation that is large
// enough and otherwise replaces it with one of max(need, minBytes) bytes; the destructor frees it (dxtex_ctx_destroy deletes the context
// once every stream that used it has drained).
template<bool Pinned>
struct GrowBuf
{
    void* p = nullptr;
    size_t bytes = 0;
    GrowBuf() = default;
    GrowBuf(const GrowBuf&) = delete;
    GrowBuf& operator=(const GrowBuf&) = delete;
    ~GrowBuf() { if (p) (void)(Pinned ? hipHostFree(p) : hipFree(p)); }
    dxtex_hresult grow(dxtex_ctx* ctx, size_t need, size_t minBytes = 1u << 20);
    uint8_t* u8() const { return static_cast<uint8_t*>(p); }
};
using DeviceBuf = GrowBuf<false>;
using PinnedBuf = GrowBuf<true>;
}

struct dxtex_ctx
{
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t evStart = nullptr, evStop = nullptr;
    float lastKernelMs = -1.0f;
    bool timing = false;
    // staging for the host-pointer entry points
    DeviceBuf stageIn, stageOut;
    // the multi-kernel BC6H/BC7 search (per-mode candidates)
    DeviceBuf scratch;
    // triangle-filter gather tables (host copies stay alive until the next call: the upload is stream-ordered)
    DeviceBuf triBuf;
    std::vector<uint8_t> triHost;
    PinnedBuf triPinned; hipEvent_t triConsumed = nullptr; bool triPending = false;
    // the result of a reduction on its way to the host or to the next kernel: ComputeMSE's four sums, the alpha-coverage and below-threshold
    // counts, the tone-map maximum. 4 doubles; the stream orders its users, and each of them (or its launcher) clears what it accumulates into
    DeviceBuf resultCell;
    // R32G32B32A32_FLOAT rows on their way into a format whose element holds several texels (launch_pack_group)
    DeviceBuf groupRows;
    // error-diffusion Convert: row buffers (launch_convert_diffuse) and the device counter of texels its merge re-ran
    DeviceBuf ditherRows, ditherRerun; uint64_t ditherTexels = 0;
    // JPEG: a colour frame's block-padded sample planes between jpeg_idct and jpeg_colour (launch_jpeg_decode) or jpeg_samples and jpeg_fdct (launch_jpeg_encode)
    DeviceBuf jpegPlanes;
    // OpenEXR: the tiles' byte sums between exr_undo_sums and exr_undo (launch_exr_undo)
    DeviceBuf exrSums;
    // dxtex_compress_many (host pointers): double-buffered pinned + device staging, copy streams on either side of ctx->stream
    struct Lane
    {
        PinnedBuf pinIn, pinOut;
        DeviceBuf devIn, devOut;
        hipEvent_t uploaded = nullptr, computed = nullptr, downloaded = nullptr;
    } lane[2];
    hipStream_t h2d = nullptr, d2h = nullptr;
    // side streams of the BC7 pipeline (modes 4 / 5 run next to each other): created on first use, destroyed with the context
    SideStreams side = {};
    bool sideTried = false, sideOk = false;
    uint64_t warmedFormats = 0;        // dxtex_ctx_prepare: destination BC formats (bit = format - 64) whose pipeline has run once on this context
    std::string lastError;
    bool profiling = false;
    Marks marks;
    // host <-> device bytes moved for this context (dxtex_ctx_transfer_bytes)
    uint64_t h2dBytes = 0, d2hBytes = 0;
};

void Marks::mark(const char* kernelName)
{
    if (used == pool.size())
    {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return;
        pool.push_back(e);
    }
    (void)hipEventRecord(pool[used++], ctx->stream);
    names.push_back(kernelName);
}

namespace
{
dxtex_hresult fail(dxtex_ctx* ctx, dxtex_hresult hr, const char* what, hipError_t e = hipSuccess)
{
    if (ctx)
    {
        ctx->lastError = what;
        if (e != hipSuccess) { ctx->lastError += ": "; ctx->lastError += hipGetErrorString(e); }
    }
    return hr;
}

// what an entry point returns for the status of the launches it queued
dxtex_hresult launched(dxtex_ctx* ctx, hipError_t e) { return e == hipSuccess ? DXTEX_S_OK : fail(ctx, DXTEX_E_FAIL, "kernel launch failed", e); }

// where launchers record their kernels' names: the context's marks while it is profiling, nowhere otherwise
Marks* marks_of(dxtex_ctx* ctx) { return ctx->profiling ? &ctx->marks : nullptr; }

// The surface of an image as the launchers take it. The only place that narrows an image's extents to 32 bits: the check_* of the entry
// points bound them.
ImgView view_of(const dxtex_image& im) { return ImgView{ im.pixels, im.rowPitch, uint32_t(im.width), uint32_t(im.height), im.format }; }

// every host <-> device copy of the library goes through here so that dxtex_ctx_transfer_bytes can account for it
inline hipError_t counted_copy(dxtex_ctx* ctx, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t stream)
{
    if (kind == hipMemcpyHostToDevice) ctx->h2dBytes += bytes;
    else if (kind == hipMemcpyDeviceToHost) ctx->d2hBytes += bytes;
    return hipMemcpyAsync(dst, src, bytes, kind, stream);
}

// rows of rowBytes between host and device through their own pitches, counted like every other transfer. A row of the packed formats can
// be longer than a pitch (see check_copy_rect): such rows travel one by one, in order, so that the later row wins as in the reference.
hipError_t counted_copy_rows(dxtex_ctx* ctx, void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t rowBytes, size_t rows, hipMemcpyKind kind)
{
    if (!rows || !rowBytes) return hipSuccess;
    if (rows == 1 || (dstPitch == rowBytes && srcPitch == rowBytes)) return counted_copy(ctx, dst, src, rowBytes * rows, kind, ctx->stream);
    if (rowBytes > dstPitch || rowBytes > srcPitch)
    {
        hipError_t e = hipSuccess;
        for (size_t y = 0; y < rows && e == hipSuccess; ++y)
            e = counted_copy(ctx, static_cast<uint8_t*>(dst) + y * dstPitch, static_cast<const uint8_t*>(src) + y * srcPitch, rowBytes, kind, ctx->stream);
        return e;
    }
    if (kind == hipMemcpyHostToDevice) ctx->h2dBytes += rowBytes * rows; else ctx->d2hBytes += rowBytes * rows;
    return hipMemcpy2DAsync(dst, dstPitch, src, srcPitch, rowBytes, rows, kind, ctx->stream);
}

#define HIP_TRY(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(ctx, (e_ == hipErrorOutOfMemory) ? DXTEX_E_OUTOFMEMORY : DXTEX_E_FAIL, #expr, e_); } while (0)

template<bool Pinned>
dxtex_hresult GrowBuf<Pinned>::grow(dxtex_ctx* ctx, size_t need, size_t minBytes)
{
    if (bytes >= need) return DXTEX_S_OK;
    if (p) { HIP_TRY(ctx, Pinned ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
    const size_t want = std::max(need, minBytes);
    HIP_TRY(ctx, Pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want));
    bytes = want;
    return DXTEX_S_OK;
}

inline size_t align256(size_t bytes) { return (bytes + 255) & ~size_t(255); }

// Consecutive parts of one allocation, each 256-byte aligned: their offsets and the bytes the allocation needs
struct Arena
{
    std::vector<size_t> at;
    size_t total = 0;
    Arena(const size_t* bytes, size_t n) { for (size_t i = 0; i < n; ++i) { at.push_back(total); total += align256(bytes[i]); } }
};

// a copy of an image whose pixels are elsewhere (in the context's staging)
dxtex_image with_pixels(const dxtex_image& im, uint8_t* pixels) { dxtex_image o = im; o.pixels = pixels; return o; }

struct ScopedDevice
{
    int prev = -1;
    explicit ScopedDevice(int dev) { (void)hipGetDevice(&prev); if (prev != dev) (void)hipSetDevice(dev); else prev = -1; }
    ~ScopedDevice() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// lazily creates the context's side streams; nullptr (= serial pipelines) if the runtime refuses
const SideStreams* side_streams(dxtex_ctx* ctx)
{
    if (!ctx->sideTried)
    {
        ctx->sideTried = true;
        bool ok = hipEventCreateWithFlags(&ctx->side.forked, hipEventDisableTiming) == hipSuccess;
        for (int k = 0; k < kSideStreams && ok; ++k)
            ok = hipStreamCreateWithFlags(&ctx->side.side[k], hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&ctx->side.joined[k], hipEventDisableTiming) == hipSuccess;
        ctx->sideOk = ok;
    }
    return ctx->sideOk ? &ctx->side : nullptr;
}

static const bool kNoTiming = dev_env("DXTEX_NO_TIMING") != nullptr;
void time_begin(dxtex_ctx* ctx) { if (!kNoTiming) (void)hipEventRecord(ctx->evStart, ctx->stream); }
void time_end(dxtex_ctx* ctx) { if (!kNoTiming) { (void)hipEventRecord(ctx->evStop, ctx->stream); ctx->timing = true; } }

// The part of ConvertScanline that Compress reaches (DirectXTexConvert.cpp:3080-3854), resolved once
// per image on the host into the (tcv, tsw) pair the tile loader applies.
void tile_conversion(const FmtInfo& in, const FmtInfo& out, uint32_t compressFlags, int* tcv, int* tsw)
{
    bool srgbIn = (compressFlags & DXTEX_COMPRESS_SRGB_IN) != 0 || (in.cls & FC_SRGB);
    bool srgbOut = (compressFlags & DXTEX_COMPRESS_SRGB_OUT) != 0 || (out.cls & FC_SRGB);
    if (in.format == FMT_A8_UNORM || in.format == FMT_R10G10B10_XR_BIAS_A2_UNORM) srgbIn = false;      // :3136-3139
    if (srgbIn && srgbOut) srgbIn = srgbOut = false;       // :3164-3167

    *tcv = TCV_NONE; *tsw = TSW_NONE;
    if (in.cls & FC_DEPTH)
    {
        // a depth source: ConvertScanline's depth branch instead of the range conversion (:3186-3291); sRGB does not apply (:3172, :3845 ask
        // for a non-depth format on the side they convert - the BC side still gets its encode step below)
        *tsw = resolve_depth_steps(in, out, 0) << 8;
        srgbIn = false;
    }
    else if (out.cls & FC_UNORM)
    {
        if (in.cls & FC_SNORM) *tcv = TCV_SNORM_TO_UNORM;
        else if (in.cls & FC_FLOAT) *tcv = TCV_SATURATE;
    }
    else if (out.cls & FC_SNORM)
    {
        if (in.cls & FC_UNORM) *tcv = TCV_UNORM_TO_SNORM;
        else if (in.cls & FC_FLOAT) *tcv = TCV_CLAMP_SNORM;
    }

    const uint32_t inRGBA = in.cls & (FC_R | FC_G | FC_B | FC_A), outRGB = out.cls & (FC_R | FC_G | FC_B);
    if (inRGBA == FC_A && !(out.cls & FC_A)) *tsw = TSW_A_TO_RGB;
    else if ((in.cls & (FC_R | FC_G | FC_B)) == FC_R)
    {
        if (outRGB == (FC_R | FC_G | FC_B)) *tsw = TSW_R_TO_RGB;
        else if (outRGB == (FC_R | FC_G)) *tsw = TSW_R_TO_RG;
    }
    if (srgbIn && (in.cls & (FC_FLOAT | FC_UNORM))) *tcv |= TCV_SRGB_TO_LINEAR;      // :3170-3180
    if (srgbOut && (out.cls & (FC_FLOAT | FC_UNORM))) *tcv |= TCV_LINEAR_TO_SRGB;    // :3843-3853
}

// Compress' argument checks (DirectXTexCompress.cpp:671-676, :741-745) and the source view the tile loaders take
dxtex_hresult compress_view(dxtex_ctx* ctx, const dxtex_image& src, int dstFormat, uint32_t flags, SrcView* view)
{
    const int srcFormat = src.format;
    const size_t width = src.width, height = src.height;
    const FmtInfo* in = format_info(srcFormat);
    const FmtInfo* out = format_info(dstFormat);
    // the reference's order (DirectXTexCompress.cpp:671-676): E_INVALIDARG for a compressed source or an uncompressed target first,
    // HRESULT_E_NOT_SUPPORTED for formats the path cannot take (typeless / planar / palettised there; anything without kernels here)
    const auto bcId = [](int f) { return (f >= 70 && f <= 84) || (f >= 94 && f <= 99); };      // IsCompressed: BC1_TYPELESS .. BC5_SNORM, BC6H_TYPELESS .. BC7_UNORM_SRGB
    if (bcId(srcFormat)) return fail(ctx, DXTEX_E_INVALIDARG, "source image is already compressed");
    if (!bcId(dstFormat)) return fail(ctx, DXTEX_E_INVALIDARG, "destination is not a BC format");
    if (!out || !(out->cls & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "destination BC format is not supported (typeless)");
    if (!in) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "source format is not supported by the MI355X path");
    // R1_UNORM: the reference refuses it (DirectXTexCompress.cpp:228-232, "we don't support compressing from monochrome"). The packed
    // two-texel formats: CompressBC steps through a row with BitsPerPixel / 8 bytes per texel (:224-235, :279), which for them is the
    // size of an ELEMENT of two texels (DirectXTexUtil.cpp:625-670) - block column k reads texels 8k.. instead of 4k.. and the right half
    // of the image reads past its rows (past the image on the last block row). Nothing defined to reproduce: refused here.
    if (in->cls & FC_GROUP) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "Compress does not take R1_UNORM or the packed two-texel formats as a source");
    if (!width || !height) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    if (width > 0xFFFFFFFCull || height > 0xFFFFFFFCull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    SrcView v;
    v.pixels = src.pixels; v.width = uint32_t(width); v.height = uint32_t(height); v.rowPitch = src.rowPitch; v.format = srcFormat;
    tile_conversion(*in, *out, flags, &v.tcv, &v.tsw);
    *view = v;
    return DXTEX_S_OK;
}

// BC7 / BC6H: the search scratch for `nblocks` blocks of `count` images (BC1-BC5 need none)
dxtex_hresult grow_scratch(dxtex_ctx* ctx, int format, uint64_t nblocks, uint32_t flags, size_t count = 1)
{
    if (is_bc7(format)) return ctx->scratch.grow(ctx, bc7_scratch_bytes(nblocks, flags, count));
    if (is_bc6h(format)) return ctx->scratch.grow(ctx, bc6h_scratch_bytes(nblocks, count));
    return DXTEX_S_OK;
}

// the BC encoders: one image (view) -> blocks of `format` at dst
dxtex_hresult encode(dxtex_ctx* ctx, const SrcView& v, uint8_t* dst, size_t dstRowPitch, int format, uint32_t flags, float threshold)
{
    const uint64_t nblocks = uint64_t((v.width + 3) / 4) * uint64_t((v.height + 3) / 4);
    const dxtex_hresult hr = grow_scratch(ctx, format, nblocks, flags);
    if (hr != DXTEX_S_OK) return hr;
    KernelMarks* marks = marks_of(ctx);
    hipError_t e;
    if (is_bc7(format)) e = launch_bc7_encode(v, dst, dstRowPitch, flags, ctx->scratch.p, ctx->stream, marks, side_streams(ctx));
    else if (is_bc6h(format)) e = launch_bc6h_encode(v, dst, dstRowPitch, format == FMT_BC6H_SF16, ctx->scratch.p, ctx->stream, marks, side_streams(ctx));
    else if (is_bc15(format)) e = launch_bc15_encode(v, dst, dstRowPitch, format, flags, threshold, ctx->stream);
    else return fail(ctx, DXTEX_E_NOT_SUPPORTED, "BC format not implemented yet");
    return launched(ctx, e);
}

dxtex_hresult submit_compress(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst, uint32_t flags, float threshold)
{
    SrcView v;
    const dxtex_hresult hr = compress_view(ctx, src, dst.format, flags, &v);
    if (hr != DXTEX_S_OK) return hr;
    return encode(ctx, v, dst.pixels, dst.rowPitch, dst.format, flags, threshold);
}

dxtex_hresult check_pair(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    if (!src->pixels || !dst->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (src->width != dst->width || src->height != dst->height) return fail(ctx, DXTEX_E_FAIL, "size mismatch");
    return DXTEX_S_OK;
}

// tight size checks for host-pointer images: a pitch below the format's minimum would make the kernels read or write past the staging
dxtex_hresult check_host_pitches(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, size_t* srcBytes, size_t* dstBytes)
{
    size_t minSrcRow = 0, minSrcSlice = 0, minDstRow = 0, minDstSlice = 0;
    if (dxtex_compute_pitch(src->format, src->width, src->height, &minSrcRow, &minSrcSlice) != DXTEX_S_OK ||
        dxtex_compute_pitch(dst->format, dst->width, dst->height, &minDstRow, &minDstSlice) != DXTEX_S_OK)
        return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    if (src->rowPitch < minSrcRow || dst->rowPitch < minDstRow) return fail(ctx, DXTEX_E_INVALIDARG, "rowPitch is smaller than the format's minimum (ComputePitch)");
    const size_t srcRows = (minSrcRow && minSrcSlice) ? minSrcSlice / minSrcRow : src->height;
    const size_t dstRows = (minDstRow && minDstSlice) ? minDstSlice / minDstRow : dst->height;
    if (src->rowPitch > SIZE_MAX / std::max<size_t>(1, srcRows) || dst->rowPitch > SIZE_MAX / std::max<size_t>(1, dstRows))
        return fail(ctx, DXTEX_E_INVALIDARG, "rowPitch x rows overflows");
    *srcBytes = src->rowPitch * srcRows;
    *dstBytes = dst->rowPitch * dstRows;
    return DXTEX_S_OK;
}

// submit() between the timing events, on the context's device: what a timed entry point does after its checks
template<class Submit>
dxtex_hresult run_timed(dxtex_ctx* ctx, Submit&& submit)
{
    ScopedDevice sd(ctx->device);
    time_begin(ctx);
    const dxtex_hresult hr = submit();
    time_end(ctx);
    return hr;
}

// Every host-pointer entry point, after its checks: the plan's two buffers grown, its uploads issued, submit(stageIn, stageOut) - which
// queues the kernels on the staged bytes - between the timing events (so dxtex_ctx_last_kernel_ms covers kernels only), the plan's downloads,
// and the call returns once they have landed. A failed submit returns at once: no download, no synchronisation. A submit that times itself
// (or runs untimed) says so with timed = false. The bases are only valid inside submit: the buffers may move when they grow.
template<class Submit>
dxtex_hresult run_plan(dxtex_ctx* ctx, const StagingPlan& plan, Submit&& submit, bool timed = true)
{
    if (!plan.ok()) return fail(ctx, DXTEX_E_INVALIDARG, "the bytes to stage overflow");
    ScopedDevice sd(ctx->device);
    dxtex_hresult hr = ctx->stageIn.grow(ctx, plan.need(STAGE_IN)); if (hr != DXTEX_S_OK) return hr;
    hr = ctx->stageOut.grow(ctx, plan.need(STAGE_OUT)); if (hr != DXTEX_S_OK) return hr;
    uint8_t* const base[2] = { ctx->stageIn.u8(), ctx->stageOut.u8() };
    for (const StageCopy& c : plan.uploads())
        HIP_TRY(ctx, counted_copy_rows(ctx, base[STAGE_IN] + c.at(), c.devPitch, c.host, c.hostPitch, c.rowBytes, c.rows, hipMemcpyHostToDevice));
    hr = timed ? run_timed(ctx, [&] { return submit(base[STAGE_IN], base[STAGE_OUT]); }) : submit(base[STAGE_IN], base[STAGE_OUT]);
    if (hr != DXTEX_S_OK) return hr;
    for (const StageCopy& c : plan.downloads())
        HIP_TRY(ctx, counted_copy_rows(ctx, c.host, c.hostPitch, base[c.part.buf] + c.at(), c.devPitch, c.rowBytes, c.rows, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DXTEX_S_OK;
}

// One flat run of bytes up and one down: the single-image entry points and the codecs' pack side
template<class Submit>
dxtex_hresult run_staged(dxtex_ctx* ctx, const void* hostIn, size_t inBytes, void* hostOut, size_t outBytes, Submit&& submit)
{
    StagingPlan plan;
    plan.upload(hostIn, plan.in(inBytes), inBytes);
    plan.download(hostOut, plan.out(outBytes), outBytes);
    return run_plan(ctx, plan, submit);
}

// The staged-rows unpack of the PNM, PNG and JPEG host forms: the `need` bytes of the file side go up as they are; the kernel writes tight
// rows (rounded up to 16 bytes, so that a width of whole groups keeps the wide route) into the output staging, and only each row's texels
// come down, through the caller's pitch. launch(stream, view) queues the kernel.
template<class Launch>
dxtex_hresult run_staged_rows(dxtex_ctx* ctx, const void* hostIn, size_t need, const dxtex_image* dst, size_t rowBytes, Launch&& launch)
{
    const size_t pitch = (rowBytes + 15) & ~size_t(15);
    StagingPlan plan;
    plan.upload(hostIn, plan.in(need), need);
    plan.download(dst->pixels, dst->rowPitch, plan.out(pitch, dst->height), 0, pitch, rowBytes, dst->height);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out)
    {
        dxtex_image staged = with_pixels(*dst, out);
        staged.rowPitch = pitch; staged.slicePitch = pitch * dst->height;
        return launched(ctx, launch(in, view_of(staged)));
    });
}

// The host-pointer twin of a single-image entry point, after its check_*: srcBytes of src and dstBytes of dst travel, and submit(src, dst)
// - what the _device twin runs on the caller's images - runs on the staged ones
template<class Submit>
dxtex_hresult run_staged_images(dxtex_ctx* ctx, const dxtex_image* src, size_t srcBytes, const dxtex_image* dst, size_t dstBytes, Submit&& submit)
{
    return run_staged(ctx, src->pixels, srcBytes, dst->pixels, dstBytes,
                      [&](uint8_t* in, uint8_t* out) { return submit(with_pixels(*src, in), with_pixels(*dst, out)); });
}

// run_staged_images with the bytes the pitch checks give (so the staging holds every byte the kernels touch)
template<class Submit>
dxtex_hresult run_host_twin(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, Submit&& submit)
{
    size_t srcBytes = 0, dstBytes = 0;
    const dxtex_hresult hr = check_host_pitches(ctx, src, dst, &srcBytes, &dstBytes);
    if (hr != DXTEX_S_OK) return hr;
    return run_staged_images(ctx, src, srcBytes, dst, dstBytes, submit);
}

// the bytes of a host image that the kernels touch (check_host_pitches for one image)
dxtex_hresult host_image_bytes(dxtex_ctx* ctx, const dxtex_image& im, size_t* bytes)
{
    size_t other = 0;
    return check_host_pitches(ctx, &im, &im, bytes, &other);
}

// Difference and merge on host pointers: a and b go up whole, into a part of the input staging each; submit(a, b, dst) runs on the staged
// images, dst with the caller's pitch; only dst's texel rows come down, so the caller's row padding stays as it was, as with the device form
template<class Submit>
dxtex_hresult run_staged_pair(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, Submit&& submit)
{
    size_t dstBytes = 0, aBytes = 0, bBytes = 0, rowBytes = 0, sliceBytes = 0;
    dxtex_hresult hr = host_image_bytes(ctx, *dst, &dstBytes);
    if (hr == DXTEX_S_OK) hr = host_image_bytes(ctx, *a, &aBytes);
    if (hr == DXTEX_S_OK) hr = host_image_bytes(ctx, *b, &bBytes);
    if (hr != DXTEX_S_OK) return hr;
    (void)dxtex_compute_pitch(dst->format, dst->width, dst->height, &rowBytes, &sliceBytes);      // (host_image_bytes has asked the same)
    StagingPlan plan;
    const StagePart pa = plan.in(aBytes), pb = plan.in(bBytes), pd = plan.out(dstBytes);
    plan.upload(a->pixels, pa, aBytes);
    plan.upload(b->pixels, pb, bBytes);
    plan.download(dst->pixels, dst->rowPitch, pd, 0, dst->rowPitch, rowBytes, rowBytes ? sliceBytes / rowBytes : 0);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out) { return submit(with_pixels(*a, in + pa.at), with_pixels(*b, in + pb.at), with_pixels(*dst, out)); });
}

// A destination whose element holds several texels (FC_GROUP) is written in two steps: the operation leaves R32G32B32A32_FLOAT rows in
// ctx->groupRows (what the reference hands to StoreScanline), launch_pack_group stores them. The stream orders the steps, so one
// buffer serves every level of a chain. launch(out) queues the operation's kernels with `out` as their destination: dst itself, or the
// float rows; `marks` is what the operation's own launcher records into.
bool is_group_format(int format) { const FmtInfo* f = format_info(format); return f && (f->cls & FC_GROUP); }
template<class Launch>
dxtex_hresult launch_into(dxtex_ctx* ctx, const ImgView& dst, KernelMarks* marks, Launch&& launch)
{
    if (!is_group_format(dst.format)) return launched(ctx, launch(dst));
    ImgView rows = { nullptr, uint64_t(dst.width) * 16, dst.width, dst.height, FMT_R32G32B32A32_FLOAT };
    const dxtex_hresult hr = ctx->groupRows.grow(ctx, rows.rowPitch * dst.height);
    if (hr != DXTEX_S_OK) return hr;
    rows.pixels = ctx->groupRows.u8();
    hipError_t e = launch(rows);
    if (e == hipSuccess) e = launch_pack_group(rows, dst, ctx->stream, marks);
    return launched(ctx, e);
}
} // namespace

extern "C"
{
dxtex_hresult dxtex_ctx_create(int device, dxtex_ctx** out)
{
    if (!out) return DXTEX_E_POINTER;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
        return DXTEX_E_FAIL;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DXTEX_E_FAIL;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    {
        std::fprintf(stderr, "dxtex_amd: device %d is %s; this library carries gfx950 code objects only\n", device, prop.gcnArchName);
        return DXTEX_E_FAIL;
    }
    dxtex_ctx* ctx = new (std::nothrow) dxtex_ctx;
    if (!ctx) return DXTEX_E_OUTOFMEMORY;
    ctx->device = device;
    ScopedDevice sd(device);
    if (hipStreamCreateWithFlags(&ctx->ownStream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->evStart) != hipSuccess || hipEventCreate(&ctx->evStop) != hipSuccess)
    {
        delete ctx;
        return DXTEX_E_FAIL;
    }
    ctx->stream = ctx->ownStream;
    ctx->marks.ctx = ctx;
    *out = ctx;
    return DXTEX_S_OK;
}

void dxtex_ctx_destroy(dxtex_ctx* ctx)
{
    if (!ctx) return;
    ScopedDevice sd(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    std::vector<hipStream_t> streams = { ctx->h2d, ctx->d2h };
    std::vector<hipEvent_t> events = ctx->marks.pool;
    events.insert(events.end(), { ctx->evStart, ctx->evStop, ctx->triConsumed, ctx->side.forked });
    for (int k = 0; k < kSideStreams; ++k) { streams.push_back(ctx->side.side[k]); events.push_back(ctx->side.joined[k]); }
    for (const dxtex_ctx::Lane& l : ctx->lane) events.insert(events.end(), { l.uploaded, l.computed, l.downloaded });
    for (hipStream_t s : streams) if (s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (hipEvent_t e : events) if (e) (void)hipEventDestroy(e);
    if (ctx->ownStream) (void)hipStreamDestroy(ctx->ownStream);
    delete ctx;        // the buffers go with it: every stream that used them has drained, and the device is still the context's
}

dxtex_hresult dxtex_ctx_set_stream(dxtex_ctx* ctx, void* hip_stream)
{
    if (!ctx) return DXTEX_E_POINTER;
    hipStream_t next = hip_stream ? static_cast<hipStream_t>(hip_stream) : ctx->ownStream;
    if (next != ctx->stream)
    {
        // the context's scratch, staging and filter tables are ordered by ONE stream: work queued on the old one must be done
        // before kernels on the new one may reuse them. The previous stream must stay alive until this call returns. A handle the
        // runtime no longer knows (the caller destroyed the stream: nothing left to wait for) is tolerated and the context switches;
        // any other error is an asynchronous failure of work that was queued on the old stream - a faulted kernel, an ECC error -
        // whose output the caller must not trust: it is reported and the context keeps its stream.
        ScopedDevice sd(ctx->device);
        const hipError_t drained = hipStreamSynchronize(ctx->stream);
        if (drained != hipSuccess)
        {
            (void)hipGetLastError();
            if (drained != hipErrorInvalidHandle && drained != hipErrorInvalidResourceHandle && drained != hipErrorContextIsDestroyed)
                return fail(ctx, DXTEX_E_FAIL, "work queued on the previous stream failed", drained);
        }
        ctx->stream = next;
    }
    return DXTEX_S_OK;
}

void* dxtex_ctx_get_stream(dxtex_ctx* ctx) { return ctx ? ctx->stream : nullptr; }

dxtex_hresult dxtex_ctx_synchronize(dxtex_ctx* ctx)
{
    if (!ctx) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DXTEX_S_OK;
}

const char* dxtex_ctx_last_error(dxtex_ctx* ctx) { return ctx ? ctx->lastError.c_str() : "null context"; }

float dxtex_ctx_last_kernel_ms(dxtex_ctx* ctx)
{
    if (!ctx || !ctx->timing) return -1.0f;
    ScopedDevice sd(ctx->device);
    if (hipEventSynchronize(ctx->evStop) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, ctx->evStart, ctx->evStop) != hipSuccess) return -1.0f;
    return ms;
}

dxtex_hresult dxtex_ctx_profile_begin(dxtex_ctx* ctx)
{
    if (!ctx) return DXTEX_E_POINTER;
    ctx->marks.reset();
    ctx->profiling = true;
    return DXTEX_S_OK;
}

dxtex_hresult dxtex_ctx_profile_end(dxtex_ctx* ctx, char* names, size_t namesBytes, float* ms, uint32_t* launches, size_t capacity, size_t* count)
{
    if (!ctx || !count) return DXTEX_E_POINTER;
    ctx->profiling = false;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // aggregate by kernel name (pointer identity: names are string literals inside the launchers)
    std::vector<const char*> uniq; std::vector<double> total; std::vector<uint32_t> n;
    Marks& m = ctx->marks;
    for (size_t i = 0; i + 1 < m.used; ++i)
    {
        if (!m.names[i]) continue;
        float t = 0.0f;
        if (hipEventElapsedTime(&t, m.pool[i], m.pool[i + 1]) != hipSuccess) continue;
        size_t k = 0;
        for (; k < uniq.size(); ++k) if (uniq[k] == m.names[i]) break;
        if (k == uniq.size()) { uniq.push_back(m.names[i]); total.push_back(0.0); n.push_back(0); }
        total[k] += t; n[k] += 1;
    }
    *count = uniq.size();
    size_t off = 0;
    for (size_t k = 0; k < uniq.size() && k < capacity; ++k)
    {
        if (ms) ms[k] = float(total[k]);
        if (launches) launches[k] = n[k];
        if (names)
        {
            const size_t len = std::strlen(uniq[k]);
            if (off + len + 1 < namesBytes) { std::memcpy(names + off, uniq[k], len); off += len; names[off++] = '\n'; }
        }
    }
    if (names && namesBytes) names[off < namesBytes ? off : namesBytes - 1] = 0;
    m.reset();
    return DXTEX_S_OK;
}

int dxtex_is_compressed(int32_t format) { return is_bc(format) ? 1 : 0; }

size_t dxtex_bits_per_pixel(int32_t format)
{
    const FmtInfo* f = format_info(format);
    return f ? f->bpp : 0;
}

dxtex_hresult dxtex_compute_pitch(int32_t format, size_t width, size_t height, size_t* rowPitch, size_t* slicePitch)
{
    if (!rowPitch || !slicePitch) return DXTEX_E_POINTER;
    const FmtInfo* f = format_info(format);
    if (!f) return DXTEX_E_INVALIDARG;
    uint64_t pitch, slice;
    if (f->cls & FC_BC)
    {
        // DirectXTexUtil.cpp:972-1029
        const uint64_t nbw = std::max<uint64_t>(1u, (uint64_t(width) + 3u) / 4u);
        const uint64_t nbh = std::max<uint64_t>(1u, (uint64_t(height) + 3u) / 4u);
        pitch = nbw * bc_block_bytes(format);
        slice = pitch * nbh;
    }
    else if (f->cls & FC_PACKED)
    {
        // two texels per element: ((width + 1) >> 1) elements of 4 (R8G8_B8G8, G8R8_G8B8, YUY2) or 8 (Y210, Y216) bytes (DirectXTexUtil.cpp:1031-1052)
        pitch = ((uint64_t(width) + 1u) >> 1) * ((f->bpp == 32) ? 8u : 4u);
        slice = pitch * uint64_t(height);
    }
    else
    {
        pitch = (uint64_t(width) * f->bpp + 7u) / 8u;   // default byte alignment, :1174-1178
        slice = pitch * uint64_t(height);
    }
    *rowPitch = size_t(pitch); *slicePitch = size_t(slice);
    return DXTEX_S_OK;
}

dxtex_hresult dxtex_compress_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags, float threshold)
{
    dxtex_hresult hr = check_pair(ctx, src, dst);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_compress(ctx, *src, *dst, flags, threshold); });
}

dxtex_hresult dxtex_compress_many_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count,
                                         uint32_t flags, float threshold)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!srcs || !dsts || !count) return fail(ctx, DXTEX_E_INVALIDARG, "empty batch");
    ScopedDevice sd(ctx->device);
    // BC7 / BC6H arrays go through the per-mode pipeline as one block list (launch_bc7_encode_many / launch_bc6h_encode_many): the pipeline's latency floor and
    // tails are paid once per 2^22 blocks instead of once per image
    bool allBc7 = count > 1, allBc6 = count > 1;
    for (size_t i = 0; i < count; ++i)
    {
        allBc7 = allBc7 && is_bc7(dsts[i].format);
        allBc6 = allBc6 && dsts[i].format == dsts[0].format && is_bc6h(dsts[i].format);
    }
    if (allBc7 || allBc6)
    {
        std::vector<BcImage> batch(count);
        uint64_t nblocks = 0;
        for (size_t i = 0; i < count; ++i)
        {
            dxtex_hresult hr = check_pair(ctx, &srcs[i], &dsts[i]);
            if (hr == DXTEX_S_OK)
                hr = compress_view(ctx, srcs[i], dsts[i].format, flags, &batch[i].src);
            if (hr != DXTEX_S_OK) return hr;
            batch[i].dst = dsts[i].pixels; batch[i].dstRowPitch = dsts[i].rowPitch;
            nblocks += uint64_t((srcs[i].width + 3) / 4) * uint64_t((srcs[i].height + 3) / 4);
        }
        const dxtex_hresult hr = grow_scratch(ctx, dsts[0].format, nblocks, flags, count);
        if (hr != DXTEX_S_OK) return hr;
        KernelMarks* marks = marks_of(ctx);
        time_begin(ctx);
        const hipError_t e = allBc7 ? launch_bc7_encode_many(batch.data(), count, flags, ctx->scratch.p, ctx->stream, marks, side_streams(ctx))
                                    : launch_bc6h_encode_many(batch.data(), count, dsts[0].format == FMT_BC6H_SF16, ctx->scratch.p, ctx->stream, marks, side_streams(ctx));
        time_end(ctx);
        return launched(ctx, e);
    }
    time_begin(ctx);
    // BC1-BC5: runs of small images of one target format (the tail of a mip chain) share a launch; everything else goes image by image
    std::vector<BcImage> small;
    int smallFormat = 0;
    auto flush_small = [&]() -> dxtex_hresult
    {
        if (small.empty()) return DXTEX_S_OK;
        const hipError_t e = launch_bc15_encode_small(small.data(), int(small.size()), smallFormat, flags, threshold, ctx->stream);
        small.clear();
        return launched(ctx, e);
    };
    for (size_t i = 0; i < count; ++i)
    {
        dxtex_hresult hr = check_pair(ctx, &srcs[i], &dsts[i]);
        if (hr == DXTEX_S_OK && is_bc15(dsts[i].format) && bc15_small_image(uint32_t(srcs[i].width), uint32_t(srcs[i].height)) && srcs[i].width <= 0xFFFFFFFFull && srcs[i].height <= 0xFFFFFFFFull)
        {
            if (!small.empty() && (smallFormat != dsts[i].format || int(small.size()) == bc15_small_batch_max())) hr = flush_small();
            BcImage im;
            if (hr == DXTEX_S_OK)
                hr = compress_view(ctx, srcs[i], dsts[i].format, flags, &im.src);
            if (hr == DXTEX_S_OK) { im.dst = dsts[i].pixels; im.dstRowPitch = dsts[i].rowPitch; small.push_back(im); smallFormat = dsts[i].format; }
        }
        else if (hr == DXTEX_S_OK)
        {
            hr = flush_small();                        // keeps the images in submission order on the stream
            if (hr == DXTEX_S_OK)
                hr = submit_compress(ctx, srcs[i], dsts[i], flags, threshold);
        }
        if (hr != DXTEX_S_OK) { time_end(ctx); return hr; }
    }
    const dxtex_hresult hrSmall = flush_small();
    time_end(ctx);
    return hrSmall;
}

// GPUCompressBC::Prepare's role (BCDirectCompute.cpp:203-369): size the context for `count` images of one shape up front.
dxtex_hresult dxtex_ctx_prepare(dxtex_ctx* ctx, size_t width, size_t height, int32_t src_format, int32_t dst_format, uint32_t flags, size_t count,
                                size_t* device_bytes)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!count) return fail(ctx, DXTEX_E_INVALIDARG, "empty batch");
    size_t srcRow = 0, srcSlice = 0, dstRow = 0, dstSlice = 0;
    SrcView v;
    dxtex_hresult hr = compress_view(ctx, { width, height, src_format, 0, 0, nullptr }, dst_format, flags, &v);      // the format / size checks of dxtex_compress
    if (hr != DXTEX_S_OK) return hr;
    if (dxtex_compute_pitch(src_format, width, height, &srcRow, &srcSlice) != DXTEX_S_OK || dxtex_compute_pitch(dst_format, width, height, &dstRow, &dstSlice) != DXTEX_S_OK)
        return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    ScopedDevice sd(ctx->device);
    const uint64_t nblocks = uint64_t((width + 3) / 4) * uint64_t((height + 3) / 4) * count;
    hr = grow_scratch(ctx, dst_format, nblocks, flags, count);
    if (hr != DXTEX_S_OK) return hr;
    // the staging of dxtex_compress (and of the warm-up below), `count` images 256-byte aligned (dxtex_compress_many stages through its lanes)
    hr = ctx->stageIn.grow(ctx, align256(srcSlice) * count); if (hr != DXTEX_S_OK) return hr;
    hr = ctx->stageOut.grow(ctx, align256(dstSlice) * count); if (hr != DXTEX_S_OK) return hr;
    if (device_bytes) *device_bytes = ctx->scratch.bytes + ctx->stageIn.bytes + ctx->stageOut.bytes;
    // GPUCompressBC::Prepare also binds the shaders the size needs (BCDirectCompute.cpp:203-369). The counterpart here: the HIP runtime loads a
    // kernel's code object on its first launch, and the BC7 / BC6H pipelines are some forty kernels plus three side streams - 19 ms on the first
    // call of a fresh process against 1.2 ms on the second (tools/cold_probe.py: a 64 x 64 image). One block of zeros goes through the same
    // pipeline now, once per destination format and context, so the first real call finds everything loaded. Nothing is returned from it.
    const uint64_t bit = (dst_format >= 64 && dst_format < 128) ? (uint64_t(1) << (dst_format - 64)) : 0;
    if (bit && !(ctx->warmedFormats & bit))
    {
        const size_t ww = std::min<size_t>(width, 4), wh = std::min<size_t>(height, 4);
        size_t wRow = 0, wSlice = 0, oRow = 0, oSlice = 0;
        if (dxtex_compute_pitch(src_format, ww, wh, &wRow, &wSlice) == DXTEX_S_OK && dxtex_compute_pitch(dst_format, ww, wh, &oRow, &oSlice) == DXTEX_S_OK &&
            wSlice <= ctx->stageIn.bytes && oSlice <= ctx->stageOut.bytes)
        {
            HIP_TRY(ctx, hipMemsetAsync(ctx->stageIn.p, 0, wSlice, ctx->stream));
            hr = submit_compress(ctx, { ww, wh, src_format, wRow, wSlice, ctx->stageIn.u8() }, { ww, wh, dst_format, oRow, oSlice, ctx->stageOut.u8() }, flags, 0.5f);
            if (hr != DXTEX_S_OK) return hr;
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            ctx->warmedFormats |= bit;
        }
    }
    return DXTEX_S_OK;
}

// Array form of dxtex_compress with host pointers (the cfg5 entry point: DirectXTexCompress.cpp:794-833 loops over the images of
// an array). The array is cut into chunks of about DXTEX_MANY_CHUNK_TEXELS texels (default 32 Mi: eight 2048^2 images, a pass
// size at which the BC6H / BC7 search pipeline runs at its large-image rate); chunk k+1 is gathered into pinned memory and
// uploaded on a copy stream while chunk k is searched on the context's stream, and payloads come back on a second copy stream:
//   host gather -> [h2d] pinIn -> devIn -> [ctx->stream] kernels -> devOut -> [d2h] pinOut -> host scatter
// with two lanes of buffers, so PCIe traffic in both directions overlaps the kernels (for BC1-BC5, where a 4096^2 image is
// 0.1-0.5 ms of kernel time and 1.6 ms of PCIe, it is the copies that overlap each other).
namespace
{
struct ManyChunk { size_t first, count; };

dxtex_hresult compress_many_pipelined(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, uint32_t flags, float threshold);
}

dxtex_hresult dxtex_compress_many(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, uint32_t flags, float threshold)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!srcs || !dsts || !count) return fail(ctx, DXTEX_E_INVALIDARG, "empty batch");
    ScopedDevice sd(ctx->device);
    const dxtex_hresult hr = compress_many_pipelined(ctx, srcs, dsts, count, flags, threshold);
    if (hr != DXTEX_S_OK)
    {
        // a failure in the middle leaves copies and kernels of earlier chunks in flight: let them finish before the caller may free
        // or reuse its images (the staging they touch belongs to the context)
        const std::string why = ctx->lastError;
        if (ctx->h2d) (void)hipStreamSynchronize(ctx->h2d);
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->d2h) (void)hipStreamSynchronize(ctx->d2h);
        ctx->lastError = why;
    }
    return hr;
}

namespace
{
dxtex_hresult compress_many_pipelined(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, uint32_t flags, float threshold)
{
    static const uint64_t chunkTexels = dev_env("DXTEX_MANY_CHUNK_TEXELS") ? std::max<uint64_t>(1, strtoull(dev_env("DXTEX_MANY_CHUNK_TEXELS"), nullptr, 10)) : (32ull << 20);
    std::vector<size_t> inBytes(count), outBytes(count);
    std::vector<ManyChunk> chunks;
    {
        ManyChunk cur = { 0, 0 };
        uint64_t texels = 0;
        for (size_t i = 0; i < count; ++i)
        {
            dxtex_hresult hr = check_pair(ctx, &srcs[i], &dsts[i]);
            if (hr == DXTEX_S_OK) { SrcView v; hr = compress_view(ctx, srcs[i], dsts[i].format, flags, &v); }
            if (hr == DXTEX_S_OK) hr = check_host_pitches(ctx, &srcs[i], &dsts[i], &inBytes[i], &outBytes[i]);
            if (hr != DXTEX_S_OK) return hr;
            const uint64_t t = uint64_t(srcs[i].width) * srcs[i].height;
            if (cur.count && texels + t > chunkTexels) { chunks.push_back(cur); cur = { i, 0 }; texels = 0; }
            ++cur.count; texels += t;
        }
        chunks.push_back(cur);
    }
    if (!ctx->h2d) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->h2d, hipStreamNonBlocking));
    if (!ctx->d2h) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->d2h, hipStreamNonBlocking));
    for (dxtex_ctx::Lane& l : ctx->lane)
    {
        if (!l.uploaded) HIP_TRY(ctx, hipEventCreateWithFlags(&l.uploaded, hipEventDisableTiming));
        if (!l.computed) HIP_TRY(ctx, hipEventCreateWithFlags(&l.computed, hipEventDisableTiming));
        if (!l.downloaded) HIP_TRY(ctx, hipEventCreateWithFlags(&l.downloaded, hipEventDisableTiming));
    }

    // payload of chunk c: pinned -> the caller's images (after its download has finished)
    auto scatter = [&](size_t c) -> dxtex_hresult
    {
        dxtex_ctx::Lane& l = ctx->lane[c & 1];
        HIP_TRY(ctx, hipEventSynchronize(l.downloaded));
        const Arena out(&outBytes[chunks[c].first], chunks[c].count);
        for (size_t k = 0; k < chunks[c].count; ++k)
            std::memcpy(dsts[chunks[c].first + k].pixels, l.pinOut.u8() + out.at[k], outBytes[chunks[c].first + k]);
        return DXTEX_S_OK;
    };

    std::vector<dxtex_image> ds, dd;
    for (size_t c = 0; c < chunks.size(); ++c)
    {
        const ManyChunk& ch = chunks[c];
        dxtex_ctx::Lane& l = ctx->lane[c & 1];
        if (c >= 2) { const dxtex_hresult hr = scatter(c - 2); if (hr != DXTEX_S_OK) return hr; }      // frees this lane's pinOut (and, stream-ordered, devOut)
        const Arena in(&inBytes[ch.first], ch.count), out(&outBytes[ch.first], ch.count);
        dxtex_hresult hr = l.pinIn.grow(ctx, in.total); if (hr != DXTEX_S_OK) return hr;
        hr = l.pinOut.grow(ctx, out.total); if (hr != DXTEX_S_OK) return hr;
        hr = l.devIn.grow(ctx, in.total); if (hr != DXTEX_S_OK) return hr;
        hr = l.devOut.grow(ctx, out.total); if (hr != DXTEX_S_OK) return hr;
        // gather (pinIn of this lane was last read by the upload of chunk c - 2, which the kernels of c - 2 waited for, which the download
        // of c - 2 waited for, which scatter(c - 2) has just waited for)
        ds.assign(srcs + ch.first, srcs + ch.first + ch.count);
        dd.assign(dsts + ch.first, dsts + ch.first + ch.count);
        for (size_t k = 0; k < ch.count; ++k)
        {
            std::memcpy(l.pinIn.u8() + in.at[k], srcs[ch.first + k].pixels, inBytes[ch.first + k]);
            ds[k].pixels = l.devIn.u8() + in.at[k];
            dd[k].pixels = l.devOut.u8() + out.at[k];
        }
        HIP_TRY(ctx, counted_copy(ctx, l.devIn.p, l.pinIn.p, in.total, hipMemcpyHostToDevice, ctx->h2d));
        HIP_TRY(ctx, hipEventRecord(l.uploaded, ctx->h2d));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, l.uploaded, 0));
        hr = dxtex_compress_many_device(ctx, ds.data(), dd.data(), ch.count, flags, threshold);
        if (hr != DXTEX_S_OK) return hr;
        HIP_TRY(ctx, hipEventRecord(l.computed, ctx->stream));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->d2h, l.computed, 0));
        HIP_TRY(ctx, counted_copy(ctx, l.pinOut.p, l.devOut.p, out.total, hipMemcpyDeviceToHost, ctx->d2h));
        HIP_TRY(ctx, hipEventRecord(l.downloaded, ctx->d2h));
        // (no wait of h2d on `computed`: the next upload into this lane's devIn belongs to chunk c + 2, and iteration c + 2 begins with
        // scatter(c), a host wait for downloaded(c), which is stream-ordered after computed(c). The upload of chunk c + 1 - the other
        // lane - therefore runs while these kernels do.)
    }
    for (size_t c = chunks.size() >= 2 ? chunks.size() - 2 : 0; c < chunks.size(); ++c)
    {
        const dxtex_hresult hr = scatter(c);
        if (hr != DXTEX_S_OK) return hr;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DXTEX_S_OK;
}
}

dxtex_hresult dxtex_compress(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags, float threshold)
{
    dxtex_hresult hr = check_pair(ctx, src, dst);
    if (hr != DXTEX_S_OK) return hr;
    { SrcView v; hr = compress_view(ctx, *src, dst->format, flags, &v); if (hr != DXTEX_S_OK) return hr; }
    return run_host_twin(ctx, src, dst, [&](const dxtex_image& s, const dxtex_image& d) { return submit_compress(ctx, s, d, flags, threshold); });
}

dxtex_hresult dxtex_encode_blocks(dxtex_ctx* ctx, int32_t bc_format, uint32_t bc_flags, float threshold,
                                  const float* rgba, size_t nblocks, uint8_t* bc)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!rgba || !bc) return fail(ctx, DXTEX_E_POINTER, "null buffer");
    const size_t bb = bc_block_bytes(bc_format);
    if (!bb) return fail(ctx, DXTEX_E_INVALIDARG, "not a BC format");
    if (!nblocks) return DXTEX_S_OK;
    // nblocks tiles of 16 x float4 == an R32G32B32A32_FLOAT image 4 texels wide and 4*nblocks high.
    return run_staged(ctx, rgba, nblocks * 256, bc, nblocks * bb, [&](uint8_t* in, uint8_t* out)
    {
        SrcView v;
        v.pixels = in; v.width = 4; v.height = uint32_t(nblocks * 4);
        v.rowPitch = 64; v.format = FMT_R32G32B32A32_FLOAT; v.tcv = TCV_NONE; v.tsw = TSW_NONE;   // raw floats, as BC_ENCODE receives them
        return encode(ctx, v, out, bb, bc_format, bc_flags, threshold);
    });
}

// DecompressBC (DirectXTexCompress.cpp:425-535): BC image -> uncompressed image of the same size, on device pointers.
static dxtex_hresult submit_decompress(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst)
{
    const FmtInfo* in = format_info(src.format);
    const FmtInfo* out = format_info(dst.format);
    if (!in || !(in->cls & FC_BC)) return fail(ctx, DXTEX_E_INVALIDARG, "source image is not block compressed");
    if (out && (out->cls & FC_BC)) return fail(ctx, DXTEX_E_INVALIDARG, "destination format is block compressed");
    if (!out || (out->cls & FC_GROUP)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "destination format is not supported by the MI355X path");
    if (!src.width || !src.height) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    return launched(ctx, launch_bc_decode(view_of(src), view_of(dst), resolve_convert_plan(*in, *out, 0), ctx->stream));
}

dxtex_hresult dxtex_decompress_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst)
{
    dxtex_hresult hr = check_pair(ctx, src, dst);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_decompress(ctx, *src, *dst); });
}

dxtex_hresult dxtex_decompress(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst)
{
    dxtex_hresult hr = check_pair(ctx, src, dst);
    if (hr != DXTEX_S_OK) return hr;
    const auto submit = [&](const dxtex_image& s, const dxtex_image& d) { return submit_decompress(ctx, s, d); };
    if (format_info(src->format) && format_info(dst->format)) return run_host_twin(ctx, src, dst, submit);
    // a format without a minimum pitch to check: staged as its pitches say, and submit_decompress rejects it
    return run_staged_images(ctx, src, src->rowPitch * std::max<size_t>(1, (src->height + 3) / 4), dst, dst->rowPitch * dst->height, submit);
}

dxtex_hresult dxtex_decode_blocks(dxtex_ctx* ctx, int32_t bc_format, const uint8_t* bc, size_t nblocks, float* rgba)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!rgba || !bc) return fail(ctx, DXTEX_E_POINTER, "null buffer");
    const size_t bb = bc_block_bytes(bc_format);
    if (!bb) return fail(ctx, DXTEX_E_INVALIDARG, "not a BC format");
    if (!nblocks) return DXTEX_S_OK;
    // nblocks blocks == a BC image 4 texels wide and 4*nblocks high; the raw decoder output is R32G32B32A32_FLOAT
    return run_staged(ctx, bc, nblocks * bb, rgba, nblocks * 256, [&](uint8_t* in, uint8_t* out)
    {
        ConvertPlan plan; plan.srgbIn = 0; plan.tcv = TCV_NONE; plan.tsw = TSW_NONE; plan.srgbOut = 0; plan.depth = 0;
        const uint32_t rows = uint32_t(nblocks * 4);
        return launched(ctx, launch_bc_decode({ in, bb, 4, rows, bc_format }, { out, 64, 4, rows, FMT_R32G32B32A32_FLOAT }, plan, ctx->stream));
    });
}
// ---- GenerateMipMaps / Resize / Convert ----------------------------------------------------------------------------------
namespace
{
constexpr uint32_t kFilterModeMask = 0xF00000u, kFilterDitherOrdered = 0x10000u, kFilterDitherDiffusion = 0x20000u;
inline bool ispow2(size_t x) { return x != 0 && (x & (x - 1)) == 0; }


// The triangle filter's gather lists of every axis of every level go to the device as one table image (ctx->triHost, then upload_tables).
// pack_triangle_axis appends one axis' lists (source -> dest texels) 16-byte aligned and returns where they start; the offsets become
// device pointers once the tables are uploaded.
struct TriAxis { size_t ofs, ent; };
TriAxis pack_triangle_axis(std::vector<uint8_t>& host, size_t source, size_t dest, bool wrap)
{
    std::vector<uint32_t> ofs; std::vector<TriEntry> ent;
    build_triangle_axis(source, dest, wrap, ofs, ent);
    auto append = [&](const void* p, size_t bytes) { const size_t at = (host.size() + 15) & ~size_t(15); host.resize(at + bytes); std::memcpy(host.data() + at, p, bytes); return at; };
    const size_t o = append(ofs.data(), ofs.size() * 4);
    return { o, append(ent.data(), std::max<size_t>(1, ent.size()) * 8) };
}
const uint32_t* tri_ofs(const uint8_t* tables, TriAxis a) { return reinterpret_cast<const uint32_t*>(tables + a.ofs); }

// The packed tables (ctx->triHost, plus 16 bytes of tail padding) go to the device through a pinned buffer of the context; an event marks
// when the last upload has been consumed, so an asynchronous (_device) call never rewrites host memory under a copy in flight.
dxtex_hresult upload_tables(dxtex_ctx* ctx)
{
    std::vector<uint8_t>& host = ctx->triHost;
    host.resize(host.size() + 16);
    dxtex_hresult hr = ctx->triBuf.grow(ctx, host.size()); if (hr != DXTEX_S_OK) return hr;
    if (ctx->triPending) { HIP_TRY(ctx, hipEventSynchronize(ctx->triConsumed)); ctx->triPending = false; }
    hr = ctx->triPinned.grow(ctx, host.size(), 1u << 16); if (hr != DXTEX_S_OK) return hr;
    if (!ctx->triConsumed) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->triConsumed, hipEventDisableTiming));
    std::memcpy(ctx->triPinned.p, host.data(), host.size());
    HIP_TRY(ctx, counted_copy(ctx, ctx->triBuf.p, ctx->triPinned.p, host.size(), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->triConsumed, ctx->stream));
    ctx->triPending = true;
    return DXTEX_S_OK;
}

// One level: src filtered into dst (through the float rows where dst's format is grouped).
dxtex_hresult submit_level(dxtex_ctx* ctx, const ImgView& src, const ImgView& dst, uint32_t mode, uint32_t flags, bool mipAlias,
                           const TriangleTables* tri, const ImgView* stale)
{
    KernelMarks* marks = marks_of(ctx);
    return launch_into(ctx, dst, marks, [&](const ImgView& out) { return launch_resize(src, out, mode, flags, mipAlias, tri, ctx->stream, stale, marks); });
}

// The triangle tables of every lv[i - 1] -> lv[i] in one upload; (*tables)[i - 1] are that level's.
dxtex_hresult upload_triangle_levels(dxtex_ctx* ctx, const ImgView* lv, size_t nlevels, uint32_t flags, std::vector<TriangleTables>* tables)
{
    ctx->triHost.clear();
    std::vector<TriAxis> x, y;
    for (size_t i = 1; i < nlevels; ++i)
    {
        x.push_back(pack_triangle_axis(ctx->triHost, lv[i - 1].width, lv[i].width, (flags & DXTEX_FILTER_WRAP_U) != 0));
        y.push_back(pack_triangle_axis(ctx->triHost, lv[i - 1].height, lv[i].height, (flags & DXTEX_FILTER_WRAP_V) != 0));
    }
    const dxtex_hresult hr = upload_tables(ctx); if (hr != DXTEX_S_OK) return hr;
    const uint8_t* d = ctx->triBuf.u8();
    for (size_t i = 0; i < x.size(); ++i) tables->push_back({ tri_ofs(d, x[i]), d + x[i].ent, tri_ofs(d, y[i]), d + y[i].ent });
    return DXTEX_S_OK;
}

// A mip chain on device-resident levels (lv[0] = the source): a launch per level until resize_tail_route() has a one-workgroup form for
// the rest of the chain.
dxtex_hresult submit_mips(dxtex_ctx* ctx, const std::vector<ImgView>& lv, uint32_t mode, uint32_t flags)
{
    std::vector<TriangleTables> tri;
    if (mode == DXTEX_FILTER_TRIANGLE)
    {
        const dxtex_hresult hr = upload_triangle_levels(ctx, lv.data(), lv.size(), flags, &tri); if (hr != DXTEX_S_OK) return hr;
    }
    StaleTap<ImgView> tap{};
    for (size_t i = 1; i < lv.size(); ++i)
    {
        const ImgView* rest = &lv[i - 1];
        const int nrest = int(lv.size() - (i - 1));
        if (resize_tail_route(rest, nrest, mode, flags) != TailRoute::None)
            return launched(ctx, launch_resize_tail(rest, nrest, mode, flags, tap.twoHigh.pixels ? &tap.twoHigh : nullptr, ctx->stream, marks_of(ctx)));
        const bool stale = tap.step(lv[i - 1], mode == DXTEX_FILTER_BOX);
        const dxtex_hresult hr = submit_level(ctx, lv[i - 1], lv[i], mode, flags, true, tri.empty() ? nullptr : &tri[i - 1], stale ? &tap.twoHigh : nullptr);
        if (hr != DXTEX_S_OK) return hr;
    }
    return DXTEX_S_OK;
}
std::vector<ImgView> views_of(const dxtex_image* levels, size_t nlevels)
{
    std::vector<ImgView> lv(nlevels);
    for (size_t i = 0; i < nlevels; ++i) lv[i] = view_of(levels[i]);
    return lv;
}

// GenerateMipMaps' checks and filter choice (DirectXTexMipmaps.cpp:2828-3017, non-WIC path)
dxtex_hresult check_mips(dxtex_ctx* ctx, const dxtex_image* levels, size_t nlevels, uint32_t filter, uint32_t* mode)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!levels || nlevels <= 1) return fail(ctx, DXTEX_E_INVALIDARG, "need at least two levels");
    const FmtInfo* f = format_info(levels[0].format);
    if (f && (f->cls & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "cannot filter a block-compressed image");
    if (!f) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "format is not supported by the MI355X path");
    size_t w = levels[0].width, h = levels[0].height;
    if (!w || !h) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    for (size_t i = 0; i < nlevels; ++i)
    {
        if (!levels[i].pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
        if (levels[i].width != w || levels[i].height != h || levels[i].format != levels[0].format)
            return fail(ctx, DXTEX_E_INVALIDARG, "levels do not form a mip chain");
        if (i + 1 < nlevels && w == 1 && h == 1) return fail(ctx, DXTEX_E_INVALIDARG, "too many levels");     // CalculateMipLevels
        w = std::max<size_t>(1, w >> 1); h = std::max<size_t>(1, h >> 1);
    }
    uint32_t m = filter & kFilterModeMask;
    if (!m) m = (ispow2(levels[0].width) && ispow2(levels[0].height)) ? DXTEX_FILTER_BOX : DXTEX_FILTER_LINEAR;
    if (m != DXTEX_FILTER_POINT && m != DXTEX_FILTER_LINEAR && m != DXTEX_FILTER_CUBIC && m != DXTEX_FILTER_BOX && m != DXTEX_FILTER_TRIANGLE)
        return fail(ctx, DXTEX_E_NOT_SUPPORTED, "unknown filter mode");
    if (m == DXTEX_FILTER_BOX && (!ispow2(levels[0].width) || !ispow2(levels[0].height)))
        return fail(ctx, DXTEX_E_FAIL, "the box filter needs power-of-two dimensions");                         // :1005
    *mode = m;
    return DXTEX_S_OK;
}
} // namespace

dxtex_hresult dxtex_generate_mips_device(dxtex_ctx* ctx, const dxtex_image* levels, size_t nlevels, uint32_t filter)
{
    uint32_t mode = 0;
    dxtex_hresult hr = check_mips(ctx, levels, nlevels, filter, &mode);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_mips(ctx, views_of(levels, nlevels), mode, filter); });
}

dxtex_hresult dxtex_generate_mips(dxtex_ctx* ctx, const dxtex_image* levels, size_t nlevels, uint32_t filter)
{
    uint32_t mode = 0;
    dxtex_hresult hr = check_mips(ctx, levels, nlevels, filter, &mode);
    if (hr != DXTEX_S_OK) return hr;
    // the whole chain in the input staging: level 0 goes up, the levels the kernels fill come down
    StagingPlan plan;
    std::vector<StagePart> part(nlevels);
    for (size_t i = 0; i < nlevels; ++i) part[i] = plan.in(levels[i].rowPitch, levels[i].height);
    plan.upload(levels[0].pixels, part[0], part[0].bytes);
    for (size_t i = 1; i < nlevels; ++i) plan.download(levels[i].pixels, part[i], part[i].bytes);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t*)
    {
        std::vector<ImgView> lv = views_of(levels, nlevels);
        for (size_t i = 0; i < nlevels; ++i) lv[i].pixels = in + part[i].at;
        return submit_mips(ctx, lv, mode, filter);
    });
}

namespace
{
// GenerateMipMaps3D's checks and filter choice (DirectXTexMipmaps.cpp:3254-3305)
dxtex_hresult check_mips3d(dxtex_ctx* ctx, const dxtex_volume* levels, size_t nlevels, uint32_t filter, uint32_t* mode)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!levels || nlevels <= 1) return fail(ctx, DXTEX_E_INVALIDARG, "need at least two levels");
    const FmtInfo* f = format_info(levels[0].format);
    if (f && (f->cls & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "cannot filter a block-compressed volume");
    if (!f || (f->cls & FC_GROUP)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "format is not supported by the MI355X path");
    size_t w = levels[0].width, h = levels[0].height, d = levels[0].depth;
    if (!w || !h || !d || d > 32767) return fail(ctx, DXTEX_E_INVALIDARG, "bad volume dimensions");           // depth > INT16_MAX, :3264
    if (filter & TF_FORCE_WIC) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "TEX_FILTER_FORCE_WIC");
    for (size_t i = 0; i < nlevels; ++i)
    {
        if (!levels[i].pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
        if (levels[i].width != w || levels[i].height != h || levels[i].depth != d || levels[i].format != levels[0].format)
            return fail(ctx, DXTEX_E_INVALIDARG, "levels do not form a volume mip chain");
        if (i + 1 < nlevels && w == 1 && h == 1 && d == 1) return fail(ctx, DXTEX_E_INVALIDARG, "too many levels");     // CalculateMipLevels3D
        w = std::max<size_t>(1, w >> 1); h = std::max<size_t>(1, h >> 1); d = std::max<size_t>(1, d >> 1);
    }
    const bool pow2 = ispow2(levels[0].width) && ispow2(levels[0].height) && ispow2(levels[0].depth);
    uint32_t m = filter & kFilterModeMask;
    if (!m) m = pow2 ? DXTEX_FILTER_BOX : DXTEX_FILTER_TRIANGLE;
    if (m != DXTEX_FILTER_POINT && m != DXTEX_FILTER_LINEAR && m != DXTEX_FILTER_CUBIC && m != DXTEX_FILTER_BOX && m != DXTEX_FILTER_TRIANGLE)
        return fail(ctx, DXTEX_E_NOT_SUPPORTED, "unknown filter mode");
    if (m == DXTEX_FILTER_BOX && !pow2) return fail(ctx, DXTEX_E_FAIL, "the box filter needs power-of-two dimensions");   // :1831-1832
    *mode = m;
    return DXTEX_S_OK;
}

// The level loop of Generate3DMips*Filter on device-resident levels: 3-D kernels while the source is more than one slice deep,
// then the reference's 2-D branches (the kernels GenerateMipMaps uses) - except the triangle filter, which has no 2-D branch.
dxtex_hresult submit_mips3d(dxtex_ctx* ctx, const std::vector<VolumeView>& lv, uint32_t mode, uint32_t flags)
{
    std::vector<TriAxis> x(lv.size()), y(lv.size()), z(lv.size());      // [i]: level i - 1 -> level i
    const uint8_t* tri = nullptr;
    if (mode == DXTEX_FILTER_TRIANGLE)
    {
        ctx->triHost.clear();
        for (size_t i = 1; i < lv.size(); ++i)
        {
            x[i] = pack_triangle_axis(ctx->triHost, lv[i - 1].width, lv[i].width, (flags & DXTEX_FILTER_WRAP_U) != 0);
            y[i] = pack_triangle_axis(ctx->triHost, lv[i - 1].height, lv[i].height, (flags & DXTEX_FILTER_WRAP_V) != 0);
            z[i] = pack_triangle_axis(ctx->triHost, lv[i - 1].depth, lv[i].depth, (flags & TF_WRAP_W) != 0);
        }
        dxtex_hresult hr = upload_tables(ctx); if (hr != DXTEX_S_OK) return hr;
        tri = ctx->triBuf.u8();
    }
    KernelMarks* marks = marks_of(ctx);
    StaleTap<VolumeView> tap{};
    for (size_t i = 1; i < lv.size(); ++i)
    {
        const VolumeView& s = lv[i - 1]; const VolumeView& d = lv[i];
        const bool stale = tap.step(s, mode == DXTEX_FILTER_BOX);
        // row 1 of the last slice pair loaded into urow1 / vrow1 at that level: slices depth-2 and depth-1 (a one-slice level only has urow1)
        ImgView staleU{}, staleV{};
        if (stale) { staleU = slice_of(tap.twoHigh, tap.twoHigh.depth >= 2 ? tap.twoHigh.depth - 2 : 0); staleV = slice_of(tap.twoHigh, tap.twoHigh.depth - 1); }
        hipError_t e;
        if (s.depth > 1 || mode == DXTEX_FILTER_TRIANGLE)
        {
            TriangleTables3 t{};
            if (tri) t = { tri_ofs(tri, x[i]), tri + x[i].ent, tri_ofs(tri, y[i]), tri + y[i].ent, tri_ofs(tri, z[i]), tri + z[i].ent };
            e = launch_resize3d(s, d, mode, flags, tri ? &t : nullptr, ctx->stream, stale ? &staleU : nullptr, stale ? &staleV : nullptr, marks);
        }
        else
            e = launch_resize(slice_of(s, 0), slice_of(d, 0), mode, flags, true, nullptr, ctx->stream, stale ? &staleU : nullptr, marks);
        const dxtex_hresult hr = launched(ctx, e);
        if (hr != DXTEX_S_OK) return hr;
    }
    return DXTEX_S_OK;
}

VolumeView view_of(const dxtex_volume& v, uint8_t* pixels)
{
    VolumeView o; o.pixels = pixels; o.rowPitch = v.rowPitch; o.slicePitch = v.slicePitch;
    o.width = uint32_t(v.width); o.height = uint32_t(v.height); o.depth = uint32_t(v.depth); o.format = v.format;
    return o;
}
} // namespace

dxtex_hresult dxtex_generate_mips3d_device(dxtex_ctx* ctx, const dxtex_volume* levels, size_t nlevels, uint32_t filter)
{
    uint32_t mode = 0;
    dxtex_hresult hr = check_mips3d(ctx, levels, nlevels, filter, &mode);
    if (hr != DXTEX_S_OK) return hr;
    std::vector<VolumeView> lv(nlevels);
    for (size_t i = 0; i < nlevels; ++i) lv[i] = view_of(levels[i], levels[i].pixels);
    return run_timed(ctx, [&] { return submit_mips3d(ctx, lv, mode, filter); });
}

dxtex_hresult dxtex_generate_mips3d(dxtex_ctx* ctx, const dxtex_volume* levels, size_t nlevels, uint32_t filter)
{
    uint32_t mode = 0;
    dxtex_hresult hr = check_mips3d(ctx, levels, nlevels, filter, &mode);
    if (hr != DXTEX_S_OK) return hr;
    StagingPlan plan;       // as dxtex_generate_mips
    std::vector<StagePart> part(nlevels);
    for (size_t i = 0; i < nlevels; ++i) part[i] = plan.in(levels[i].slicePitch, levels[i].depth);
    plan.upload(levels[0].pixels, part[0], part[0].bytes);
    for (size_t i = 1; i < nlevels; ++i) plan.download(levels[i].pixels, part[i], part[i].bytes);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t*)
    {
        std::vector<VolumeView> lv(nlevels);
        for (size_t i = 0; i < nlevels; ++i) lv[i] = view_of(levels[i], in + part[i].at);
        return submit_mips3d(ctx, lv, mode, filter);
    });
}

namespace
{
// Resize's checks and filter choice (DirectXTexResize.cpp:807-843, :854-930)
dxtex_hresult check_resize(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, uint32_t* mode)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    if (!dst->width || !dst->height || !src->width || !src->height) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    if (src->width > 0xFFFFFFFFull || src->height > 0xFFFFFFFFull || dst->width > 0xFFFFFFFFull || dst->height > 0xFFFFFFFFull)
        return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    if (!src->pixels || !dst->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    const FmtInfo* f = format_info(src->format);
    if (f && (f->cls & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "cannot resize a block-compressed image");
    if (!f) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "format is not supported by the MI355X path");
    if (src->format != dst->format) return fail(ctx, DXTEX_E_INVALIDARG, "Resize keeps the format");
    uint32_t m = filter & kFilterModeMask;
    const bool half = ((dst->width << 1) == src->width) && ((dst->height << 1) == src->height);
    if (!m) m = half ? DXTEX_FILTER_BOX : DXTEX_FILTER_LINEAR;
    if (m != DXTEX_FILTER_POINT && m != DXTEX_FILTER_LINEAR && m != DXTEX_FILTER_CUBIC && m != DXTEX_FILTER_BOX && m != DXTEX_FILTER_TRIANGLE)
        return fail(ctx, DXTEX_E_NOT_SUPPORTED, "unknown filter mode");
    if (m == DXTEX_FILTER_BOX && !half) return fail(ctx, DXTEX_E_FAIL, "the box filter needs an exact 2:1 reduction");   // :319-320
    *mode = m;
    return DXTEX_S_OK;
}

// Resize of one image: no mip aliasing, never the tail
dxtex_hresult submit_resize(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst, uint32_t mode, uint32_t filter)
{
    const ImgView lv[2] = { view_of(src), view_of(dst) };
    std::vector<TriangleTables> tri;
    if (mode == DXTEX_FILTER_TRIANGLE)
    {
        const dxtex_hresult hr = upload_triangle_levels(ctx, lv, 2, filter, &tri); if (hr != DXTEX_S_OK) return hr;
    }
    return submit_level(ctx, lv[0], lv[1], mode, filter, false, tri.empty() ? nullptr : &tri[0], nullptr);
}
} // namespace

dxtex_hresult dxtex_resize_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter)
{
    uint32_t mode = 0;
    dxtex_hresult hr = check_resize(ctx, src, dst, filter, &mode);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_resize(ctx, *src, *dst, mode, filter); });
}

dxtex_hresult dxtex_resize(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter)
{
    uint32_t mode = 0;
    dxtex_hresult hr = check_resize(ctx, src, dst, filter, &mode);
    if (hr != DXTEX_S_OK) return hr;
    return run_host_twin(ctx, src, dst, [&](const dxtex_image& s, const dxtex_image& d) { return submit_resize(ctx, s, d, mode, filter); });
}

namespace
{
// ConvertEx's checks (DirectXTexConvert.cpp:5107-5125)
dxtex_hresult check_convert(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, ConvertPlan* plan)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    if (src->format == dst->format) return fail(ctx, DXTEX_E_INVALIDARG, "source and destination formats are the same");
    if (!src->pixels || !dst->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    const FmtInfo* in = format_info(src->format);
    const FmtInfo* out = format_info(dst->format);
    if ((in && (in->cls & FC_BC)) || (out && (out->cls & FC_BC))) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "Convert does not take block-compressed formats");
    if (!in || !out) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "format is not supported by the MI355X path");
    if (src->width != dst->width || src->height != dst->height) return fail(ctx, DXTEX_E_FAIL, "size mismatch");
    *plan = resolve_convert_plan(*in, *out, filter);
    return DXTEX_S_OK;
}

// development knob (libdxtex_amd_dev.so only): texels per speculated segment of the error-diffusion kernel; 0 = its default
static const uint32_t kDitherSegment = dev_env("DXTEX_DITHER_SEGMENT") ? uint32_t(strtoul(dev_env("DXTEX_DITHER_SEGMENT"), nullptr, 10)) : 0u;

// the conversion kernel, through float rows + the pack kernel when the destination's element holds several texels. ConvertCustom's
// branches (:4820-4910): TEX_FILTER_DITHER_DIFFUSION first, then TEX_FILTER_DITHER; z is the slice of a volume (ordered dithering's phase).
dxtex_hresult submit_convert(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst, const ConvertPlan& basePlan, float threshold,
                             uint32_t filter, uint32_t z)
{
    const ImgView sv = view_of(src);
    int dither = CONVERT_DITHER_NONE;
    ConvertPlan plan = basePlan;
    if ((filter & (kFilterDitherDiffusion | kFilterDitherOrdered)) && dither_spec(dst.format).valid)
    {
        // a dithered store sees ConvertScanline's NaNs as they are (XMVectorClamp keeps them)
        if (plan.tcv == TCV_CLAMP_SNORM) plan.tcv = TCV_CLAMP_SNORM_NAN;
        else if (plan.tcv == TCV_X2BIAS_TO_UNORM) plan.tcv = TCV_X2BIAS_TO_UNORM_NAN;
    }
    if (filter & kFilterDitherDiffusion)
    {
        if (dither_spec(dst.format).valid)
        {
            dxtex_hresult hr = ctx->ditherRows.grow(ctx, convert_diffuse_scratch_bytes(sv.width));
            if (hr != DXTEX_S_OK) return hr;
            if (!ctx->ditherRerun.p)
            {
                hr = ctx->ditherRerun.grow(ctx, sizeof(unsigned long long), sizeof(unsigned long long)); if (hr != DXTEX_S_OK) return hr;
                HIP_TRY(ctx, hipMemsetAsync(ctx->ditherRerun.p, 0, sizeof(unsigned long long), ctx->stream));
            }
            ctx->ditherTexels += uint64_t(src.width) * src.height;
            return launched(ctx, launch_convert_diffuse(sv, view_of(dst), plan, threshold, ctx->ditherRows.p, static_cast<unsigned long long*>(ctx->ditherRerun.p),
                                                        kDitherSegment, ctx->stream));
        }
        dither = CONVERT_DITHER_ZERO_ERROR;      // no dithered store: StoreScanline after the zero error row
    }
    else if (filter & kFilterDitherOrdered) dither = CONVERT_DITHER_ORDERED;
    KernelMarks* marks = marks_of(ctx);
    return launch_into(ctx, view_of(dst), marks, [&](const ImgView& out) { return launch_convert(sv, out, plan, threshold, ctx->stream, dither, z, marks); });
}
} // namespace

dxtex_hresult dxtex_convert_slice_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, float threshold, uint32_t z)
{
    ConvertPlan plan;
    dxtex_hresult hr = check_convert(ctx, src, dst, filter, &plan);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_convert(ctx, *src, *dst, plan, threshold, filter, z); });
}

dxtex_hresult dxtex_convert_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, float threshold)
{
    return dxtex_convert_slice_device(ctx, src, dst, filter, threshold, 0);
}

dxtex_hresult dxtex_convert(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, float threshold)
{
    return dxtex_convert_slice(ctx, src, dst, filter, threshold, 0);
}

dxtex_hresult dxtex_convert_dither_stats(dxtex_ctx* ctx, uint64_t* rerunTexels, uint64_t* texels)
{
    if (!ctx || !rerunTexels || !texels) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    unsigned long long n = 0;
    if (ctx->ditherRerun.p)
    {
        HIP_TRY(ctx, counted_copy(ctx, &n, ctx->ditherRerun.p, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    *rerunTexels = n; *texels = ctx->ditherTexels;
    return DXTEX_S_OK;
}

dxtex_hresult dxtex_convert_slice(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, float threshold, uint32_t z)
{
    ConvertPlan plan;
    dxtex_hresult hr = check_convert(ctx, src, dst, filter, &plan);
    if (hr != DXTEX_S_OK) return hr;
    return run_host_twin(ctx, src, dst, [&](const dxtex_image& s, const dxtex_image& d) { return submit_convert(ctx, s, d, plan, threshold, filter, z); });
}

namespace
{
// E_INVALIDARG where the bytes of src's rows and dst's rows intersect (images of a non-zero size)
dxtex_hresult check_no_overlap(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst)
{
    size_t srcRow = 0, srcSlice = 0, dstRow = 0, dstSlice = 0;
    if (dxtex_compute_pitch(src.format, src.width, src.height, &srcRow, &srcSlice) != DXTEX_S_OK ||
        dxtex_compute_pitch(dst.format, dst.width, dst.height, &dstRow, &dstSlice) != DXTEX_S_OK)
        return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src.pixels), d0 = reinterpret_cast<uintptr_t>(dst.pixels);
    const uintptr_t s1 = s0 + src.rowPitch * (srcSlice / std::max<size_t>(1, srcRow) - 1) + srcRow;
    const uintptr_t d1 = d0 + dst.rowPitch * (dstSlice / std::max<size_t>(1, dstRow) - 1) + dstRow;
    if (s0 < d1 && d0 < s1) return fail(ctx, DXTEX_E_INVALIDARG, "source and destination pixels overlap");
    return DXTEX_S_OK;
}

// ComputeNormalMap's checks (DirectXTexNormalMaps.cpp:257-283, ComputeNMap :83-94), in its order; the destination's class decides the
// encoding. Formats format_info() does not know (GetConvertFlags has no entry for any of them) are not supported here.
dxtex_hresult check_normal_map(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags, bool* unorm)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    if (!src->pixels || !dst->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    const auto valid = [](int f) { return f >= 1 && f <= 191; };
    if (!valid(src->format) || !valid(dst->format)) return fail(ctx, DXTEX_E_INVALIDARG, "invalid format");
    if ((flags & NMAP_CHANNEL_MASK) > NMAP_CHANNEL_LUMINANCE) return fail(ctx, DXTEX_E_INVALIDARG, "invalid channel selector");
    const FmtInfo* in = format_info(src->format);
    const FmtInfo* out = format_info(dst->format);
    if (!in || !out || ((in->cls | out->cls) & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "format is not supported by ComputeNormalMap");
    if (!(out->cls & (FC_UNORM | FC_SNORM | FC_FLOAT))) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "destination is not a UNORM, SNORM or FLOAT format");
    if (src->width != dst->width || src->height != dst->height) return fail(ctx, DXTEX_E_FAIL, "size mismatch");
    if (!src->width || !src->height) return DXTEX_S_OK;
    // the stencil reads rows above and below the one it writes: it cannot run in place
    const dxtex_hresult hr = check_no_overlap(ctx, *src, *dst);
    if (hr != DXTEX_S_OK) return hr;
    *unorm = (out->cls & FC_UNORM) != 0;
    return DXTEX_S_OK;
}

// the normal-map kernel, through float rows + the pack kernel when the destination's element holds several texels
dxtex_hresult submit_normal_map(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst, uint32_t flags, float amplitude, bool unorm)
{
    // (launch_normal_map records no kernel names, and so neither does the pack that follows it)
    return launch_into(ctx, view_of(dst), nullptr, [&](const ImgView& out) { return launch_normal_map(view_of(src), out, flags, amplitude, unorm, ctx->stream); });
}
} // namespace

dxtex_hresult dxtex_compute_normal_map_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags, float amplitude)
{
    bool unorm = false;
    const dxtex_hresult hr = check_normal_map(ctx, src, dst, flags, &unorm);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_normal_map(ctx, *src, *dst, flags, amplitude, unorm); });
}

dxtex_hresult dxtex_compute_normal_map(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags, float amplitude)
{
    bool unorm = false;
    dxtex_hresult hr = check_normal_map(ctx, src, dst, flags, &unorm);
    if (hr != DXTEX_S_OK) return hr;
    return run_host_twin(ctx, src, dst, [&](const dxtex_image& s, const dxtex_image& d) { return submit_normal_map(ctx, s, d, flags, amplitude, unorm); });
}

namespace
{
// TransformImage's checks (DirectXTexMisc.cpp:606-700), in its order, over `count` source / destination pairs of one format; resolves what
// the kernel needs of the descriptor. Formats format_info() does not know are not supported.
dxtex_hresult check_transform(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, const dxtex_transform* t, XformArgs* args)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!t) return fail(ctx, DXTEX_E_POINTER, "null transform");
    if (!srcs || !dsts || !count) return fail(ctx, DXTEX_E_INVALIDARG, "no images");
    if (t->op > DXTEX_TRANSFORM_RECONSTRUCT_Z) return fail(ctx, DXTEX_E_INVALIDARG, "unknown transform op");
    const int format = srcs[0].format;
    const FmtInfo* f = format_info(format);
    if (!f || (f->cls & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "TransformImage does not take planar, palettised, compressed or typeless formats");
    for (size_t i = 0; i < count; ++i)
    {
        const dxtex_image& s = srcs[i];
        const dxtex_image& d = dsts[i];
        if (s.width > 0xFFFFFFFFull || s.height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
        if (s.format != format || d.format != format) return fail(ctx, DXTEX_E_FAIL, "format mismatch");
        if (s.width != d.width || s.height != d.height) return fail(ctx, DXTEX_E_FAIL, "size mismatch");
        if (!s.pixels || !d.pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
        if (s.width && s.height) { const dxtex_hresult hr = check_no_overlap(ctx, s, d); if (hr != DXTEX_S_OK) return hr; }
    }
    XformArgs a = {};
    for (int k = 0; k < 4; ++k)
    {
        if (t->op == DXTEX_TRANSFORM_SWIZZLE && t->swizzle[k] > 3) return fail(ctx, DXTEX_E_INVALIDARG, "swizzle index above 3");
        a.swz[k] = t->swizzle[k] & 3u;
        if (t->zero[k]) a.zero |= 1u << k;
        if (t->one[k]) a.one |= 1u << k;
    }
    xf_color_key_value(t->colorKey & 0xFFFFFFu, a.key);
    // FormatDataType (DirectXTexConvert.cpp:5529-5553): the convert-type bits are exactly UNORM
    a.unorm = (f->cls & (FC_UNORM | FC_SNORM | FC_FLOAT | FC_UINT | FC_SINT)) == FC_UNORM;
    *args = a;
    return DXTEX_S_OK;
}

// the transform of `count` images on the stream; for TONEMAP every source is reduced into the context's result word before the first
// destination is written, and the apply kernels read it there
dxtex_hresult submit_transform(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, uint32_t op, const XformArgs& args)
{
    KernelMarks* marks = marks_of(ctx);
    uint32_t* maxBits = nullptr;
    if (op == DXTEX_TRANSFORM_TONEMAP)
    {
        const dxtex_hresult hr = ctx->resultCell.grow(ctx, 4 * sizeof(double)); if (hr != DXTEX_S_OK) return hr;
        maxBits = static_cast<uint32_t*>(ctx->resultCell.p);
        HIP_TRY(ctx, hipMemsetAsync(maxBits, 0, sizeof(uint32_t), ctx->stream));
        for (size_t i = 0; i < count; ++i)
        {
            const dxtex_hresult hr1 = launched(ctx, launch_tonemap_max(view_of(srcs[i]), maxBits, ctx->stream, marks));
            if (hr1 != DXTEX_S_OK) return hr1;
        }
    }
    for (size_t i = 0; i < count; ++i)
    {
        if (!srcs[i].width || !srcs[i].height) continue;
        const ImgView sv = view_of(srcs[i]);
        const dxtex_hresult hr = launch_into(ctx, view_of(dsts[i]), marks, [&](const ImgView& out) { return launch_transform(sv, out, op, args, maxBits, ctx->stream, marks); });
        if (hr != DXTEX_S_OK) return hr;
    }
    return DXTEX_S_OK;
}
} // namespace

dxtex_hresult dxtex_transform_images_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, const dxtex_transform* t)
{
    XformArgs args;
    const dxtex_hresult hr = check_transform(ctx, srcs, dsts, count, t, &args);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_transform(ctx, srcs, dsts, count, t->op, args); });
}

dxtex_hresult dxtex_transform_image(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, const dxtex_transform* t)
{
    XformArgs args;
    dxtex_hresult hr = check_transform(ctx, src, dst, src && dst ? 1 : 0, t, &args);
    if (hr != DXTEX_S_OK) return hr;
    return run_host_twin(ctx, src, dst, [&](const dxtex_image& s, const dxtex_image& d) { return submit_transform(ctx, &s, &d, 1, t->op, args); });
}

namespace
{
// The colour rotation's checks over `count` source / destination pairs of one format: TransformImage's (check_transform), with texconv's
// own rules for the operation and the paper-white level (texconv.cpp:1545-1553, :1891-1903); resolves the matrix and the curve.
dxtex_hresult check_rotate_color(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, uint32_t rotate, float nits,
                                 RotateArgs* args, int* curve)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!srcs || !dsts || !count) return fail(ctx, DXTEX_E_INVALIDARG, "no images");
    const int format = srcs[0].format;
    const FmtInfo* f = format_info(format);
    if (!f || (f->cls & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "the colour rotation does not take planar, palettised, compressed or typeless formats");
    if (!rotate_resolve(rotate, nits, *args, *curve)) return fail(ctx, DXTEX_E_INVALIDARG, "unknown colour rotation");
    if (!rotate_nits_valid(nits)) return fail(ctx, DXTEX_E_INVALIDARG, "the paper-white level must be above 0 and at most 10000 nits");
    for (size_t i = 0; i < count; ++i)
    {
        const dxtex_image& s = srcs[i];
        const dxtex_image& d = dsts[i];
        if (s.width > 0xFFFFFFFFull || s.height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
        if (s.format != format || d.format != format) return fail(ctx, DXTEX_E_FAIL, "format mismatch");
        if (s.width != d.width || s.height != d.height) return fail(ctx, DXTEX_E_FAIL, "size mismatch");
        if (!s.pixels || !d.pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
        if (s.width && s.height) { const dxtex_hresult hr = check_no_overlap(ctx, s, d); if (hr != DXTEX_S_OK) return hr; }
    }
    return DXTEX_S_OK;
}

dxtex_hresult submit_rotate_color(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, int curve, const RotateArgs& args)
{
    KernelMarks* marks = marks_of(ctx);
    for (size_t i = 0; i < count; ++i)
    {
        if (!srcs[i].width || !srcs[i].height) continue;
        const ImgView sv = view_of(srcs[i]);
        const dxtex_hresult hr = launch_into(ctx, view_of(dsts[i]), marks, [&](const ImgView& out) { return launch_rotate_color(sv, out, curve, args, ctx->stream, marks); });
        if (hr != DXTEX_S_OK) return hr;
    }
    return DXTEX_S_OK;
}
} // namespace

dxtex_hresult dxtex_rotate_color_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, uint32_t rotate, float paperWhiteNits)
{
    RotateArgs args;
    int curve = 0;
    const dxtex_hresult hr = check_rotate_color(ctx, srcs, dsts, count, rotate, paperWhiteNits, &args, &curve);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_rotate_color(ctx, srcs, dsts, count, curve, args); });
}

dxtex_hresult dxtex_rotate_color(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t rotate, float paperWhiteNits)
{
    RotateArgs args;
    int curve = 0;
    const dxtex_hresult hr = check_rotate_color(ctx, src, dst, src && dst ? 1 : 0, rotate, paperWhiteNits, &args, &curve);
    if (hr != DXTEX_S_OK) return hr;
    return run_host_twin(ctx, src, dst, [&](const dxtex_image& s, const dxtex_image& d) { return submit_rotate_color(ctx, &s, &d, 1, curve, args); });
}

namespace
{
// The checks of the RGBE pair, in the order include/dxtex_amd.h states. `rgbe` is the R8G8B8A8_UINT side, `flt` the float side.
dxtex_hresult check_rgbe(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, bool decode, float exposure)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !dst) return fail(ctx, DXTEX_E_POINTER, "null image");
    if (!src->pixels || !dst->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    const dxtex_image& rgbe = decode ? *src : *dst;
    const dxtex_image& flt = decode ? *dst : *src;
    const size_t floatBytes = rgbe_source_bytes(flt.format);
    if (rgbe.format != FMT_R8G8B8A8_UINT || !(decode ? flt.format == FMT_R32G32B32A32_FLOAT : floatBytes != 0))
        return fail(ctx, DXTEX_E_NOT_SUPPORTED, decode ? "RGBE decode is R8G8B8A8_UINT to R32G32B32A32_FLOAT" : "RGBE encode is R32G32B32A32_FLOAT, R32G32B32_FLOAT or R16G16B16A16_FLOAT to R8G8B8A8_UINT");
    if (src->width != dst->width || src->height != dst->height) return fail(ctx, DXTEX_E_FAIL, "size mismatch");
    if (src->width > 0xFFFFFFFFull || src->height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    if (rgbe.rowPitch < rgbe.width * 4u || flt.rowPitch < flt.width * floatBytes) return fail(ctx, DXTEX_E_INVALIDARG, "rowPitch is smaller than the row");
    if (src->width && src->height) { const dxtex_hresult hr = check_no_overlap(ctx, *src, *dst); if (hr != DXTEX_S_OK) return hr; }
    if (decode && !(exposure > 0.0f && exposure <= 3.402823466e+38f)) return fail(ctx, DXTEX_E_INVALIDARG, "the exposure must be a finite positive number");
    return DXTEX_S_OK;
}

dxtex_hresult submit_rgbe(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst, bool decode, float exposure)
{
    if (decode) return launched(ctx, launch_rgbe_decode(view_of(src), view_of(dst), 1.0f / exposure, ctx->stream, marks_of(ctx)));
    return launched(ctx, launch_rgbe_encode(view_of(src), view_of(dst), ctx->stream, marks_of(ctx)));
}

// The RGBE pairs, one body: `device` runs the kernel on the caller's device images, else the host images go through the staging
dxtex_hresult rgbe(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, bool decode, float exposure, bool device)
{
    const dxtex_hresult hr = check_rgbe(ctx, src, dst, decode, exposure);
    if (hr != DXTEX_S_OK) return hr;
    if (device) return run_timed(ctx, [&] { return submit_rgbe(ctx, *src, *dst, decode, exposure); });
    return run_host_twin(ctx, src, dst, [&](const dxtex_image& s, const dxtex_image& d) { return submit_rgbe(ctx, s, d, decode, exposure); });
}
} // namespace

dxtex_hresult dxtex_rgbe_decode_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, float exposure) { return rgbe(ctx, src, dst, true, exposure, true); }
dxtex_hresult dxtex_rgbe_decode(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, float exposure) { return rgbe(ctx, src, dst, true, exposure, false); }
dxtex_hresult dxtex_rgbe_encode_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst) { return rgbe(ctx, src, dst, false, 1.0f, true); }
dxtex_hresult dxtex_rgbe_encode(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst) { return rgbe(ctx, src, dst, false, 1.0f, false); }

namespace
{
static_assert(DXTEX_TGA_RIGHT_TO_LEFT == TGA_RIGHT_TO_LEFT && DXTEX_TGA_TOP_DOWN == TGA_TOP_DOWN && DXTEX_TGA_ALLOW_ALL_ZERO_ALPHA == TGA_ALLOW_ALL_ZERO_ALPHA,
              "dxtex_tga.h's flags are the public ones");

// The tail the TGA, PNM and PNG checks share: the image's rows against its pitch, and the file side - `need` bytes at `stream`, named
// `noun` in the message - apart from the rowBytes-wide rows of the image
dxtex_hresult check_stream_image(dxtex_ctx* ctx, const char* noun, const void* stream, size_t need, const dxtex_image* image, size_t rowBytes)
{
    if (image->rowPitch < rowBytes) return fail(ctx, DXTEX_E_INVALIDARG, "rowPitch is smaller than the row");
    if (image->rowPitch > SIZE_MAX / image->height) return fail(ctx, DXTEX_E_INVALIDARG, "rowPitch x rows overflows");
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(stream), s1 = s0 + need;
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(image->pixels), i1 = i0 + image->rowPitch * (image->height - 1) + rowBytes;
    if (s0 < i1 && i0 < s1) return fail(ctx, DXTEX_E_INVALIDARG, (std::string(noun) + " and image pixels overlap").c_str());
    return DXTEX_S_OK;
}

// The checks of the TGA four, in the order include/dxtex_amd.h states. `image` is the dxtex_image side, *rowBytes a row of its texels;
// *kind = the reader's kind or the writer's row (dxtex_tga.h's tables).
dxtex_hresult check_tga(dxtex_ctx* ctx, const void* stream, size_t streamBytes, uint32_t bytesPerTexel, bool paletted, const dxtex_image* image, bool unpack, int* kind,
                        size_t* rowBytes)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!stream) return fail(ctx, DXTEX_E_POINTER, "null texel stream");
    if (!image) return fail(ctx, DXTEX_E_POINTER, "null image");
    if (!image->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    const TgaPackRow row = tga_pack_row(image->format);
    *kind = unpack ? tga_unpack_kind(image->format, bytesPerTexel, paletted) : row.bytesPerTexel == bytesPerTexel ? row.row : -1;
    if (*kind < 0) return fail(ctx, DXTEX_E_NOT_SUPPORTED, unpack ? "no TGA reader case for this bytes per texel, format and palette" : "no TGA writer case for this format and bytes per texel");
    if (!image->width || !image->height || image->width > 65535 || image->height > 65535) return fail(ctx, DXTEX_E_INVALIDARG, "a TGA image is 1 to 65535 texels wide and high");
    *rowBytes = image->width * (unpack ? tga_image_bytes(*kind) : tga_row_image_bytes(row));
    const size_t need = image->width * image->height * bytesPerTexel;
    const dxtex_hresult hr = check_stream_image(ctx, "texel stream", stream, need, image, *rowBytes);
    if (hr != DXTEX_S_OK) return hr;
    if (streamBytes != need) return fail(ctx, DXTEX_E_FAIL, "the texel stream is not width * height * bytes per texel long");
    return DXTEX_S_OK;
}

// The reader's kernels on device pointers. The two alpha ORs live in the context's result cell, the answer goes to `answer` (device memory;
// null: behind the ORs). A kind without an alpha rule runs no alpha kernel: its answer is known (1 for 24 bits into R8G8B8A8, else 0).
dxtex_hresult submit_tga_unpack(dxtex_ctx* ctx, const uint8_t* stream, int kind, uint32_t flags, const uint32_t* palette, const dxtex_image& dst, uint32_t* answer)
{
    const dxtex_hresult hr = ctx->resultCell.grow(ctx, 4 * sizeof(double)); if (hr != DXTEX_S_OK) return hr;
    uint32_t* cell = static_cast<uint32_t*>(ctx->resultCell.p);
    if (!tga_has_alpha_rule(kind) && answer) HIP_TRY(ctx, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(answer), kind == TGA_RGB_RGBA ? 1 : 0, 1, ctx->stream));
    return launched(ctx, launch_tga_unpack(stream, kind, flags, palette, view_of(dst), cell, answer ? answer : cell + 2, ctx->stream, marks_of(ctx)));
}

// The TGA pairs, one body each: `device` runs the kernels on the caller's device pointers, else the host pointers go through the staging.
// The host reader's answer comes down with the pixels.
dxtex_hresult tga_unpack(dxtex_ctx* ctx, const void* texels, size_t texelBytes, uint32_t bytesPerTexel, uint32_t flags, const uint32_t* palette, const dxtex_image* dst,
                         uint32_t* opaque, bool device)
{
    if (!device && ctx && !opaque) return fail(ctx, DXTEX_E_POINTER, "null alpha answer");
    int kind; size_t rowBytes;
    dxtex_hresult hr = check_tga(ctx, texels, texelBytes, bytesPerTexel, palette != nullptr, dst, true, &kind, &rowBytes);
    if (hr != DXTEX_S_OK) return hr;
    if (device) return run_timed(ctx, [&] { return submit_tga_unpack(ctx, static_cast<const uint8_t*>(texels), kind, flags, palette, *dst, opaque); });
    *opaque = kind == TGA_RGB_RGBA ? 1u : 0u;
    // a kind with an alpha rule leaves its answer in a second part of the output staging, and it comes down behind the pixels
    StagingPlan plan;
    plan.upload(texels, plan.in(texelBytes), texelBytes);
    const StagePart pixels = plan.out(dst->rowPitch, dst->height), answer = plan.out(tga_has_alpha_rule(kind) ? sizeof(uint32_t) : 0);
    plan.download(dst->pixels, pixels, pixels.bytes);
    plan.download(opaque, answer, answer.bytes);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out)
    {
        return submit_tga_unpack(ctx, in, kind, flags, palette, with_pixels(*dst, out), answer.bytes ? reinterpret_cast<uint32_t*>(out + answer.at) : nullptr);
    });
}

dxtex_hresult tga_pack(dxtex_ctx* ctx, const dxtex_image* src, uint32_t bytesPerTexel, void* texels, size_t texelBytes, bool device)
{
    int row; size_t rowBytes;
    const dxtex_hresult hr = check_tga(ctx, texels, texelBytes, bytesPerTexel, false, src, false, &row, &rowBytes);
    if (hr != DXTEX_S_OK) return hr;
    auto pack = [&](const dxtex_image& s, uint8_t* out) { return launched(ctx, launch_tga_pack(view_of(s), row, bytesPerTexel, out, ctx->stream, marks_of(ctx))); };
    if (device) return run_timed(ctx, [&] { return pack(*src, static_cast<uint8_t*>(texels)); });
    return run_staged(ctx, src->pixels, src->rowPitch * (src->height - 1) + rowBytes, texels, texelBytes, [&](uint8_t* in, uint8_t* out) { return pack(with_pixels(*src, in), out); });
}
} // namespace

dxtex_hresult dxtex_tga_unpack_device(dxtex_ctx* ctx, const void* texels, size_t texelBytes, uint32_t bytesPerTexel, uint32_t flags, const uint32_t* palette,
                                      const dxtex_image* dst, uint32_t* opaqueDevice)
{
    return tga_unpack(ctx, texels, texelBytes, bytesPerTexel, flags, palette, dst, opaqueDevice, true);
}

dxtex_hresult dxtex_tga_unpack(dxtex_ctx* ctx, const void* texels, size_t texelBytes, uint32_t bytesPerTexel, uint32_t flags, const uint32_t* palette,
                               const dxtex_image* dst, uint32_t* opaque)
{
    return tga_unpack(ctx, texels, texelBytes, bytesPerTexel, flags, palette, dst, opaque, false);
}

dxtex_hresult dxtex_tga_pack_device(dxtex_ctx* ctx, const dxtex_image* src, uint32_t bytesPerTexel, void* texels, size_t texelBytes)
{
    return tga_pack(ctx, src, bytesPerTexel, texels, texelBytes, true);
}

dxtex_hresult dxtex_tga_pack(dxtex_ctx* ctx, const dxtex_image* src, uint32_t bytesPerTexel, void* texels, size_t texelBytes)
{
    return tga_pack(ctx, src, bytesPerTexel, texels, texelBytes, false);
}

namespace
{
static_assert(DXTEX_DDS_ROW_COPY == ROW_COPY && DXTEX_DDS_ROW_888 == ROW_888 && DXTEX_DDS_ROW_P8 == ROW_P8 && DXTEX_DDS_ROW_WUV10 == ROW_WUV10 && DXTEX_DDS_ROW_OPS == ROW_OPS,
              "dxtex_dds.h's ops are the public ones");

// The checks of the DDS four, in the order include/dxtex_amd.h states; fills `jobs` with one descriptor per image. unpack: `images` are the
// destinations, bytesPerTexel the op's file texel (1 for ROW_COPY, whose widths count bytes); pack24: the B8G8R8X8 sources, 3.
dxtex_hresult check_dds(dxtex_ctx* ctx, const void* file, size_t fileBytes, bool unpack, uint32_t op, const uint32_t* palette, const dxtex_image* images,
                        const size_t* offsets, const size_t* pitches, size_t count, std::vector<DdsImage>* jobs)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!file) return fail(ctx, DXTEX_E_POINTER, unpack ? "null payload" : "null output");
    if (!images || !offsets || !pitches) return fail(ctx, DXTEX_E_POINTER, "null images, offsets or pitches");
    for (size_t i = 0; i < count; ++i)
        if (!images[i].pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (!count) return fail(ctx, DXTEX_E_INVALIDARG, "no images");
    if (unpack && op >= uint32_t(ROW_OPS)) return fail(ctx, DXTEX_E_INVALIDARG, "unknown DDS row op");
    if (unpack && dds_has_palette(int(op)) != (palette != nullptr)) return fail(ctx, DXTEX_E_INVALIDARG, palette ? "this DDS row op takes no palette" : "this DDS row op needs a palette");
    const int format = images[0].format;
    const int target = unpack ? dds_target(int(op), format) : DDS_TO_8888;
    size_t probeRow = 0, probeSlice = 0;
    if (unpack ? (target < 0 || (op == ROW_SWIZZLE && target == DDS_TO_BYTES) || (op == ROW_COPY && dxtex_compute_pitch(format, 1, 1, &probeRow, &probeSlice) != DXTEX_S_OK))
               : format != FMT_B8G8R8X8_UNORM)
        return fail(ctx, DXTEX_E_NOT_SUPPORTED, unpack ? "no DDS reader case for this row op and destination format" : "the 24-bit DDS rows are written from B8G8R8X8_UNORM");
    const uint32_t fileTexel = !unpack ? 3u : op == ROW_COPY ? 1u : dds_file_bytes(int(op));
    const size_t imageTexel = !unpack ? 4u : dds_image_bytes(target);
    jobs->resize(count);
    for (size_t i = 0; i < count; ++i)
    {
        const dxtex_image& im = images[i];
        if (im.format != format) return fail(ctx, DXTEX_E_INVALIDARG, "the images of one call share a format");
        // texels per row fit the kernels' 32-bit x with four to a lane; a copy works in bytes, and its own limit is on rowBytes below
        if ((!(unpack && op == ROW_COPY) && im.width > 0x3FFFFFFFull) || im.height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
        const size_t words = (unpack && target == DDS_TO_YUY2) ? (im.width + 1) / 2 : im.width;          // a YUY2 word holds two texels
        size_t rowBytes = words * imageTexel, rows = im.height;
        if (unpack && op == ROW_COPY)
        {
            // in bytes: the format's own rows (block rows of a compressed image, every plane's rows of a planar one)
            size_t slice = 0;
            if (dxtex_compute_pitch(format, im.width, im.height, &rowBytes, &slice) != DXTEX_S_OK || rowBytes > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
            rows = (im.width && im.height && rowBytes) ? slice / rowBytes : 0;
        }
        if (!im.width || !im.height) { (*jobs)[i] = DdsImage{}; continue; }
        if (rows > 0xFFFFFFFFull || im.rowPitch < rowBytes || im.rowPitch > (SIZE_MAX - rowBytes) / rows) return fail(ctx, DXTEX_E_INVALIDARG, "the image is too small for its rows: rowPitch is smaller than the row, or rowPitch x rows overflows");
        DdsImage& j = (*jobs)[i];
        j = DdsImage{ offsets[i], pitches[i], im.pixels, im.rowPitch, uint32_t(unpack && op == ROW_COPY ? rowBytes : words), uint32_t(rows) };
        if (!dds_image_in_payload(j, fileTexel, fileBytes)) return fail(ctx, DXTEX_E_INVALIDARG, unpack ? "an image's rows reach past the payload" : "an image's rows reach past the output");
        // the two sides apart: the kernels read one while they write the other
        const uintptr_t f0 = reinterpret_cast<uintptr_t>(file) + j.fileOffset, f1 = f0 + (rows - 1) * j.filePitch + size_t(j.width) * fileTexel;
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(im.pixels), i1 = i0 + (rows - 1) * im.rowPitch + rowBytes;
        if (f0 < i1 && i0 < f1) return fail(ctx, DXTEX_E_INVALIDARG, "payload and image pixels overlap");
    }
    return DXTEX_S_OK;
}

// The DDS pairs, one body each: `device` runs the kernel on the caller's device pointers, else the host pointers go through the staging -
// the file side flat, each image's rows as a part of their own at the caller's pitch, and only the rows' texels travel on the image side
dxtex_hresult dds_unpack(dxtex_ctx* ctx, const void* payload, size_t payloadBytes, uint32_t op, uint32_t opaque, const uint32_t* palette, const dxtex_image* dsts,
                         const size_t* srcOffsets, const size_t* srcRowPitches, size_t count, bool device)
{
    std::vector<DdsImage> jobs;
    const dxtex_hresult hr = check_dds(ctx, payload, payloadBytes, true, op, palette, dsts, srcOffsets, srcRowPitches, count, &jobs);
    if (hr != DXTEX_S_OK) return hr;
    auto unpack = [&](const uint8_t* file)
    { return launched(ctx, launch_dds_unpack(file, payloadBytes, int(op), dsts[0].format, opaque != 0, palette, jobs.data(), jobs.size(), ctx->stream, marks_of(ctx))); };
    if (device) return run_timed(ctx, [&] { return unpack(static_cast<const uint8_t*>(payload)); });
    const size_t imageTexel = op == ROW_COPY ? 1u : dds_image_bytes(dds_target(int(op), dsts[0].format));
    StagingPlan plan;
    plan.upload(payload, plan.in(payloadBytes), payloadBytes);
    std::vector<StagePart> part(count);
    for (size_t i = 0; i < count; ++i)
    {
        const size_t rowBytes = jobs[i].width * imageTexel;
        part[i] = plan.out(jobs[i].rows ? (jobs[i].rows - 1) * size_t(jobs[i].pitch) + rowBytes : 0);      // (check_dds has bounded the span)
        plan.download(dsts[i].pixels, dsts[i].rowPitch, part[i], 0, jobs[i].pitch, rowBytes, jobs[i].rows);
    }
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out)
    {
        for (size_t i = 0; i < count; ++i) jobs[i].pixels = out + part[i].at;
        return unpack(in);
    });
}

dxtex_hresult dds_pack24(dxtex_ctx* ctx, const dxtex_image* srcs, const size_t* dstOffsets, const size_t* dstRowPitches, size_t count, void* out, size_t outBytes, bool device)
{
    std::vector<DdsImage> jobs;
    const dxtex_hresult hr = check_dds(ctx, out, outBytes, false, 0, nullptr, srcs, dstOffsets, dstRowPitches, count, &jobs);
    if (hr != DXTEX_S_OK) return hr;
    auto pack = [&](uint8_t* file) { return launched(ctx, launch_dds_pack24(jobs.data(), jobs.size(), file, outBytes, ctx->stream, marks_of(ctx))); };
    if (device) return run_timed(ctx, [&] { return pack(static_cast<uint8_t*>(out)); });
    StagingPlan plan;
    const StagePart file = plan.out(outBytes);
    std::vector<StagePart> part(count);
    for (size_t i = 0; i < count; ++i)
    {
        const size_t width = jobs[i].width;
        part[i] = plan.in(jobs[i].rows ? (jobs[i].rows - 1) * size_t(jobs[i].pitch) + width * 4u : 0);
        plan.upload(srcs[i].pixels, srcs[i].rowPitch, part[i], 0, jobs[i].pitch, width * 4u, jobs[i].rows);
        plan.download(static_cast<uint8_t*>(out) + jobs[i].fileOffset, jobs[i].filePitch, file, jobs[i].fileOffset, jobs[i].filePitch, width * 3u, jobs[i].rows);
    }
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* staged)
    {
        for (size_t i = 0; i < count; ++i) jobs[i].pixels = in + part[i].at;
        return pack(staged);
    });
}
} // namespace

dxtex_hresult dxtex_dds_unpack_device(dxtex_ctx* ctx, const void* payload, size_t payloadBytes, uint32_t op, uint32_t opaque, const uint32_t* palette,
                                      const dxtex_image* dsts, const size_t* srcOffsets, const size_t* srcRowPitches, size_t count)
{
    return dds_unpack(ctx, payload, payloadBytes, op, opaque, palette, dsts, srcOffsets, srcRowPitches, count, true);
}

dxtex_hresult dxtex_dds_unpack(dxtex_ctx* ctx, const void* payload, size_t payloadBytes, uint32_t op, uint32_t opaque, const uint32_t* palette,
                               const dxtex_image* dsts, const size_t* srcOffsets, const size_t* srcRowPitches, size_t count)
{
    return dds_unpack(ctx, payload, payloadBytes, op, opaque, palette, dsts, srcOffsets, srcRowPitches, count, false);
}

dxtex_hresult dxtex_dds_pack24_device(dxtex_ctx* ctx, const dxtex_image* srcs, const size_t* dstOffsets, const size_t* dstRowPitches, size_t count, void* out, size_t outBytes)
{ return dds_pack24(ctx, srcs, dstOffsets, dstRowPitches, count, out, outBytes, true); }
dxtex_hresult dxtex_dds_pack24(dxtex_ctx* ctx, const dxtex_image* srcs, const size_t* dstOffsets, const size_t* dstRowPitches, size_t count, void* out, size_t outBytes)
{ return dds_pack24(ctx, srcs, dstOffsets, dstRowPitches, count, out, outBytes, false); }

namespace
{
static_assert(DXTEX_PNM_P6 == PNM_P6 && DXTEX_PNM_PF == PNM_PF && DXTEX_PNM_Pf == PNM_Pf && DXTEX_PNM_PH == PNM_PH && DXTEX_PNM_Ph == PNM_Ph &&
              DXTEX_PNM_BIG_ENDIAN == PNM_BIG_ENDIAN, "dxtex_pnm.h's kinds and flag are the public ones");

// The checks of the PNM four, in the order include/dxtex_amd.h states. *source = the writer's PnmSource (pack); *rowBytes = a row of the
// image side, *need = the samples the call moves.
dxtex_hresult check_pnm(dxtex_ctx* ctx, const void* samples, size_t sampleBytes, uint32_t kind, uint32_t maxval, uint32_t flags, const dxtex_image* image, bool unpack,
                        int* source, size_t* rowBytes, size_t* need)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!samples) return fail(ctx, DXTEX_E_POINTER, "null samples");
    if (!image) return fail(ctx, DXTEX_E_POINTER, "null image");
    if (!image->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (kind >= PNM_KINDS) return fail(ctx, DXTEX_E_INVALIDARG, "unknown PNM kind");
    if (unpack && kind == PNM_P6 && (maxval < 1 || maxval > 255)) return fail(ctx, DXTEX_E_INVALIDARG, "a P6 maxval is 1 to 255");
    if (flags & ~uint32_t(PNM_BIG_ENDIAN)) return fail(ctx, DXTEX_E_INVALIDARG, "unknown PNM flag bits");
    if (!image->width || !image->height || !sampleBytes) return fail(ctx, DXTEX_E_INVALIDARG, "empty image or no samples");
    if (image->width > 0xFFFFFFFFull || image->height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    size_t imageTexel;
    if (unpack)
    {
        if (image->format != pnm_unpack_format(int(kind))) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "this PNM kind does not unpack into this format");
        imageTexel = pnm_image_bytes(int(kind));
    }
    else
    {
        *source = pnm_pack_source(image->format);
        if (*source < 0 || pnm_source_kind(*source) != int(kind)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "no PNM writer case for this kind and format");
        imageTexel = pnm_source_bytes(*source);
    }
    const size_t fileTexel = pnm_file_bytes(int(kind));
    if (image->width > SIZE_MAX / 16 / image->height) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    *need = image->width * image->height * fileTexel;
    *rowBytes = image->width * imageTexel;
    if (sampleBytes < *need) return fail(ctx, DXTEX_E_INVALIDARG, "fewer samples than width * height texels");
    return check_stream_image(ctx, "samples", samples, *need, image, *rowBytes);
}

// The PNM pairs, one body each: `device` runs the kernel on the caller's device pointers, else the host pointers go through the staging
dxtex_hresult pnm_unpack(dxtex_ctx* ctx, const void* samples, size_t sampleBytes, uint32_t kind, uint32_t maxval, uint32_t flags, const dxtex_image* dst, bool device)
{
    size_t rowBytes, need;
    const dxtex_hresult hr = check_pnm(ctx, samples, sampleBytes, kind, maxval, flags, dst, true, nullptr, &rowBytes, &need);
    if (hr != DXTEX_S_OK) return hr;
    auto unpack = [&](const uint8_t* stream, const ImgView& view) { return launch_pnm_unpack(stream, int(kind), maxval, flags, view, ctx->stream, marks_of(ctx)); };
    if (device) return run_timed(ctx, [&] { return launched(ctx, unpack(static_cast<const uint8_t*>(samples), view_of(*dst))); });
    return run_staged_rows(ctx, samples, need, dst, rowBytes, unpack);
}

dxtex_hresult pnm_pack(dxtex_ctx* ctx, const dxtex_image* src, uint32_t kind, void* samples, size_t sampleBytes, bool device)
{
    int source; size_t rowBytes, need;
    const dxtex_hresult hr = check_pnm(ctx, samples, sampleBytes, kind, 255, 0, src, false, &source, &rowBytes, &need);
    if (hr != DXTEX_S_OK) return hr;
    auto pack = [&](const dxtex_image& s, uint8_t* out) { return launched(ctx, launch_pnm_pack(view_of(s), source, out, ctx->stream, marks_of(ctx))); };
    if (device) return run_timed(ctx, [&] { return pack(*src, static_cast<uint8_t*>(samples)); });
    return run_staged(ctx, src->pixels, src->rowPitch * (src->height - 1) + rowBytes, samples, need, [&](uint8_t* in, uint8_t* out) { return pack(with_pixels(*src, in), out); });
}
} // namespace

dxtex_hresult dxtex_pnm_unpack_device(dxtex_ctx* ctx, const void* samples, size_t sampleBytes, uint32_t kind, uint32_t maxval, uint32_t flags, const dxtex_image* dst)
{
    return pnm_unpack(ctx, samples, sampleBytes, kind, maxval, flags, dst, true);
}

dxtex_hresult dxtex_pnm_unpack(dxtex_ctx* ctx, const void* samples, size_t sampleBytes, uint32_t kind, uint32_t maxval, uint32_t flags, const dxtex_image* dst)
{
    return pnm_unpack(ctx, samples, sampleBytes, kind, maxval, flags, dst, false);
}

dxtex_hresult dxtex_pnm_pack_device(dxtex_ctx* ctx, const dxtex_image* src, uint32_t kind, void* samples, size_t sampleBytes)
{
    return pnm_pack(ctx, src, kind, samples, sampleBytes, true);
}

dxtex_hresult dxtex_pnm_pack(dxtex_ctx* ctx, const dxtex_image* src, uint32_t kind, void* samples, size_t sampleBytes)
{
    return pnm_pack(ctx, src, kind, samples, sampleBytes, false);
}

namespace
{
static_assert(DXTEX_PNG_G1 == PNG_G1 && DXTEX_PNG_G2 == PNG_G2 && DXTEX_PNG_G4 == PNG_G4 && DXTEX_PNG_G8 == PNG_G8 && DXTEX_PNG_G16 == PNG_G16 && DXTEX_PNG_GA8 == PNG_GA8 &&
              DXTEX_PNG_GA16 == PNG_GA16 && DXTEX_PNG_RGB8 == PNG_RGB8 && DXTEX_PNG_RGB16 == PNG_RGB16 && DXTEX_PNG_RGBA8 == PNG_RGBA8 && DXTEX_PNG_RGBA16 == PNG_RGBA16 &&
              DXTEX_PNG_P1 == PNG_P1 && DXTEX_PNG_P2 == PNG_P2 && DXTEX_PNG_P4 == PNG_P4 && DXTEX_PNG_P8 == PNG_P8 && DXTEX_PNG_BGR == PNG_BGR,
              "dxtex_png.h's kinds and flag are the public ones");

// The checks of the PNG four, in the order include/dxtex_amd.h states. *source = the writer's PngSource (pack); *rowBytes = a row of the
// image side, *fileRow = a row of the file side, *need = the bytes the call moves on the file side. table: the palette kinds' 256 words.
dxtex_hresult check_png(dxtex_ctx* ctx, const void* rows, size_t rowsBytes, uint32_t kind, uint32_t flags, const uint32_t* palette, uint32_t paletteCount,
                        const dxtex_image* image, bool unpack, int* source, size_t* rowBytes, size_t* fileRow, size_t* need, uint32_t (*table)[256])
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!rows) return fail(ctx, DXTEX_E_POINTER, "null rows");
    if (!image) return fail(ctx, DXTEX_E_POINTER, "null image");
    if (!image->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (unpack)
    {
        if (kind >= PNG_KINDS) return fail(ctx, DXTEX_E_INVALIDARG, "unknown PNG kind");
        if (flags & ~uint32_t(PNG_BGR)) return fail(ctx, DXTEX_E_INVALIDARG, "unknown PNG flag bits");
        if (png_is_palette(int(kind)) != (palette != nullptr)) return fail(ctx, DXTEX_E_INVALIDARG, palette ? "this PNG kind takes no palette" : "this PNG kind needs a palette");
        if (palette && (paletteCount < 1 || paletteCount > 256)) return fail(ctx, DXTEX_E_INVALIDARG, "a PNG palette has 1 to 256 entries");
    }
    if (!image->width || !image->height || !rowsBytes) return fail(ctx, DXTEX_E_INVALIDARG, "empty image or no rows");
    // texels per row fit the kernels' 32-bit x with a group to a lane
    if (image->width > 0x1FFFFFFFull || image->height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    size_t imageTexel;
    if (unpack)
    {
        if (!png_unpack_pairs(int(kind), flags, image->format)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "this PNG kind and flags do not unpack into this format");
        imageTexel = png_image_bytes(int(kind));
        *fileRow = size_t(png_row_bytes(int(kind), image->width));
        for (uint32_t i = 0; palette && i < 256; ++i) (*table)[i] = i < paletteCount ? palette[i] : 0xFF000000u;
    }
    else
    {
        *source = png_pack_source(image->format);
        if (*source < 0) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "no PNG writer case for this format");
        imageTexel = png_source_bytes(*source);
        *fileRow = image->width * png_source_file_bytes(*source);
    }
    if (*fileRow > SIZE_MAX / image->height) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    *need = *fileRow * image->height;
    *rowBytes = image->width * imageTexel;
    if (rowsBytes < *need) return fail(ctx, DXTEX_E_INVALIDARG, "fewer bytes than height rows");
    return check_stream_image(ctx, "rows", rows, *need, image, *rowBytes);
}

// The PNG pairs, one body each: `device` runs the kernel on the caller's device pointers, else the host pointers go through the staging
dxtex_hresult png_unpack(dxtex_ctx* ctx, const void* rows, size_t rowsBytes, uint32_t kind, uint32_t flags, const uint32_t* palette, uint32_t paletteCount, const dxtex_image* dst,
                         bool device)
{
    size_t rowBytes, fileRow, need; uint32_t table[256];
    const dxtex_hresult hr = check_png(ctx, rows, rowsBytes, kind, flags, palette, paletteCount, dst, true, nullptr, &rowBytes, &fileRow, &need, &table);
    if (hr != DXTEX_S_OK) return hr;
    auto unpack = [&](const uint8_t* stream, const ImgView& view) { return launch_png_unpack(stream, int(kind), flags, palette ? table : nullptr, view, ctx->stream, marks_of(ctx)); };
    if (device) return run_timed(ctx, [&] { return launched(ctx, unpack(static_cast<const uint8_t*>(rows), view_of(*dst))); });
    return run_staged_rows(ctx, rows, need, dst, rowBytes, unpack);
}

dxtex_hresult png_pack(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes, bool device)
{
    int source; size_t rowBytes, fileRow, need;
    const dxtex_hresult hr = check_png(ctx, rows, rowsBytes, 0, 0, nullptr, 0, src, false, &source, &rowBytes, &fileRow, &need, nullptr);
    if (hr != DXTEX_S_OK) return hr;
    auto pack = [&](const dxtex_image& s, uint8_t* out) { return launched(ctx, launch_png_pack(view_of(s), source, out, ctx->stream, marks_of(ctx))); };
    if (device) return run_timed(ctx, [&] { return pack(*src, static_cast<uint8_t*>(rows)); });
    return run_staged(ctx, src->pixels, src->rowPitch * (src->height - 1) + rowBytes, rows, need, [&](uint8_t* in, uint8_t* out) { return pack(with_pixels(*src, in), out); });
}
} // namespace

dxtex_hresult dxtex_png_unpack_device(dxtex_ctx* ctx, const void* rows, size_t rowsBytes, uint32_t kind, uint32_t flags, const uint32_t* palette, uint32_t paletteCount,
                                      const dxtex_image* dst)
{
    return png_unpack(ctx, rows, rowsBytes, kind, flags, palette, paletteCount, dst, true);
}

dxtex_hresult dxtex_png_unpack(dxtex_ctx* ctx, const void* rows, size_t rowsBytes, uint32_t kind, uint32_t flags, const uint32_t* palette, uint32_t paletteCount,
                               const dxtex_image* dst)
{
    return png_unpack(ctx, rows, rowsBytes, kind, flags, palette, paletteCount, dst, false);
}

dxtex_hresult dxtex_png_pack_device(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes) { return png_pack(ctx, src, rows, rowsBytes, true); }
dxtex_hresult dxtex_png_pack(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes) { return png_pack(ctx, src, rows, rowsBytes, false); }

namespace
{
static_assert(DXTEX_EXR_UINT == EXR_UINT && DXTEX_EXR_HALF == EXR_HALF && DXTEX_EXR_FLOAT == EXR_FLOAT && DXTEX_EXR_ABSENT == EXR_ABSENT, "dxtex_exr.h's channel types are the public ones");
static_assert(sizeof(dxtex_exr_chunk) == sizeof(ExrChunk) && sizeof(dxtex_exr_channel) == sizeof(ExrChannel), "dxtex_exr.h's descriptors are the public ones");

// The checks of dxtex_exr_unpack[_device], in the order include/dxtex_amd.h states. *layout and *list = what the launchers take.
dxtex_hresult check_exr_unpack(dxtex_ctx* ctx, const void* stream, size_t streamBytes, const dxtex_exr_chunk* chunks, size_t chunkCount, const dxtex_exr_channel* channels,
                               uint32_t scanlineBytes, const dxtex_image* items, size_t itemCount, ExrLayout* layout, std::vector<ExrChunk>* list)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!stream) return fail(ctx, DXTEX_E_POINTER, "null stream");
    if (!chunks) return fail(ctx, DXTEX_E_POINTER, "null chunk descriptors");
    if (!channels) return fail(ctx, DXTEX_E_POINTER, "null channel table");
    if (!items) return fail(ctx, DXTEX_E_POINTER, "null items");
    for (size_t i = 0; i < itemCount && i < kExrItemsMax; ++i) if (!items[i].pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (!chunkCount) return fail(ctx, DXTEX_E_INVALIDARG, "no chunks");
    if (!itemCount || itemCount > kExrItemsMax) return fail(ctx, DXTEX_E_INVALIDARG, "1 to 6 items");
    const size_t width = items[0].width, height = items[0].height;
    if (!width || !height) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    if (width > 0x0FFFFFFFull || height > 0x0FFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    for (uint32_t c = 0; c < 4; ++c) if (channels[c].type > EXR_ABSENT) return fail(ctx, DXTEX_E_INVALIDARG, "unknown channel type");
    if (!scanlineBytes) return fail(ctx, DXTEX_E_INVALIDARG, "a scanline of no bytes");
    for (size_t i = 0; i < itemCount; ++i) if (items[i].format != FMT_R16G16B16A16_FLOAT) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "EXR chunks unpack into R16G16B16A16_FLOAT");
    for (size_t i = 1; i < itemCount; ++i) if (items[i].width != width || items[i].height != height) return fail(ctx, DXTEX_E_INVALIDARG, "items of different sizes");
    for (uint32_t c = 0; c < 4; ++c)
        if (channels[c].type != EXR_ABSENT && (channels[c].offset > scanlineBytes || uint64_t(width) * exr_type_bytes(channels[c].type) > scanlineBytes - channels[c].offset))
            return fail(ctx, DXTEX_E_INVALIDARG, "a channel's samples leave the scanline");
    const uint64_t rows = uint64_t(height) * itemCount;
    uint64_t end = 0;
    list->resize(chunkCount);
    for (size_t i = 0; i < chunkCount; ++i)
    {
        const dxtex_exr_chunk& c = chunks[i];
        if (c.coded > 1u || !c.rows || c.offset > streamBytes || c.bytes > streamBytes - c.offset) return fail(ctx, DXTEX_E_INVALIDARG, "a chunk descriptor leaves the stream");
        if (uint64_t(c.rows) * scanlineBytes != c.bytes) return fail(ctx, DXTEX_E_INVALIDARG, "a chunk is not rows * scanlineBytes long");
        if (c.firstRow >= rows || c.rows > rows - c.firstRow) return fail(ctx, DXTEX_E_INVALIDARG, "a chunk names rows outside the window");
        if (c.offset < end) return fail(ctx, DXTEX_E_INVALIDARG, "chunk descriptors overlap or are not in stream order");
        end = c.offset + c.bytes;
        (*list)[i] = ExrChunk{ c.offset, c.bytes, c.firstRow, c.rows, c.coded };
    }
    const size_t rowBytes = width * 8;
    for (size_t i = 0; i < itemCount; ++i)
    {
        const dxtex_hresult hr = check_stream_image(ctx, "stream", stream, streamBytes, &items[i], rowBytes);
        if (hr != DXTEX_S_OK) return hr;
    }
    *layout = ExrLayout{ uint32_t(width), uint32_t(rows), uint32_t(height), scanlineBytes,
                         { { channels[0].offset, channels[0].type }, { channels[1].offset, channels[1].type }, { channels[2].offset, channels[2].type }, { channels[3].offset, channels[3].type } } };
    return DXTEX_S_OK;
}

// exr_undo in place, then exr_texels: what both forms queue
dxtex_hresult submit_exr_unpack(dxtex_ctx* ctx, uint8_t* stream, const std::vector<ExrChunk>& list, const ExrLayout& layout, const dxtex_image* items, size_t itemCount)
{
    const dxtex_hresult hr = ctx->exrSums.grow(ctx, std::max<size_t>(1, exr_undo_sums_count(list.data(), list.size())) * sizeof(uint32_t), 1u << 16);
    if (hr != DXTEX_S_OK) return hr;
    ImgView views[kExrItemsMax];
    for (size_t i = 0; i < itemCount; ++i) views[i] = view_of(items[i]);
    hipError_t e = launch_exr_undo(stream, list.data(), list.size(), static_cast<uint32_t*>(ctx->exrSums.p), ctx->stream, marks_of(ctx));
    if (e == hipSuccess) e = launch_exr_texels(stream, list.data(), list.size(), layout, views, itemCount, ctx->stream, marks_of(ctx));
    return launched(ctx, e);
}

dxtex_hresult check_exr_pack(dxtex_ctx* ctx, const dxtex_image* src, const void* scanlines, size_t scanlineBytes, int* source, size_t* rowBytes, size_t* need)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src) return fail(ctx, DXTEX_E_POINTER, "null image");
    if (!src->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (!scanlines) return fail(ctx, DXTEX_E_POINTER, "null scanlines");
    if (!src->width || !src->height) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    if (src->width > 0x0FFFFFFFull || src->height > 0x0FFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    *source = exr_pack_source(src->format);
    if (*source < 0) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "no EXR writer case for this format");
    *need = src->width * src->height * kExrFileTexelBytes;
    *rowBytes = src->width * exr_source_bytes(*source);
    if (scanlineBytes < *need) return fail(ctx, DXTEX_E_INVALIDARG, "fewer than width * height * 8 bytes of scanlines");
    return check_stream_image(ctx, "scanlines", scanlines, *need, src, *rowBytes);
}

dxtex_hresult exr_pack(dxtex_ctx* ctx, const dxtex_image* src, void* scanlines, size_t scanlineBytes, bool device)
{
    int source; size_t rowBytes, need;
    const dxtex_hresult hr = check_exr_pack(ctx, src, scanlines, scanlineBytes, &source, &rowBytes, &need);
    if (hr != DXTEX_S_OK) return hr;
    auto pack = [&](const dxtex_image& s, uint8_t* out) { return launched(ctx, launch_exr_pack(view_of(s), source, out, ctx->stream, marks_of(ctx))); };
    if (device) return run_timed(ctx, [&] { return pack(*src, static_cast<uint8_t*>(scanlines)); });
    return run_staged(ctx, src->pixels, src->rowPitch * (src->height - 1) + rowBytes, scanlines, need, [&](uint8_t* in, uint8_t* out) { return pack(with_pixels(*src, in), out); });
}
} // namespace

dxtex_hresult dxtex_exr_unpack_device(dxtex_ctx* ctx, void* stream, size_t streamBytes, const dxtex_exr_chunk* chunks, size_t chunkCount,
                                      const dxtex_exr_channel* channels, uint32_t scanlineBytes, const dxtex_image* items, size_t itemCount)
{
    ExrLayout layout; std::vector<ExrChunk> list;
    const dxtex_hresult hr = check_exr_unpack(ctx, stream, streamBytes, chunks, chunkCount, channels, scanlineBytes, items, itemCount, &layout, &list);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_exr_unpack(ctx, static_cast<uint8_t*>(stream), list, layout, items, itemCount); });
}

dxtex_hresult dxtex_exr_unpack(dxtex_ctx* ctx, const void* stream, size_t streamBytes, const dxtex_exr_chunk* chunks, size_t chunkCount,
                               const dxtex_exr_channel* channels, uint32_t scanlineBytes, const dxtex_image* items, size_t itemCount)
{
    ExrLayout layout; std::vector<ExrChunk> list;
    dxtex_hresult hr = check_exr_unpack(ctx, stream, streamBytes, chunks, chunkCount, channels, scanlineBytes, items, itemCount, &layout, &list);
    if (hr != DXTEX_S_OK) return hr;
    // the stream goes up as it is; the items' rows are written tight (rounded up to 16 bytes) into the output staging, one item behind
    // another, and only each row's texels come down, through the caller's pitches
    const size_t rowBytes = size_t(layout.width) * 8, pitch = (rowBytes + 15) & ~size_t(15), itemBytes = pitch * layout.itemRows;
    StagingPlan plan;
    plan.upload(stream, plan.in(streamBytes), streamBytes);
    const StagePart rows = plan.out(itemBytes, itemCount);
    for (size_t i = 0; i < itemCount; ++i) plan.download(items[i].pixels, items[i].rowPitch, rows, i * itemBytes, pitch, rowBytes, layout.itemRows);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out)
    {
        dxtex_image staged[kExrItemsMax];
        for (size_t i = 0; i < itemCount; ++i)
        {
            staged[i] = with_pixels(items[i], out + i * itemBytes);
            staged[i].rowPitch = pitch; staged[i].slicePitch = itemBytes;
        }
        return submit_exr_unpack(ctx, in, list, layout, staged, itemCount);
    });
}

dxtex_hresult dxtex_exr_pack_device(dxtex_ctx* ctx, const dxtex_image* src, void* scanlines, size_t scanlineBytes) { return exr_pack(ctx, src, scanlines, scanlineBytes, true); }
dxtex_hresult dxtex_exr_pack(dxtex_ctx* ctx, const dxtex_image* src, void* scanlines, size_t scanlineBytes) { return exr_pack(ctx, src, scanlines, scanlineBytes, false); }

namespace
{
static_assert(DXTEX_TIFF_GREY1 == TIFF_GREY1 && DXTEX_TIFF_GREY32F == TIFF_GREY32F && DXTEX_TIFF_PAL1 == TIFF_PAL1 && DXTEX_TIFF_PAL8 == TIFF_PAL8 && DXTEX_TIFF_RGB8 == TIFF_RGB8 &&
              DXTEX_TIFF_RGBA16 == TIFF_RGBA16 && DXTEX_TIFF_RGBA32F == TIFF_RGBA32F && TIFF_KINDS == 14u, "dxtex_tiff.h's kinds are the public ones");
static_assert(sizeof(dxtex_tiff_segment) == sizeof(TiffSegment) && sizeof(dxtex_tiff_layout) == sizeof(TiffLayout), "dxtex_tiff.h's descriptors are the public ones");

// The checks of dxtex_tiff_unpack[_device], in the order include/dxtex_amd.h states. *l and *list = what the launchers take; *copies = the
// file is its image already and every segment a run of whole rows.
dxtex_hresult check_tiff_unpack(dxtex_ctx* ctx, const void* stream, size_t streamBytes, const dxtex_tiff_segment* segments, size_t count, const dxtex_tiff_layout* layout,
                                const uint32_t* palette, const dxtex_image* dst, TiffLayout* l, std::vector<TiffSegment>* list, bool* copies)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!stream) return fail(ctx, DXTEX_E_POINTER, "null stream");
    if (!segments) return fail(ctx, DXTEX_E_POINTER, "null segment descriptors");
    if (!layout) return fail(ctx, DXTEX_E_POINTER, "null layout");
    if (!dst) return fail(ctx, DXTEX_E_POINTER, "null image");
    if (!dst->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (layout->kind < TIFF_KINDS && tiff_is_palette(layout->kind) && !palette) return fail(ctx, DXTEX_E_POINTER, "this TIFF kind needs a palette");
    if (!count) return fail(ctx, DXTEX_E_INVALIDARG, "no segments");
    if (!dst->width || !dst->height) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    if (dst->width > 0x0FFFFFFFull || dst->height > 0x0FFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    if (dst->width != layout->width || dst->height != layout->height) return fail(ctx, DXTEX_E_INVALIDARG, "the image is not the layout's size");
    if (layout->kind >= TIFF_KINDS) return fail(ctx, DXTEX_E_INVALIDARG, "unknown TIFF kind");
    const TiffKindRow kind = tiff_kind_row(layout->kind);
    if (layout->bits != kind.bits || layout->samples != kind.samples) return fail(ctx, DXTEX_E_INVALIDARG, "bits or samples are not the kind's");
    if (layout->predictor < 1u || layout->predictor > 3u) return fail(ctx, DXTEX_E_INVALIDARG, "predictor 1, 2 or 3");
    if (!tiff_predictor_fits(layout->predictor, layout->bits)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "predictor 2 takes 8- or 16-bit samples, predictor 3 32-bit ones");
    if (!tiff_unpacks_into(layout->kind, dst->format)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "this TIFF kind does not unpack into this format");
    *l = TiffLayout{ layout->width, layout->height, layout->bits, layout->samples, layout->kind, layout->predictor, layout->bigEndian ? 1u : 0u,
                     layout->planar && layout->samples > 1u ? 1u : 0u, layout->whiteIsZero ? 1u : 0u, layout->opaque && layout->samples == 4u ? 1u : 0u };
    const uint32_t rowSamples = l->planar ? 1u : l->samples, planes = l->planar ? l->samples : 1u;
    const size_t rowBytes = dst->width * kind.imageBytes;
    *copies = tiff_is_native(*l);
    uint64_t end = 0;
    list->resize(count);
    for (size_t i = 0; i < count; ++i)
    {
        const dxtex_tiff_segment& s = segments[i];
        if (!s.rows || !s.cols || s.firstRow >= l->height || s.rows > l->height - s.firstRow || s.firstCol >= l->width || s.cols > l->width - s.firstCol || s.plane >= planes)
            return fail(ctx, DXTEX_E_INVALIDARG, "a segment descriptor leaves the image");
        if (s.rowBytes < tiff_row_bytes(s.cols, rowSamples, l->bits) || (l->bits > 8u && s.rowBytes % (l->bits / 8u)))
            return fail(ctx, DXTEX_E_INVALIDARG, "a segment's rowBytes is smaller than its columns need");
        if (s.offset > streamBytes || uint64_t(s.rows) * s.rowBytes > streamBytes - s.offset) return fail(ctx, DXTEX_E_INVALIDARG, "a segment descriptor leaves the stream");
        if (s.offset < end) return fail(ctx, DXTEX_E_INVALIDARG, "segment descriptors overlap or are not in stream order");
        end = s.offset + uint64_t(s.rows) * s.rowBytes;
        *copies = *copies && s.firstCol == 0 && s.cols == l->width && s.rowBytes == rowBytes;
        (*list)[i] = TiffSegment{ s.offset, s.firstRow, s.rows, s.firstCol, s.cols, s.rowBytes, s.plane };
    }
    return check_stream_image(ctx, "stream", stream, streamBytes, dst, rowBytes);
}

// what both forms queue: row copies for a file that is its image, else tiff_undo in place and tiff_texels
dxtex_hresult submit_tiff_unpack(dxtex_ctx* ctx, uint8_t* stream, const std::vector<TiffSegment>& list, const TiffLayout& l, const uint32_t* palette, const dxtex_image& dst, bool copies)
{
    if (copies)
    {
        for (const TiffSegment& s : list)
            HIP_TRY(ctx, hipMemcpy2DAsync(dst.pixels + size_t(s.firstRow) * dst.rowPitch, dst.rowPitch, stream + s.offset, s.rowBytes, s.rowBytes, s.rows, hipMemcpyDeviceToDevice, ctx->stream));
        return DXTEX_S_OK;
    }
    uint32_t table[256] = {};
    if (palette) std::copy(palette, palette + 256, table);
    hipError_t e = launch_tiff_undo(stream, list.data(), list.size(), l, ctx->stream, marks_of(ctx));
    if (e == hipSuccess) e = launch_tiff_texels(stream, list.data(), list.size(), l, palette ? table : nullptr, view_of(dst), ctx->stream, marks_of(ctx));
    return launched(ctx, e);
}

dxtex_hresult tiff_pack(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes, bool device)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src) return fail(ctx, DXTEX_E_POINTER, "null image");
    if (!src->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (!rows) return fail(ctx, DXTEX_E_POINTER, "null rows");
    if (!src->width || !src->height) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    if (src->width > 0x0FFFFFFFull || src->height > 0x0FFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    const TiffSource source = tiff_pack_source(src->format);
    if (!source.bits) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "no TIFF writer case for this format");
    const size_t fileRow = src->width * source.fileBytes, need = fileRow * src->height, rowBytes = src->width * source.imageBytes;
    if (rowsBytes < need) return fail(ctx, DXTEX_E_INVALIDARG, "fewer bytes of rows than the file's texels");
    const dxtex_hresult hr = check_stream_image(ctx, "rows", rows, need, src, rowBytes);
    if (hr != DXTEX_S_OK) return hr;
    auto pack = [&](const dxtex_image& s, uint8_t* out) -> dxtex_hresult
    {
        if (source.bgr) return launched(ctx, launch_tiff_pack(view_of(s), out, ctx->stream, marks_of(ctx)));
        HIP_TRY(ctx, hipMemcpy2DAsync(out, fileRow, s.pixels, s.rowPitch, fileRow, s.height, hipMemcpyDeviceToDevice, ctx->stream));          // the rows are the file's: no kernel
        return DXTEX_S_OK;
    };
    if (device) return run_timed(ctx, [&] { return pack(*src, static_cast<uint8_t*>(rows)); });
    return run_staged(ctx, src->pixels, src->rowPitch * (src->height - 1) + rowBytes, rows, need, [&](uint8_t* in, uint8_t* out) { return pack(with_pixels(*src, in), out); });
}
} // namespace

dxtex_hresult dxtex_tiff_unpack_device(dxtex_ctx* ctx, void* stream, size_t streamBytes, const dxtex_tiff_segment* segments, size_t segmentCount,
                                       const dxtex_tiff_layout* layout, const uint32_t* palette, const dxtex_image* dst)
{
    TiffLayout l; std::vector<TiffSegment> list; bool copies;
    const dxtex_hresult hr = check_tiff_unpack(ctx, stream, streamBytes, segments, segmentCount, layout, palette, dst, &l, &list, &copies);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_tiff_unpack(ctx, static_cast<uint8_t*>(stream), list, l, palette, *dst, copies); });
}

dxtex_hresult dxtex_tiff_unpack(dxtex_ctx* ctx, const void* stream, size_t streamBytes, const dxtex_tiff_segment* segments, size_t segmentCount,
                                const dxtex_tiff_layout* layout, const uint32_t* palette, const dxtex_image* dst)
{
    TiffLayout l; std::vector<TiffSegment> list; bool copies;
    const dxtex_hresult hr = check_tiff_unpack(ctx, stream, streamBytes, segments, segmentCount, layout, palette, dst, &l, &list, &copies);
    if (hr != DXTEX_S_OK) return hr;
    // the stream goes up as it is; the rows are written tight (rounded up to 16 bytes) into the output staging and only each row's texels
    // come down, through the caller's pitch
    const size_t rowBytes = size_t(l.width) * tiff_kind_row(l.kind).imageBytes, pitch = (rowBytes + 15) & ~size_t(15);
    StagingPlan plan;
    plan.upload(stream, plan.in(streamBytes), streamBytes);
    plan.download(dst->pixels, dst->rowPitch, plan.out(pitch, dst->height), 0, pitch, rowBytes, dst->height);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out)
    {
        dxtex_image staged = with_pixels(*dst, out);
        staged.rowPitch = pitch; staged.slicePitch = pitch * dst->height;
        return submit_tiff_unpack(ctx, in, list, l, palette, staged, copies);
    });
}

dxtex_hresult dxtex_tiff_pack_device(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes) { return tiff_pack(ctx, src, rows, rowsBytes, true); }
dxtex_hresult dxtex_tiff_pack(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes) { return tiff_pack(ctx, src, rows, rowsBytes, false); }

namespace
{
static_assert(DXTEX_JPEG_GREY == JPEG_GREY && DXTEX_JPEG_YCBCR == JPEG_YCBCR && DXTEX_JPEG_RGB == JPEG_RGB, "dxtex_jpeg.h's colour kinds are the public ones");

// The checks of the JPEG four, in the order include/dxtex_amd.h states; `image` is dst of a decode and src of an encode. *f = the frame as
// the launchers take it, *need = the bytes of its coefficients, *rowBytes = a row of the image, *bgr = an encode's source has B before R.
dxtex_hresult check_jpeg(dxtex_ctx* ctx, const void* coefficients, size_t coefficientBytes, const dxtex_jpeg_frame* frame, const dxtex_image* image, bool encode, JpegFrame* f,
                         size_t* need, size_t* rowBytes, bool* bgr = nullptr)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!coefficients) return fail(ctx, DXTEX_E_POINTER, "null coefficients");
    if (!frame) return fail(ctx, DXTEX_E_POINTER, "null frame");
    if (!image) return fail(ctx, DXTEX_E_POINTER, "null image");
    if (!image->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (frame->colour > DXTEX_JPEG_RGB) return fail(ctx, DXTEX_E_INVALIDARG, "unknown JPEG colour");
    if (frame->components != (frame->colour == DXTEX_JPEG_GREY ? 1u : 3u)) return fail(ctx, DXTEX_E_INVALIDARG, "the component count does not match the colour");
    if (!frame->width || !frame->height || frame->width > 65535u || frame->height > 65535u) return fail(ctx, DXTEX_E_INVALIDARG, "a JPEG frame is 1 to 65535 texels wide and high");
    if (image->width != frame->width || image->height != frame->height) return fail(ctx, DXTEX_E_INVALIDARG, "the image is not the frame's size");
    if (reinterpret_cast<uintptr_t>(coefficients) & 1u) return fail(ctx, DXTEX_E_INVALIDARG, "coefficients at an odd address");
    for (uint32_t c = 0; c < frame->components; ++c)
    {
        const dxtex_jpeg_component& k = frame->component[c];
        if (k.quant > 3u) return fail(ctx, DXTEX_E_INVALIDARG, "a quantiser index above 3");
        if (k.h < 1u || k.h > 4u || k.v < 1u || k.v > 4u) return fail(ctx, DXTEX_E_INVALIDARG, "sampling factors are 1 to 4");
    }
    if (encode && frame->colour == DXTEX_JPEG_RGB) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "RGB-coded JPEG frames are not written");
    // sampling: luma 1x1, 2x1 or 2x2 over 1x1 chroma; grey 1x1
    const uint32_t hmax = frame->component[0].h, vmax = frame->component[0].v;
    bool sampling = (hmax == 1u && vmax == 1u) || (frame->components == 3u && hmax == 2u && vmax <= 2u);
    for (uint32_t c = 1; c < frame->components; ++c) sampling = sampling && frame->component[c].h == 1u && frame->component[c].v == 1u;
    if (!sampling) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "JPEG sampling other than 1x1, 2x1 or 2x2 luma over 1x1 chroma");
    const bool grey = frame->colour == DXTEX_JPEG_GREY;
    const int texel = jpeg_texel_of(image->format);
    if (grey ? texel != JPEG_TEXEL_GREY : !(texel == JPEG_TEXEL_RGBA || (encode && texel == JPEG_TEXEL_BGRX)))
        return fail(ctx, DXTEX_E_NOT_SUPPORTED, encode ? "this format does not encode as this JPEG colour" : "this JPEG colour does not decode into this format");
    if (bgr) *bgr = texel == JPEG_TEXEL_BGRX;
    f->width = frame->width; f->height = frame->height; f->components = frame->components; f->colour = int(frame->colour);
    uint64_t at = 0;
    for (uint32_t c = 0; c < frame->components; ++c)
    {
        const dxtex_jpeg_component& k = frame->component[c];
        if (k.blocksPerRow != jpeg_padded_blocks(frame->width, k.h, hmax) || k.blockRows != jpeg_padded_blocks(frame->height, k.v, vmax) || k.offset != at)
            return fail(ctx, DXTEX_E_INVALIDARG, "block counts or offsets that are not the frame's");
        f->comp[c] = JpegComponent{ k.h, k.v, k.quant, k.blocksPerRow, k.blockRows, k.offset };
        at += uint64_t(k.blocksPerRow) * k.blockRows * 64u;
    }
    for (uint32_t c = 0; encode && c < frame->components; ++c)
        for (uint32_t k = 0; k < 64; ++k)
            if (!frame->quant[frame->component[c].quant][k]) return fail(ctx, DXTEX_E_INVALIDARG, "a quantiser entry of 0");
    std::memcpy(f->quant, frame->quant, sizeof(f->quant));
    *need = size_t(at) * sizeof(int16_t);
    *rowBytes = size_t(frame->width) * (grey ? 1u : 4u);
    if (coefficientBytes < *need) return fail(ctx, DXTEX_E_INVALIDARG, "fewer bytes than the frame's coefficients");
    return check_stream_image(ctx, "coefficients", coefficients, *need, image, *rowBytes);
}

// the planes of frame f between a JPEG pair's two kernels, in memory of the context
dxtex_hresult grow_jpeg_planes(dxtex_ctx* ctx, const JpegFrame& f)
{
    ScopedDevice sd(ctx->device);
    return ctx->jpegPlanes.grow(ctx, jpeg_plane_bytes(f));
}

// The JPEG pairs, one body each: `device` runs the kernels on the caller's device pointers, else the host pointers go through the staging.
// The planes between the two kernels live in memory of the context.
dxtex_hresult jpeg_decode(dxtex_ctx* ctx, const void* coefficients, size_t coefficientBytes, const dxtex_jpeg_frame* frame, const dxtex_image* dst, bool device)
{
    JpegFrame f; size_t need, rowBytes;
    const dxtex_hresult hr = check_jpeg(ctx, coefficients, coefficientBytes, frame, dst, false, &f, &need, &rowBytes);
    if (hr != DXTEX_S_OK) return hr;
    const dxtex_hresult grown = grow_jpeg_planes(ctx, f);
    if (grown != DXTEX_S_OK) return grown;
    auto decode = [&](const uint8_t* stream, const ImgView& view)
    { return launch_jpeg_decode(reinterpret_cast<const int16_t*>(stream), f, view, ctx->jpegPlanes.u8(), ctx->stream, marks_of(ctx)); };
    if (device) return run_timed(ctx, [&] { return launched(ctx, decode(static_cast<const uint8_t*>(coefficients), view_of(*dst))); });
    return run_staged_rows(ctx, coefficients, need, dst, rowBytes, decode);
}

dxtex_hresult jpeg_encode(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_jpeg_frame* frame, void* coefficients, size_t coefficientBytes, bool device)
{
    JpegFrame f; size_t need, rowBytes; bool bgr;
    const dxtex_hresult hr = check_jpeg(ctx, coefficients, coefficientBytes, frame, src, true, &f, &need, &rowBytes, &bgr);
    if (hr != DXTEX_S_OK) return hr;
    const dxtex_hresult grown = grow_jpeg_planes(ctx, f);
    if (grown != DXTEX_S_OK) return grown;
    auto encode = [&](const dxtex_image& s, void* out)
    { return launched(ctx, launch_jpeg_encode(view_of(s), bgr, f, static_cast<int16_t*>(out), ctx->jpegPlanes.u8(), ctx->stream, marks_of(ctx))); };
    if (device) return run_timed(ctx, [&] { return encode(*src, coefficients); });
    return run_staged(ctx, src->pixels, src->rowPitch * (src->height - 1) + rowBytes, coefficients, need, [&](uint8_t* in, uint8_t* out) { return encode(with_pixels(*src, in), out); });
}
} // namespace

dxtex_hresult dxtex_jpeg_decode_device(dxtex_ctx* ctx, const void* coefficients, size_t coefficientBytes, const dxtex_jpeg_frame* frame, const dxtex_image* dst)
{
    return jpeg_decode(ctx, coefficients, coefficientBytes, frame, dst, true);
}

dxtex_hresult dxtex_jpeg_decode(dxtex_ctx* ctx, const void* coefficients, size_t coefficientBytes, const dxtex_jpeg_frame* frame, const dxtex_image* dst)
{
    return jpeg_decode(ctx, coefficients, coefficientBytes, frame, dst, false);
}

dxtex_hresult dxtex_jpeg_encode_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_jpeg_frame* frame, void* coefficients, size_t coefficientBytes)
{
    return jpeg_encode(ctx, src, frame, coefficients, coefficientBytes, true);
}

dxtex_hresult dxtex_jpeg_encode(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_jpeg_frame* frame, void* coefficients, size_t coefficientBytes)
{
    return jpeg_encode(ctx, src, frame, coefficients, coefficientBytes, false);
}

namespace
{
// PremultiplyAlpha's checks (DirectXTexPMAlpha.cpp:214-231)
dxtex_hresult check_pmalpha(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    if (!src->pixels || !dst->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    const FmtInfo* f = format_info(src->format);
    if (!f || (f->cls & FC_BC) || !(f->cls & FC_A)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "PremultiplyAlpha needs an uncompressed format with alpha");
    if (src->width > 0xFFFFFFFFull || src->height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    if (src->format != dst->format || src->width != dst->width || src->height != dst->height) return fail(ctx, DXTEX_E_FAIL, "size or format mismatch");
    return DXTEX_S_OK;
}

dxtex_hresult submit_pmalpha(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst, uint32_t flags)
{
    return launched(ctx, launch_pmalpha(view_of(src), view_of(dst), flags, ctx->stream, marks_of(ctx)));
}

// EstimateAlphaScaleForCoverage (DirectXTexMipmaps.cpp:310-352) around the device coverage count
dxtex_hresult alpha_coverage(dxtex_ctx* ctx, const dxtex_image& im, float scale, float alphaReference, float* coverage)
{
    dxtex_hresult hr = ctx->resultCell.grow(ctx, 4 * sizeof(double)); if (hr != DXTEX_S_OK) return hr;
    hr = launched(ctx, launch_alpha_coverage(view_of(im), scale, alphaReference, static_cast<unsigned long long*>(ctx->resultCell.p), ctx->stream,
                                             marks_of(ctx)));
    if (hr != DXTEX_S_OK) return hr;
    unsigned long long n = 0;
    HIP_TRY(ctx, counted_copy(ctx, &n, ctx->resultCell.p, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const float cscale = static_cast<float>((im.width - 1) * (im.height - 1) * 8 * 8);      // :299-303
    *coverage = (cscale > 0.f) ? static_cast<float>(size_t(n)) / cscale : 0.0f;
    return DXTEX_S_OK;
}

dxtex_hresult check_coverage_chain(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, size_t nlevels)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !dst || !nlevels) return fail(ctx, DXTEX_E_INVALIDARG, "empty mip chain");
    const FmtInfo* f = format_info(src[0].format);
    if (f && (f->cls & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "ScaleMipMapsAlphaForCoverage does not take block-compressed formats");
    if (!f || (f->cls & FC_GROUP)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "format is not supported by the MI355X path");
    for (size_t i = 0; i < nlevels; ++i)
    {
        if (!src[i].pixels || !dst[i].pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
        if (src[i].format != src[0].format || dst[i].format != src[0].format || src[i].width != dst[i].width || src[i].height != dst[i].height)
            return fail(ctx, DXTEX_E_FAIL, "level size or format mismatch");
    }
    return DXTEX_S_OK;
}

// the body of ScaleMipMapsAlphaForCoverage (:3503-3553) on device-resident levels
dxtex_hresult submit_coverage_chain(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, size_t nlevels, float alphaReference)
{
    float target = 0.0f;
    dxtex_hresult hr = alpha_coverage(ctx, src[0], 1.0f, alphaReference, &target);
    if (hr != DXTEX_S_OK) return hr;
    const FmtInfo* f = format_info(src[0].format);
    const size_t rowBytes = (src[0].width * f->bpp + 7) / 8;
    HIP_TRY(ctx, hipMemcpy2DAsync(dst[0].pixels, dst[0].rowPitch, src[0].pixels, src[0].rowPitch, std::min(rowBytes, std::min(src[0].rowPitch, dst[0].rowPitch)), src[0].height,
                                  hipMemcpyDeviceToDevice, ctx->stream));
    for (size_t level = 1; level < nlevels; ++level)
    {
        float lo = 0.0f, hi = 4.0f, scale = 1.0f;
        for (int i = 0; i < 10; ++i)
        {
            float cov = 0.0f;
            hr = alpha_coverage(ctx, src[level], scale, alphaReference, &cov);
            if (hr != DXTEX_S_OK) return hr;
            if (cov < target) lo = scale;
            else if (cov > target) hi = scale;
            else break;
            scale = (lo + hi) * 0.5f;
        }
        hr = launched(ctx, launch_scale_alpha(view_of(src[level]), view_of(dst[level]), scale, ctx->stream, marks_of(ctx)));
        if (hr != DXTEX_S_OK) return hr;
    }
    return DXTEX_S_OK;
}
} // namespace

dxtex_hresult dxtex_premultiply_alpha_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags)
{
    dxtex_hresult hr = check_pmalpha(ctx, src, dst);
    if (hr != DXTEX_S_OK) return hr;
    return run_timed(ctx, [&] { return submit_pmalpha(ctx, *src, *dst, flags); });
}

dxtex_hresult dxtex_premultiply_alpha(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags)
{
    dxtex_hresult hr = check_pmalpha(ctx, src, dst);
    if (hr != DXTEX_S_OK) return hr;
    return run_host_twin(ctx, src, dst, [&](const dxtex_image& s, const dxtex_image& d) { return submit_pmalpha(ctx, s, d, flags); });
}

dxtex_hresult dxtex_scale_mips_alpha_for_coverage_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, size_t nlevels, float alphaReference)
{
    dxtex_hresult hr = check_coverage_chain(ctx, src, dst, nlevels);
    if (hr != DXTEX_S_OK) return hr;
    ScopedDevice sd(ctx->device);
    return submit_coverage_chain(ctx, src, dst, nlevels, alphaReference);
}

dxtex_hresult dxtex_scale_mips_alpha_for_coverage(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, size_t nlevels, float alphaReference)
{
    dxtex_hresult hr = check_coverage_chain(ctx, src, dst, nlevels);
    if (hr != DXTEX_S_OK) return hr;
    StagingPlan plan;
    std::vector<StagePart> ps(nlevels), pd(nlevels);
    for (size_t i = 0; i < nlevels; ++i)
    {
        ps[i] = plan.in(src[i].rowPitch, src[i].height); pd[i] = plan.out(dst[i].rowPitch, dst[i].height);
        plan.upload(src[i].pixels, ps[i], ps[i].bytes);
        plan.download(dst[i].pixels, pd[i], pd[i].bytes);
    }
    // (the chain reads its counts back as it goes: untimed, as the device form is)
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out)
    {
        std::vector<dxtex_image> s(nlevels), d(nlevels);
        for (size_t i = 0; i < nlevels; ++i) { s[i] = with_pixels(src[i], in + ps[i].at); d[i] = with_pixels(dst[i], out + pd[i].at); }
        HIP_TRY(ctx, hipMemsetAsync(out, 0, plan.need(STAGE_OUT), ctx->stream));
        return submit_coverage_chain(ctx, s.data(), d.data(), nlevels, alphaReference);
    }, false);
}

dxtex_hresult dxtex_compute_mse_device(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, double mse[4])
{
    dxtex_hresult hr = check_pair(ctx, a, b);
    if (hr != DXTEX_S_OK) return hr;
    if (!mse) return fail(ctx, DXTEX_E_POINTER, "null result");
    const FmtInfo* fa = format_info(a->format);
    const FmtInfo* fb = format_info(b->format);
    if (!fa || !fb || (fa->cls & FC_BC) || (fb->cls & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "ComputeMSE takes uncompressed images (decompress first)");
    ScopedDevice sd(ctx->device);
    hr = ctx->resultCell.grow(ctx, 4 * sizeof(double)); if (hr != DXTEX_S_OK) return hr;
    hr = launched(ctx, launch_mse(view_of(*a), view_of(*b), static_cast<double*>(ctx->resultCell.p), ctx->stream, marks_of(ctx)));
    if (hr != DXTEX_S_OK) return hr;
    double sum[4];
    HIP_TRY(ctx, counted_copy(ctx, sum, ctx->resultCell.p, sizeof(sum), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const double n = double(a->width) * double(a->height);
    for (int c = 0; c < 4; ++c) mse[c] = sum[c] / n;
    return DXTEX_S_OK;
}

// ---- texdiag's diagnostics: Analyze, AnalyzeBC, ComputeMSE with flags, Difference ------------------------------------------------------
namespace
{
// an uncompressed image the scanline layer loads, of a size the kernels index: what all but AnalyzeBC take
dxtex_hresult check_diag_image(dxtex_ctx* ctx, const dxtex_image& im)
{
    if (!im.pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    const FmtInfo* f = format_info(im.format);
    if (!f || (f->cls & FC_BC)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "the diagnostics take uncompressed images of a loadable format (decompress first)");
    if (im.width > 0xFFFFFFFFull || im.height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    return DXTEX_S_OK;
}

dxtex_hresult check_analyze(dxtex_ctx* ctx, const dxtex_image* images, size_t count, dxtex_image_stats* stats)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!stats) return fail(ctx, DXTEX_E_POINTER, "null result");
    if (!images || !count) return fail(ctx, DXTEX_E_INVALIDARG, "no images");
    for (size_t i = 0; i < count; ++i)
    {
        const dxtex_hresult hr = check_diag_image(ctx, images[i]); if (hr != DXTEX_S_OK) return hr;
        if (!images[i].width || !images[i].height) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    }
    return DXTEX_S_OK;
}

// both passes of every image into one accumulator each, one copy back, then the reference's figures
dxtex_hresult submit_analyze(dxtex_ctx* ctx, const dxtex_image* images, size_t count, dxtex_image_stats* stats)
{
    dxtex_hresult hr = ctx->resultCell.grow(ctx, count * sizeof(AnalyzeAcc)); if (hr != DXTEX_S_OK) return hr;
    AnalyzeAcc* acc = static_cast<AnalyzeAcc*>(ctx->resultCell.p);
    hr = run_timed(ctx, [&]
    {
        HIP_TRY(ctx, hipMemsetAsync(acc, 0, count * sizeof(AnalyzeAcc), ctx->stream));
        for (size_t i = 0; i < count; ++i)
        {
            const dxtex_hresult hr1 = launched(ctx, launch_analyze(view_of(images[i]), acc + i, ctx->stream, marks_of(ctx)));
            if (hr1 != DXTEX_S_OK) return hr1;
        }
        return DXTEX_S_OK;
    });
    if (hr != DXTEX_S_OK) return hr;
    std::vector<AnalyzeAcc> host(count);
    HIP_TRY(ctx, counted_copy(ctx, host.data(), acc, count * sizeof(AnalyzeAcc), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < count; ++i)
    {
        const double n = double(images[i].width) * double(images[i].height);
        dxtex_image_stats& s = stats[i];
        for (int c = 0; c < 4; ++c)
        {
            s.min[c] = dg_min_of(host[i].minKeyInv[c]);
            s.max[c] = dg_max_of(host[i].maxKey[c]);
            s.avg[c] = host[i].sum[c] / n;
            s.variance[c] = host[i].variance[c];
            s.specials[c] = host[i].specials[c];
        }
        s.luminance = dg_float(host[i].lumBits);
    }
    return DXTEX_S_OK;
}

dxtex_hresult check_analyze_bc(dxtex_ctx* ctx, const dxtex_image* image, const uint64_t* hist, const uint64_t* blocks)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!hist || !blocks) return fail(ctx, DXTEX_E_POINTER, "null result");
    if (!image) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    if (!image->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (!is_bc(image->format) || !dg_bc_block_bytes(image->format)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "AnalyzeBC takes a block-compressed image");
    if (image->width > 0xFFFFFFFFull || image->height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    return DXTEX_S_OK;
}

// the histogram of `image` into hist (device memory, kBcHistBins counters)
dxtex_hresult submit_bc_hist(dxtex_ctx* ctx, const dxtex_image& image, unsigned long long* hist)
{
    HIP_TRY(ctx, hipMemsetAsync(hist, 0, kBcHistBins * sizeof(unsigned long long), ctx->stream));
    return launched(ctx, launch_bc_hist(view_of(image), hist, ctx->stream, marks_of(ctx)));
}
uint64_t bc_block_count(const dxtex_image& image) { return uint64_t((image.width + 3) / 4) * uint64_t((image.height + 3) / 4); }

dxtex_hresult check_difference(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!a || !b || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    if (!a->pixels || !b->pixels || !dst->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (a->width != b->width || a->height != b->height || a->width != dst->width || a->height != dst->height) return fail(ctx, DXTEX_E_FAIL, "size mismatch");
    const dxtex_hresult hr = check_diag_image(ctx, *a); if (hr != DXTEX_S_OK) return hr;
    if (b->format != FMT_R32G32B32A32_FLOAT) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "the second image of Difference must be R32G32B32A32_FLOAT (convert it first)");
    if (dst->format != a->format) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "the difference map has the first image's format");
    if (b->rowPitch % 16) return fail(ctx, DXTEX_E_INVALIDARG, "the second image's rowPitch must be a multiple of 16 (its rows are read as float4)");
    return DXTEX_S_OK;
}

dxtex_hresult submit_difference(dxtex_ctx* ctx, const dxtex_image& a, const dxtex_image& b, const dxtex_image& dst, uint32_t diffColor, float threshold)
{
    if (!a.width || !a.height) return DXTEX_S_OK;
    KernelMarks* marks = marks_of(ctx);
    const ImgView av = view_of(a), bv = view_of(b);
    return launch_into(ctx, view_of(dst), marks, [&](const ImgView& out) { return launch_difference(av, bv, out, diffColor & 0xFFFFFFu, threshold, ctx->stream, marks); });
}
} // namespace

dxtex_hresult dxtex_compute_mse_flags_device(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, uint32_t cmse_flags, double mse[4])
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!a || !b) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    if (!a->pixels || !b->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (!mse) return fail(ctx, DXTEX_E_POINTER, "null result");
    if (a->width != b->width || a->height != b->height) return fail(ctx, DXTEX_E_INVALIDARG, "size mismatch");     // DirectXTexMisc.cpp:398
    dxtex_hresult hr = check_diag_image(ctx, *a); if (hr != DXTEX_S_OK) return hr;
    hr = check_diag_image(ctx, *b); if (hr != DXTEX_S_OK) return hr;
    if (!a->width || !a->height) return fail(ctx, DXTEX_E_INVALIDARG, "empty image");
    ScopedDevice sd(ctx->device);
    hr = ctx->resultCell.grow(ctx, 4 * sizeof(double)); if (hr != DXTEX_S_OK) return hr;
    hr = run_timed(ctx, [&] { return launched(ctx, launch_mse_flags(view_of(*a), view_of(*b), cmse_flags, static_cast<double*>(ctx->resultCell.p), ctx->stream, marks_of(ctx))); });
    if (hr != DXTEX_S_OK) return hr;
    double sum[4];
    HIP_TRY(ctx, counted_copy(ctx, sum, ctx->resultCell.p, sizeof(sum), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const double n = double(a->width) * double(a->height);
    for (int c = 0; c < 4; ++c) mse[c] = sum[c] / n;
    return DXTEX_S_OK;
}

dxtex_hresult dxtex_analyze_device(dxtex_ctx* ctx, const dxtex_image* images, size_t count, dxtex_image_stats* stats_out)
{
    const dxtex_hresult hr = check_analyze(ctx, images, count, stats_out);
    if (hr != DXTEX_S_OK) return hr;
    ScopedDevice sd(ctx->device);
    return submit_analyze(ctx, images, count, stats_out);
}

dxtex_hresult dxtex_analyze(dxtex_ctx* ctx, const dxtex_image* images, size_t count, dxtex_image_stats* stats_out)
{
    dxtex_hresult hr = check_analyze(ctx, images, count, stats_out);
    if (hr != DXTEX_S_OK) return hr;
    // every image a part of the input staging; nothing comes down through it (submit_analyze times itself and brings its figures back)
    StagingPlan plan;
    std::vector<StagePart> part(count);
    for (size_t i = 0; i < count; ++i)
    {
        size_t bytes = 0;
        hr = host_image_bytes(ctx, images[i], &bytes); if (hr != DXTEX_S_OK) return hr;
        part[i] = plan.in(bytes);
        plan.upload(images[i].pixels, part[i], bytes);
    }
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t*)
    {
        std::vector<dxtex_image> staged(count);
        for (size_t i = 0; i < count; ++i) staged[i] = with_pixels(images[i], in + part[i].at);
        return submit_analyze(ctx, staged.data(), count, stats_out);
    }, false);
}

dxtex_hresult dxtex_analyze_bc_device(dxtex_ctx* ctx, const dxtex_image* image, uint64_t hist[15], uint64_t* blocks)
{
    dxtex_hresult hr = check_analyze_bc(ctx, image, hist, blocks);
    if (hr != DXTEX_S_OK) return hr;
    ScopedDevice sd(ctx->device);
    hr = ctx->resultCell.grow(ctx, kBcHistBins * sizeof(unsigned long long)); if (hr != DXTEX_S_OK) return hr;
    hr = run_timed(ctx, [&] { return submit_bc_hist(ctx, *image, static_cast<unsigned long long*>(ctx->resultCell.p)); });
    if (hr != DXTEX_S_OK) return hr;
    HIP_TRY(ctx, counted_copy(ctx, hist, ctx->resultCell.p, kBcHistBins * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *blocks = bc_block_count(*image);
    return DXTEX_S_OK;
}

dxtex_hresult dxtex_analyze_bc(dxtex_ctx* ctx, const dxtex_image* image, uint64_t hist[15], uint64_t* blocks)
{
    dxtex_hresult hr = check_analyze_bc(ctx, image, hist, blocks);
    if (hr != DXTEX_S_OK) return hr;
    size_t bytes = 0;
    hr = host_image_bytes(ctx, *image, &bytes);
    if (hr != DXTEX_S_OK) return hr;
    hr = run_staged(ctx, image->pixels, bytes, hist, kBcHistBins * sizeof(uint64_t),
                    [&](uint8_t* in, uint8_t* out) { return submit_bc_hist(ctx, with_pixels(*image, in), reinterpret_cast<unsigned long long*>(out)); });
    if (hr != DXTEX_S_OK) return hr;
    *blocks = bc_block_count(*image);
    return DXTEX_S_OK;
}

dxtex_hresult dxtex_difference_device(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, uint32_t diffColor, float threshold)
{
    const dxtex_hresult hr = check_difference(ctx, a, b, dst);
    if (hr != DXTEX_S_OK) return hr;
    if (reinterpret_cast<uintptr_t>(b->pixels) % 16) return fail(ctx, DXTEX_E_INVALIDARG, "the second image's pixels must be 16-byte aligned");
    return run_timed(ctx, [&] { return submit_difference(ctx, *a, *b, *dst, diffColor, threshold); });
}

dxtex_hresult dxtex_difference(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, uint32_t diffColor, float threshold)
{
    dxtex_hresult hr = check_difference(ctx, a, b, dst);
    if (hr != DXTEX_S_OK) return hr;
    return run_staged_pair(ctx, a, b, dst, [&](const dxtex_image& sa, const dxtex_image& sb, const dxtex_image& sd) { return submit_difference(ctx, sa, sb, sd, diffColor, threshold); });
}

// ---- CopyRectangle and texassemble's merge ----------------------------------------------------------------------------------------------
namespace
{
// IsPlanar / IsPalettized (DirectXTexUtil.cpp): with IsCompressed, what CopyRectangle refuses first (:286-289)
bool copy_refused_format(int f)
{
    const bool bc = (f >= 70 && f <= 84) || (f >= 94 && f <= 99);
    const bool planar = f == 103 || f == 104 || f == 105 || f == 106 || f == 110 || f == 118 || f == 119 || f == 120 || f == 130;     // NV12 P010 P016 420_OPAQUE NV11, Xbox depth planes, P208
    const bool palettised = f >= 111 && f <= 114;       // AI44 IA44 P8 A8P8
    return bc || planar || palettised;
}

// CopyRectangle's checks in its order (DirectXTexMisc.cpp:283-311, :328, :365), then this project's additions; appends the rectangle's job
// (two where its destination rows overlap each other) to `jobs`.
dxtex_hresult check_copy_rect(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_rect& r, const dxtex_image& dst, uint32_t filter, size_t xOffset, size_t yOffset,
                              std::vector<CopyJob>* jobs)
{
    if (!src.pixels || !dst.pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (copy_refused_format(src.format) || copy_refused_format(dst.format))
        return fail(ctx, DXTEX_E_NOT_SUPPORTED, "CopyRectangle does not take compressed, planar or palettised formats");
    // (written so that no sum wraps: x + w > width  <=>  w > width || x > width - w)
    if (!r.w || !r.h || r.w > src.width || r.x > src.width - r.w || r.h > src.height || r.y > src.height - r.h)
        return fail(ctx, DXTEX_E_INVALIDARG, "the rectangle is empty or outside the source");
    if (r.w > dst.width || xOffset > dst.width - r.w || r.h > dst.height || yOffset > dst.height - r.h)
        return fail(ctx, DXTEX_E_INVALIDARG, "the rectangle at its offset is outside the destination");
    const FmtInfo* in = format_info(src.format);
    const FmtInfo* out = format_info(dst.format);
    // BitsPerPixel() == 0 (:303-305, :341-343): a value that names no format; below 8 bits: R1_UNORM (:307-311, :345-349)
    const auto known = [](int f) { return (f >= 1 && f <= 120) || (f >= 130 && f <= 132) || (f >= 189 && f <= 191); };
    for (const int f : { src.format, dst.format })
    {
        if (!known(f)) return fail(ctx, DXTEX_E_INVALIDARG, "unknown format");
        if (f == FMT_R1_UNORM) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "CopyRectangle does not take R1_UNORM");
    }
    if (!in || !out) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "format is not supported by the MI355X path");
    if (src.width > 0xFFFFFFFFull || src.height > 0xFFFFFFFFull || dst.width > 0xFFFFFFFFull || dst.height > 0xFFFFFFFFull)
        return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    const bool same = src.format == dst.format;
    if (!same && ((in->cls | out->cls) & FC_GROUP))
        return fail(ctx, DXTEX_E_NOT_SUPPORTED, "CopyRectangle between different formats does not take the packed two-texel formats");
    const uint64_t sbpp = copy_texel_bytes(*in), dbpp = copy_texel_bytes(*out);
    const uint64_t rowsS = uint64_t(src.height), rowsD = uint64_t(dst.height);
    if (src.rowPitch > UINT64_MAX / std::max<uint64_t>(1, rowsS) || dst.rowPitch > UINT64_MAX / std::max<uint64_t>(1, rowsD))
        return fail(ctx, DXTEX_E_INVALIDARG, "rowPitch x rows overflows");
    // the bytes of the last row touched must end inside rowPitch * height on both sides: the reference's E_FAIL (:328, :365), made a
    // check of the destination's end too (the reference's same-format test, pDest > pEndDest, lets a write run past the image)
    const uint64_t srcFirst = uint64_t(r.y) * src.rowPitch + uint64_t(r.x) * sbpp, srcLast = srcFirst + uint64_t(r.h - 1) * src.rowPitch + uint64_t(r.w) * sbpp;
    const uint64_t dstFirst = uint64_t(yOffset) * dst.rowPitch + uint64_t(xOffset) * dbpp, dstLast = dstFirst + uint64_t(r.h - 1) * dst.rowPitch + uint64_t(r.w) * dbpp;
    if (srcLast > src.rowPitch * rowsS || dstLast > dst.rowPitch * rowsD) return fail(ctx, DXTEX_E_FAIL, "the rectangle's bytes run past the end of an image");
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src.pixels) + srcFirst, s1 = reinterpret_cast<uintptr_t>(src.pixels) + srcLast;
    const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst.pixels) + dstFirst, d1 = reinterpret_cast<uintptr_t>(dst.pixels) + dstLast;
    if (s0 < d1 && d0 < s1) return fail(ctx, DXTEX_E_INVALIDARG, "source and destination pixels overlap");

    CopyJob j = {};
    j.srcPitch = src.rowPitch; j.dstPitch = dst.rowPitch;
    j.height = uint32_t(r.h);
    j.srcFormat = src.format; j.dstFormat = dst.format;
    if (same)
    {
        j.src = src.pixels + srcFirst; j.dst = dst.pixels + dstFirst;
        const uint64_t rowBytes = uint64_t(r.w) * sbpp;
        j.vec = copy_access_bytes(s0, d0, src.rowPitch, dst.rowPitch, j.height);
        if (rowBytes / j.vec + 16u > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "rectangle too large");      // width + tail (below 16) stays a uint32_t
        j.width = uint32_t(rowBytes / j.vec); j.tail = uint32_t(rowBytes % j.vec);
        if (j.height > 1 && rowBytes > dst.rowPitch)
        {
            // A row of the packed formats can be longer than the destination's pitch: consecutive rows then write the same bytes, and in the
            // reference's row-by-row memcpy the later row wins. Row y + 1 covers everything of row y from its pitch on, so every row but the
            // last moves its first dstPitch bytes only and the last row moves all of its bytes: the same result, with no byte written twice.
            CopyJob last = j;
            last.src += uint64_t(j.height - 1) * j.srcPitch; last.dst += uint64_t(j.height - 1) * j.dstPitch;
            last.height = 1;
            last.vec = copy_access_bytes(reinterpret_cast<uintptr_t>(last.src), reinterpret_cast<uintptr_t>(last.dst), 0, 0, 1);
            last.width = uint32_t(rowBytes / last.vec); last.tail = uint32_t(rowBytes % last.vec);
            j.height -= 1;
            j.width = uint32_t(dst.rowPitch / j.vec); j.tail = uint32_t(dst.rowPitch % j.vec);
            jobs->push_back(j);
            jobs->push_back(last);
            return DXTEX_S_OK;
        }
    }
    else
    {
        j.src = src.pixels + uint64_t(r.y) * src.rowPitch; j.dst = dst.pixels + uint64_t(yOffset) * dst.rowPitch;
        j.width = uint32_t(r.w); j.sx = uint32_t(r.x); j.dx = uint32_t(xOffset);
        j.plan = resolve_convert_plan(*in, *out, filter & ~(kFilterDitherOrdered | kFilterDitherDiffusion));      // CopyRectangle never dithers
    }
    jobs->push_back(j);
    return DXTEX_S_OK;
}

dxtex_hresult check_merge(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, const uint32_t* permute, const uint32_t* zero,
                          const uint32_t* one, MergeArgs* args)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!a || !b || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    if (!permute || !zero || !one) return fail(ctx, DXTEX_E_POINTER, "null permute / zero / one");
    if (!a->pixels || !b->pixels || !dst->pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    const dxtex_hresult hr = check_diag_image(ctx, *a); if (hr != DXTEX_S_OK) return hr;
    if (b->format != FMT_R32G32B32A32_FLOAT) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "the second image of a merge must be R32G32B32A32_FLOAT (convert it first)");
    if (dst->format != a->format) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "the merged image has the first image's format");
    if (a->width != b->width || a->height != b->height || a->width != dst->width || a->height != dst->height) return fail(ctx, DXTEX_E_FAIL, "size mismatch");
    if (b->rowPitch % 16) return fail(ctx, DXTEX_E_INVALIDARG, "the second image's rowPitch must be a multiple of 16 (its rows are read as float4)");
    MergeArgs m = {};
    for (int k = 0; k < 4; ++k)
    {
        if (permute[k] > 7) return fail(ctx, DXTEX_E_INVALIDARG, "permute index above 7");
        m.sel[k] = permute[k];
        if (zero[k]) m.zero |= 1u << k;
        if (one[k]) m.one |= 1u << k;
    }
    if (a->width && a->height)
    {
        dxtex_hresult ov = check_no_overlap(ctx, *a, *dst); if (ov != DXTEX_S_OK) return ov;
        ov = check_no_overlap(ctx, *b, *dst); if (ov != DXTEX_S_OK) return ov;
    }
    *args = m;
    return DXTEX_S_OK;
}

dxtex_hresult submit_merge(dxtex_ctx* ctx, const dxtex_image& a, const dxtex_image& b, const dxtex_image& dst, const MergeArgs& args)
{
    if (!a.width || !a.height) return DXTEX_S_OK;
    KernelMarks* marks = marks_of(ctx);
    const ImgView av = view_of(a), bv = view_of(b);
    return launch_into(ctx, view_of(dst), marks, [&](const ImgView& out) { return launch_merge(av, bv, out, args, ctx->stream, marks); });
}
} // namespace

dxtex_hresult dxtex_copy_rectangles_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_rect* rects, const dxtex_image* dsts, const size_t* xOffsets,
                                           const size_t* yOffsets, size_t count, uint32_t filter)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!srcs || !rects || !dsts || !xOffsets || !yOffsets || !count) return fail(ctx, DXTEX_E_INVALIDARG, "no rectangles");
    std::vector<CopyJob> jobs;
    jobs.reserve(count);
    for (size_t i = 0; i < count; ++i)
    {
        const dxtex_hresult hr = check_copy_rect(ctx, srcs[i], rects[i], dsts[i], filter, xOffsets[i], yOffsets[i], &jobs);
        if (hr != DXTEX_S_OK) return hr;
    }
    return run_timed(ctx, [&] { return launched(ctx, launch_copy_rects(jobs.data(), jobs.size(), ctx->stream, marks_of(ctx))); });
}

dxtex_hresult dxtex_copy_rectangle(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_rect* rect, const dxtex_image* dst, uint32_t filter, size_t xOffset, size_t yOffset)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !rect || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image or rectangle");
    std::vector<CopyJob> host, jobs;
    const dxtex_hresult hr = check_copy_rect(ctx, *src, *rect, *dst, filter, xOffset, yOffset, &host);
    if (hr != DXTEX_S_OK) return hr;
    // Only the rectangle travels: its rows go up into a tight image in the staging, the same rectangle of a tight destination comes back
    // into the caller's rows. (Nothing else of the caller's destination is read or written, so its other bytes stay as they were.)
    const size_t sbpp = copy_texel_bytes(*format_info(src->format)), dbpp = copy_texel_bytes(*format_info(dst->format));
    const size_t upRow = rect->w * sbpp, downRow = rect->w * dbpp;
    StagingPlan plan;
    plan.upload(src->pixels + rect->y * src->rowPitch + rect->x * sbpp, src->rowPitch, plan.in(upRow, rect->h), 0, upRow, upRow, rect->h);
    plan.download(dst->pixels + yOffset * dst->rowPitch + xOffset * dbpp, dst->rowPitch, plan.out(downRow, rect->h), 0, downRow, downRow, rect->h);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out)
    {
        dxtex_image s = *src, d = *dst;
        s.width = d.width = rect->w; s.height = d.height = rect->h;
        s.rowPitch = upRow; d.rowPitch = downRow;
        s.slicePitch = upRow * rect->h; d.slicePitch = downRow * rect->h;
        s.pixels = in; d.pixels = out;
        const dxtex_hresult staged = check_copy_rect(ctx, s, { 0, 0, rect->w, rect->h }, d, filter, 0, 0, &jobs);
        return staged != DXTEX_S_OK ? staged : launched(ctx, launch_copy_rects(jobs.data(), jobs.size(), ctx->stream, marks_of(ctx)));
    });
}

// ---- ConvertToSinglePlane ------------------------------------------------------------------------------------------------------------------
namespace
{
const char* plane_error(int32_t hr, const dxtex_image& src)
{
    if (hr == kPlanePointer) return "null pixels";
    if (hr == kPlaneNotSupported) return "this planar format has no single-plane form";
    if (hr == kPlaneFail) return "the destination's size differs from the source's";
    if (!plane_is_planar(src.format)) return "the source format is not planar";
    return "ConvertToSinglePlane: odd size (a width that is no multiple of four for NV11), or pitches, alignment, destination format or overlap";
}

// plane_check (dxtex_plane.h) on the caller's images: pitches are the caller's, nothing is computed from the format
dxtex_hresult check_single_plane(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst, PlaneJob* job)
{
    const PlaneImage s = { src.width, src.height, src.format, src.rowPitch, src.slicePitch, uint64_t(reinterpret_cast<uintptr_t>(src.pixels)) };
    const PlaneImage d = { dst.width, dst.height, dst.format, dst.rowPitch, dst.slicePitch, uint64_t(reinterpret_cast<uintptr_t>(dst.pixels)) };
    const int32_t hr = plane_check(s, d, job);
    return hr == kPlaneOk ? DXTEX_S_OK : fail(ctx, hr, plane_error(hr, src));
}
} // namespace

int32_t dxtex_planar_to_single(int32_t format) { return plane_to_single(format); }

dxtex_hresult dxtex_convert_to_single_plane_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!srcs || !dsts || !count) return fail(ctx, DXTEX_E_INVALIDARG, "no images");
    std::vector<PlaneJob> jobs(count);
    for (size_t i = 0; i < count; ++i)
    {
        const dxtex_hresult hr = check_single_plane(ctx, srcs[i], dsts[i], &jobs[i]);
        if (hr != DXTEX_S_OK) return hr;
    }
    return run_timed(ctx, [&] { return launched(ctx, launch_single_plane(jobs.data(), jobs.size(), ctx->stream, marks_of(ctx))); });
}

dxtex_hresult dxtex_convert_to_single_plane(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    PlaneJob host, job;
    const dxtex_hresult hr = check_single_plane(ctx, *src, *dst, &host);
    if (hr != DXTEX_S_OK) return hr;
    if (!host.elems || !host.units) return DXTEX_S_OK;
    // The source goes up as it is, slicePitch bytes with the caller's pitches; the destination in the staging has rows of the element bytes
    // rounded up to 16 (so the wide route can run), and only the elements the kernel writes come back into the caller's rows: the end guard
    // leaves whole rows first and then cut ones (plane_pairs does not grow with the unit), the whole rows in one copy.
    const size_t rowBytes = size_t(host.elems) * plane_elem_bytes(host), rows = src->height, pitch = (rowBytes + 15u) & ~size_t(15);
    const size_t unitRows = host.nv11 ? 1 : 2;
    StagingPlan plan;
    plan.upload(src->pixels, plan.in(src->slicePitch), src->slicePitch);
    const StagePart staged = plan.out(pitch, rows);
    uint32_t whole = 0;
    while (whole < host.units && plane_written_elems(host, whole) == host.elems) ++whole;
    plan.download(dst->pixels, dst->rowPitch, staged, 0, pitch, rowBytes, whole * unitRows);
    for (uint32_t unit = whole; unit < host.units; ++unit)
        for (size_t y = unit * unitRows; y < (unit + 1) * unitRows; ++y)
            plan.download(dst->pixels + y * dst->rowPitch, dst->rowPitch, staged, y * pitch, pitch, size_t(plane_written_elems(host, unit)) * plane_elem_bytes(host), 1);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out)
    {
        dxtex_image s = with_pixels(*src, in), d = with_pixels(*dst, out);
        d.rowPitch = pitch; d.slicePitch = pitch * rows;
        const dxtex_hresult again = check_single_plane(ctx, s, d, &job);
        return again != DXTEX_S_OK ? again : launched(ctx, launch_single_plane(&job, 1, ctx->stream, marks_of(ctx)));
    });
}

// ---- FlipRotate ------------------------------------------------------------------------------------------------------------------------
namespace
{
// bytes of a texel FlipRotate moves, 0 where it refuses the format: compressed and two-texel packed formats and R1_UNORM; planar, palettised
// and typeless formats and values that name no format are not in the table at all
uint32_t flip_texel_bytes(int format)
{
    const FmtInfo* f = format_info(format);
    if (!f || (f->cls & (FC_BC | FC_GROUP)) || (f->bpp % 8u)) return 0;
    return fr_texel_bytes_ok(f->bpp / 8u) ? f->bpp / 8u : 0;
}

// The checks in the order include/dxtex_amd.h gives, and the resolved job.
dxtex_hresult check_flip_rotate(dxtex_ctx* ctx, const dxtex_image& src, const dxtex_image& dst, uint32_t flags, FlipJob* job)
{
    if (!src.pixels || !dst.pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
    if (!fr_flags_legal(flags)) return fail(ctx, DXTEX_E_INVALIDARG, "flags are not TEX_FR_FLAGS that name an operation");
    const uint32_t texel = flip_texel_bytes(src.format);
    if (!texel) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "FlipRotate takes formats of one texel of 1, 2, 4, 8, 12 or 16 bytes an element");
    const FlipOp op = fr_resolve(flags);
    if (dst.format != src.format) return fail(ctx, DXTEX_E_FAIL, "the destination's format differs from the source's");
    if (dst.width != (op.transpose ? src.height : src.width) || dst.height != (op.transpose ? src.width : src.height))
        return fail(ctx, DXTEX_E_FAIL, "the destination's size is not the turned source's");
    if (src.width > 0x7FFFFFFFull || src.height > 0x7FFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image too large");
    const uint64_t srcRow = src.width * texel, dstRow = dst.width * texel;
    if (src.rowPitch < srcRow || dst.rowPitch < dstRow) return fail(ctx, DXTEX_E_INVALIDARG, "a rowPitch is below its row's bytes");
    if ((src.height && src.rowPitch > UINT64_MAX / src.height) || (dst.height && dst.rowPitch > UINT64_MAX / dst.height))
        return fail(ctx, DXTEX_E_INVALIDARG, "rowPitch x rows overflows");
    FlipJob j = {};
    j.src = src.pixels; j.dst = dst.pixels;
    j.srcPitch = src.rowPitch; j.dstPitch = dst.rowPitch;
    j.width = uint32_t(dst.width); j.height = uint32_t(dst.height);
    j.texel = texel;
    j.mirrorX = op.mirrorX; j.mirrorY = op.mirrorY;
    if (src.width && src.height)
    {
        // the bytes read and the bytes written: from the first row to the end of the last row's texels
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(src.pixels), s1 = s0 + (src.height - 1) * src.rowPitch + srcRow;
        const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst.pixels), d1 = d0 + (dst.height - 1) * dst.rowPitch + dstRow;
        if (s0 < d1 && d0 < s1) return fail(ctx, DXTEX_E_INVALIDARG, "source and destination pixels overlap");
    }
    fr_choose_route(&j, op.transpose != 0);
    *job = j;
    return DXTEX_S_OK;
}
} // namespace

dxtex_hresult dxtex_flip_rotate_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, uint32_t flags)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!srcs || !dsts || !count) return fail(ctx, DXTEX_E_INVALIDARG, "no images");
    std::vector<FlipJob> jobs(count);
    for (size_t i = 0; i < count; ++i)
    {
        const dxtex_hresult hr = check_flip_rotate(ctx, srcs[i], dsts[i], flags, &jobs[i]);
        if (hr != DXTEX_S_OK) return hr;
    }
    return run_timed(ctx, [&] { return launched(ctx, launch_flip_rotate(jobs.data(), jobs.size(), ctx->stream, marks_of(ctx))); });
}

dxtex_hresult dxtex_flip_rotate(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!src || !dst) return fail(ctx, DXTEX_E_INVALIDARG, "null image");
    FlipJob host, job;
    const dxtex_hresult hr = check_flip_rotate(ctx, *src, *dst, flags, &host);
    if (hr != DXTEX_S_OK) return hr;
    if (!host.width || !host.height) return DXTEX_S_OK;
    // Only the rows' texels travel: the source goes up into rows of its bytes rounded up to 16 (so that the wide form can run), the
    // destination's texels come back from such rows into the caller's. Nothing else of the caller's destination is read or written.
    const size_t upRow = size_t(src->width) * host.texel, downRow = size_t(dst->width) * host.texel;
    const size_t upPitch = (upRow + 15u) & ~size_t(15), downPitch = (downRow + 15u) & ~size_t(15);
    StagingPlan plan;
    plan.upload(src->pixels, src->rowPitch, plan.in(upPitch, src->height), 0, upPitch, upRow, src->height);
    plan.download(dst->pixels, dst->rowPitch, plan.out(downPitch, dst->height), 0, downPitch, downRow, dst->height);
    return run_plan(ctx, plan, [&](uint8_t* in, uint8_t* out)
    {
        dxtex_image s = with_pixels(*src, in), d = with_pixels(*dst, out);
        s.rowPitch = upPitch; s.slicePitch = upPitch * src->height;
        d.rowPitch = downPitch; d.slicePitch = downPitch * dst->height;
        const dxtex_hresult staged = check_flip_rotate(ctx, s, d, flags, &job);
        return staged != DXTEX_S_OK ? staged : launched(ctx, launch_flip_rotate(&job, 1, ctx->stream, marks_of(ctx)));
    });
}

dxtex_hresult dxtex_merge_image_device(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, const uint32_t permute[4],
                                       const uint32_t zero[4], const uint32_t one[4])
{
    MergeArgs args;
    const dxtex_hresult hr = check_merge(ctx, a, b, dst, permute, zero, one, &args);
    if (hr != DXTEX_S_OK) return hr;
    if (reinterpret_cast<uintptr_t>(b->pixels) % 16) return fail(ctx, DXTEX_E_INVALIDARG, "the second image's pixels must be 16-byte aligned");
    return run_timed(ctx, [&] { return submit_merge(ctx, *a, *b, *dst, args); });
}

dxtex_hresult dxtex_merge_image(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, const uint32_t permute[4], const uint32_t zero[4],
                                const uint32_t one[4])
{
    MergeArgs args;
    dxtex_hresult hr = check_merge(ctx, a, b, dst, permute, zero, one, &args);
    if (hr != DXTEX_S_OK) return hr;
    return run_staged_pair(ctx, a, b, dst, [&](const dxtex_image& sa, const dxtex_image& sb, const dxtex_image& sd) { return submit_merge(ctx, sa, sb, sd, args); });
}

dxtex_hresult dxtex_device_alloc(dxtex_ctx* ctx, size_t bytes, void** out)
{
    if (!ctx || !out) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, hipMalloc(out, bytes ? bytes : 1));
    return DXTEX_S_OK;
}
dxtex_hresult dxtex_device_free(dxtex_ctx* ctx, void* p)
{
    if (!ctx) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, hipFree(p));
    return DXTEX_S_OK;
}
dxtex_hresult dxtex_memcpy_h2d(dxtex_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, counted_copy(ctx, dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DXTEX_S_OK;
}
dxtex_hresult dxtex_memcpy_d2h(dxtex_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, counted_copy(ctx, dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return DXTEX_S_OK;
}

// ---- the device-resident pipeline's helpers -------------------------------------------------------------------------------------------
dxtex_hresult dxtex_device_memset(dxtex_ctx* ctx, void* p, int value, size_t bytes)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!p) return fail(ctx, DXTEX_E_POINTER, "null buffer");
    ScopedDevice sd(ctx->device);
    if (bytes) HIP_TRY(ctx, hipMemsetAsync(p, value, bytes, ctx->stream));
    return DXTEX_S_OK;
}
dxtex_hresult dxtex_copy_rows_device(dxtex_ctx* ctx, void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t rowBytes, size_t rows)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!dst || !src) return fail(ctx, DXTEX_E_POINTER, "null buffer");
    if (rowBytes > dstPitch || rowBytes > srcPitch) return fail(ctx, DXTEX_E_INVALIDARG, "row is wider than a pitch");
    ScopedDevice sd(ctx->device);
    if (rowBytes && rows) HIP_TRY(ctx, hipMemcpy2DAsync(dst, dstPitch, src, srcPitch, rowBytes, rows, hipMemcpyDeviceToDevice, ctx->stream));
    return DXTEX_S_OK;
}
dxtex_hresult dxtex_memcpy_h2d_async(dxtex_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, counted_copy(ctx, dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return DXTEX_S_OK;
}
dxtex_hresult dxtex_memcpy_d2h_async(dxtex_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!ctx) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, counted_copy(ctx, dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return DXTEX_S_OK;
}
dxtex_hresult dxtex_memcpy_rows_d2h_async(dxtex_ctx* ctx, void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t rowBytes, size_t rows)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!dst || !src) return fail(ctx, DXTEX_E_POINTER, "null buffer");
    if (rowBytes > dstPitch || rowBytes > srcPitch) return fail(ctx, DXTEX_E_INVALIDARG, "row is wider than a pitch");
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, counted_copy_rows(ctx, dst, dstPitch, src, srcPitch, rowBytes, rows, hipMemcpyDeviceToHost));
    return DXTEX_S_OK;
}
dxtex_hresult dxtex_host_alloc(dxtex_ctx* ctx, size_t bytes, void** out)
{
    if (!ctx || !out) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return DXTEX_S_OK;
}
dxtex_hresult dxtex_host_free(dxtex_ctx* ctx, void* p)
{
    if (!ctx) return DXTEX_E_POINTER;
    ScopedDevice sd(ctx->device);
    HIP_TRY(ctx, hipHostFree(p));
    return DXTEX_S_OK;
}

dxtex_hresult dxtex_alpha_all_opaque_device(dxtex_ctx* ctx, const dxtex_image* images, size_t count, int* opaque)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (!opaque) return fail(ctx, DXTEX_E_POINTER, "null result");
    *opaque = 0;
    if (!images || !count) return fail(ctx, DXTEX_E_INVALIDARG, "no images");
    const FmtInfo* f = format_info(images[0].format);
    if (!f || (f->cls & FC_GROUP)) return fail(ctx, DXTEX_E_NOT_SUPPORTED, "format is not supported by the MI355X path");
    // HasAlpha (DirectXTexUtil.cpp:340-372): of the BC formats BC1 / BC2 / BC3 / BC7 carry alpha (BC4 / BC5 have no A channel in the format
    // table, BC6H has one there but carries none); a format without alpha is opaque (:805-806)
    const bool bc = (f->cls & FC_BC) != 0;
    if (!(f->cls & FC_A) || is_bc6h(f->format)) { *opaque = 1; return DXTEX_S_OK; }
    ScopedDevice sd(ctx->device);
    dxtex_hresult hr = ctx->resultCell.grow(ctx, 4 * sizeof(double)); if (hr != DXTEX_S_OK) return hr;
    unsigned long long* counter = static_cast<unsigned long long*>(ctx->resultCell.p);
    HIP_TRY(ctx, hipMemsetAsync(counter, 0, sizeof(unsigned long long), ctx->stream));
    for (size_t i = 0; i < count; ++i)
    {
        const dxtex_image& im = images[i];
        if (!im.pixels) return fail(ctx, DXTEX_E_POINTER, "null pixels");
        if (im.format != images[0].format) return fail(ctx, DXTEX_E_FAIL, "format mismatch");
        if (!im.width || !im.height || im.width > 0xFFFFFFFFull || im.height > 0xFFFFFFFFull) return fail(ctx, DXTEX_E_INVALIDARG, "image size");
        hipError_t e;
        if (bc)
        {
            // IsAlphaAllOpaqueBC decodes every block to floats and tests the texels inside the image against 0.99
            const size_t pitch = im.width * 16;
            hr = ctx->stageOut.grow(ctx, pitch * im.height); if (hr != DXTEX_S_OK) return hr;
            const dxtex_image decoded = { im.width, im.height, FMT_R32G32B32A32_FLOAT, pitch, pitch * im.height, ctx->stageOut.u8() };
            hr = submit_decompress(ctx, im, decoded);
            if (hr != DXTEX_S_OK) return hr;
            e = launch_alpha_below(view_of(decoded), 0.99f, counter, ctx->stream, marks_of(ctx));
        }
        else
            e = launch_alpha_below(view_of(im), 0.997f, counter, ctx->stream, marks_of(ctx));
        hr = launched(ctx, e);
        if (hr != DXTEX_S_OK) return hr;
    }
    unsigned long long n = 0;
    HIP_TRY(ctx, counted_copy(ctx, &n, counter, sizeof(n), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *opaque = n ? 0 : 1;
    return DXTEX_S_OK;
}

dxtex_hresult dxtex_ctx_transfer_bytes(dxtex_ctx* ctx, uint64_t* h2d_bytes, uint64_t* d2h_bytes, int reset)
{
    if (!ctx) return DXTEX_E_POINTER;
    if (h2d_bytes) *h2d_bytes = ctx->h2dBytes;
    if (d2h_bytes) *d2h_bytes = ctx->d2hBytes;
    if (reset) ctx->h2dBytes = ctx->d2hBytes = 0;
    return DXTEX_S_OK;
}
} // extern "C"

// ---- ONE image over several contexts (one process, N GPUs - or N contexts of one GPU) -------------------------------------------------
// Blocks are independent (DirectXTexCompress.cpp:257-281 is the reference's own split of an image's block rows over OpenMP threads), and a
// destination row of a 2:1 filter needs a bounded window of source rows (cubic: one source row above the pair it covers and one below,
// filters.h:176-179). So an image in host memory is cut into stripes of (block) rows, one per context, each stripe goes through the
// single-context entry point on a thread of its own, and the stripes land in the caller's destination: the bytes of the one-context call.
namespace
{
// Returns the first failing stripe's result and, through *failed, its index (so that the caller can surface that context's error text).
template<class F>
dxtex_hresult run_stripes(size_t n, F&& stripe, size_t* failed = nullptr)
{
    std::vector<dxtex_hresult> hr(n, DXTEX_S_OK);
    std::vector<std::thread> workers;
    // (a stripe that runs out of host memory reports it like any other failure: nothing may leave a worker thread as an exception)
    auto guarded = [&](size_t i) { try { hr[i] = stripe(i); } catch (...) { hr[i] = DXTEX_E_OUTOFMEMORY; } };
    try { for (size_t i = 1; i < n; ++i) workers.emplace_back(guarded, i); }
    catch (...) { for (std::thread& t : workers) t.join(); return DXTEX_E_OUTOFMEMORY; }
    guarded(0);
    for (std::thread& t : workers) t.join();
    for (size_t i = 0; i < n; ++i) if (hr[i] != DXTEX_S_OK) { if (failed) *failed = i; return hr[i]; }
    return DXTEX_S_OK;
}

// Every stripe runs on a context of its own (a context's staging buffers and stream serve one call at a time): the same context twice is
// the caller's error. A failing stripe's text is copied to the first context, where the caller of a multi-context call looks for it.
dxtex_hresult check_distinct(dxtex_ctx* const* ctxs, size_t nctx)
{
    for (size_t i = 0; i < nctx; ++i)
        for (size_t j = i + 1; j < nctx; ++j)
            if (ctxs[i] == ctxs[j]) return fail(ctxs[0], DXTEX_E_INVALIDARG, "the same context listed twice");
    return DXTEX_S_OK;
}
dxtex_hresult surface_stripe_error(dxtex_ctx* const* ctxs, dxtex_hresult hr, size_t failed)
{
    if (hr != DXTEX_S_OK && failed != 0)
    {
        try { ctxs[0]->lastError = "stripe " + std::to_string(failed) + ": " + ctxs[failed]->lastError; } catch (...) { }
    }
    return hr;
}
} // namespace

extern "C" {
dxtex_hresult dxtex_compress_multi(dxtex_ctx* const* ctxs, size_t nctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags, float threshold)
{
    if (!ctxs || !nctx || !ctxs[0]) return DXTEX_E_POINTER;
    for (size_t i = 0; i < nctx; ++i) if (!ctxs[i]) return DXTEX_E_POINTER;
    if (!src || !dst) return fail(ctxs[0], DXTEX_E_INVALIDARG, "null image");
    const size_t nbh = (src->height + 3) / 4;
    const size_t n = std::max<size_t>(1, std::min(nctx, nbh));
    if (n == 1 || src->width != dst->width || src->height != dst->height) return dxtex_compress(ctxs[0], src, dst, flags, threshold);      // (a mismatch is the single call's error to report)
    // the whole image is validated ONCE, before any stripe pointer is formed from it (a stripe's `pixels + y0 * rowPitch` of a null image
    // would pass the stripes' own null test): the checks of the single-context call, on the first context
    dxtex_hresult hr = check_pair(ctxs[0], src, dst);
    if (hr != DXTEX_S_OK) return hr;
    { size_t sb = 0, db = 0; hr = check_host_pitches(ctxs[0], src, dst, &sb, &db); if (hr != DXTEX_S_OK) return hr; }
    hr = check_distinct(ctxs, n); if (hr != DXTEX_S_OK) return hr;
    size_t failed = 0;
    hr = run_stripes(n, [&](size_t i) -> dxtex_hresult
    {
        const size_t b0 = nbh * i / n, b1 = nbh * (i + 1) / n;            // block rows [b0, b1)
        if (b1 <= b0) return DXTEX_S_OK;
        const size_t y0 = b0 * 4, rows = std::min(src->height, b1 * 4) - y0;
        dxtex_image s = *src, d = *dst;
        s.pixels = src->pixels + y0 * src->rowPitch; s.height = rows; s.slicePitch = src->rowPitch * rows;
        d.pixels = dst->pixels + b0 * dst->rowPitch; d.height = rows; d.slicePitch = dst->rowPitch * (b1 - b0);
        return dxtex_compress(ctxs[i], &s, &d, flags, threshold);
    }, &failed);
    return surface_stripe_error(ctxs, hr, failed);
}

dxtex_hresult dxtex_generate_mips_multi(dxtex_ctx* const* ctxs, size_t nctx, const dxtex_image* levels, size_t nlevels, uint32_t filter)
{
    if (!ctxs || !nctx) return DXTEX_E_POINTER;
    for (size_t i = 0; i < nctx; ++i) if (!ctxs[i]) return DXTEX_E_POINTER;
    uint32_t mode = 0;
    const dxtex_hresult hc = check_mips(ctxs[0], levels, nlevels, filter, &mode);
    if (hc != DXTEX_S_OK) return hc;
    { const dxtex_hresult hd = check_distinct(ctxs, nctx); if (hd != DXTEX_S_OK) return hd; }
    const uint32_t explicitFilter = (filter & ~kFilterModeMask) | mode;      // the sub-chains below must not choose again (a stripe is not a power of two high)
    // A level is split while it is an exact halving, large enough to be worth a context of its own, and filtered by a kernel whose taps
    // are a fixed window around the destination row: point / box (the 2 x 2 source texels), linear and cubic with clamp addressing in V
    // (u = (y + 0.5) * 2 - 0.5 is exact in fp32, so a stripe's rows get the weights the whole image's rows get). The triangle filter (a
    // gather over the whole axis) and V wrap / mirror go to the first context whole, as does the chain below kSplitMinRows.
    //
    // Round 6: the stripes stay RESIDENT. A context computes rows of every split level from its own copy of the level above and never
    // exchanges anything: destination rows [a, b) of a level come from source rows [2 a - 2, 2 b + 2) of the level above (cubic reads one
    // row above the pair it covers and one below, filters.h:176-179; a sub-image is resized with one throw-away destination row on either
    // inner side, whose taps run into the sub-image's clamped edge), so working back from the stripe a context owns at the LAST split level
    // gives the rows it needs of every level above - its own stripe plus a halo that doubles per level (3 * 2^k rows k levels up: 48 rows
    // of level 0 for four split levels, against stripes of hundreds). One upload per context (its rows of level 0), the levels chained on
    // the device, one download per context (its stripes of levels 1 ... L): every byte crosses the host link once, and on N GPUs no byte
    // crosses between them. (Round 5 went host -> device -> host once per level and stripe.)
    constexpr size_t kSplitMinRows = 256;
    const bool splittable = nctx > 1 && (mode == DXTEX_FILTER_POINT || mode == DXTEX_FILTER_BOX || mode == DXTEX_FILTER_LINEAR || mode == DXTEX_FILTER_CUBIC) &&
                            !(filter & (DXTEX_FILTER_WRAP_V | DXTEX_FILTER_MIRROR_V));
    size_t lv = 1;      // levels [1, lv) are split
    for (; splittable && lv < nlevels; ++lv)
    {
        const dxtex_image& S = levels[lv - 1];
        const dxtex_image& D = levels[lv];
        if (S.width != 2 * D.width || S.height != 2 * D.height || D.height < kSplitMinRows || D.height < 4 * nctx) break;
    }
    const size_t L = lv - 1;                          // the last split level (0: nothing to split)
    if (L >= 1)
    {
        struct Rows { size_t a, b; };
        size_t failed = 0;
        const dxtex_hresult hr = run_stripes(nctx, [&](size_t i) -> dxtex_hresult
        {
            dxtex_ctx* ctx = ctxs[i];
            auto owned = [&](size_t l) { const size_t H = levels[l].height; return Rows{ H * i / nctx, H * (i + 1) / nctx }; };
            // C[l]: rows of level l this context must hold CORRECT; E[l]: rows it computes (C[l] plus the throw-away rows); S[l - 1] = [2 E[l].a, 2 E[l].b):
            // the sub-image of level l - 1 they are computed from
            std::vector<Rows> C(L + 1), E(L + 1);
            C[L] = owned(L);
            for (size_t l = L; l >= 1; --l)
            {
                const size_t H = levels[l].height;
                E[l] = Rows{ C[l].a ? C[l].a - 1 : 0, std::min(C[l].b + 1, H) };
                C[l - 1] = Rows{ 2 * E[l].a, 2 * E[l].b };
                if (l - 1 >= 1)                       // the level above is an output too: its own stripe must be inside what is held (it is: the halo grows faster than the stripes' rounding)
                {
                    const Rows o = owned(l - 1);
                    C[l - 1].a = std::min(C[l - 1].a, o.a); C[l - 1].b = std::max(C[l - 1].b, o.b);
                }
            }
            E[0] = C[0];
            if (C[L].b <= C[L].a) return DXTEX_S_OK;
            // one arena for the context's rows of every level (the staging buffer of the single-image calls, reused across calls)
            std::vector<size_t> bytes(L + 1);
            for (size_t l = 0; l <= L; ++l) bytes[l] = (E[l].b - E[l].a) * levels[l].rowPitch;
            const Arena a(bytes.data(), L + 1);
            ScopedDevice sd(ctx->device);
            dxtex_hresult h = ctx->stageIn.grow(ctx, a.total); if (h != DXTEX_S_OK) return h;
            uint8_t* arena = ctx->stageIn.u8();
            // rows [a, b) of level l as one copy: whole pitches, the last row only as far as its texels go (a host image may end there)
            auto span = [&](size_t l, const Rows& r) -> size_t
            {
                size_t minRow = 0, minSlice = 0;
                (void)dxtex_compute_pitch(levels[l].format, levels[l].width, 1, &minRow, &minSlice);
                return (r.b - r.a - 1) * levels[l].rowPitch + minRow;
            };
            HIP_TRY(ctx, counted_copy(ctx, arena + a.at[0], levels[0].pixels + E[0].a * levels[0].rowPitch, span(0, E[0]), hipMemcpyHostToDevice, ctx->stream));
            time_begin(ctx);
            for (size_t l = 1; l <= L; ++l)
            {
                const size_t s0 = 2 * E[l].a;         // first row of the source sub-image, inside [E[l - 1].a, E[l - 1].b)
                dxtex_image s = levels[l - 1], d = levels[l];
                s.pixels = arena + a.at[l - 1] + (s0 - E[l - 1].a) * levels[l - 1].rowPitch; s.height = 2 * (E[l].b - E[l].a);
                d.pixels = arena + a.at[l]; d.height = E[l].b - E[l].a;
                h = submit_resize(ctx, s, d, mode, explicitFilter);
                if (h != DXTEX_S_OK) { time_end(ctx); return h; }
            }
            time_end(ctx);
            for (size_t l = 1; l <= L; ++l)
            {
                const Rows o = owned(l);
                if (o.b <= o.a) continue;
                HIP_TRY(ctx, counted_copy(ctx, levels[l].pixels + o.a * levels[l].rowPitch, arena + a.at[l] + (o.a - E[l].a) * levels[l].rowPitch, span(l, o), hipMemcpyDeviceToHost, ctx->stream));
            }
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            return DXTEX_S_OK;
        }, &failed);
        if (hr != DXTEX_S_OK) return surface_stripe_error(ctxs, hr, failed);
    }
    if (lv >= nlevels) return DXTEX_S_OK;
    return dxtex_generate_mips(ctxs[0], levels + (lv - 1), nlevels - (lv - 1), explicitFilter);       // the rest of the chain from the last level filled
}
} // extern "C"
