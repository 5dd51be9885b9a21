// Internal launcher prototypes (one per .hip translation unit). Everything is stream-ordered and
// returns the launch status; no launcher synchronises or allocates.
#pragma once
#include "dxtex_device.h"
#include "dxtex_dev.h"

namespace dxtex
{
// Optional per-kernel timing hook: launchers call mark(name) immediately before each kernel they enqueue;
// the context turns consecutive marks into hipEvent pairs on the launch stream.
struct KernelMarks
{
    virtual void mark(const char* kernelName) = 0;
protected:
    ~KernelMarks() = default;
};

hipError_t launch_bc15_encode(const SrcView& src, uint8_t* dst, uint64_t dstRowPitch, int dstFormat,
                              uint32_t flags, float threshold, hipStream_t stream);

// BC7: `scratch` must hold bc7_scratch_bytes(total number of 4x4 blocks, flags, number of images) bytes of device memory.
// The _many form runs an array of images (a mip chain, a texture array) through the per-mode pipeline as one block list.
struct BcImage { SrcView src; uint8_t* dst; uint64_t dstRowPitch; };
// BC1-BC5: up to bc15_small_batch_max() images that satisfy bc15_small_image() (at most 256 x 256 texels) in ONE launch - the tail
// of a mip chain, whose levels would otherwise each cost the latency of a kernel's slowest block.
bool bc15_small_image(uint32_t width, uint32_t height);
int bc15_small_batch_max();
hipError_t launch_bc15_encode_small(const BcImage* images, int count, int dstFormat, uint32_t flags, float threshold, hipStream_t stream);
// Two extra streams (and the events that fork / join them) for pipelines that are independent of each other until the last kernel:
// owned by the context (one set per context and device, destroyed with it); nullptr = everything on `stream`.
constexpr int kSideStreams = 3;
struct SideStreams { hipStream_t side[kSideStreams]; hipEvent_t forked; hipEvent_t joined[kSideStreams]; };
size_t bc7_scratch_bytes(uint64_t nblocks, uint32_t flags, size_t nimages = 1);
hipError_t launch_bc7_encode(const SrcView& src, uint8_t* dst, uint64_t dstRowPitch, uint32_t flags,
                             void* scratch, hipStream_t stream, KernelMarks* marks, const SideStreams* side = nullptr);
hipError_t launch_bc7_encode_many(const BcImage* images, size_t count, uint32_t flags, void* scratch, hipStream_t stream, KernelMarks* marks,
                                  const SideStreams* side = nullptr);

// BC6H (UF16 / SF16): `scratch` must hold bc6h_scratch_bytes(number of 4x4 blocks) bytes of device memory.
size_t bc6h_scratch_bytes(uint64_t nblocks, size_t nimages = 1);
hipError_t launch_bc6h_encode(const SrcView& src, uint8_t* dst, uint64_t dstRowPitch, bool isSigned, void* scratch,
                              hipStream_t stream, KernelMarks* marks, const SideStreams* side = nullptr);
hipError_t launch_bc6h_encode_many(const BcImage* images, size_t count, bool isSigned, void* scratch, hipStream_t stream, KernelMarks* marks,
                                   const SideStreams* side = nullptr);

// The one host-and-device description of a 2-D surface: `height` rows of `width` texels of `format`, `rowPitch` bytes apart. Every scanline
// launcher and the BC decoder take their surfaces as views (for a BC surface width and height count texels too), and the scanline kernels
// receive them as they are. A source is only read through its view.
struct ImgView
{
    uint8_t* pixels;
    uint64_t rowPitch;
    uint32_t width, height;
    int format;
};

// BC -> uncompressed (DecompressBC). `plan` = resolve_convert_plan(bc format, target format, TEX_FILTER_DEFAULT). The size is dst's.
struct ConvertPlan;
hipError_t launch_bc_decode(const ImgView& src, const ImgView& dst, const ConvertPlan& plan, hipStream_t stream);

// Convert (ConvertCustom): same size (src's; dst matches it), different format. dither = CONVERT_DITHER_*: ORDERED applies
// StoreScanlineDither's ordered branch (rows counted from the top of the given image, slice z); ZERO_ERROR adds the zero error row of the
// diffusion branch before a store that does not dither (the formats dither_spec() marks invalid).
enum : int { CONVERT_DITHER_NONE = 0, CONVERT_DITHER_ORDERED = 1, CONVERT_DITHER_ZERO_ERROR = 2 };
hipError_t launch_convert(const ImgView& src, const ImgView& dst, const ConvertPlan& plan, float threshold, hipStream_t stream,
                          int dither = CONVERT_DITHER_NONE, uint32_t z = 0, KernelMarks* marks = nullptr);
// Error-diffusion Convert of one image (a destination format with a dithered store; the size is src's) in one workgroup; `scratch` holds
// convert_diffuse_scratch_bytes(width) bytes of device memory; the texels the merge re-ran are added to *rerun (device memory).
// segLen = texels per speculated segment of a row (0: the default).
size_t convert_diffuse_scratch_bytes(uint32_t width);
hipError_t launch_convert_diffuse(const ImgView& src, const ImgView& dst, const ConvertPlan& plan, float threshold, void* scratch,
                                  unsigned long long* rerun, uint32_t segLen, hipStream_t stream);

// ComputeNormalMap of one image (the size is src's): dst's rows receive what the reference hands to StoreScanline (R32G32B32A32_FLOAT
// rows for launch_pack_group when the destination packs several texels per element); unorm = the destination format is UNORM (its
// encoding). flags = CNMAP_FLAGS. Source and destination must not overlap.
hipError_t launch_normal_map(const ImgView& src, const ImgView& dst, uint32_t flags, float amplitude, bool unorm, hipStream_t stream);

// TransformImage of one image (the size is src's) with one of texconv's per-texel ops (op = XFORM_*, args resolved by the caller, see
// dxtex_transform.h): LoadScanline -> op -> StoreScanline with threshold 0. dst's rows as for launch_normal_map (R32G32B32A32_FLOAT rows
// for launch_pack_group where the destination packs several texels). XFORM_TONEMAP reads the maximum luminance's bits from maxBits (device
// memory), which launch_tonemap_max folds each image of the set into (the caller zeroes it first).
struct XformArgs;
hipError_t launch_transform(const ImgView& src, const ImgView& dst, uint32_t op, const XformArgs& args, const uint32_t* maxBits, hipStream_t stream,
                            KernelMarks* marks = nullptr);
hipError_t launch_tonemap_max(const ImgView& src, uint32_t* maxBits, hipStream_t stream, KernelMarks* marks = nullptr);

// texconv's colour rotation of one image (the size is src's): LoadScanline -> the operation's matrix and curve (curve = ROTATE_CURVE_*,
// args resolved by the caller with rotate_resolve, see dxtex_rotate.h) on r, g and b -> StoreScanline with threshold 0. dst's rows as for
// launch_normal_map. A format of DXTEX_QUAD_FORMATS with 16-byte aligned rows on both sides takes four texels per lane (rotate_color.hip).
struct RotateArgs;
hipError_t launch_rotate_color(const ImgView& src, const ImgView& dst, int curve, const RotateArgs& args, hipStream_t stream, KernelMarks* marks = nullptr);

// Radiance RGBE texels (rgbe.hip; the arithmetic is in dxtex_rgbe.h), one image, the size is src's and dst matches it. Decode: R8G8B8A8_UINT
// rows of shared-exponent texels -> R32G32B32A32_FLOAT rows, scale = 1 / exposure. Encode: R32G32B32A32_FLOAT, R32G32B32_FLOAT or
// R16G16B16A16_FLOAT rows -> RGBE rows. A float side whose base and pitch are multiples of its texel (16 bytes; 8 for halves) takes one
// access per texel (<wide>), every other one an access per channel (<narrow>). Source and destination must not overlap.
hipError_t launch_rgbe_decode(const ImgView& src, const ImgView& dst, float scale, hipStream_t stream, KernelMarks* marks = nullptr);
hipError_t launch_rgbe_encode(const ImgView& src, const ImgView& dst, hipStream_t stream, KernelMarks* marks = nullptr);

// Truevision TGA texels (tga.hip; the rules are in dxtex_tga.h). Unpack: `stream` = dst.width * dst.height texels in file order, kind = a
// TgaKind that matches dst.format, flags = TgaFlags, palette = 256 host words for TGA_PALETTE (passed by value: free to go on return).
// For a kind with an alpha rule alphaWord[0..1] (device) are cleared and receive the two ORs, and the opaque pass behind the unpack leaves
// the answer in *answer (device); the other kinds touch neither. Pack: src's rows -> stream, row = a TgaRow. Wide / narrow: see tga.hip.
hipError_t launch_tga_unpack(const uint8_t* stream, int kind, uint32_t flags, const uint32_t* palette, const ImgView& dst, uint32_t* alphaWord, uint32_t* answer,
                             hipStream_t stream_, KernelMarks* marks = nullptr);
hipError_t launch_tga_pack(const ImgView& src, int row, uint32_t bytesPerTexel, uint8_t* stream, hipStream_t stream_, KernelMarks* marks = nullptr);

// DDS texels (dds.hip; the rules are in dxtex_dds.h). One DdsImage per image of the texture: where its rows lie in the file's payload
// (fileOffset, filePitch) and in device memory (pixels, pitch); `width` texels a row (row BYTES for ROW_COPY, which also carries planar rows
// and block rows), `rows` rows. kDdsBatchMax of them go into one launch, by value. Unpack: payload (device, as in the file) -> the images;
// op = a DdsRowOp, format = the result format (dds_target(op, format) picks the variant), opaque = CV_NOALPHA, palette = 256 host words for
// ROW_P8 / ROW_A8P8 (passed by value: free to go on return). Pack24: B8G8R8X8 images -> `out` at the file's pitches, 3 bytes a texel. Both
// check every descriptor against the payload's size before they queue anything (hipErrorInvalidValue). Wide / narrow: see dds.hip.
struct DdsImage { uint64_t fileOffset, filePitch; uint8_t* pixels; uint64_t pitch; uint32_t width, rows; };
constexpr int kDdsBatchMax = 32;
// the file side of `im`, rows of width * bytesPerTexel bytes, lies inside payloadBytes (and its rows do not run into each other)
inline bool dds_image_in_payload(const DdsImage& im, uint32_t bytesPerTexel, size_t payloadBytes)
{
    if (!im.width || !im.rows) return true;
    const uint64_t rowBytes = uint64_t(im.width) * bytesPerTexel;
    if (im.rows > 1u && (im.filePitch < rowBytes || im.filePitch > (UINT64_MAX - rowBytes) / (im.rows - 1u))) return false;
    const uint64_t span = uint64_t(im.rows - 1u) * im.filePitch + rowBytes;
    return im.fileOffset <= payloadBytes && span <= payloadBytes - im.fileOffset;
}
hipError_t launch_dds_unpack(const uint8_t* payload, size_t payloadBytes, int op, int format, bool opaque, const uint32_t* palette, const DdsImage* images, size_t count,
                             hipStream_t stream, KernelMarks* marks = nullptr);
hipError_t launch_dds_pack24(const DdsImage* images, size_t count, uint8_t* out, size_t outBytes, hipStream_t stream, KernelMarks* marks = nullptr);

// Portable pixmap texels (pnm.hip; the rules are in dxtex_pnm.h). Unpack: `stream` = dst.width * dst.height texels in file order, kind = a
// PnmKind that matches dst.format, maxval = 1..255 (read by PNM_P6 only), flags = PnmFlags. Pack: src's rows -> stream, source = the
// PnmSource of src.format. Neither touches memory outside the stream's texels and each image row's `width` texels. Wide / narrow: see pnm.hip.
hipError_t launch_pnm_unpack(const uint8_t* stream, int kind, uint32_t maxval, uint32_t flags, const ImgView& dst, hipStream_t stream_, KernelMarks* marks = nullptr);
hipError_t launch_pnm_pack(const ImgView& src, int source, uint8_t* stream, hipStream_t stream_, KernelMarks* marks = nullptr);

// PNG texels (png.hip; the rules are in dxtex_png.h). Unpack: `stream` = dst.height unfiltered rows of png_row_bytes(kind, dst.width)
// bytes, kind = a PngKind that matches dst.format, flags = PngFlags, palette = 256 host words (png_palette_table's) for a palette kind,
// passed by value: free to go on return. Pack: src's rows -> stream, source = the PngSource of src.format. Neither touches memory outside
// the stream's rows and each image row's `width` texels. Wide / narrow: see png.hip.
hipError_t launch_png_unpack(const uint8_t* stream, int kind, uint32_t flags, const uint32_t* palette, const ImgView& dst, hipStream_t stream_, KernelMarks* marks = nullptr);
hipError_t launch_png_pack(const ImgView& src, int source, uint8_t* stream, hipStream_t stream_, KernelMarks* marks = nullptr);

// JPEG samples (jpeg.hip; the rules are in dxtex_jpeg.h). `frame` is what the entry points have checked (include/dxtex_amd.h's layout):
// jpeg_idct dequantises and transforms every block of every component in one launch - a grey frame straight into dst, a colour frame into
// block-padded planes at `planes`, jpeg_plane_bytes(frame) bytes of device memory (0 for grey) - and jpeg_colour upsamples, transforms and
// stores each texel of dst. Nothing outside each row's `width` texels is written. Wide / narrow: see jpeg.hip.
struct JpegComponent { uint32_t h, v, quant, blocksPerRow, blockRows; uint64_t offset; };
struct JpegFrame { uint32_t width, height, components; int colour; JpegComponent comp[3]; uint16_t quant[4][64]; };
size_t jpeg_plane_bytes(const JpegFrame& frame);
hipError_t launch_jpeg_decode(const int16_t* coefficients, const JpegFrame& frame, const ImgView& dst, uint8_t* planes, hipStream_t stream, KernelMarks* marks = nullptr);
// The other direction (jpeg_encode.hip): src is R8_UNORM for a grey frame or a 32-bit colour format, B before R with `bgr`, for a YCbCr one.
// jpeg_samples transforms, downsamples and pads a colour frame into the same planes, jpeg_fdct transforms and quantises every block of
// every component in one launch into the reader's coefficient layout at `coefficients` (any even address). src is not written.
hipError_t launch_jpeg_encode(const ImgView& src, bool bgr, const JpegFrame& frame, int16_t* coefficients, uint8_t* planes, hipStream_t stream, KernelMarks* marks = nullptr);

// OpenEXR scanline chunks (exr.hip; the rules are in dxtex_exr.h). The caller has checked every descriptor against the stream and the
// layout. launch_exr_undo runs the byte-wise prefix sum of every coded chunk in place (`sums`: exr_undo_sums_count(chunks, count) words of
// device memory, read and written only where a coded chunk is longer than kExrUndoTile); launch_exr_texels then writes the rows of every
// chunk into the R16G16B16A16_FLOAT items, row y of the window at row y % itemRows of item y / itemRows. launch_exr_pack: the writer's
// rows, 8 * width bytes each (the A, B, G, R half planes), from level 0 of an image of one of dxtex_exr.h's sources.
struct ExrChunk;
struct ExrLayout;
size_t exr_undo_sums_count(const ExrChunk* chunks, size_t count);
hipError_t launch_exr_undo(uint8_t* stream, const ExrChunk* chunks, size_t count, uint32_t* sums, hipStream_t stream_, KernelMarks* marks = nullptr);
hipError_t launch_exr_texels(const uint8_t* stream, const ExrChunk* chunks, size_t count, const ExrLayout& layout, const ImgView* items, size_t itemCount,
                             hipStream_t stream_, KernelMarks* marks = nullptr);
hipError_t launch_exr_pack(const ImgView& src, int source, uint8_t* stream, hipStream_t stream_, KernelMarks* marks = nullptr);

// TIFF strips and tiles (tiff.hip; the rules are in dxtex_tiff.h). The caller has checked every descriptor against the stream, the layout
// and the image. launch_tiff_undo runs the predictor of every row of every segment in place (nothing for predictor 1);
// launch_tiff_texels then writes every segment's texels into dst, whose format is the kind's (palette: 256 words for the palette kinds).
// launch_tiff_pack: the writer's tight rows from level 0 of a B8G8R8A8 (4 bytes a texel) or B8G8R8X8 (3) image; the writer's other
// sources are row copies.
struct TiffSegment;
struct TiffLayout;
hipError_t launch_tiff_undo(uint8_t* stream, const TiffSegment* segments, size_t count, const TiffLayout& layout, hipStream_t stream_, KernelMarks* marks = nullptr);
hipError_t launch_tiff_texels(const uint8_t* stream, const TiffSegment* segments, size_t count, const TiffLayout& layout, const uint32_t* palette, const ImgView& dst,
                              hipStream_t stream_, KernelMarks* marks = nullptr);
hipError_t launch_tiff_pack(const ImgView& src, uint8_t* rows, hipStream_t stream_, KernelMarks* marks = nullptr);

// CopyRectangle: `count` resolved rectangles (dxtex_copyrect.h; the caller has checked every bound), kCopyBatchMax of them per launch.
// texassemble's merge of a (any loadable format) and b (R32G32B32A32_FLOAT, 16-byte aligned rows) into dst, whose rows are as for
// launch_normal_map; the size is a's.
struct CopyJob;
struct MergeArgs;
hipError_t launch_copy_rects(const CopyJob* jobs, size_t count, hipStream_t stream, KernelMarks* marks = nullptr);
hipError_t launch_merge(const ImgView& a, const ImgView& b, const ImgView& dst, const MergeArgs& args, hipStream_t stream, KernelMarks* marks = nullptr);

// ConvertToSinglePlane: `count` resolved images (dxtex_plane.h; plane_check has checked every bound), kPlaneBatchMax of them per launch.
struct PlaneJob;
hipError_t launch_single_plane(const PlaneJob* jobs, size_t count, hipStream_t stream, KernelMarks* marks = nullptr);

// FlipRotate: `count` resolved images (dxtex_fliprotate.h; the caller has checked every bound). One launch per route - rows, tiles - per
// kFlipBatchMax jobs of it.
struct FlipJob;
hipError_t launch_flip_rotate(const FlipJob* jobs, size_t count, hipStream_t stream, KernelMarks* marks = nullptr);

// Resize / one mip level: src is filtered (as src.format) into dst, whose rows are written in dst.format (R32G32B32A32_FLOAT rows for
// launch_pack_group, src.format otherwise). filterMode = TEX_FILTER_POINT..TRIANGLE (already resolved, never 0); filterFlags carries the
// wrap / mirror / sRGB bits. `tri` (device pointers) is required for TEX_FILTER_TRIANGLE: per destination column / row
// ofs[i]..ofs[i+1] indexes (source index, fp32 weight bits) pairs, see triangle_filter.h. `stale` (box mips only): StaleTap's level where
// the tap applies (its row 1 is what is read, see resize_box_kernel), else nullptr.
struct TriangleTables { const uint32_t* ofsX; const void* entX; const uint32_t* ofsY; const void* entY; };
hipError_t launch_resize(const ImgView& src, const ImgView& dst, uint32_t filterMode, uint32_t filterFlags, bool mipAlias,
                         const TriangleTables* tri, hipStream_t stream, const ImgView* stale = nullptr, KernelMarks* marks = nullptr);

// Formats whose element holds several texels (FC_GROUP): R32G32B32A32_FLOAT rows -> dst's format, with StoreScanline's pair / bit packing.
// The size is dst's.
hipError_t launch_pack_group(const ImgView& rows, const ImgView& dst, hipStream_t stream, KernelMarks* marks = nullptr);

// The box filter's fourth tap on a W x 1 source (Generate2DMipsBoxFilter, DirectXTexMipmaps.cpp:1017-1027; Generate3DMipsBoxFilter,
// :1849-1869): the reference points urow3 (and vrow3) at row 1 of its second-row buffer once, before the level loop, and does not re-point
// it when a 1-high source makes the second row alias the first. One tracker per chain; step() takes each level's source in chain order and
// says whether the tap applies to that level: the filter is box and the source is 1 high and more than 1 wide. It then reads row 1 of
// `twoHigh`, the most recent source level at least 2 high; with none (pixels == nullptr) it is off.
template<class View>        // ImgView, VolumeView
struct StaleTap
{
    View twoHigh;
    __host__ __device__ bool step(const View& src, bool box)
    {
        if (src.height >= 2u) twoHigh = src;
        return box && src.height == 1u && src.width > 1u && twoHigh.pixels != nullptr;
    }
};

// The tail of a 2-D mip chain in one workgroup. levels[0] = the first source level, levels[1..] = the levels generated from it, each the
// next one's source, all of levels[0]'s format. resize_tail_route() is the one place that decides whether the rest of a chain has such a
// form: Generic (resize_tail_kernel: point / linear / box, the arithmetic of launch_resize with mipAlias) or HalvingLds (box / cubic on
// RGBA8 with clamp addressing, every level an exact halving, staged in LDS), or None: this level takes a launch of its own.
// launch_resize_tail asks it again and fails for None. twoHigh = the chain's StaleTap state before levels[0], or nullptr: the launcher
// steps it on through the tail's levels and hands the kernel each level's stale view.
enum class TailRoute { None, Generic, HalvingLds };
TailRoute resize_tail_route(const ImgView* levels, int nlevels, uint32_t filterMode, uint32_t filterFlags);
hipError_t launch_resize_tail(const ImgView* levels, int nlevels, uint32_t filterMode, uint32_t filterFlags,
                              const ImgView* twoHigh, hipStream_t stream, KernelMarks* marks = nullptr);

// Volume mips (Generate3DMips*Filter): one level whose source is more than one slice deep. Slices of a level are `slicePitch` apart.
struct VolumeView { uint8_t* pixels; uint64_t rowPitch, slicePitch; uint32_t width, height, depth; int format; };
// slice z of a volume level as a 2-D surface
__host__ __device__ inline ImgView slice_of(const VolumeView& v, uint32_t z)
{
    return ImgView{ v.pixels + uint64_t(z) * v.slicePitch, v.rowPitch, v.width, v.height, v.format };
}
struct TriangleTables3 { const uint32_t* ofsX; const void* entX; const uint32_t* ofsY; const void* entY; const uint32_t* ofsZ; const void* entZ; };
// staleU / staleV (box only, both or neither): the slices whose row 1 the reference's never re-pointed urow3 / vrow3 still see, see resize3d_box_kernel.
hipError_t launch_resize3d(const VolumeView& src, const VolumeView& dst, uint32_t filterMode, uint32_t filterFlags, const TriangleTables3* tri,
                           hipStream_t stream, const ImgView* staleU = nullptr, const ImgView* staleV = nullptr, KernelMarks* marks = nullptr);

// ComputeMSE: out4 (device) receives the per-channel SUM of squared differences; divide by width * height (a's; b matches it) on the host.
hipError_t launch_mse(const ImgView& a, const ImgView& b, double* out4, hipStream_t stream, KernelMarks* marks = nullptr);
// ---- texdiag's diagnostics (diag.hip; the per-texel rules are in dxtex_diag.h) ----
// Analyze of one image, both passes: *acc (device, zeroed by the caller) receives the raw accumulators; dg_min_of / dg_max_of and a
// division by width * height turn them into the reference's figures on the host.
struct AnalyzeAcc
{
    uint32_t maxKey[4];                 // max of dg_key(v) over the values that are not NaN; 0 = none
    uint32_t minKeyInv[4];              // max of ~dg_key(v): the complement of the minimum's key; 0 = none
    uint32_t lumBits, pad;              // bits of the maximum luminance (+0 or above)
    double sum[4];                      // pass 1: sum of v
    double variance[4];                 // pass 2: sum of (v - float(sum / N))^2
    unsigned long long specials[4];     // values that are not finite
};
hipError_t launch_analyze(const ImgView& src, AnalyzeAcc* acc, hipStream_t stream, KernelMarks* marks = nullptr);
// ComputeMSE with CMSE_FLAGS (the bits the two formats imply are added here): out4 as for launch_mse.
hipError_t launch_mse_flags(const ImgView& a, const ImgView& b, uint32_t flags, double* out4, hipStream_t stream, KernelMarks* marks = nullptr);
// AnalyzeBC: hist[kBcHistBins] (device, zeroed by the caller) receives the block-mode histogram of the ceil(w / 4) x ceil(h / 4) blocks.
constexpr uint32_t kBcHistBins = 15;
hipError_t launch_bc_hist(const ImgView& src, unsigned long long* hist, hipStream_t stream, KernelMarks* marks = nullptr);
// Difference's map: a in any loadable format, b in R32G32B32A32_FLOAT (16-byte aligned rows), dst's rows as for launch_normal_map.
hipError_t launch_difference(const ImgView& a, const ImgView& b, const ImgView& dst, uint32_t diffColor, float threshold, hipStream_t stream,
                             KernelMarks* marks = nullptr);

// PremultiplyAlpha / DemultiplyAlpha (DirectXTexPMAlpha.cpp:30-205); pmFlags = TEX_PMALPHA_*. Size and format are src's; dst matches them.
hipError_t launch_pmalpha(const ImgView& src, const ImgView& dst, uint32_t pmFlags, hipStream_t stream, KernelMarks* marks = nullptr);
// ScaleAlpha and CalculateAlphaCoverage (DirectXTexMipmaps.cpp:143-305); *count receives the number of covered sub-samples.
// launch_scale_alpha: size and format are src's; dst matches them.
hipError_t launch_scale_alpha(const ImgView& src, const ImgView& dst, float scale, hipStream_t stream, KernelMarks* marks = nullptr);
hipError_t launch_alpha_coverage(const ImgView& src, float scale, float alphaReference, unsigned long long* count, hipStream_t stream,
                                 KernelMarks* marks = nullptr);
// IsAlphaAllOpaque's scan: *count (device, NOT cleared here) is incremented by the number of texels with alpha < threshold
hipError_t launch_alpha_below(const ImgView& src, float threshold, unsigned long long* count, hipStream_t stream, KernelMarks* marks = nullptr);
} // namespace dxtex
