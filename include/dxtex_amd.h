/*
 * dxtex_amd.h - C ABI of the MI355X-native DirectXTex hot path (libdxtex_amd.so).
 *
 * Drop-in boundary: these entry points are what a maintainer of microsoft/DirectXTex would bind in place
 * of the library's own GPU plugin (GPUCompressBC, DirectXTex/BCDirectCompute.h:15-68) and of the CPU
 * loops behind Compress / Decompress / GenerateMipMaps / Convert / Resize. Plain pointers and sizes only;
 * every function returns an HRESULT with the reference's values (DirectXTexP.h:210-234).
 *
 *   reference interface                                         replaced by
 *   ----------------------------------------------------------  -----------------------------------------
 *   GPUCompressBC::Initialize(ID3D11Device*)   BCDirectCompute.h:26   dxtex_ctx_create
 *   GPUCompressBC::Prepare(w,h,flags,fmt,aw)   BCDirectCompute.h:28   dxtex_ctx_prepare (optional: sizes the search scratch and the staging now instead of
 *                                                                     on first use; alphaWeight belongs to the D3D11 BC7 shader and has no counterpart in
 *                                                                     the CPU-path encoders reproduced here)
 *   GPUCompressBC::Compress(src,dst)           BCDirectCompute.h:30   dxtex_compress / dxtex_compress_device
 *   CompressBC / CompressBC_Parallel           DirectXTexCompress.cpp:72-372   dxtex_compress
 *   DecompressBC                               DirectXTexCompress.cpp:425-535  dxtex_decompress
 *   BC_ENCODE / BC_DECODE fn-ptr hooks         BC.h:318-343           dxtex_encode_blocks / dxtex_decode_blocks
 *   Generate2DMips{Point,Box,Linear,Cubic,Triangle}Filter  DirectXTexMipmaps.cpp:907-1602  dxtex_generate_mips
 *   ConvertCustom                              DirectXTexConvert.cpp:4804-4913 dxtex_convert
 *   Resize*Filter                              DirectXTexResize.cpp:255-803    dxtex_resize
 *   ComputeNMap                                DirectXTexNormalMaps.cpp:77-240 dxtex_compute_normal_map
 *   TransformImage / EvaluateImage with        DirectXTexMisc.cpp:179-263      dxtex_transform_image
 *     texconv's swizzle, tone-map, colour-key,   texconv.cpp:2645-3301
 *     invert-Y and reconstruct-Z lambdas
 *   TransformImage with texconv's colour       texconv.cpp:2696-2964           dxtex_rotate_color
 *     rotation lambdas (HDR10, Rec.2020, P3)
 *   ComputeMSE_ with CMSE_FLAGS                DirectXTexMisc.cpp:27-176       dxtex_compute_mse_flags_device
 *   texdiag's Analyze / AnalyzeBC / Difference Texdiag/texdiag.cpp:698-1320    dxtex_analyze / dxtex_analyze_bc / dxtex_difference
 *   CopyRectangle                              DirectXTexMisc.cpp:275-381      dxtex_copy_rectangle / dxtex_copy_rectangles_device
 *   texassemble's merge lambda                 Texassemble/texassemble.cpp:2236-2268  dxtex_merge_image
 *   FlipRotate                                 DirectXTexFlipRotate.cpp:185-381 dxtex_flip_rotate / dxtex_flip_rotate_device
 *   ConvertToSinglePlane                       DirectXTexConvert.cpp:4912-5077, :5411-5523  dxtex_convert_to_single_plane[_device]
 *   LoadFromHDRMemory's float pass,            DirectXTexHDR.cpp:887-901, :328-407  dxtex_rgbe_decode / dxtex_rgbe_encode
 *     FloatToRGBE / HalfToRGBE
 *   CopyPixels / UncompressPixels' texel half, DirectXTexTGA.cpp:396-1180;     dxtex_tga_unpack / dxtex_tga_pack
 *     Copy24bppScanline / the swizzle of         :1288, :2249-2330
 *     SaveToTGAMemory
 *   CopyImage's row conversions, the 24-bit    DirectXTexDDS.cpp:1518-1808     dxtex_dds_unpack / dxtex_dds_pack24
 *     rows of SaveToDDSMemory
 *   LoadFromPortablePixMap[HDR]'s texel loops, Texconv/PortablePixMap.cpp      dxtex_pnm_unpack / dxtex_pnm_pack
 *     the rows of SaveToPortablePixMap[HDR]      :209-223, :595-681, :392-422, :720-735
 *   LoadFromPNGFile's / SaveToPNGFile's         Auxiliary/DirectXTexPNG.cpp     dxtex_png_unpack / dxtex_png_pack
 *     per-texel transforms                       :126-225, :315-404
 *   LoadFromJPEGFile behind the Huffman walk:   Auxiliary/DirectXTexJPEG.cpp    dxtex_jpeg_decode
 *     libjpeg's jidctint.c, jdsample.c, jdcolor.c  :184-238
 *   SaveToJPEGFile in front of the Huffman coder: Auxiliary/DirectXTexJPEG.cpp    dxtex_jpeg_encode
 *     libjpeg's jccolor.c, jcsample.c, jfdctint.c  :240-300
 *   LoadFromEXRFile behind the inflater (the    Auxiliary/DirectXTexEXR.cpp     dxtex_exr_unpack / dxtex_exr_pack
 *     library's delta undo, plane interleave,    :286-321, :529-650
 *     RgbaInputFile's fill and conversion), the
 *     half planes of SaveToEXRFile
 *
 * Threading: a context is bound to one GPU and one HIP stream; use one context per GPU (or per host
 * thread). Contexts share nothing. No function retains caller pointers past its return, except the
 * *_device variants, which are asynchronous on the context's stream.
 */
#ifndef DXTEX_AMD_H
#define DXTEX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t dxtex_hresult;

#define DXTEX_S_OK                 ((dxtex_hresult)0)
#define DXTEX_E_FAIL               ((dxtex_hresult)0x80004005)
#define DXTEX_E_INVALIDARG         ((dxtex_hresult)0x80070057)
#define DXTEX_E_OUTOFMEMORY        ((dxtex_hresult)0x8007000E)
#define DXTEX_E_POINTER            ((dxtex_hresult)0x80004003)
#define DXTEX_E_ABORT              ((dxtex_hresult)0x80004004)
#define DXTEX_E_NOTIMPL            ((dxtex_hresult)0x80004001)
#define DXTEX_E_UNEXPECTED         ((dxtex_hresult)0x8000FFFF)
#define DXTEX_E_NOT_SUPPORTED      ((dxtex_hresult)0x80070032)  /* HRESULT_FROM_WIN32(ERROR_NOT_SUPPORTED) */
#define DXTEX_E_ARITHMETIC_OVERFLOW ((dxtex_hresult)0x80070216)

/* TEX_COMPRESS_FLAGS, bit-for-bit (DirectXTex.h:887-917). */
#define DXTEX_COMPRESS_DEFAULT          0u
#define DXTEX_COMPRESS_RGB_DITHER       0x10000u
#define DXTEX_COMPRESS_A_DITHER         0x20000u
#define DXTEX_COMPRESS_DITHER           0x30000u
#define DXTEX_COMPRESS_UNIFORM          0x40000u
#define DXTEX_COMPRESS_BC7_USE_3SUBSETS 0x80000u
#define DXTEX_COMPRESS_BC7_QUICK        0x100000u
#define DXTEX_COMPRESS_SRGB_IN          0x1000000u
#define DXTEX_COMPRESS_SRGB_OUT         0x2000000u
#define DXTEX_COMPRESS_PARALLEL         0x10000000u

/* TEX_FILTER_FLAGS subset (DirectXTex.h:741-793). */
#define DXTEX_FILTER_DEFAULT   0u
#define DXTEX_FILTER_WRAP_U    0x1u
#define DXTEX_FILTER_WRAP_V    0x2u
#define DXTEX_FILTER_MIRROR_U  0x10u
#define DXTEX_FILTER_MIRROR_V  0x20u
#define DXTEX_FILTER_POINT     0x100000u
#define DXTEX_FILTER_LINEAR    0x200000u
#define DXTEX_FILTER_CUBIC     0x300000u
#define DXTEX_FILTER_BOX       0x400000u
#define DXTEX_FILTER_TRIANGLE  0x500000u
#define DXTEX_FILTER_MODE_MASK 0xF00000u

/* Mirrors DirectX::Image (DirectXTex.h:437-445); `format` is a DXGI_FORMAT value. */
typedef struct dxtex_image
{
    size_t   width;
    size_t   height;
    int32_t  format;
    size_t   rowPitch;
    size_t   slicePitch;
    uint8_t* pixels;
} dxtex_image;

typedef struct dxtex_ctx dxtex_ctx;

/* ---- context ---------------------------------------------------------------------------------- */

/* Binds a context to HIP device `device` and creates its stream. Fails with DXTEX_E_FAIL when no
 * gfx950-capable device is visible: there is no CPU fallback anywhere in this library. */
dxtex_hresult dxtex_ctx_create(int device, dxtex_ctx** out);
void          dxtex_ctx_destroy(dxtex_ctx* ctx);
/* Run subsequent work on a caller-owned hipStream_t (e.g. the current PyTorch stream); NULL restores
 * the context's own stream. Waits for the work queued on the previous stream, which must outlive this call (a handle
 * the runtime no longer knows is tolerated); DXTEX_E_FAIL, stream unchanged, if that work failed asynchronously. */
dxtex_hresult dxtex_ctx_set_stream(dxtex_ctx* ctx, void* hip_stream);
void*         dxtex_ctx_get_stream(dxtex_ctx* ctx);
dxtex_hresult dxtex_ctx_synchronize(dxtex_ctx* ctx);
/* Human-readable description of the last failure on this context (never NULL). */
const char*   dxtex_ctx_last_error(dxtex_ctx* ctx);
/* Device time in milliseconds of the kernels launched by the most recent call on this context
 * (hipEvent pair on the context's stream, transfers excluded); -1 if nothing was timed. */
float         dxtex_ctx_last_kernel_ms(dxtex_ctx* ctx);

/* Per-kernel device timing. Between profile_begin and profile_end every kernel this context launches is
 * bracketed by hipEvents on the launch stream. profile_end synchronises the stream and returns, per
 * distinct kernel, the summed duration in ms and the number of launches; `names` receives the kernel
 * names separated by '\n'. Used by bench.py for the roofline object. */
dxtex_hresult dxtex_ctx_profile_begin(dxtex_ctx* ctx);
dxtex_hresult dxtex_ctx_profile_end(dxtex_ctx* ctx, char* names, size_t names_bytes, float* total_ms,
                                    uint32_t* launches, size_t capacity, size_t* count);

/* ---- format utilities (DirectXTexUtil.cpp:340-1186) ------------------------------------------- */

int           dxtex_is_compressed(int32_t format);
size_t        dxtex_bits_per_pixel(int32_t format);
/* ComputePitch (DirectXTexUtil.cpp:961-1186) with CP_FLAGS_NONE. */
dxtex_hresult dxtex_compute_pitch(int32_t format, size_t width, size_t height, size_t* rowPitch, size_t* slicePitch);

/* ---- Compress / Decompress -------------------------------------------------------------------- */

/* The counterpart of GPUCompressBC::Prepare (BCDirectCompute.h:31, BCDirectCompute.cpp:203-369; called once per size from
 * DirectXTexCompressGPU.cpp:392-442): allocates everything a later dxtex_compress* of `count` images of this size and these
 * formats needs - the BC6H / BC7 search scratch and, for the host-pointer entry points, the device staging buffers - so that
 * the compress calls themselves allocate nothing - and, as Prepare binds its shaders, runs one block of zeros through the format's
 * pipeline once per context so that the kernels' code objects and the side streams exist before the first real call (a fresh process:
 * first 64 x 64 BC7 call 19 ms without, about 1 ms with). Optional: without it the buffers grow on first use. Same format checks and
 * error codes as dxtex_compress. Returns the bytes of device memory the context now holds in `device_bytes` (may be NULL). */
dxtex_hresult dxtex_ctx_prepare(dxtex_ctx* ctx, size_t width, size_t height, int32_t src_format, int32_t dst_format,
                                uint32_t compress_flags, size_t count, size_t* device_bytes);

/* Host images in, host image out: H2D copy, kernels, D2H copy, synchronous. `dst` must already describe
 * a BC image of the same width/height (ScratchImage::Initialize2D layout). Error behaviour follows
 * CompressBC (DirectXTexCompress.cpp:72-205): E_POINTER for null pixels, HRESULT_E_NOT_SUPPORTED for an
 * unsupported source/destination format, E_INVALIDARG for a compressed source. */
dxtex_hresult dxtex_compress(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst,
                             uint32_t compress_flags, float threshold);

/* Same, but `src->pixels` / `dst->pixels` are device pointers on the context's GPU; asynchronous on the
 * context's stream. This is the entry point the benchmark times (inputs resident in HBM). */
dxtex_hresult dxtex_compress_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst,
                                    uint32_t compress_flags, float threshold);

/* Batch of `count` independent images (texture array, mip chain, atlas pages: the array overload of Compress,
 * DirectXTexCompress.cpp:722-846) on device memory; one stream-ordered submission. BC6H / BC7 arrays go through the
 * search pipeline as one block list, so many small images cost what one image of the same total size costs. */
dxtex_hresult dxtex_compress_many_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts,
                                         size_t count, uint32_t compress_flags, float threshold);
/* Same with host pointers; returns when the payloads are back. The images are cut into chunks of about 32 Mi texels
 * (DXTEX_MANY_CHUNK_TEXELS overrides); two sets of pinned staging + device buffers alternate so that the upload of chunk k+1
 * and the download of chunk k-1 run on copy streams while chunk k's kernels run. The bytes written are those of
 * `count` separate dxtex_compress calls. */
dxtex_hresult dxtex_compress_many(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts,
                                  size_t count, uint32_t compress_flags, float threshold);

/* BC -> uncompressed (R8G8B8A8_UNORM, R16G16B16A16_FLOAT, R32G32B32A32_FLOAT, R8_UNORM/SNORM, R8G8_*).
 * Host and device variants as above. */
dxtex_hresult dxtex_decompress(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst);
dxtex_hresult dxtex_decompress_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst);

/* Block-level hooks with the reference's BC_ENCODE / BC_DECODE shape (BC.h:318-343): `rgba` holds
 * nblocks x 16 texels x 4 floats (row-major 4x4 tiles) in host memory, `bc` nblocks x 8|16 bytes.
 * `threshold` is only read for BC1. */
dxtex_hresult dxtex_encode_blocks(dxtex_ctx* ctx, int32_t bc_format, uint32_t bc_flags, float threshold,
                                  const float* rgba, size_t nblocks, uint8_t* bc);
dxtex_hresult dxtex_decode_blocks(dxtex_ctx* ctx, int32_t bc_format, const uint8_t* bc, size_t nblocks, float* rgba);

/* ---- GenerateMipMaps / Convert / Resize -------------------------------------------------------- */

/* Fills levels[1..nlevels-1] from levels[0] (each level from the previous *stored* level,
 * DirectXTexMipmaps.cpp:1036-1037). All levels share levels[0].format. `filter` = TEX_FILTER_FLAGS. */
dxtex_hresult dxtex_generate_mips(dxtex_ctx* ctx, const dxtex_image* levels, size_t nlevels, uint32_t filter);
dxtex_hresult dxtex_generate_mips_device(dxtex_ctx* ctx, const dxtex_image* levels, size_t nlevels, uint32_t filter);

/* GenerateMipMaps3D (DirectXTex.h:853-858, DirectXTexMipmaps.cpp:3254-3361): volume textures. A level is `depth` slices of
 * `slicePitch` bytes starting at `pixels` (the layout ScratchImage::Initialize3D gives a level, DirectXTexImage.cpp:228-262);
 * levels[0] holds the base slices, levels[1..] are filled, each from the STORED previous level. Level i is
 * max(1, w>>i) x max(1, h>>i) x max(1, d>>i). filter 0 = box when all three dimensions are powers of two, else triangle. */
typedef struct dxtex_volume
{
    size_t   width, height, depth;
    int32_t  format;
    size_t   rowPitch, slicePitch;
    uint8_t* pixels;
} dxtex_volume;
dxtex_hresult dxtex_generate_mips3d(dxtex_ctx* ctx, const dxtex_volume* levels, size_t nlevels, uint32_t filter);
dxtex_hresult dxtex_generate_mips3d_device(dxtex_ctx* ctx, const dxtex_volume* levels, size_t nlevels, uint32_t filter);

/* Convert = ConvertCustom (DirectXTexConvert.cpp:4804-4913), all three of its branches, byte for byte:
 *   TEX_FILTER_DITHER_DIFFUSION (0x20000, checked first: with both bits set diffusion runs): Floyd-Steinberg error diffusion
 *     (StoreScanlineDither with an error buffer): serpentine rows (even rows left to right, odd rows right to left), 7/16 of a texel's
 *     divided error to the next texel of its row, 3/16, 5/16, 1/16 to the next row; vError restarts at zero on every row. One GPU
 *     workgroup per image, exact for every input (the serial chain is run as speculated segments merged exactly, see dxtex_dither.h).
 *   TEX_FILTER_DITHER (0x10000): ordered dithering, offset g_Dither[(z & 3) + (y & 3) * 8 + (x & 3)] with y the row within the image.
 *   Destination formats with a dithered store: R16G16B16A16_{UNORM,UINT,SNORM,SINT}, R10G10B10A2_{UNORM,UINT}, R10G10B10_XR_BIAS_A2_UNORM,
 *   R8G8B8A8_{UNORM,UNORM_SRGB,UINT,SNORM,SINT}, R16G16_*, D24_UNORM_S8_UINT, R8G8_*, D16_UNORM, R16_*, R8_*, A8_UNORM, B5G6R5_UNORM,
 *   B5G5R5A1_UNORM, B8G8R8A8_UNORM[_SRGB], B8G8R8X8_UNORM[_SRGB] (X written as 0), B4G4R4A4_UNORM, A4B4G4R4_UNORM. Every other
 *   format is stored undithered; under diffusion after the zero error row was added (so -0.0 becomes +0.0 in float destinations).
 * dxtex_convert[_device] are slice 0; dxtex_convert_slice[_device] take the slice z of a volume (0..depth-1 within its mip level),
 * which only ordered dithering reads. */
dxtex_hresult dxtex_convert(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, float threshold);
dxtex_hresult dxtex_convert_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, float threshold);
dxtex_hresult dxtex_convert_slice(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, float threshold, uint32_t z);
dxtex_hresult dxtex_convert_slice_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter, float threshold, uint32_t z);
/* Diagnostics of error diffusion on this context, cumulative: texels converted with diffusion into a dithered format, and how many of
 * them the exact merge had to run a second (or further) time. Waits for the context's stream (copies 8 bytes to the host). */
dxtex_hresult dxtex_convert_dither_stats(dxtex_ctx* ctx, uint64_t* rerunTexels, uint64_t* texels);

/* ComputeNormalMap (DirectXTexNormalMaps.cpp:77-240) of one height map: src and dst have the same size, dst->format is a UNORM, SNORM or
 * FLOAT format (it may equal src->format). flags = CNMAP_FLAGS: channel (flags & 0xf: 0 or 1 red, 2 green, 3 blue, 4 alpha, 5 luminance),
 * DXTEX_CNMAP_MIRROR_U / _V (repeat the edge texel instead of wrapping), DXTEX_CNMAP_INVERT_SIGN, DXTEX_CNMAP_COMPUTE_OCCLUSION (alpha =
 * occlusion term, else 1). HRESULTs: E_INVALIDARG for a bad channel, a format outside 1..191 or overlapping pixels; NOT_SUPPORTED for
 * block-compressed or unknown formats and for destinations that are not UNORM / SNORM / FLOAT; E_FAIL for a size mismatch. Under
 * MIRROR_V the row above row 0 is row 0 (the reference's memcpy there is defined only for 16-byte texels with a tight pitch). */
#define DXTEX_CNMAP_CHANNEL_RED        0x1u
#define DXTEX_CNMAP_CHANNEL_GREEN      0x2u
#define DXTEX_CNMAP_CHANNEL_BLUE       0x3u
#define DXTEX_CNMAP_CHANNEL_ALPHA      0x4u
#define DXTEX_CNMAP_CHANNEL_LUMINANCE  0x5u
#define DXTEX_CNMAP_MIRROR_U           0x1000u
#define DXTEX_CNMAP_MIRROR_V           0x2000u
#define DXTEX_CNMAP_MIRROR             0x3000u
#define DXTEX_CNMAP_INVERT_SIGN        0x4000u
#define DXTEX_CNMAP_COMPUTE_OCCLUSION  0x8000u
dxtex_hresult dxtex_compute_normal_map(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags, float amplitude);
dxtex_hresult dxtex_compute_normal_map_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags, float amplitude);

/* TransformImage (DirectXTexMisc.cpp:606-700) with one of texconv's per-texel lambdas, described instead of passed as a function:
 * LoadScanline -> op -> StoreScanline (threshold 0), no sRGB conversion. Channels an op does not write keep their bits.
 *   SWIZZLE        out[k] = in[swizzle[k]] (0..3), then 0 where zero[k], then 1 where one[k] (texconv.cpp:2645-2694)
 *   TONEMAP        Reinhard with the maximum luminance (r * 0.3 + g * 0.59) + b * 0.11 over ALL the sources of the call, taken before any
 *                  destination is written; alpha kept (:2966-3044)
 *   COLOR_KEY      colorKey = 0x00RRGGBB: a texel within 0.2 of the key in r, g and b becomes (0, 0, 0, 0), every other one gets alpha 1
 *                  (:3134-3191; texconv runs it only where HasAlpha(format))
 *   INVERT_Y       g = 1 - g (:3193-3240)
 *   RECONSTRUCT_Z  b = sqrt(1 - (x^2 + y^2)), on x * 2 - 1 and with * 0.5 + 0.5 when FormatDataType(format) is UNORM (:3242-3301)
 * Source and destination share format and size. HRESULTs: NOT_SUPPORTED for planar, palettised, compressed, typeless and unknown formats;
 * E_INVALIDARG for a width or height above UINT32_MAX, a bad op or swizzle index and overlapping pixels; E_FAIL for a format or size
 * mismatch between the images; E_POINTER for null pixels. */
#define DXTEX_TRANSFORM_SWIZZLE        0u
#define DXTEX_TRANSFORM_TONEMAP        1u
#define DXTEX_TRANSFORM_COLOR_KEY      2u
#define DXTEX_TRANSFORM_INVERT_Y       3u
#define DXTEX_TRANSFORM_RECONSTRUCT_Z  4u
typedef struct dxtex_transform
{
    uint32_t op;            /* DXTEX_TRANSFORM_* */
    uint32_t swizzle[4];    /* SWIZZLE: source channel of each output channel */
    uint32_t zero[4];       /* SWIZZLE: non-zero = the output channel is 0 */
    uint32_t one[4];        /* SWIZZLE: non-zero = the output channel is 1 (after zero) */
    uint32_t colorKey;      /* COLOR_KEY: 0x00RRGGBB (the high byte is ignored) */
} dxtex_transform;
/* host pointers, one image, through the context's staging; returns when the destination has landed */
dxtex_hresult dxtex_transform_image(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, const dxtex_transform* t);
/* device pointers, `count` images of one format (a mip chain, an array, volume slices): asynchronous on the context's stream */
dxtex_hresult dxtex_transform_images_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, const dxtex_transform* t);

/* texconv's HDR colour rotation (Texconv/texconv.cpp:2696-2964): r, g and b move between the Rec.709, Rec.2020 and Display-P3 (D65)
 * primaries, and into or out of HDR10 - Rec.2020 with the SMPTE ST.2084 curve, where paperWhiteNits is the level of linear 1.0.
 * LoadScanline -> lambda -> StoreScanline (threshold 0); alpha keeps its bits; source and destination share format and size. The values
 * are texconv's ROTATE_* (texconv.cpp:181-188). texconv converts to R16G16B16A16_FLOAT before HDR10_TO_709 and P3D65_TO_709; that is the
 * caller's step here (dxtex_convert). powf is the correctly rounded one; a channel whose arithmetic gives a NaN is a NaN of any payload.
 * HRESULTs: NOT_SUPPORTED for planar, palettised, compressed, typeless and unknown formats; E_INVALIDARG for a rotate outside 1..8, a
 * paperWhiteNits outside (0, 10000] (a NaN included: texconv's rule for -nits), a width or height above UINT32_MAX and overlapping
 * pixels; E_FAIL for a format or size mismatch between the images; E_POINTER for null pixels. */
#define DXTEX_ROTATE_709_TO_HDR10     1u
#define DXTEX_ROTATE_HDR10_TO_709     2u
#define DXTEX_ROTATE_709_TO_2020      3u
#define DXTEX_ROTATE_2020_TO_709      4u
#define DXTEX_ROTATE_P3D65_TO_HDR10   5u
#define DXTEX_ROTATE_P3D65_TO_2020    6u
#define DXTEX_ROTATE_709_TO_P3D65     7u
#define DXTEX_ROTATE_P3D65_TO_709     8u
/* host pointers, one image, through the context's staging; returns when the destination has landed */
dxtex_hresult dxtex_rotate_color(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t rotate, float paperWhiteNits);
/* device pointers, `count` images of one format and any sizes (a mip chain, an array): asynchronous on the context's stream */
dxtex_hresult dxtex_rotate_color_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, uint32_t rotate, float paperWhiteNits);

/* Radiance RGBE (.hdr) texels, the per-texel half of the codec (the run-length coder is byte-serial and stays with the caller). One image
 * per call. The RGBE side is a dxtex_image of DXGI_FORMAT_R8G8B8A8_UINT: the four raw bytes of each shared-exponent texel.
 *   decode   RGBE -> R32G32B32A32_FLOAT: channel = (1 / exposure) * ldexpf(byte + 0.5f, exponent byte - 136), alpha 1
 *            (DirectXTexHDR.cpp:887-901). As there, a zero exponent byte is no special case: (0, 0, 0, 0) decodes to 2^-137, a denormal.
 *   encode   R32G32B32A32_FLOAT, R32G32B32_FLOAT or R16G16B16A16_FLOAT -> RGBE: FloatToRGBE / HalfToRGBE (:328-407). A negative or NaN
 *            channel counts as 0. The reference converts a NaN to a byte where a channel is +Inf, which is undefined; here a texel whose
 *            largest channel is not finite becomes four zero bytes.
 * HRESULTs, in this order: E_POINTER for a null image or null pixels; NOT_SUPPORTED for any other format on either side (SaveToHDRMemory's
 * answer); E_FAIL for a size mismatch; E_INVALIDARG for a row pitch smaller than the row, a width or height above UINT32_MAX, overlapping
 * pixels, or an exposure that is not a finite positive number. Pixels and pitches are aligned to the side's channel (1, 2 or 4 bytes). */
/* host pointers, through the context's staging; returns when the destination has landed */
dxtex_hresult dxtex_rgbe_decode(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, float exposure);
dxtex_hresult dxtex_rgbe_encode(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst);
/* device pointers: asynchronous on the context's stream */
dxtex_hresult dxtex_rgbe_decode_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, float exposure);
dxtex_hresult dxtex_rgbe_encode_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst);

/* Truevision TGA (.tga) texels, the per-texel half of the codec (header, palette bytes and run-length packets are byte-serial and stay
 * with the caller). One image per call. The file side is the texel stream: `texelBytes` bytes, tight rows of width * bytesPerTexel, in
 * the file's order - its first row is the image's bottom row unless DXTEX_TGA_TOP_DOWN, its first texel the rightmost one if
 * DXTEX_TGA_RIGHT_TO_LEFT (bits 5 and 4 of the file's descriptor).
 *   unpack   stream -> dst, through dst's pitch, both flips applied (CopyPixels, DirectXTexTGA.cpp:738-1180):
 *              bytesPerTexel  dst->format       texel
 *              1              R8_UNORM          the byte
 *              2              B5G5R5A1_UNORM    the word; alpha counts as 0 or 255 by bit 15
 *              3              R8G8B8A8_UNORM    B, G, R -> R, G, B, 255: opaque by construction
 *              3              B8G8R8X8_UNORM    B, G, R, 0 (TGA_FLAGS_BGR); no alpha rule
 *              4              R8G8B8A8_UNORM    B, G, R, A -> R, G, B, A
 *              4              B8G8R8A8_UNORM    the word (TGA_FLAGS_BGR)
 *              1, palette     R8G8B8A8_UNORM    palette[index]; `palette` = 256 words in host memory, read before the call returns
 *                             or B8G8R8X8_UNORM (ReadPalette's table: zero words outside the file's colour map); no alpha rule
 *            The alpha rule (2 and 4 bytes): where every alpha is zero and DXTEX_TGA_ALLOW_ALL_ZERO_ALPHA is not set, every alpha is made
 *            opaque (255; bit 15). The answer is 1 if the image is opaque - made so, found so, or 24 bits into R8G8B8A8 - else 0: the
 *            reference's S_FALSE / S_OK. It is independent of the order in which the device visits the texels.
 *   pack     level 0 of src -> the stream the writer emits, top-down and left-to-right (SaveToTGAMemory, :2249-2330): R8G8B8A8_UNORM[_SRGB]
 *            with R and B swapped (4 bytes), B8G8R8A8_UNORM[_SRGB] (4), B8G8R8X8_UNORM[_SRGB] without X (3), R8_UNORM / A8_UNORM (1),
 *            B5G5R5A1_UNORM (2)
 * HRESULTs, in this order: E_POINTER for a null stream, image, pixels or (host form of unpack) answer; NOT_SUPPORTED for a format /
 * bytesPerTexel / palette combination outside the tables above; E_INVALIDARG for a width or height of zero or above 65535, a row pitch
 * smaller than the row, or a stream that overlaps the pixels; E_FAIL for texelBytes != width * height * bytesPerTexel. */
#define DXTEX_TGA_RIGHT_TO_LEFT          0x1u
#define DXTEX_TGA_TOP_DOWN               0x2u
#define DXTEX_TGA_ALLOW_ALL_ZERO_ALPHA   0x4u
/* host pointers, through the context's staging; returns when the destination (and *opaque) has landed */
dxtex_hresult dxtex_tga_unpack(dxtex_ctx* ctx, const void* texels, size_t texelBytes, uint32_t bytesPerTexel, uint32_t flags, const uint32_t* palette,
                               const dxtex_image* dst, uint32_t* opaque);
dxtex_hresult dxtex_tga_pack(dxtex_ctx* ctx, const dxtex_image* src, uint32_t bytesPerTexel, void* texels, size_t texelBytes);
/* device pointers (the palette stays a host pointer): asynchronous on the context's stream. opaqueDevice: a dword of device memory that
 * receives the answer in stream order, or NULL. The stream may start at any byte; one that starts on a multiple of 4 takes the wide route. */
dxtex_hresult dxtex_tga_unpack_device(dxtex_ctx* ctx, const void* texels, size_t texelBytes, uint32_t bytesPerTexel, uint32_t flags, const uint32_t* palette,
                                      const dxtex_image* dst, uint32_t* opaqueDevice);
dxtex_hresult dxtex_tga_pack_device(dxtex_ctx* ctx, const dxtex_image* src, uint32_t bytesPerTexel, void* texels, size_t texelBytes);

/* DDS (.dds) texels, the per-texel half of the codec (header, refusals and size checks are byte-serial and stay with the caller). One call
 * takes every image of a texture - array items, mip levels, depth slices. The file side is the payload as it is in the file: image i's
 * rows start srcOffsets[i] bytes into it and lie srcRowPitches[i] bytes apart (the file's pitch rule, DDS_FLAGS_LEGACY_DWORD and the
 * 8 / 16 / 24 bpp rules included: they only change these numbers). DDS_FLAGS_BAD_DXTN_TAILS is an offset too: a level smaller than a block
 * points at the last stored level's bytes.
 *   unpack   payload -> dsts[i], each through its own pitch; all of one format (the conversions of CopyImage, DirectXTexDDS.cpp:1518-1808).
 *            `opaque` forces alpha (the reader's CONV_FLAGS_NOALPHA) where the op carries one.
 *              op                    file bytes  dsts' format                 texel
 *              DXTEX_DDS_ROW_COPY    any         any the library sizes        the bytes, row by row (block rows of a compressed image, every
 *                                                                             plane's rows of a planar one); opaque: the alpha of the 32:32:32:32,
 *                                                                             16:16:16:16, 10:10:10:2, 8:8:8:8, 5:5:5:1 / 4:4:4:4 and A8 classes is set
 *              DXTEX_DDS_ROW_SWIZZLE 4           R8G8B8A8 / B8G8R8A8 / B8G8R8X8 families   red and blue trade places
 *                                                R10G10B10A2 family           the outer 10-bit fields trade places
 *                                                YUY2                         UYVY -> YUY2
 *              _565 _5551 _4444 _ABGR4 _8332 _A8L8 _L6V5U5   2   R8G8B8A8_UNORM   the legacy expansions (565 with the reference's green quirk)
 *              _888                  3           R8G8B8A8_UNORM               B, G, R -> R, G, B, 255
 *              _332                  1           R8G8B8A8_UNORM, B5G6R5_UNORM
 *              _44                   1           R8G8B8A8_UNORM, B4G4R4A4_UNORM
 *              _L8                   1           R8G8B8A8_UNORM
 *              _P8                   1           R8G8B8A8_UNORM               palette[index]; `palette` = 256 words in host memory, read before
 *              _A8P8                 2           R8G8B8A8_UNORM               the call returns; A8P8 ORs the texel's alpha onto the entry's
 *              _L16                  2           R16G16B16A16_UNORM
 *              _L8U8V8               4           R8G8B8A8_UNORM
 *              _WUV10                4           R10G10B10A2_UNORM
 *   pack24   B8G8R8X8_UNORM images -> the writer's 24-bit rows (DDS_FLAGS_FORCE_24BPP_RGB): image i's rows go dstOffsets[i] bytes into `out`,
 *            dstRowPitches[i] apart, 3 bytes a texel. Bytes of `out` outside those rows are not written.
 * HRESULTs, in this order: E_POINTER for a null payload / output, image array, offsets, pitches or pixels; E_INVALIDARG for zero images, an
 * unknown op, a palette that is missing or unwanted; NOT_SUPPORTED for an (op, format) pair outside the table (pack24: any format but
 * B8G8R8X8_UNORM); E_INVALIDARG for images of different formats, a destination too small for its rows (rowPitch below width x texel), a
 * file pitch below the row, rows that reach past payloadBytes / outBytes, or a file side that overlaps the pixels. Nothing is written on
 * any failure. An image of zero width or height is skipped. Row padding of an image is never written. */
#define DXTEX_DDS_ROW_COPY     0u
#define DXTEX_DDS_ROW_SWIZZLE  1u
#define DXTEX_DDS_ROW_565      2u
#define DXTEX_DDS_ROW_5551     3u
#define DXTEX_DDS_ROW_4444     4u
#define DXTEX_DDS_ROW_ABGR4    5u
#define DXTEX_DDS_ROW_888      6u
#define DXTEX_DDS_ROW_332      7u
#define DXTEX_DDS_ROW_8332     8u
#define DXTEX_DDS_ROW_P8       9u
#define DXTEX_DDS_ROW_A8P8     10u
#define DXTEX_DDS_ROW_44       11u
#define DXTEX_DDS_ROW_L8       12u
#define DXTEX_DDS_ROW_L16      13u
#define DXTEX_DDS_ROW_A8L8     14u
#define DXTEX_DDS_ROW_L6V5U5   15u
#define DXTEX_DDS_ROW_L8U8V8   16u
#define DXTEX_DDS_ROW_WUV10    17u
#define DXTEX_DDS_ROW_OPS      18u
/* host pointers, through the context's staging: the payload goes up as it is, each image's rows come down; returns when they have landed */
dxtex_hresult dxtex_dds_unpack(dxtex_ctx* ctx, const void* payload, size_t payloadBytes, uint32_t op, uint32_t opaque, const uint32_t* palette,
                               const dxtex_image* dsts, const size_t* srcOffsets, const size_t* srcRowPitches, size_t count);
dxtex_hresult dxtex_dds_pack24(dxtex_ctx* ctx, const dxtex_image* srcs, const size_t* dstOffsets, const size_t* dstRowPitches, size_t count, void* out, size_t outBytes);
/* device pointers (the palette and the three arrays stay host pointers): asynchronous on the context's stream, 32 images to a launch. The
 * payload may start at any byte; an image whose rows are dword-aligned on the file side and 16-byte aligned on the image side (see
 * csrc/dds.hip for the exact rule) takes the wide route. */
dxtex_hresult dxtex_dds_unpack_device(dxtex_ctx* ctx, const void* payload, size_t payloadBytes, uint32_t op, uint32_t opaque, const uint32_t* palette,
                                      const dxtex_image* dsts, const size_t* srcOffsets, const size_t* srcRowPitches, size_t count);
dxtex_hresult dxtex_dds_pack24_device(dxtex_ctx* ctx, const dxtex_image* srcs, const size_t* dstOffsets, const size_t* dstRowPitches, size_t count, void* out, size_t outBytes);

/* Portable pixmap (.ppm, .pfm, .phm) texels, the per-texel half of the codec (the text header is byte-serial and stays with the caller,
 * as do the ASCII samples of a P3 file). One image per call. The file side is the samples behind the header: tight rows of width * texel
 * bytes; a .ppm is top-down, a .pfm / .phm stores the image's bottom row first. At least width * height * texel bytes; more are ignored.
 *   unpack   samples -> dst, through dst's pitch (LoadFromPortablePixMap[HDR], Texconv/PortablePixMap.cpp:209-223, :595-681):
 *              kind           file texel      dst->format           texel
 *              DXTEX_PNM_P6   3 bytes R G B   R8G8B8A8_UNORM        c_i = 255 * byte_i / maxval (integer), c_0 | c_1 << 8 | c_2 << 16 | 0xff000000
 *                                                                   in 32-bit unsigned arithmetic: no clamp, a sample above maxval spills upwards
 *              DXTEX_PNM_PF   3 x f32         R32G32B32A32_FLOAT    the elements, alpha 1.0f
 *              DXTEX_PNM_Pf   1 x f32         R32_FLOAT             the element
 *              DXTEX_PNM_PH   3 x f16         R16G16B16A16_FLOAT    the elements, alpha 0x3c00
 *              DXTEX_PNM_Ph   1 x f16         R16_FLOAT             the element
 *            DXTEX_PNM_BIG_ENDIAN swaps the bytes of every 2- or 4-byte element; nothing else looks at a float's bits. maxval is read by
 *            DXTEX_PNM_P6 only.
 *   pack     level 0 of src -> the samples the writer emits (SaveToPortablePixMap[HDR], :361-443, :688-758):
 *              DXTEX_PNM_P6   R8G8B8A8_UNORM[_SRGB], B8G8R8A8_UNORM[_SRGB], B8G8R8X8_UNORM[_SRGB] -> R, G, B, top-down
 *              DXTEX_PNM_PF   R32G32B32A32_FLOAT, R32G32B32_FLOAT, R16G16B16A16_FLOAT (widened exactly) -> 3 little-endian floats, bottom row first
 *              DXTEX_PNM_Pf   R32_FLOAT -> 1 little-endian float, bottom row first
 *            DXTEX_PNM_PH and DXTEX_PNM_Ph are never written (NOT_SUPPORTED).
 * HRESULTs, in this order: E_POINTER for null samples, image or pixels; E_INVALIDARG for an unknown kind, a maxval outside 1..255 with
 * DXTEX_PNM_P6, unknown flag bits, a width, height or sampleBytes of zero; NOT_SUPPORTED for a kind and format that do not pair up per the
 * tables; E_INVALIDARG for sampleBytes below width * height * texel bytes, a row pitch smaller than the row, or samples that overlap the
 * pixels. Bytes of the image outside width * texel bytes of each row, and samples behind width * height * texel bytes, are not written. */
#define DXTEX_PNM_P6          0u
#define DXTEX_PNM_PF          1u
#define DXTEX_PNM_Pf          2u
#define DXTEX_PNM_PH          3u
#define DXTEX_PNM_Ph          4u
#define DXTEX_PNM_BIG_ENDIAN  0x1u
/* host pointers, through the context's staging: the samples go up as they are, the rows come down through the image's pitch */
dxtex_hresult dxtex_pnm_unpack(dxtex_ctx* ctx, const void* samples, size_t sampleBytes, uint32_t kind, uint32_t maxval, uint32_t flags, const dxtex_image* dst);
dxtex_hresult dxtex_pnm_pack(dxtex_ctx* ctx, const dxtex_image* src, uint32_t kind, void* samples, size_t sampleBytes);
/* device pointers: asynchronous on the context's stream. The samples may start at any byte; see csrc/pnm.hip for the alignment that takes
 * the wide route (a width that is a multiple of 4, samples on a multiple of 4, 8 or 16 bytes by kind, image rows on 16). */
dxtex_hresult dxtex_pnm_unpack_device(dxtex_ctx* ctx, const void* samples, size_t sampleBytes, uint32_t kind, uint32_t maxval, uint32_t flags, const dxtex_image* dst);
dxtex_hresult dxtex_pnm_pack_device(dxtex_ctx* ctx, const dxtex_image* src, uint32_t kind, void* samples, size_t sampleBytes);

/* PNG (.png) texels, the per-texel half of the codec (chunks, CRCs, inflate and the row filters are byte-serial and stay with the caller).
 * One image per call. The file side is the unfiltered image data: tight rows of ceil(width * bits / 8) bytes, no filter byte, top-down.
 * At least height such rows; more bytes are ignored.
 *   unpack   rows -> dst, through dst's pitch (Update and GuessFormat, Auxiliary/DirectXTexPNG.cpp:126-225):
 *              kind                     bits a texel   dst->format                                   texel
 *              DXTEX_PNG_G1 / G2 / G4   1, 2, 4        R8_UNORM                                      sample * 255, 85, 17; first texel in the high bits
 *              DXTEX_PNG_G8 / G16       8, 16          R8_UNORM / R16_UNORM                          the sample, 16 bits swapped to little-endian
 *              DXTEX_PNG_GA8 / GA16     16, 32         R8G8B8A8_UNORM / R16G16B16A16_UNORM           g, g, g, a
 *              DXTEX_PNG_RGB8           24             R8G8B8A8_UNORM[_SRGB]; B8G8R8X8_UNORM[_SRGB] with DXTEX_PNG_BGR   r, g, b, 0xff
 *              DXTEX_PNG_RGBA8          32             R8G8B8A8_UNORM[_SRGB]; B8G8R8A8_UNORM[_SRGB] with DXTEX_PNG_BGR   r, g, b, a
 *              DXTEX_PNG_RGB16 / RGBA16 48, 64         R16G16B16A16_UNORM                            swapped; the filler is 0xffff
 *              DXTEX_PNG_P1 .. P8       1, 2, 4, 8     as DXTEX_PNG_RGB8                             palette[index]
 *            palette (the palette kinds only; NULL otherwise): paletteCount words R | G << 8 | B << 16 | A << 24 in host memory, read
 *            before the call returns, 1 to 256 of them; an index at or past paletteCount gives opaque black (0xff000000). DXTEX_PNG_BGR
 *            exchanges the first and third byte of the texel of DXTEX_PNG_RGB8, DXTEX_PNG_RGBA8 and the palette kinds, and with it the
 *            format they pair with; the other kinds ignore it.
 *   pack     level 0 of src -> the rows the writer emits (WriteImage, :315-404): R8_UNORM -> grey 8, R16_UNORM -> grey 16 (big-endian),
 *            R8G8B8A8 / B8G8R8A8_UNORM[_SRGB] -> R, G, B, A, R16G16B16A16_UNORM -> RGBA 16 (big-endian), B8G8R8X8_UNORM[_SRGB] -> R, G, B.
 *            width * height * (1, 2, 4, 4, 8, 3) bytes.
 * No sample is premultiplied or gamma-corrected: see host/DirectXTexAMD.h on where this departs from the reference.
 * HRESULTs, in this order: E_POINTER for null rows, image or pixels; E_INVALIDARG for an unknown kind, unknown flag bits, a palette that
 * is missing, unasked for or of a count outside 1..256, a width, height or byte count of zero; NOT_SUPPORTED for a kind, flag and format
 * that do not pair up per the tables; E_INVALIDARG for fewer bytes than the rows take, a row pitch smaller than the row, or rows that
 * overlap the pixels. Bytes of the image outside each row's texels, and bytes behind the rows, are not written. */
#define DXTEX_PNG_G1      0u
#define DXTEX_PNG_G2      1u
#define DXTEX_PNG_G4      2u
#define DXTEX_PNG_G8      3u
#define DXTEX_PNG_G16     4u
#define DXTEX_PNG_GA8     5u
#define DXTEX_PNG_GA16    6u
#define DXTEX_PNG_RGB8    7u
#define DXTEX_PNG_RGB16   8u
#define DXTEX_PNG_RGBA8   9u
#define DXTEX_PNG_RGBA16  10u
#define DXTEX_PNG_P1      11u
#define DXTEX_PNG_P2      12u
#define DXTEX_PNG_P4      13u
#define DXTEX_PNG_P8      14u
#define DXTEX_PNG_BGR     0x1u
/* host pointers, through the context's staging: the rows go up as they are, the image comes down through its pitch */
dxtex_hresult dxtex_png_unpack(dxtex_ctx* ctx, const void* rows, size_t rowsBytes, uint32_t kind, uint32_t flags, const uint32_t* palette, uint32_t paletteCount,
                               const dxtex_image* dst);
dxtex_hresult dxtex_png_pack(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes);
/* device pointers (the palette stays a host pointer): asynchronous on the context's stream. The rows may start at any byte; see
 * csrc/png.hip for the alignment that takes the wide route. */
dxtex_hresult dxtex_png_unpack_device(dxtex_ctx* ctx, const void* rows, size_t rowsBytes, uint32_t kind, uint32_t flags, const uint32_t* palette, uint32_t paletteCount,
                                      const dxtex_image* dst);
dxtex_hresult dxtex_png_pack_device(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes);

/* JPEG (.jpg) samples: everything behind the Huffman walk, which is byte-serial and stays with the caller. One image per call. The file
 * side is the frame and its quantised coefficients: int16, 64 a block in natural (row-major) order, blocks in raster order per component,
 * one component after another from offset 0 with nothing between them, each component padded to whole MCUs:
 * blocksPerRow = ceil(width / (8 hmax)) * h and blockRows = ceil(height / (8 vmax)) * v. The call dequantises, runs libjpeg's JDCT_ISLOW
 * inverse DCT (jidctint.c), its fancy upsampling (jdsample.c) and its YCbCr -> RGB (jdcolor.c) and stores through dst's pitch:
 *   colour             components   sampling (luma over 1x1 chroma)   dst->format              texel
 *   DXTEX_JPEG_GREY    1            1x1                               R8_UNORM                 the sample
 *   DXTEX_JPEG_YCBCR   3            1x1, 2x1, 2x2                     R8G8B8A8_UNORM[_SRGB]    r, g, b, 0xff after the transform
 *   DXTEX_JPEG_RGB     3            1x1, 2x1, 2x2                     R8G8B8A8_UNORM[_SRGB]    the three samples, 0xff
 * All arithmetic is 32-bit and wraps, so every input has one result, the one csrc/dxtex_jpeg.h gives on the host; it is libjpeg's wherever
 * libjpeg's own arithmetic does not overflow. More coefficient bytes than the frame takes are ignored.
 * HRESULTs, in this order: E_POINTER for null coefficients, frame, image or pixels; E_INVALIDARG for an unknown colour, a component count
 * that does not match it, a width or height of 0 or above 65535, an image that is not the frame's size, coefficients at an odd address, a
 * quantiser index above 3 or a sampling factor outside 1..4; NOT_SUPPORTED for sampling outside the table or a format that does not pair
 * with the colour; E_INVALIDARG for block counts or offsets that are not the frame's, fewer bytes than the frame takes, a row pitch smaller
 * than the row, or coefficients that overlap the pixels. Bytes of the image outside each row's texels are not written. */
#define DXTEX_JPEG_GREY   0u
#define DXTEX_JPEG_YCBCR  1u
#define DXTEX_JPEG_RGB    2u
typedef struct dxtex_jpeg_component
{
    uint32_t h, v;                 /* sampling factors */
    uint32_t quant;                /* index into dxtex_jpeg_frame.quant */
    uint32_t blocksPerRow, blockRows;
    uint32_t reserved;             /* 0 */
    uint64_t offset;               /* of the component's first coefficient, in coefficients (not bytes) */
} dxtex_jpeg_component;
typedef struct dxtex_jpeg_frame
{
    uint32_t width, height;
    uint32_t components;           /* 1 or 3 */
    uint32_t colour;               /* DXTEX_JPEG_* */
    dxtex_jpeg_component component[3];
    uint16_t quant[4][64];         /* natural order; entries a component does not name are ignored */
} dxtex_jpeg_frame;
/* host pointers, through the context's staging: the coefficients go up as they are, the image comes down through its pitch */
dxtex_hresult dxtex_jpeg_decode(dxtex_ctx* ctx, const void* coefficients, size_t coefficientBytes, const dxtex_jpeg_frame* frame, const dxtex_image* dst);
/* device pointers (the frame stays a host pointer, read before the call returns): asynchronous on the context's stream. The coefficients
 * may start at any even byte; see csrc/jpeg.hip for the alignments that take 16-byte loads and the wide route of jpeg_colour. */
dxtex_hresult dxtex_jpeg_decode_device(dxtex_ctx* ctx, const void* coefficients, size_t coefficientBytes, const dxtex_jpeg_frame* frame, const dxtex_image* dst);
/* The other direction: everything in front of the Huffman coder, which stays with the caller. The call runs libjpeg's RGB -> YCbCr
 * (jccolor.c), its edge replication (jcprepct.c), its 2x1 / 2x2 chroma average without smoothing (jcsample.c), its JDCT_ISLOW forward DCT
 * (jfdctint.c), its quantiser (jcdctmgr.c: the value over 8 * entry, rounded half away from zero) and its dummy blocks (jccoefct.c: all AC
 * zero, the DC of the block coded before) and writes the frame's coefficients in the layout above:
 *   colour             components   sampling (luma over 1x1 chroma)   src->format
 *   DXTEX_JPEG_GREY    1            1x1                               R8_UNORM
 *   DXTEX_JPEG_YCBCR   3            1x1, 2x1, 2x2                     R8G8B8A8_UNORM[_SRGB], B8G8R8A8_UNORM[_SRGB], B8G8R8X8_UNORM[_SRGB]
 * Alpha or X is ignored. The quantiser entries are the frame's own, 1 to 65535. Arithmetic is 32-bit, that of csrc/dxtex_jpeg.h on the host.
 * HRESULTs, in dxtex_jpeg_decode's order: E_POINTER for null coefficients, frame, image or pixels; E_INVALIDARG for an unknown colour, a
 * component count that does not match it, a width or height of 0 or above 65535, an image that is not the frame's size, coefficients at an
 * odd address, a quantiser index above 3 or a sampling factor outside 1..4; NOT_SUPPORTED for DXTEX_JPEG_RGB, sampling outside the table
 * or a format that does not pair with the colour; E_INVALIDARG for block counts or offsets that are not the frame's, an entry of 0 in a
 * quantiser table a component names, fewer coefficient bytes than the frame takes, a row pitch smaller than the row, or coefficients that
 * overlap the pixels. Bytes behind the frame's coefficients are not written; the image is not written. */
/* host pointers, through the context's staging: the image's rows go up, the coefficients come down */
dxtex_hresult dxtex_jpeg_encode(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_jpeg_frame* frame, void* coefficients, size_t coefficientBytes);
/* device pointers (the frame stays a host pointer, read before the call returns): asynchronous on the context's stream. The coefficients
 * may start at any even byte; see csrc/jpeg_encode.hip for the alignments that take 16-byte stores and the wide route of jpeg_samples. */
dxtex_hresult dxtex_jpeg_encode_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_jpeg_frame* frame, void* coefficients, size_t coefficientBytes);

/* OpenEXR (.exr) scanline chunks: everything behind the header walk, the offset table, the inflater and the RLE packets, which are
 * byte-serial and stay with the caller (Auxiliary/DirectXTexEXR.cpp reads through the OpenEXR library; csrc/dxtex_exr.h states the rules).
 * The file side is ONE STREAM of the chunks' expanded bytes and a descriptor per chunk. A chunk holds `rows` scanlines of scanlineBytes
 * each: for each scanline, for each channel of the file in name order, `width` samples. It is plain, or coded - what a ZIP, ZIPS or RLE
 * chunk expands to: delta-coded bytes in two planes.
 *   unpack   undoes every coded chunk (the byte-wise prefix sum, exr_undo; the planes are addressed, not moved), then writes every
 *            chunk's rows (exr_texels): R, G, B and A are gathered through `channels` (entry 0 R .. 3 A: the byte offset of the channel's
 *            samples within a scanline and DXTEX_EXR_UINT / _HALF / _FLOAT, or DXTEX_EXR_ABSENT), converted to half - HALF as bits; FLOAT
 *            rounded to nearest even, but a finite value beyond +-65504 becomes the infinity and a NaN keeps its top mantissa bits; UINT
 *            likewise, above 65504 +Inf - and an absent R, G or B reads 0, an absent A 1.0. Row y of the window lands at row
 *            y % items[0].height of items[y / items[0].height]: one item, or the six faces of an environment map.
 *   pack     level 0 of src -> the writer's scanlines, tight: for each row `width` halves of A, then of B, of G, of R (8 bytes a texel).
 *            R16G16B16A16_FLOAT moves as bits; R32G32B32A32_FLOAT and R32G32B32_FLOAT (alpha 1.0) convert by XMConvertFloatToHalf.
 * HRESULTs of unpack, in this order: E_POINTER for a null stream, chunks, channels, items or pixels; E_INVALIDARG for no chunks, no items
 * or more than six, a width or height of zero, an unknown channel type or a scanlineBytes of zero; NOT_SUPPORTED for items that are not
 * R16G16B16A16_FLOAT; E_INVALIDARG for items of different sizes, an offset in the channel table that leaves a scanline, a descriptor that
 * leaves the stream, is not rows * scanlineBytes long, names rows outside the window or overlaps the one before it (descriptors are in
 * ascending stream order), a row pitch smaller than the row, or a stream that overlaps an item's pixels.
 * HRESULTs of pack: E_POINTER for a null image, pixels or scanlines; E_INVALIDARG for a width or height of zero; NOT_SUPPORTED for any
 * other format; E_INVALIDARG for fewer than width * height * 8 bytes, a row pitch smaller than the row, or scanlines that overlap the
 * pixels. Bytes of the items outside each row's texels, and rows no chunk names, are not written. */
#define DXTEX_EXR_UINT    0u
#define DXTEX_EXR_HALF    1u
#define DXTEX_EXR_FLOAT   2u
#define DXTEX_EXR_ABSENT  3u
typedef struct dxtex_exr_chunk
{
    uint64_t offset;               /* of the chunk's first byte in the stream */
    uint32_t bytes;                /* rows * scanlineBytes */
    uint32_t firstRow, rows;       /* of the window, from its top */
    uint32_t coded;                /* 0 plain, 1 coded */
} dxtex_exr_chunk;
typedef struct dxtex_exr_channel { uint32_t offset, type; } dxtex_exr_channel;
/* host pointers, through the context's staging: the stream goes up as it is (and is not written), the rows come down through the items'
 * pitches */
dxtex_hresult dxtex_exr_unpack(dxtex_ctx* ctx, const void* stream, size_t streamBytes, const dxtex_exr_chunk* chunks, size_t chunkCount,
                               const dxtex_exr_channel* channels, uint32_t scanlineBytes, const dxtex_image* items, size_t itemCount);
dxtex_hresult dxtex_exr_pack(dxtex_ctx* ctx, const dxtex_image* src, void* scanlines, size_t scanlineBytes);
/* device pointers (the descriptors and the channel table stay host pointers, read before the call returns): asynchronous on the
 * context's stream. THE STREAM IS WRITTEN: its coded chunks are left undone in place. It may start at any byte; see csrc/exr.hip for the
 * alignments that take the wide routes (stream and coded chunks on multiples of 16). */
dxtex_hresult dxtex_exr_unpack_device(dxtex_ctx* ctx, void* stream, size_t streamBytes, const dxtex_exr_chunk* chunks, size_t chunkCount,
                                      const dxtex_exr_channel* channels, uint32_t scanlineBytes, const dxtex_image* items, size_t itemCount);
dxtex_hresult dxtex_exr_pack_device(dxtex_ctx* ctx, const dxtex_image* src, void* scanlines, size_t scanlineBytes);

/* TIFF (.tif) strips and tiles: everything behind the header, the IFD walk, LZW, PackBits and inflate, which are byte-serial and stay with
 * the caller (the reference reads TIFF through WIC; csrc/dxtex_tiff.h states the rules). The file side is ONE STREAM of the segments'
 * expanded bytes and a descriptor per segment - a strip, a tile, or one of either of one plane where planes are separate - still
 * predictor-coded, in the file's byte order, at the file's bits per sample; rows start on byte boundaries.
 *   unpack   undoes the predictor of every row in place (tiff_undo: predictor 2 is a prefix sum over 8- or 16-bit elements with a stride
 *            of samples per pixel, and leaves big-endian 16-bit rows little-endian; predictor 3 is that sum over the row's bytes, and its
 *            four byte planes are addressed, not regrouped), then writes every segment's texels (tiff_texels) into dst, whose format is
 *            the kind's: R8_UNORM for GREY1 / 4 / 8 (multiplied out, WhiteIsZero inverted), R16_UNORM, R32_FLOAT, R8G8B8A8_UNORM for
 *            the palette kinds (`palette`: the 256 words to store), RGB8 and RGBA8 (or its _SRGB twin), R16G16B16A16_UNORM,
 *            R32G32B32_FLOAT, R32G32B32A32_FLOAT; a missing alpha, and a fourth sample under `opaque`, is the depth's maximum.
 *            A file that is its image already (chunky strips, predictor 1, little-endian or 8-bit, GREY8 / 16 / 32F, RGBA8 / 16 / 32F or
 *            RGB32F, nothing inverted or forced) is row copies and no kernel.
 *   pack     level 0 of src -> the writer's tight rows: R8_UNORM, R16_UNORM, R32_FLOAT, R8G8B8A8_UNORM[_SRGB], R16G16B16A16_UNORM,
 *            R32G32B32_FLOAT and R32G32B32A32_FLOAT as they are (row copies, no kernel), B8G8R8A8_UNORM[_SRGB] as RGBA and
 *            B8G8R8X8_UNORM[_SRGB] as RGB at 3 bytes a texel (tiff_pack).
 * HRESULTs of unpack, in this order: E_POINTER for a null stream, segments, layout, dst or pixels, or a palette kind without a palette;
 * E_INVALIDARG for no segments, a width or height of zero or other than the layout's, an unknown kind, bits or samples that are not the
 * kind's, a predictor other than 1, 2, 3; NOT_SUPPORTED for a predictor that does not fit the bits (2: 8 or 16, 3: 32) or a dst format
 * that is not the kind's; E_INVALIDARG for a descriptor that leaves the stream, the image or its plane count, whose rowBytes is smaller
 * than its columns need, or that overlaps the one before it (descriptors are in ascending stream order), a row pitch smaller than the
 * row, or a stream that overlaps the pixels.
 * HRESULTs of pack: E_POINTER for a null image, pixels or rows; E_INVALIDARG for a width or height of zero; NOT_SUPPORTED for any other
 * format; E_INVALIDARG for fewer than height * width * (file bytes a texel) bytes of rows, a row pitch smaller than the row, or rows
 * that overlap the pixels. Bytes of dst outside each row's texels, and texels no segment names, are not written. */
#define DXTEX_TIFF_GREY1    0u
#define DXTEX_TIFF_GREY4    1u
#define DXTEX_TIFF_GREY8    2u
#define DXTEX_TIFF_GREY16   3u
#define DXTEX_TIFF_GREY32F  4u
#define DXTEX_TIFF_PAL1     5u
#define DXTEX_TIFF_PAL4     6u
#define DXTEX_TIFF_PAL8     7u
#define DXTEX_TIFF_RGB8     8u
#define DXTEX_TIFF_RGBA8    9u
#define DXTEX_TIFF_RGB16    10u
#define DXTEX_TIFF_RGBA16   11u
#define DXTEX_TIFF_RGB32F   12u
#define DXTEX_TIFF_RGBA32F  13u
typedef struct dxtex_tiff_segment
{
    uint64_t offset;               /* of the segment's first byte in the stream */
    uint32_t firstRow, rows;       /* of the image */
    uint32_t firstCol, cols;       /* of the image; a tile's row may hold more columns than cols */
    uint32_t rowBytes;             /* of one row of the segment */
    uint32_t plane;                /* 0 unless planes are separate */
} dxtex_tiff_segment;
typedef struct dxtex_tiff_layout
{
    uint32_t width, height;
    uint32_t bits, samples;        /* the kind's */
    uint32_t kind;                 /* DXTEX_TIFF_* */
    uint32_t predictor;            /* 1, 2 or 3 */
    uint32_t bigEndian;            /* an MM file */
    uint32_t planar;               /* PlanarConfiguration 2 and more than one sample */
    uint32_t whiteIsZero;
    uint32_t opaque;               /* the fourth sample is not alpha: it reads as the maximum */
} dxtex_tiff_layout;
/* host pointers, through the context's staging: the stream goes up as it is (and is not written), the rows come down through dst's pitch */
dxtex_hresult dxtex_tiff_unpack(dxtex_ctx* ctx, const void* stream, size_t streamBytes, const dxtex_tiff_segment* segments, size_t segmentCount,
                                const dxtex_tiff_layout* layout, const uint32_t* palette, const dxtex_image* dst);
dxtex_hresult dxtex_tiff_pack(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes);
/* device pointers (the descriptors, the layout and the palette stay host pointers, read before the call returns): asynchronous on the
 * context's stream. THE STREAM IS WRITTEN where the file has a predictor: its rows are left undone in place. It may start at any byte;
 * see csrc/tiff.hip for the alignments that take the wide routes. */
dxtex_hresult dxtex_tiff_unpack_device(dxtex_ctx* ctx, void* stream, size_t streamBytes, const dxtex_tiff_segment* segments, size_t segmentCount,
                                       const dxtex_tiff_layout* layout, const uint32_t* palette, const dxtex_image* dst);
dxtex_hresult dxtex_tiff_pack_device(dxtex_ctx* ctx, const dxtex_image* src, void* rows, size_t rowsBytes);

dxtex_hresult dxtex_resize(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter);
dxtex_hresult dxtex_resize_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t filter);

/* ---- one image over several contexts (in-process strong scaling) --------------------------------
 * The role of the reference's own split of one image over its workers (CompressBC_Parallel hands block rows to OpenMP threads,
 * DirectXTexCompress.cpp:257-281): `ctxs` are nctx contexts - normally one per GPU of the node, several on one GPU work too - and the
 * image in HOST memory is cut into stripes of block rows (Compress) or destination rows with the filter's halo of source rows
 * (GenerateMipMaps: exact-halving levels of at least 256 rows, point / box / linear / cubic, no V wrap / mirror; everything else runs on
 * ctxs[0]). Each stripe goes through the single-context entry point on its own thread; the result is byte for byte that of
 * dxtex_compress / dxtex_generate_mips on one context. Errors: the first failing stripe's code (its text in that context's last_error). */
dxtex_hresult dxtex_compress_multi(dxtex_ctx* const* ctxs, size_t nctx, const dxtex_image* src, const dxtex_image* dst,
                                   uint32_t flags, float threshold);
dxtex_hresult dxtex_generate_mips_multi(dxtex_ctx* const* ctxs, size_t nctx, const dxtex_image* levels, size_t nlevels, uint32_t filter);

/* ComputeMSE (DirectXTexMisc.cpp:27-176) for two same-size images on the device: per-channel MSE in
 * mse[4] over [0,1] floats. Used for PSNR reporting without a D2H round trip. */
dxtex_hresult dxtex_compute_mse_device(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, double mse[4]);

/* ---- texdiag's diagnostics (Texdiag/texdiag.cpp: analyze, compare, diff) ------------------------------------------------------------
 * All four take uncompressed images of a format the scanline layer loads (decompress first: the host layer does); DXTEX_E_NOT_SUPPORTED
 * otherwise. Results are read back in one device-to-host copy per call, which synchronises the stream. */

/* CMSE_FLAGS, bit-for-bit (DirectXTex.h:1022-1038). */
#define DXTEX_CMSE_DEFAULT          0x0u
#define DXTEX_CMSE_IMAGE1_SRGB      0x1u
#define DXTEX_CMSE_IMAGE2_SRGB      0x2u
#define DXTEX_CMSE_IGNORE_RED       0x10u
#define DXTEX_CMSE_IGNORE_GREEN     0x20u
#define DXTEX_CMSE_IGNORE_BLUE      0x40u
#define DXTEX_CMSE_IGNORE_ALPHA     0x80u
#define DXTEX_CMSE_IMAGE1_X2_BIAS   0x100u
#define DXTEX_CMSE_IMAGE2_X2_BIAS   0x200u
/* ComputeMSE_ (DirectXTexMisc.cpp:27-176) with every CMSE_FLAGS bit: v^2.2 on r, g, b of an sRGB image, then v * 2 - 1 under X2_BIAS, the
 * ignored channels zero; the flags the two formats imply (:47-91) are added. Accumulated in fp64. E_INVALIDARG for a size mismatch. */
dxtex_hresult dxtex_compute_mse_flags_device(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, uint32_t cmse_flags, double mse[4]);

/* Analyze (texdiag.cpp:698-787) over LoadScanline's floats, per channel (r, g, b, a). The reference's quirks stay: `variance` is the raw
 * sum of (v - float(avg))^2, not divided by the texel count (its square root is texdiag's "Std Dev"); luminance is the maximum of
 * (r * 0.3 + g * 0.59) + b * 0.11, never below 0; min / max start from +FLT_MAX / -FLT_MAX. Stated deviation: a NaN takes no part in min,
 * max or luminance (the reference's minps / maxps make that depend on texel order) and is only counted in `specials` with the
 * infinities; -0 orders below +0. min, max, luminance and specials are exact and deterministic; avg and variance are fp64 sums whose
 * last bits depend on the order workgroups finish in. */
typedef struct dxtex_image_stats
{
    float    min[4], max[4];
    double   avg[4], variance[4];
    float    luminance;
    uint64_t specials[4];
} dxtex_image_stats;
/* `count` images (a mip chain, an array, volume slices; formats and sizes may differ), one result each, all read back in one copy.
 * E_POINTER for null pixels or a null result; E_INVALIDARG for no images, an empty image or one above UINT32_MAX texels a side. */
dxtex_hresult dxtex_analyze_device(dxtex_ctx* ctx, const dxtex_image* images, size_t count, dxtex_image_stats* stats_out);
dxtex_hresult dxtex_analyze(dxtex_ctx* ctx, const dxtex_image* images, size_t count, dxtex_image_stats* stats_out);

/* AnalyzeBC (texdiag.cpp:906-1226): the block-mode histogram of one BC image. BC1: hist[0] four-colour, hist[1] three-colour blocks; BC2:
 * none; BC3 alpha / BC4 red: hist[0] eight-value, hist[1] six-value blocks; BC5: the same for red, hist[2] / hist[3] for green; BC6H:
 * hist[1..14] by mode, hist[0] reserved prefixes; BC7: hist[0..7] by mode, hist[8] a zero mode byte. *blocks = ceil(w / 4) * ceil(h / 4)
 * (the reference walks rowPitch / block bytes per row and so counts padding; with tight pitches the two agree).
 * DXTEX_E_NOT_SUPPORTED for a format that is not block-compressed. */
dxtex_hresult dxtex_analyze_bc_device(dxtex_ctx* ctx, const dxtex_image* image, uint64_t hist[15], uint64_t* blocks);
dxtex_hresult dxtex_analyze_bc(dxtex_ctx* ctx, const dxtex_image* image, uint64_t hist[15], uint64_t* blocks);

/* Difference's per-texel map (texdiag.cpp:1285-1309): d = |a - b| on r, g, b with alpha 1; where diffColor (0x00RRGGBB) is not 0 and all
 * three of d are >= threshold the texel becomes that colour (bytes * 1/255, alpha 1). `b` is R32G32B32A32_FLOAT (texdiag converts image
 * 2 first; its rowPitch - and, for the device form, its pointer - a multiple of 16, else E_INVALIDARG), `dst` has a's format and size;
 * stored with StoreScanline's default threshold; row padding of `dst` is not written by either form. E_FAIL for a size mismatch;
 * DXTEX_E_NOT_SUPPORTED for compressed or unknown formats, b not R32G32B32A32_FLOAT, or dst->format != a->format. */
dxtex_hresult dxtex_difference_device(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, uint32_t diffColor, float threshold);
dxtex_hresult dxtex_difference(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, uint32_t diffColor, float threshold);

/* ---- CopyRectangle and texassemble's merge ---------------------------------------------------------------------------------------- */

/* Mirrors DirectX::Rect (DirectXTex.h). */
typedef struct dxtex_rect { size_t x, y, w, h; } dxtex_rect;

/* CopyRectangle (DirectXTexMisc.cpp:275-381): the w x h texels at (x, y) of src into dst at (xOffset, yOffset).
 *   Same format: the rows' bytes are moved as the reference's memcpy moves them, a texel counting BitsPerPixel / 8 bytes - for the packed
 *   two-texel formats (R8G8_B8G8, G8R8_G8B8, YUY2: 4; Y210, Y216: 8) that is an element of two texels, so a row of the rectangle runs
 *   into the image's next row, there as here; where consecutive rows then write the same destination bytes, the later row's are the
 *   ones that stay, as after the reference's row-by-row memcpy.
 *   Different formats: LoadScanline -> ConvertScanline(filter) -> StoreScanline with its default threshold; never dithered (the dither
 *   bits of `filter` are ignored). Stated deviation: the packed two-texel formats are refused on this route (DXTEX_E_NOT_SUPPORTED); the
 *   reference pairs texels from the rectangle's left edge, whatever the parity of x.
 * Bytes of dst outside the rectangle, row padding included, are not written.
 * HRESULTs, in the reference's order (:283-311): E_POINTER for null pixels; DXTEX_E_NOT_SUPPORTED for compressed, planar and palettised
 * formats; E_INVALIDARG for an empty rectangle, one outside src, or one that at its offset is outside dst, and for a value that names no
 * format; DXTEX_E_NOT_SUPPORTED for R1_UNORM; E_FAIL where the rectangle's bytes run past rowPitch * height of either image (the
 * reference tests the source's end and, between different formats, the destination's). Added here: DXTEX_E_NOT_SUPPORTED for formats the
 * scanline layer does not load (typeless ones among them), E_INVALIDARG where the bytes read and the bytes written overlap.
 * dxtex_copy_rectangle: host pointers; uploads the rectangle's rows only and downloads the rows it wrote only.
 * dxtex_copy_rectangles_device: `count` independent rectangles on device memory, asynchronous on the context's stream, ONE kernel launch
 * per 32 rectangles (the jobs travel in the kernel's argument block). All are checked before anything is queued. Rectangles of one
 * call must not write bytes another one of the call reads or writes. */
dxtex_hresult dxtex_copy_rectangle(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_rect* rect, const dxtex_image* dst, uint32_t filter,
                                   size_t xOffset, size_t yOffset);
dxtex_hresult dxtex_copy_rectangles_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_rect* rects, const dxtex_image* dsts,
                                           const size_t* xOffsets, const size_t* yOffsets, size_t count, uint32_t filter);

/* texassemble's merge (Texassemble/texassemble.cpp:2236-2268): per texel out[k] = (permute[k] < 4 ? a : b)[permute[k] & 3] (XMVectorPermute),
 * then 0 where zero[k], then 1 where one[k]; a through LoadScanline, `b` R32G32B32A32_FLOAT (texassemble converts image 2 first; its
 * rowPitch - and, for the device form, its pointer - a multiple of 16, else E_INVALIDARG); stored in a's format with StoreScanline's
 * default threshold. Channels are moved, never computed. dst has a's format and size; its row padding is not written by either form.
 * E_INVALIDARG for a permute index above 7 or overlapping pixels; E_FAIL for a size mismatch; DXTEX_E_NOT_SUPPORTED for compressed or
 * unknown formats, b not R32G32B32A32_FLOAT, or dst->format != a->format. */
dxtex_hresult dxtex_merge_image(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, const uint32_t permute[4],
                                const uint32_t zero[4], const uint32_t one[4]);
dxtex_hresult dxtex_merge_image_device(dxtex_ctx* ctx, const dxtex_image* a, const dxtex_image* b, const dxtex_image* dst, const uint32_t permute[4],
                                       const uint32_t zero[4], const uint32_t one[4]);

/* ---- FlipRotate (DirectXTex.h:723-737, DirectXTexFlipRotate.cpp) ----------------------------------------------------------------------- */

/* TEX_FR_FLAGS with the reference's values. Legal: flags != 0 && (flags & ~0x1B) == 0, fifteen values; anything else is E_INVALIDARG. */
#define DXTEX_FR_ROTATE0          0x0u
#define DXTEX_FR_ROTATE90         0x1u
#define DXTEX_FR_ROTATE180        0x2u
#define DXTEX_FR_ROTATE270        0x3u
#define DXTEX_FR_FLIP_HORIZONTAL  0x08u
#define DXTEX_FR_FLIP_VERTICAL    0x10u

/* `src` turned CLOCKWISE by the angle, then mirrored left-right if FLIP_HORIZONTAL is set, then mirrored top-bottom if FLIP_VERTICAL is
 * set, into `dst`. With src as [h][w] texels:  out = rot90(src, k = -(flags & 3));  H: out = out[:, ::-1];  V: out = out[::-1].
 * Per texel (xd, yd) of the W x H result (W, H = h, w for 90 / 270, else w, h): x1 = H-flag ? W - 1 - xd : xd, y1 = V-flag ? H - 1 - yd : yd;
 * the source texel is (x1, y1) for 0, (y1, h - 1 - x1) for 90, (w - 1 - x1, h - 1 - y1) for 180, (w - 1 - y1, x1) for 270. The fifteen flag
 * words are the eight symmetries of the rectangle: {2, 24} {1, 27} {3, 25} {8, 18} {16, 10} {9, 19} {11, 17} and {26}, the identity.
 * dst has src's format; its size is src's, or the swapped one for 90 / 270. Its rowPitch may be any value at least as large as the row; its
 * row padding and everything outside it are not written, so a destination may be a cell of a larger image (a pointer into it and its pitch).
 * Formats: texels move as bytes and are never loaded or stored through a float row. Every format this library knows whose element is one
 * texel of 1, 2, 4, 8, 12 or 16 bytes is taken, depth and integer formats included. DXTEX_E_NOT_SUPPORTED for compressed formats (as the
 * reference), planar, palettised and typeless formats, the two-texel packed formats and R1_UNORM, and a value that names no format.
 * DEPARTURES from the reference, stated: (1) it hands the flag word to WIC, whose documentation does not say whether a flip combined with a
 * rotation is applied before or after it; its tools never combine them, so the order above is this library's and nothing can check it.
 * (2) It sends formats WIC lacks through R32G32B32A32_FLOAT (or half) and back, which is not the identity (R32_UINT above 2^24); here bits
 * are kept. (3) It would convert the packed formats; here they are refused.
 * HRESULTs, in this order: E_POINTER for null pixels; E_INVALIDARG for illegal flags; DXTEX_E_NOT_SUPPORTED for the formats above; E_FAIL
 * for a format or size mismatch between a pair (the reference's :354-381); E_INVALIDARG for a rowPitch below its row's bytes or a side
 * above 2^31 - 1, and where the bytes read and the bytes written overlap.
 * dxtex_flip_rotate: host pointers, through the context's staging; uploads the source rows' texels and downloads the result rows' texels only.
 * dxtex_flip_rotate_device: `count` independent pairs on device memory, asynchronous on the context's stream; all are checked before
 * anything is queued. ONE kernel launch per route per 32 images (the jobs travel in the kernel's argument block): the four symmetries
 * that keep width and height are row moves, 16 bytes a lane where both first-row addresses, both pitches and the row's byte count are
 * multiples of 16 (and the texel is not 12 bytes), a texel a lane otherwise; the four that exchange them go through a padded LDS tile with
 * both global sides coalesced. Pairs of one call must not write bytes another one of the call reads or writes. */
dxtex_hresult dxtex_flip_rotate(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags);
dxtex_hresult dxtex_flip_rotate_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count, uint32_t flags);

/* ---- ConvertToSinglePlane (DirectXTexConvert.cpp:4912-5077, :5411-5523) ------------------------------------------------------------- */

/* PlanarToSingle (:4916-4939): NV12 (103) and NV11 (110) -> YUY2 (107), P010 (104) -> Y210 (108), P016 (105) -> Y216 (109); 0 where a
 * format has no single-plane form. A separate door: the planar formats stay unknown to every other entry point of this header
 * (dxtex_bits_per_pixel is 0 for them, dxtex_compute_pitch does not take them). */
int32_t       dxtex_planar_to_single(int32_t format);

/* The planar image `src` interleaved into `dst`, which has the same size and the format dxtex_planar_to_single(src->format).
 *   4:2:0 (NV12: 1-byte samples; P010 / P016: 2-byte samples): element k of destination rows 2c and 2c + 1 is
 *     (Y[row][2k], U, Y[row][2k + 1], V) with U, V the samples 2k and 2k + 1 of chroma row c. The chroma plane starts at byte
 *     height * rowPitch of the source, its rows are rowPitch apart.
 *   NV11 (4:1:1): chroma pair j of row y, at byte height * rowPitch + y * (rowPitch >> 1) + 2j, feeds elements 2j and 2j + 1 of row y,
 *     whose luma is samples 4j .. 4j + 3 of luma row y.
 *   The reference's end guard is kept byte for byte (`if ((sPtrUV + 1) >= sourceE) break;` with sourceE = pixels + slicePitch): a chroma
 *     pair whose second sample lies at or beyond slicePitch is not read, and neither it nor any later pair of that chroma row is written.
 *     With ComputePitch's slicePitch that never happens; with a smaller slicePitch the tail of the last rows of dst stays as it was.
 * Both pitches of both images are the caller's; nothing is derived from the format. No byte at or beyond src->pixels + src->slicePitch is
 * read; only the written elements of dst are written, never its row padding.
 * HRESULTs, in the reference's order (:5413-5424, :5005-5030): E_INVALIDARG for a source format that is not planar; E_POINTER for null
 * pixels; DXTEX_E_NOT_SUPPORTED for a planar format without a single-plane form (420_OPAQUE, P208, V208, V408, the Xbox depth planes);
 * E_INVALIDARG for an odd width or height (NV12, P010, P016) or a width that is no multiple of four (NV11). Added here, where the
 * reference would read outside the image it was handed or has no destination of the caller's to get wrong, in this order: E_INVALIDARG
 * for dst->format != dxtex_planar_to_single(src->format); E_FAIL for a destination of another size; E_INVALIDARG for a source rowPitch
 * below the row's bytes, for slicePitch < height * rowPitch, for an odd pointer or pitch with the 16-bit formats, for a destination
 * rowPitch below its row's bytes, and where the bytes read and the bytes written overlap.
 * dxtex_convert_to_single_plane: host pointers, through the context's staging; uploads slicePitch bytes, downloads the elements it wrote.
 * dxtex_convert_to_single_plane_device: `count` independent images on device memory, asynchronous on the context's stream, ONE kernel
 * launch per 32 images (the jobs travel in the kernel's argument block). All are checked before anything is queued. Per image the
 * 16-byte route runs when the row starts of luma and chroma are 8-byte aligned and those of dst 16-byte aligned, else element by element. */
dxtex_hresult dxtex_convert_to_single_plane(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst);
dxtex_hresult dxtex_convert_to_single_plane_device(dxtex_ctx* ctx, const dxtex_image* srcs, const dxtex_image* dsts, size_t count);

/* PremultiplyAlpha / its REVERSE (DirectXTex.h:864-884, DirectXTexPMAlpha.cpp:214-262): same size and format on both sides,
 * the format must carry alpha (else DXTEX_E_NOT_SUPPORTED). `flags` = TEX_PMALPHA_FLAGS. */
#define DXTEX_PMALPHA_DEFAULT      0x0u
#define DXTEX_PMALPHA_IGNORE_SRGB  0x1u
#define DXTEX_PMALPHA_REVERSE      0x2u
#define DXTEX_PMALPHA_SRGB_IN      0x1000000u
#define DXTEX_PMALPHA_SRGB_OUT     0x2000000u
dxtex_hresult dxtex_premultiply_alpha(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags);
dxtex_hresult dxtex_premultiply_alpha_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, uint32_t flags);

/* ScaleMipMapsAlphaForCoverage (DirectXTex.h:848-851, DirectXTexMipmaps.cpp:3483-3556) for one mip chain: dst[0] = src[0];
 * every further level gets its alpha scaled so that its coverage at `alphaReference` matches level 0's (10-step bisection,
 * :310-352). src[i] and dst[i] have the same size and format. */
dxtex_hresult dxtex_scale_mips_alpha_for_coverage(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, size_t nlevels, float alphaReference);
dxtex_hresult dxtex_scale_mips_alpha_for_coverage_device(dxtex_ctx* ctx, const dxtex_image* src, const dxtex_image* dst, size_t nlevels, float alphaReference);

/* ---- device memory helpers (so non-HIP hosts can stay resident in HBM) -------------------------- */
dxtex_hresult dxtex_device_alloc(dxtex_ctx* ctx, size_t bytes, void** out);
dxtex_hresult dxtex_device_free(dxtex_ctx* ctx, void* p);
dxtex_hresult dxtex_memcpy_h2d(dxtex_ctx* ctx, void* dst, const void* src, size_t bytes);
dxtex_hresult dxtex_memcpy_d2h(dxtex_ctx* ctx, void* dst, const void* src, size_t bytes);

/* ---- the device-resident pipeline (texconv's resize -> convert -> mipmaps -> compress chain, Texconv/texconv.cpp:2609, 3109, 3434,
 * 3711, with ONE upload of the source and ONE download of the final payload; the reference's own GPU path keeps its intermediate
 * in device memory the same way, DirectXTexCompressGPU.cpp:34-140) -------------------------------------------------------------
 * The *_device entry points above are the steps; these are what a host needs around them. All are stream-ordered on the context's
 * stream unless stated. */
/* hipMemsetAsync on the context's stream: a device image starts zero-filled like ScratchImage's memory (DirectXTexImage.cpp:376). */
dxtex_hresult dxtex_device_memset(dxtex_ctx* ctx, void* p, int value, size_t bytes);
/* Device-to-device copy of `rows` rows of `rowBytes` bytes between two pitched images (Setup2DMips' copy of the base image into
 * the top of the chain, DirectXTexMipmaps.cpp:851-904). */
dxtex_hresult dxtex_copy_rows_device(dxtex_ctx* ctx, void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t rowBytes, size_t rows);
/* Asynchronous transfers on the context's stream (host memory from dxtex_host_alloc is page-locked, so these overlap with the
 * kernels of other contexts of the same GPU and return at once; with pageable memory they are staged by the runtime). The host
 * buffer must stay valid until dxtex_ctx_synchronize. */
dxtex_hresult dxtex_memcpy_h2d_async(dxtex_ctx* ctx, void* dst, const void* src, size_t bytes);
dxtex_hresult dxtex_memcpy_d2h_async(dxtex_ctx* ctx, void* dst, const void* src, size_t bytes);
/* `rows` rows of `rowBytes` bytes from a pitched device image into pitched host memory: ONE strided copy on the stream (a plain one where
 * both pitches are the row), counted by dxtex_ctx_transfer_bytes as rowBytes * rows. E_INVALIDARG for a row wider than a pitch. */
dxtex_hresult dxtex_memcpy_rows_d2h_async(dxtex_ctx* ctx, void* dst, size_t dstPitch, const void* src, size_t srcPitch, size_t rowBytes, size_t rows);
/* Page-locked host memory for the two ends of the pipeline. */
dxtex_hresult dxtex_host_alloc(dxtex_ctx* ctx, size_t bytes, void** out);
dxtex_hresult dxtex_host_free(dxtex_ctx* ctx, void* p);
/* ScratchImage::IsAlphaAllOpaque (DirectXTexImage.cpp:800-852) over `count` device images of one format: *opaque = 1 when every
 * texel's alpha is >= 0.997 (uncompressed; LoadScanline's alpha) or >= 0.99 (BC1 / BC2 / BC3 / BC7, decoded as IsAlphaAllOpaqueBC
 * does, DirectXTexCompress.cpp:537-625), or when the format has no alpha. Synchronises the stream (4 bytes come back). */
dxtex_hresult dxtex_alpha_all_opaque_device(dxtex_ctx* ctx, const dxtex_image* images, size_t count, int* opaque);
/* Bytes this context has moved over PCIe since its creation or the last reset (every host <-> device copy the library issues for
 * it, staging and tables included): what tests/ and bench.py use to show that a resident pipeline uploads the source once and
 * downloads the payload once. */
dxtex_hresult dxtex_ctx_transfer_bytes(dxtex_ctx* ctx, uint64_t* h2d_bytes, uint64_t* d2h_bytes, int reset);

#ifdef __cplusplus
}
#endif
#endif /* DXTEX_AMD_H */
