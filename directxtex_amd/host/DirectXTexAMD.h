// DirectXTexAMD.h - C++ host layer of the MI355X DirectXTex hot path.
//
// Keeps the reference's API surface for the path (DirectXTex.h:187-216 TexMetadata, :437-498 Image / ScratchImage,
// :799-846 Resize / Convert / GenerateMipMaps, :929-968 Compress / Decompress, :1021 ComputeMSE): same type and
// function names, argument order and meaning, HRESULT codes and ownership rules ("ScratchImage in, ScratchImage out",
// the callee Release()s and re-initialises the output and releases it again on failure). Everything below the
// signatures is new: the functions validate like the reference, allocate the output with ScratchImage, and hand
// `dxtex_image` views to the C ABI (include/dxtex_amd.h), i.e. to HIP kernels. There is no CPU compute path.
//
// Where the reference takes an ID3D11Device* (DirectXTex.h:946-963) these take a Device (a dxtex_ctx bound to one
// MI355X). One Device per GPU / host thread; Devices share nothing.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <vector>

struct dxtex_ctx;

namespace DirectXTexAMD
{
using HRESULT = int32_t;
constexpr HRESULT S_OK = 0;
constexpr HRESULT E_FAIL = HRESULT(0x80004005);
constexpr HRESULT E_INVALIDARG = HRESULT(0x80070057);
constexpr HRESULT E_OUTOFMEMORY = HRESULT(0x8007000E);
constexpr HRESULT E_POINTER = HRESULT(0x80004003);
constexpr HRESULT E_NOTIMPL = HRESULT(0x80004001);
constexpr HRESULT E_ABORT = HRESULT(0x80004004);
constexpr HRESULT E_UNEXPECTED = HRESULT(0x8000FFFF);
constexpr HRESULT HRESULT_E_NOT_SUPPORTED = HRESULT(0x80070032);
constexpr HRESULT HRESULT_E_ARITHMETIC_OVERFLOW = HRESULT(0x80070216);
inline bool FAILED(HRESULT hr) noexcept { return hr < 0; }
inline bool SUCCEEDED(HRESULT hr) noexcept { return hr >= 0; }

// DXGI_FORMAT values this layer understands (public DXGI numbering).
// The public DXGI numbering. The container side of the library (ScratchImage, pitches, DDS) knows every format; the GPU
// entry points work on the subset IsSupportedOnDevice() names and return HRESULT_E_NOT_SUPPORTED for the rest.
enum DXGI_FORMAT : uint32_t
{
    DXGI_FORMAT_UNKNOWN = 0,
    DXGI_FORMAT_R32G32B32A32_TYPELESS = 1, DXGI_FORMAT_R32G32B32A32_FLOAT = 2, DXGI_FORMAT_R32G32B32A32_UINT = 3, DXGI_FORMAT_R32G32B32A32_SINT = 4,
    DXGI_FORMAT_R32G32B32_TYPELESS = 5, DXGI_FORMAT_R32G32B32_FLOAT = 6, DXGI_FORMAT_R32G32B32_UINT = 7, DXGI_FORMAT_R32G32B32_SINT = 8,
    DXGI_FORMAT_R16G16B16A16_TYPELESS = 9, DXGI_FORMAT_R16G16B16A16_FLOAT = 10, DXGI_FORMAT_R16G16B16A16_UNORM = 11, DXGI_FORMAT_R16G16B16A16_UINT = 12,
    DXGI_FORMAT_R16G16B16A16_SNORM = 13, DXGI_FORMAT_R16G16B16A16_SINT = 14,
    DXGI_FORMAT_R32G32_TYPELESS = 15, DXGI_FORMAT_R32G32_FLOAT = 16, DXGI_FORMAT_R32G32_UINT = 17, DXGI_FORMAT_R32G32_SINT = 18,
    DXGI_FORMAT_R32G8X24_TYPELESS = 19, DXGI_FORMAT_D32_FLOAT_S8X24_UINT = 20, DXGI_FORMAT_R32_FLOAT_X8X24_TYPELESS = 21, DXGI_FORMAT_X32_TYPELESS_G8X24_UINT = 22,
    DXGI_FORMAT_R10G10B10A2_TYPELESS = 23, DXGI_FORMAT_R10G10B10A2_UNORM = 24, DXGI_FORMAT_R10G10B10A2_UINT = 25, DXGI_FORMAT_R11G11B10_FLOAT = 26,
    DXGI_FORMAT_R8G8B8A8_TYPELESS = 27, DXGI_FORMAT_R8G8B8A8_UNORM = 28, DXGI_FORMAT_R8G8B8A8_UNORM_SRGB = 29, DXGI_FORMAT_R8G8B8A8_UINT = 30,
    DXGI_FORMAT_R8G8B8A8_SNORM = 31, DXGI_FORMAT_R8G8B8A8_SINT = 32,
    DXGI_FORMAT_R16G16_TYPELESS = 33, DXGI_FORMAT_R16G16_FLOAT = 34, DXGI_FORMAT_R16G16_UNORM = 35, DXGI_FORMAT_R16G16_UINT = 36,
    DXGI_FORMAT_R16G16_SNORM = 37, DXGI_FORMAT_R16G16_SINT = 38,
    DXGI_FORMAT_R32_TYPELESS = 39, DXGI_FORMAT_D32_FLOAT = 40, DXGI_FORMAT_R32_FLOAT = 41, DXGI_FORMAT_R32_UINT = 42, DXGI_FORMAT_R32_SINT = 43,
    DXGI_FORMAT_R24G8_TYPELESS = 44, DXGI_FORMAT_D24_UNORM_S8_UINT = 45, DXGI_FORMAT_R24_UNORM_X8_TYPELESS = 46, DXGI_FORMAT_X24_TYPELESS_G8_UINT = 47,
    DXGI_FORMAT_R8G8_TYPELESS = 48, DXGI_FORMAT_R8G8_UNORM = 49, DXGI_FORMAT_R8G8_UINT = 50, DXGI_FORMAT_R8G8_SNORM = 51, DXGI_FORMAT_R8G8_SINT = 52,
    DXGI_FORMAT_R16_TYPELESS = 53, DXGI_FORMAT_R16_FLOAT = 54, DXGI_FORMAT_D16_UNORM = 55, DXGI_FORMAT_R16_UNORM = 56, DXGI_FORMAT_R16_UINT = 57,
    DXGI_FORMAT_R16_SNORM = 58, DXGI_FORMAT_R16_SINT = 59,
    DXGI_FORMAT_R8_TYPELESS = 60, DXGI_FORMAT_R8_UNORM = 61, DXGI_FORMAT_R8_UINT = 62, DXGI_FORMAT_R8_SNORM = 63, DXGI_FORMAT_R8_SINT = 64,
    DXGI_FORMAT_A8_UNORM = 65, DXGI_FORMAT_R1_UNORM = 66, DXGI_FORMAT_R9G9B9E5_SHAREDEXP = 67,
    DXGI_FORMAT_R8G8_B8G8_UNORM = 68, DXGI_FORMAT_G8R8_G8B8_UNORM = 69,
    DXGI_FORMAT_BC1_TYPELESS = 70, DXGI_FORMAT_BC1_UNORM = 71, DXGI_FORMAT_BC1_UNORM_SRGB = 72,
    DXGI_FORMAT_BC2_TYPELESS = 73, DXGI_FORMAT_BC2_UNORM = 74, DXGI_FORMAT_BC2_UNORM_SRGB = 75,
    DXGI_FORMAT_BC3_TYPELESS = 76, DXGI_FORMAT_BC3_UNORM = 77, DXGI_FORMAT_BC3_UNORM_SRGB = 78,
    DXGI_FORMAT_BC4_TYPELESS = 79, DXGI_FORMAT_BC4_UNORM = 80, DXGI_FORMAT_BC4_SNORM = 81,
    DXGI_FORMAT_BC5_TYPELESS = 82, DXGI_FORMAT_BC5_UNORM = 83, DXGI_FORMAT_BC5_SNORM = 84,
    DXGI_FORMAT_B5G6R5_UNORM = 85, DXGI_FORMAT_B5G5R5A1_UNORM = 86, DXGI_FORMAT_B8G8R8A8_UNORM = 87, DXGI_FORMAT_B8G8R8X8_UNORM = 88,
    DXGI_FORMAT_R10G10B10_XR_BIAS_A2_UNORM = 89, DXGI_FORMAT_B8G8R8A8_TYPELESS = 90, DXGI_FORMAT_B8G8R8A8_UNORM_SRGB = 91,
    DXGI_FORMAT_B8G8R8X8_TYPELESS = 92, DXGI_FORMAT_B8G8R8X8_UNORM_SRGB = 93,
    DXGI_FORMAT_BC6H_TYPELESS = 94, DXGI_FORMAT_BC6H_UF16 = 95, DXGI_FORMAT_BC6H_SF16 = 96,
    DXGI_FORMAT_BC7_TYPELESS = 97, DXGI_FORMAT_BC7_UNORM = 98, DXGI_FORMAT_BC7_UNORM_SRGB = 99,
    DXGI_FORMAT_AYUV = 100, DXGI_FORMAT_Y410 = 101, DXGI_FORMAT_Y416 = 102, DXGI_FORMAT_NV12 = 103, DXGI_FORMAT_P010 = 104, DXGI_FORMAT_P016 = 105,
    DXGI_FORMAT_420_OPAQUE = 106, DXGI_FORMAT_YUY2 = 107, DXGI_FORMAT_Y210 = 108, DXGI_FORMAT_Y216 = 109, DXGI_FORMAT_NV11 = 110,
    DXGI_FORMAT_AI44 = 111, DXGI_FORMAT_IA44 = 112, DXGI_FORMAT_P8 = 113, DXGI_FORMAT_A8P8 = 114, DXGI_FORMAT_B4G4R4A4_UNORM = 115,
    XBOX_DXGI_FORMAT_R10G10B10_7E3_A2_FLOAT = 116, XBOX_DXGI_FORMAT_R10G10B10_6E4_A2_FLOAT = 117,
    DXGI_FORMAT_P208 = 130, DXGI_FORMAT_V208 = 131, DXGI_FORMAT_V408 = 132,
    DXGI_FORMAT_SAMPLER_FEEDBACK_MIN_MIP_OPAQUE = 189, DXGI_FORMAT_SAMPLER_FEEDBACK_MIP_REGION_USED_OPAQUE = 190, DXGI_FORMAT_A4B4G4R4_UNORM = 191,
    // the console formats share 189 and 190 with the sampler-feedback names above (DirectXTexP.h's XBOX_DXGI_FORMAT_* constants); every
    // function of this library reads the two numbers as these
    XBOX_DXGI_FORMAT_R10G10B10_SNORM_A2_UNORM = 189, XBOX_DXGI_FORMAT_R4G4_UNORM = 190,
};

enum TEX_DIMENSION : uint32_t { TEX_DIMENSION_TEXTURE1D = 2, TEX_DIMENSION_TEXTURE2D = 3, TEX_DIMENSION_TEXTURE3D = 4 };

// TEX_COMPRESS_FLAGS / TEX_FILTER_FLAGS: the reference's values (DirectXTex.h:741-793, :887-917)
enum TEX_COMPRESS_FLAGS : uint32_t
{
    TEX_COMPRESS_DEFAULT = 0, TEX_COMPRESS_RGB_DITHER = 0x10000, TEX_COMPRESS_A_DITHER = 0x20000, TEX_COMPRESS_DITHER = 0x30000,
    TEX_COMPRESS_UNIFORM = 0x40000, TEX_COMPRESS_BC7_USE_3SUBSETS = 0x80000, TEX_COMPRESS_BC7_QUICK = 0x100000,
    TEX_COMPRESS_SRGB_IN = 0x1000000, TEX_COMPRESS_SRGB_OUT = 0x2000000, TEX_COMPRESS_SRGB = 0x3000000, TEX_COMPRESS_PARALLEL = 0x10000000,
};
enum TEX_FILTER_FLAGS : uint32_t
{
    TEX_FILTER_DEFAULT = 0, TEX_FILTER_WRAP_U = 0x1, TEX_FILTER_WRAP_V = 0x2, TEX_FILTER_WRAP = 0x7,
    TEX_FILTER_MIRROR_U = 0x10, TEX_FILTER_MIRROR_V = 0x20, TEX_FILTER_MIRROR = 0x70, TEX_FILTER_FLOAT_X2BIAS = 0x200,
    TEX_FILTER_RGB_COPY_RED = 0x1000, TEX_FILTER_RGB_COPY_GREEN = 0x2000, TEX_FILTER_RGB_COPY_BLUE = 0x4000, TEX_FILTER_RGB_COPY_ALPHA = 0x8000,
    TEX_FILTER_DITHER = 0x10000, TEX_FILTER_DITHER_DIFFUSION = 0x20000,
    TEX_FILTER_POINT = 0x100000, TEX_FILTER_LINEAR = 0x200000, TEX_FILTER_CUBIC = 0x300000, TEX_FILTER_BOX = 0x400000, TEX_FILTER_FANT = 0x400000,
    TEX_FILTER_TRIANGLE = 0x500000, TEX_FILTER_SRGB_IN = 0x1000000, TEX_FILTER_SRGB_OUT = 0x2000000, TEX_FILTER_SRGB = 0x3000000,
};
constexpr float TEX_THRESHOLD_DEFAULT = 0.5f;

// Format facts for every DXGI format (DirectXTex.inl:57-60, DirectXTexUtil.cpp:340-960)
constexpr bool IsValid(DXGI_FORMAT fmt) noexcept { return uint32_t(fmt) >= 1 && uint32_t(fmt) <= 191; }
bool IsCompressed(DXGI_FORMAT fmt) noexcept;
bool IsPacked(DXGI_FORMAT fmt) noexcept;
bool IsPlanar(DXGI_FORMAT fmt) noexcept;
bool IsPalettized(DXGI_FORMAT fmt) noexcept;
bool IsSRGB(DXGI_FORMAT fmt) noexcept;
bool HasAlpha(DXGI_FORMAT fmt) noexcept;
bool IsVideo(DXGI_FORMAT fmt) noexcept;
bool IsDepthStencil(DXGI_FORMAT fmt) noexcept;
bool IsBGR(DXGI_FORMAT fmt) noexcept;
bool IsTypeless(DXGI_FORMAT fmt, bool partialTypeless = true) noexcept;
size_t BitsPerColor(DXGI_FORMAT fmt) noexcept;            // the widest channel; 0 for palettised formats
size_t BytesPerBlock(DXGI_FORMAT fmt) noexcept;           // 8 / 16 for BC formats, else 0
DXGI_FORMAT MakeLinear(DXGI_FORMAT fmt) noexcept;
DXGI_FORMAT MakeTypeless(DXGI_FORMAT fmt) noexcept;
DXGI_FORMAT MakeTypelessUNORM(DXGI_FORMAT fmt) noexcept;
DXGI_FORMAT MakeTypelessFLOAT(DXGI_FORMAT fmt) noexcept;
DXGI_FORMAT MakeSRGB(DXGI_FORMAT fmt) noexcept;
size_t BitsPerPixel(DXGI_FORMAT fmt) noexcept;
// true for the formats the GPU entry points (Compress, Convert, Resize, ...) accept
bool IsSupportedOnDevice(DXGI_FORMAT fmt) noexcept;
// ComputePitch / ComputeScanlines (DirectXTexUtil.cpp:961-1247). CP_FLAGS values as in the reference (DirectXTex.h:104-137).
enum CP_FLAGS : uint32_t
{
    CP_FLAGS_NONE = 0, CP_FLAGS_LEGACY_DWORD = 0x1, CP_FLAGS_PARAGRAPH = 0x2, CP_FLAGS_YMM = 0x4, CP_FLAGS_ZMM = 0x8, CP_FLAGS_PAGE4K = 0x200,
    CP_FLAGS_BAD_DXTN_TAILS = 0x1000, CP_FLAGS_24BPP = 0x10000, CP_FLAGS_16BPP = 0x20000, CP_FLAGS_8BPP = 0x40000,
};
HRESULT ComputePitch(DXGI_FORMAT fmt, size_t width, size_t height, size_t& rowPitch, size_t& slicePitch, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
size_t ComputeScanlines(DXGI_FORMAT fmt, size_t height) noexcept;
// the standard shape of a 64 KiB tile of a tiled resource (DirectXTexUtil.cpp:1251-1405)
struct TileShape { size_t width, height, depth; };
// CalculateMipLevels (DirectXTexMipmaps.cpp:40-69): mipLevels == 0 asks for the full chain
HRESULT ComputeTileShape(DXGI_FORMAT fmt, TEX_DIMENSION dimension, TileShape& tiling) noexcept;
bool CalculateMipLevels(size_t width, size_t height, size_t& mipLevels) noexcept;
bool CalculateMipLevels3D(size_t width, size_t height, size_t depth, size_t& mipLevels) noexcept;

enum TEX_MISC_FLAG : uint32_t { TEX_MISC_TEXTURECUBE = 0x4 };
enum TEX_MISC_FLAG2 : uint32_t { TEX_MISC2_ALPHA_MODE_MASK = 0x7 };
enum TEX_ALPHA_MODE : uint32_t
{
    TEX_ALPHA_MODE_UNKNOWN = 0, TEX_ALPHA_MODE_STRAIGHT = 1, TEX_ALPHA_MODE_PREMULTIPLIED = 2, TEX_ALPHA_MODE_OPAQUE = 3, TEX_ALPHA_MODE_CUSTOM = 4,
};

struct TexMetadata
{
    size_t width = 0, height = 0, depth = 0, arraySize = 0, mipLevels = 0;
    uint32_t miscFlags = 0, miscFlags2 = 0;
    DXGI_FORMAT format = DXGI_FORMAT_UNKNOWN;
    TEX_DIMENSION dimension = TEX_DIMENSION_TEXTURE2D;
    // index = item * mipLevels + mip for 1D / 2D textures (DirectXTexUtil.cpp:1695-1740)
    size_t ComputeIndex(size_t mip, size_t item, size_t slice) const noexcept;
    // D3D11CalcSubresource / D3D12CalcSubresource (DirectXTexUtil.cpp:1744-1806); uint32_t(-1) when out of range
    uint32_t CalculateSubresource(size_t mip, size_t item) const noexcept;
    uint32_t CalculateSubresource(size_t mip, size_t item, size_t plane) const noexcept;
    bool IsVolumemap() const noexcept { return dimension == TEX_DIMENSION_TEXTURE3D; }
    bool IsCubemap() const noexcept { return (miscFlags & TEX_MISC_TEXTURECUBE) != 0; }
    // the alpha mode lives in the low three bits of miscFlags2 (DirectXTex.h:174-207)
    bool IsPMAlpha() const noexcept { return (miscFlags2 & TEX_MISC2_ALPHA_MODE_MASK) == TEX_ALPHA_MODE_PREMULTIPLIED; }
    void SetAlphaMode(TEX_ALPHA_MODE mode) noexcept { miscFlags2 = (miscFlags2 & ~uint32_t(TEX_MISC2_ALPHA_MODE_MASK)) | uint32_t(mode); }
    TEX_ALPHA_MODE GetAlphaMode() const noexcept { return TEX_ALPHA_MODE(miscFlags2 & TEX_MISC2_ALPHA_MODE_MASK); }
};

struct Image
{
    size_t width = 0, height = 0;
    DXGI_FORMAT format = DXGI_FORMAT_UNKNOWN;
    size_t rowPitch = 0, slicePitch = 0;
    uint8_t* pixels = nullptr;
};

// One 16-byte-aligned, zero-filled allocation; images laid out item-major, then by mip (DirectXTexImage.cpp:173-209).
class ScratchImage
{
public:
    ScratchImage() noexcept = default;
    ScratchImage(ScratchImage&& o) noexcept { *this = static_cast<ScratchImage&&>(o); }
    ScratchImage& operator=(ScratchImage&& o) noexcept;
    ScratchImage(const ScratchImage&) = delete;
    ScratchImage& operator=(const ScratchImage&) = delete;
    ~ScratchImage() { Release(); }

    // any valid, non-palettised DXGI format can be held (DirectXTexImage.cpp:300-505); flags select the pitch rule
    HRESULT Initialize(const TexMetadata& mdata, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    HRESULT Initialize1D(DXGI_FORMAT fmt, size_t length, size_t arraySize, size_t mipLevels, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    HRESULT Initialize2D(DXGI_FORMAT fmt, size_t width, size_t height, size_t arraySize, size_t mipLevels, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    HRESULT Initialize3D(DXGI_FORMAT fmt, size_t width, size_t height, size_t depth, size_t mipLevels, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    HRESULT InitializeCube(DXGI_FORMAT fmt, size_t width, size_t height, size_t nCubes, size_t mipLevels, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    // copies of caller images (DirectXTexImage.cpp:534-723): one image, an array, cubemaps (a multiple of six), a volume
    HRESULT InitializeFromImage(const Image& srcImage, bool allow1D = false, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    HRESULT InitializeArrayFromImages(const Image* images, size_t nImages, bool allow1D = false, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    HRESULT InitializeCubeFromImages(const Image* images, size_t nImages, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    HRESULT Initialize3DFromImages(const Image* images, size_t depth, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    bool OverrideFormat(DXGI_FORMAT f) noexcept;               // relabels the pixels (same size per texel is the caller's business)
    void Release() noexcept;

    const TexMetadata& GetMetadata() const noexcept { return m_metadata; }
    const Image* GetImage(size_t mip, size_t item, size_t slice) const noexcept;
    const Image* GetImages() const noexcept { return m_images.get(); }
    size_t GetImageCount() const noexcept { return m_nimages; }
    uint8_t* GetPixels() const noexcept { return m_memory; }
    size_t GetPixelsSize() const noexcept { return m_size; }

private:
    size_t m_nimages = 0, m_size = 0;
    TexMetadata m_metadata;
    std::unique_ptr<Image[]> m_images;
    uint8_t* m_memory = nullptr;
};

// The MI355X counterpart of the ID3D11Device* the reference's GPU overloads take.
class Device
{
public:
    Device() noexcept = default;
    ~Device();
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    HRESULT Create(int hipDevice) noexcept;          // E_FAIL when no gfx950 device is visible
    // GPUCompressBC::Prepare's role (BCDirectCompute.h:28): size the encoder's scratch and staging for `count` images of this
    // shape now, so that the Compress calls that follow allocate nothing. Optional.
    HRESULT Prepare(size_t width, size_t height, DXGI_FORMAT srcFormat, DXGI_FORMAT bcFormat, TEX_COMPRESS_FLAGS flags, size_t count) noexcept;
    explicit operator bool() const noexcept { return m_ctx != nullptr; }
    dxtex_ctx* Get() const noexcept { return m_ctx; }
    const char* LastError() const noexcept;
    // Granularity of the progress / cancel callbacks of CompressEx / ConvertEx on ONE image: the image goes to the GPU as bands of
    // whole (block) rows of about this many blocks / texels, and the callback is asked between bands. 0 keeps the default
    // (2^18 blocks, 2^24 texels: large enough to fill the GPU). The bytes written never depend on it.
    void SetProgressBands(size_t compressBlocks, size_t convertTexels) noexcept { m_bandBlocks = compressBlocks; m_bandTexels = convertTexels; }
    size_t ProgressBandBlocks() const noexcept { return m_bandBlocks; }
    size_t ProgressBandTexels() const noexcept { return m_bandTexels; }
private:
    dxtex_ctx* m_ctx = nullptr;
    size_t m_bandBlocks = 0, m_bandTexels = 0;
};

// ---- the path's entry points (shapes of DirectXTex.h:799-846, :946-968, :1021) ----------------------------------------
HRESULT Compress(Device& device, const Image& srcImage, DXGI_FORMAT format, TEX_COMPRESS_FLAGS compress, float threshold, ScratchImage& cImage) noexcept;
HRESULT Compress(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, DXGI_FORMAT format,
                 TEX_COMPRESS_FLAGS compress, float threshold, ScratchImage& cImages) noexcept;
// CompressEx (DirectXTex.h:922-944). statusCallBack(done, total) -> false cancels: the result is released and E_ABORT
// returned. One image reports rows (the image goes to the GPU as bands of block rows, asked between bands); a set
// reports images. alphaWeight belongs to the reference's DirectCompute BC7 encoder and is not used here either way.
constexpr float TEX_ALPHA_WEIGHT_DEFAULT = 1.0f;
using StatusCallback = std::function<bool(size_t, size_t)>;
struct CompressOptions { TEX_COMPRESS_FLAGS flags; float threshold; float alphaWeight; };
HRESULT CompressEx(Device& device, const Image& srcImage, DXGI_FORMAT format, const CompressOptions& options, ScratchImage& cImage,
                   StatusCallback statusCallBack = nullptr);
HRESULT CompressEx(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, DXGI_FORMAT format,
                   const CompressOptions& options, ScratchImage& cImages, StatusCallback statusCallBack = nullptr);
// ONE image over several devices (normally one Device per GPU of the node): the image's block rows - for GenerateMipMaps the destination
// rows of its large levels, with the filter's halo of source rows - are dealt out over the devices, each stripe on a thread of its own
// (dxtex_compress_multi / dxtex_generate_mips_multi). The role of CompressBC_Parallel's split over OpenMP threads
// (DirectXTexCompress.cpp:257-281); the result is byte for byte that of the single-device overload.
HRESULT Compress(Device* const* devices, size_t ndevices, const Image& srcImage, DXGI_FORMAT format, TEX_COMPRESS_FLAGS compress, float threshold,
                 ScratchImage& cImage) noexcept;
HRESULT GenerateMipMaps(Device* const* devices, size_t ndevices, const Image& baseImage, TEX_FILTER_FLAGS filter, size_t levels, ScratchImage& mipChain) noexcept;
// format == DXGI_FORMAT_UNKNOWN picks the default target (DefaultDecompress, DirectXTexCompress.cpp:377-421)
HRESULT Decompress(Device& device, const Image& cImage, DXGI_FORMAT format, ScratchImage& image) noexcept;
HRESULT Decompress(Device& device, const Image* cImages, size_t nimages, const TexMetadata& metadata, DXGI_FORMAT format, ScratchImage& images) noexcept;
// levels == 0 generates the full chain
HRESULT GenerateMipMaps(Device& device, const Image& baseImage, TEX_FILTER_FLAGS filter, size_t levels, ScratchImage& mipChain) noexcept;
HRESULT GenerateMipMaps(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, TEX_FILTER_FLAGS filter,
                        size_t levels, ScratchImage& mipChain) noexcept;
// volume textures (DirectXTex.h:853-858): the base slices are `depth` images of one size
HRESULT GenerateMipMaps3D(Device& device, const Image* baseImages, size_t depth, TEX_FILTER_FLAGS filter, size_t levels, ScratchImage& mipChain) noexcept;
HRESULT GenerateMipMaps3D(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, TEX_FILTER_FLAGS filter, size_t levels,
                          ScratchImage& mipChain) noexcept;
HRESULT Resize(Device& device, const Image& srcImage, size_t width, size_t height, TEX_FILTER_FLAGS filter, ScratchImage& image) noexcept;
HRESULT Resize(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, size_t width, size_t height,
               TEX_FILTER_FLAGS filter, ScratchImage& result) noexcept;
HRESULT Convert(Device& device, const Image& srcImage, DXGI_FORMAT format, TEX_FILTER_FLAGS filter, float threshold, ScratchImage& image) noexcept;
HRESULT Convert(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, DXGI_FORMAT format,
                TEX_FILTER_FLAGS filter, float threshold, ScratchImage& result) noexcept;
// ConvertEx (DirectXTex.h:812-832), callback as for CompressEx
struct ConvertOptions { TEX_FILTER_FLAGS filter; float threshold; };
HRESULT ConvertEx(Device& device, const Image& srcImage, DXGI_FORMAT format, const ConvertOptions& options, ScratchImage& image,
                  StatusCallback statusCallBack = nullptr);
HRESULT ConvertEx(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, DXGI_FORMAT format,
                  const ConvertOptions& options, ScratchImage& result, StatusCallback statusCallBack = nullptr);
// mse = sum of the per-channel values, mseV[4] the per-channel MSE over [0,1] floats
// PremultiplyAlpha (DirectXTex.h:864-884). TEX_PMALPHA_FLAGS values as in the reference.
enum TEX_PMALPHA_FLAGS : uint32_t
{
    TEX_PMALPHA_DEFAULT = 0, TEX_PMALPHA_IGNORE_SRGB = 0x1, TEX_PMALPHA_REVERSE = 0x2,
    TEX_PMALPHA_SRGB_IN = 0x1000000, TEX_PMALPHA_SRGB_OUT = 0x2000000, TEX_PMALPHA_SRGB = 0x3000000,
};
HRESULT PremultiplyAlpha(Device& device, const Image& srcImage, TEX_PMALPHA_FLAGS flags, ScratchImage& image) noexcept;
HRESULT PremultiplyAlpha(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, TEX_PMALPHA_FLAGS flags, ScratchImage& result) noexcept;
// ComputeNormalMap (DirectXTex.h:973-1002). CNMAP_FLAGS values as in the reference; the channel is flags & 0xf (0 = red). The array form
// treats every image (mip level, array item, volume slice) as an independent 2-D height map. On failure the output is released.
enum CNMAP_FLAGS : uint32_t
{
    CNMAP_DEFAULT = 0, CNMAP_CHANNEL_RED = 0x1, CNMAP_CHANNEL_GREEN = 0x2, CNMAP_CHANNEL_BLUE = 0x3, CNMAP_CHANNEL_ALPHA = 0x4,
    CNMAP_CHANNEL_LUMINANCE = 0x5, CNMAP_MIRROR_U = 0x1000, CNMAP_MIRROR_V = 0x2000, CNMAP_MIRROR = 0x3000, CNMAP_INVERT_SIGN = 0x4000,
    CNMAP_COMPUTE_OCCLUSION = 0x8000,
};
inline CNMAP_FLAGS operator|(CNMAP_FLAGS a, CNMAP_FLAGS b) noexcept { return CNMAP_FLAGS(uint32_t(a) | uint32_t(b)); }
HRESULT ComputeNormalMap(Device& device, const Image& srcImage, CNMAP_FLAGS flags, float amplitude, DXGI_FORMAT format, ScratchImage& normalMap) noexcept;
HRESULT ComputeNormalMap(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, CNMAP_FLAGS flags, float amplitude,
                         DXGI_FORMAT format, ScratchImage& normalMaps) noexcept;
// TransformImage (DirectXTex.h:918-929) with one of texconv's per-texel lambdas as a descriptor, since a std::function cannot run on the
// GPU: TexTransform mirrors dxtex_transform (include/dxtex_amd.h, which states each op). ParseSwizzleMask is texconv's
// (texconv.cpp:1157-1248, plus its 1-4 character rule): it fills a SWIZZLE descriptor and returns false for a bad mask. The array form
// uploads the set once, transforms it on the device (TONEMAP takes its maximum over every image passed) and downloads it once. The result
// has the source's metadata; on failure it is released.
enum TEX_TRANSFORM_OP : uint32_t
{
    TEX_TRANSFORM_SWIZZLE = 0, TEX_TRANSFORM_TONEMAP = 1, TEX_TRANSFORM_COLOR_KEY = 2, TEX_TRANSFORM_INVERT_Y = 3, TEX_TRANSFORM_RECONSTRUCT_Z = 4,
};
struct TexTransform
{
    TEX_TRANSFORM_OP op = TEX_TRANSFORM_SWIZZLE;
    uint32_t swizzle[4] = { 0, 1, 2, 3 };      // SWIZZLE: source channel of each output channel
    uint32_t zero[4] = {};                     // SWIZZLE: non-zero = the output channel is 0
    uint32_t one[4] = {};                      // SWIZZLE: non-zero = the output channel is 1
    uint32_t colorKey = 0;                     // COLOR_KEY: 0x00RRGGBB
};
bool ParseSwizzleMask(const char* mask, TexTransform& transform) noexcept;
bool IsIdentitySwizzle(const TexTransform& transform) noexcept;       // texconv.cpp:2646-2648: the swizzle step does not run
HRESULT TransformImage(Device& device, const Image& srcImage, const TexTransform& transform, ScratchImage& result) noexcept;
HRESULT TransformImage(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, const TexTransform& transform,
                       ScratchImage& result) noexcept;
// texconv's HDR colour rotation (Texconv/texconv.cpp:2696-2964), the TransformImage lambdas it runs for -rotatecolor: r, g and b move
// between the Rec.709, Rec.2020 and Display-P3 (D65) primaries, and into or out of HDR10 (Rec.2020 with the SMPTE ST.2084 curve;
// paperWhiteNits, in (0, 10000], is the level of linear 1.0 and is read by the three HDR10 operations only). The values are texconv's
// ROTATE_* (texconv.cpp:181-188). Checks and HRESULTs are TransformImage's, with E_INVALIDARG for a bad operation or paper-white level.
// texconv converts to R16G16B16A16_FLOAT before HDR10_TO_709 and P3D65_TO_709 (:2699-2733): that step is the caller's (Convert). The
// array form uploads the set once, rotates it on the device and downloads it once. The result has the source's metadata; on failure it
// is released.
enum TEX_ROTATE_COLOR : uint32_t
{
    TEX_ROTATE_709_TO_HDR10 = 1, TEX_ROTATE_HDR10_TO_709 = 2, TEX_ROTATE_709_TO_2020 = 3, TEX_ROTATE_2020_TO_709 = 4,
    TEX_ROTATE_P3D65_TO_HDR10 = 5, TEX_ROTATE_P3D65_TO_2020 = 6, TEX_ROTATE_709_TO_P3D65 = 7, TEX_ROTATE_P3D65_TO_709 = 8,
};
HRESULT RotateColor(Device& device, const Image& srcImage, TEX_ROTATE_COLOR rotate, float paperWhiteNits, ScratchImage& result) noexcept;
HRESULT RotateColor(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, TEX_ROTATE_COLOR rotate, float paperWhiteNits,
                    ScratchImage& result) noexcept;
// FlipRotate (DirectXTex.h:723-737, DirectXTexFlipRotate.cpp:185-381) with the device in front. The flags are the reference's values; the
// result is the source turned CLOCKWISE by the angle, then mirrored left-right if FLIP_HORIZONTAL is set, then mirrored top-bottom if
// FLIP_VERTICAL is set (include/dxtex_amd.h states the rule per texel; DirectXTexAMD_FlipRotate.cpp is the one place that reads it).
// STATED DEPARTURES: the reference hands the flag word to WIC, whose documentation does not say whether a flip combined with a rotation
// is applied before or after it, and its tools never combine them - the order above is this project's and nothing can check it. Texels
// move as bytes: where the reference sends a format WIC lacks through float and back (not the identity for R32_UINT above 2^24), bits
// are kept here; the two-texel packed formats, which the reference would convert, are refused with the compressed ones
// (HRESULT_E_NOT_SUPPORTED), as are planar, palettised and typeless formats and R1_UNORM.
// Checks and their order are the reference's (:191-203, :290-297, :335-381). The metadata are the source's with width and height
// exchanged for 90 / 270: mip levels, array size, depth, dimension, the cube flag and the alpha mode are kept, and whatever Initialize
// refuses is refused. Every item, mip and depth slice goes into ONE batched call. On failure the result is released.
enum TEX_FR_FLAGS : uint32_t
{
    TEX_FR_ROTATE0 = 0x0, TEX_FR_ROTATE90 = 0x1, TEX_FR_ROTATE180 = 0x2, TEX_FR_ROTATE270 = 0x3, TEX_FR_FLIP_HORIZONTAL = 0x08, TEX_FR_FLIP_VERTICAL = 0x10,
};
inline TEX_FR_FLAGS operator|(TEX_FR_FLAGS a, TEX_FR_FLAGS b) noexcept { return TEX_FR_FLAGS(uint32_t(a) | uint32_t(b)); }
HRESULT FlipRotate(Device& device, const Image& srcImage, TEX_FR_FLAGS flags, ScratchImage& image) noexcept;
HRESULT FlipRotate(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, TEX_FR_FLAGS flags, ScratchImage& result) noexcept;
// ScaleMipMapsAlphaForCoverage (DirectXTex.h:848-851): mipChain must already be initialised with the chain's layout
HRESULT ScaleMipMapsAlphaForCoverage(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, size_t item,
                                     float alphaReference, ScratchImage& mipChain) noexcept;

HRESULT ComputeMSE(Device& device, const Image& image1, const Image& image2, float& mse, float* mseV) noexcept;

// ---- texdiag's diagnostics (Texdiag/texdiag.cpp: analyze, compare, diff) on the device (DirectXTexAMD_Diag.cpp) ------------------------
// Every input goes up once; compressed inputs are decompressed there to R32G32B32A32_FLOAT, as the reference's wrappers do
// (DirectXTexMisc.cpp:409-470, :489-501); only the figures - or Difference's map - come back.
enum CMSE_FLAGS : uint32_t
{
    CMSE_DEFAULT = 0, CMSE_IMAGE1_SRGB = 0x1, CMSE_IMAGE2_SRGB = 0x2, CMSE_IGNORE_RED = 0x10, CMSE_IGNORE_GREEN = 0x20, CMSE_IGNORE_BLUE = 0x40,
    CMSE_IGNORE_ALPHA = 0x80, CMSE_IMAGE1_X2_BIAS = 0x100, CMSE_IMAGE2_X2_BIAS = 0x200,
};
inline CMSE_FLAGS operator|(CMSE_FLAGS a, CMSE_FLAGS b) noexcept { return CMSE_FLAGS(uint32_t(a) | uint32_t(b)); }
// ComputeMSE with CMSE_FLAGS (DirectXTex.h:1041), accumulated in fp64; the five-argument form above keeps its behaviour
HRESULT ComputeMSE(Device& device, const Image& image1, const Image& image2, float& mse, float* mseV, CMSE_FLAGS flags) noexcept;
// texdiag's AnalyzeData (texdiag.cpp:668-696), per channel r, g, b, a; what each figure is: dxtex_image_stats in include/dxtex_amd.h
struct AnalyzeData
{
    float imageMin[4], imageMax[4];
    double imageAvg[4], imageVariance[4], imageStdDev[4];
    float luminance;
    uint64_t specials[4];
};
HRESULT Analyze(Device& device, const Image& image, AnalyzeData& result) noexcept;
// every image of a set (mips, items, slices) in one upload and one read-back: results[nimages]
HRESULT Analyze(Device& device, const Image* images, size_t nimages, const TexMetadata& metadata, AnalyzeData* results) noexcept;
// texdiag's AnalyzeBCData (:790-857): blockHist as dxtex_analyze_bc states it
struct AnalyzeBCData { uint64_t blocks; uint64_t blockHist[15]; };
HRESULT AnalyzeBC(Device& device, const Image& image, AnalyzeBCData& result) noexcept;
// Difference (texdiag.cpp:1229-1320): image 2 is converted to R32G32B32A32_FLOAT under dwFilter (so an _SRGB image 2 is linearised and
// image 1 is not, as there), the map is made in image 1's format (R32G32B32A32_FLOAT if it was compressed) and converted to `format`.
HRESULT Difference(Device& device, const Image& image1, const Image& image2, TEX_FILTER_FLAGS dwFilter, DXGI_FORMAT format, uint32_t diffColor,
                   float threshold, ScratchImage& result) noexcept;

// ---- the device-resident pipeline ---------------------------------------------------------------------------------------------------
// texconv runs resize -> convert -> mipmaps -> compress (Texconv/texconv.cpp:2609, 3109, 3434, 3711) as four ScratchImage -> ScratchImage calls;
// on a GPU that is four uploads and four downloads around a millisecond of kernels. The reference's own GPU path keeps its intermediate on
// the device (DirectXTexCompressGPU.cpp:34-140 converts on the way in, BCDirectCompute.cpp:373-642 reads the result back once). Here the
// whole chain can stay there: a DeviceScratchImage is a ScratchImage whose blob lives in HBM - same layout (item-major, then mips), same
// pitches, zero-filled - and every step below takes one and produces one with the SAME validation, error codes and kernels as the
// host-memory overload of the same name. Upload() is the chain's one host -> device copy, Download() its one device -> host copy.
class DeviceScratchImage
{
public:
    DeviceScratchImage() noexcept = default;
    DeviceScratchImage(DeviceScratchImage&& o) noexcept { *this = static_cast<DeviceScratchImage&&>(o); }
    DeviceScratchImage& operator=(DeviceScratchImage&& o) noexcept;
    DeviceScratchImage(const DeviceScratchImage&) = delete;
    DeviceScratchImage& operator=(const DeviceScratchImage&) = delete;
    ~DeviceScratchImage() { Release(); }

    // allocates and zero-fills (stream-ordered) device memory laid out like ScratchImage::Initialize(mdata, flags); the Device must outlive the image
    HRESULT Initialize(Device& device, const TexMetadata& mdata, CP_FLAGS flags = CP_FLAGS_NONE) noexcept;
    // Initialize + ONE host -> device copy of the source's blob (same layout on both sides)
    HRESULT Upload(Device& device, const ScratchImage& src) noexcept;
    // caller images of any pitch (nimages must match the metadata's image count): one copy per image when the pitches agree, else per row
    HRESULT Upload(Device& device, const Image* images, size_t nimages, const TexMetadata& metadata) noexcept;
    // dst.Initialize(metadata) + ONE device -> host copy; returns after the copy
    HRESULT Download(ScratchImage& dst) const noexcept;
    bool OverrideFormat(DXGI_FORMAT f) noexcept;
    void Release() noexcept;

    const TexMetadata& GetMetadata() const noexcept { return m_metadata; }
    // Image views whose `pixels` are DEVICE pointers: valid arguments for the *_device entry points of the C ABI, not for host code
    const Image* GetImage(size_t mip, size_t item, size_t slice) const noexcept;
    const Image* GetImages() const noexcept { return m_images.get(); }
    size_t GetImageCount() const noexcept { return m_nimages; }
    uint8_t* GetPixels() const noexcept { return m_memory; }
    size_t GetPixelsSize() const noexcept { return m_size; }
    Device* GetDevice() const noexcept { return m_device; }

private:
    Device* m_device = nullptr;
    size_t m_nimages = 0, m_size = 0;
    TexMetadata m_metadata;
    std::unique_ptr<Image[]> m_images;
    uint8_t* m_memory = nullptr;
};

// The images ScratchImage::Initialize(mdata, flags) would make, without their memory: `pixels` of each holds its byte offset into the blob
// of pixelBytes bytes. Same argument checks and HRESULTs; allocates the array only.
HRESULT LayoutScratchImage(const TexMetadata& mdata, CP_FLAGS flags, std::unique_ptr<Image[]>& images, size_t& nimages, size_t& pixelBytes, size_t& mipLevels) noexcept;

// The steps, resident: same argument meaning and HRESULTs as the (Image*, nimages, metadata) overloads above; all work is queued on the
// Device's stream and the result may be handed to the next step at once. `src` and the result must belong to `device`.
HRESULT Compress(Device& device, const DeviceScratchImage& src, DXGI_FORMAT format, TEX_COMPRESS_FLAGS compress, float threshold, DeviceScratchImage& cImages) noexcept;
HRESULT Decompress(Device& device, const DeviceScratchImage& cImages, DXGI_FORMAT format, DeviceScratchImage& images) noexcept;
HRESULT GenerateMipMaps(Device& device, const DeviceScratchImage& src, TEX_FILTER_FLAGS filter, size_t levels, DeviceScratchImage& mipChain) noexcept;
HRESULT GenerateMipMaps3D(Device& device, const DeviceScratchImage& src, TEX_FILTER_FLAGS filter, size_t levels, DeviceScratchImage& mipChain) noexcept;
HRESULT Resize(Device& device, const DeviceScratchImage& src, size_t width, size_t height, TEX_FILTER_FLAGS filter, DeviceScratchImage& result) noexcept;
HRESULT Convert(Device& device, const DeviceScratchImage& src, DXGI_FORMAT format, TEX_FILTER_FLAGS filter, float threshold, DeviceScratchImage& result) noexcept;
HRESULT PremultiplyAlpha(Device& device, const DeviceScratchImage& src, TEX_PMALPHA_FLAGS flags, DeviceScratchImage& result) noexcept;
HRESULT ComputeNormalMap(Device& device, const DeviceScratchImage& src, CNMAP_FLAGS flags, float amplitude, DXGI_FORMAT format, DeviceScratchImage& normalMaps) noexcept;
HRESULT TransformImage(Device& device, const DeviceScratchImage& src, const TexTransform& transform, DeviceScratchImage& result) noexcept;
HRESULT RotateColor(Device& device, const DeviceScratchImage& src, TEX_ROTATE_COLOR rotate, float paperWhiteNits, DeviceScratchImage& result) noexcept;
// resident: ONE batched call on the Device's stream, no byte crosses PCIe
HRESULT FlipRotate(Device& device, const DeviceScratchImage& src, TEX_FR_FLAGS flags, DeviceScratchImage& result) noexcept;
// the diagnostics on resident images: image 0 of each side for ComputeMSE and Difference, every image (results[GetImageCount()]) for Analyze / AnalyzeBC
HRESULT ComputeMSE(Device& device, const DeviceScratchImage& image1, const DeviceScratchImage& image2, float& mse, float* mseV, CMSE_FLAGS flags) noexcept;
// image index1 of one texture against image index2 of the other (GetImages() order). A compressed texture is decompressed whole on every call:
// a caller with many pairs hands over Decompress's result instead.
HRESULT ComputeMSE(Device& device, const DeviceScratchImage& image1, size_t index1, const DeviceScratchImage& image2, size_t index2, float& mse, float* mseV,
                   CMSE_FLAGS flags) noexcept;
HRESULT Analyze(Device& device, const DeviceScratchImage& images, AnalyzeData* results) noexcept;
HRESULT AnalyzeBC(Device& device, const DeviceScratchImage& images, AnalyzeBCData* results) noexcept;
HRESULT Difference(Device& device, const DeviceScratchImage& image1, const DeviceScratchImage& image2, TEX_FILTER_FLAGS dwFilter, DXGI_FORMAT format,
                   uint32_t diffColor, float threshold, DeviceScratchImage& result) noexcept;
// every array item of a mip chain (the per-item loop texconv runs, texconv.cpp:3470-3490); the 10-step bisection per level reads 8 bytes back per step
HRESULT ScaleMipMapsAlphaForCoverage(Device& device, const DeviceScratchImage& src, float alphaReference, DeviceScratchImage& mipChain) noexcept;
// level 0 of every array item / depth slice as a texture with one mip level (what texconv keeps before it regenerates a chain, texconv.cpp:3324-3380)
HRESULT CopyTopLevels(Device& device, const DeviceScratchImage& src, DeviceScratchImage& result) noexcept;
// ScratchImage::IsAlphaAllOpaque (DirectXTexImage.cpp:800-852) as a device reduction; false on any failure, like the reference. The Image form takes
// device-resident images of one format (e.g. the top levels of a chain).
bool IsAlphaAllOpaque(Device& device, const DeviceScratchImage& image) noexcept;
bool IsAlphaAllOpaque(Device& device, const Image* deviceImages, size_t nimages) noexcept;
// ---- ConvertToSinglePlane (DirectXTexAMD_Plane.cpp) --------------------------------------------------------------------------------------
// ConvertToSinglePlane (DirectXTex.h:826-831, DirectXTexConvert.cpp:5411-5523) with the device in front: NV12 / NV11 -> YUY2, P010 -> Y210,
// P016 -> Y216, the reference's validation, end guard and release-on-failure (see dxtex_convert_to_single_plane in dxtex_amd.h). The
// planar formats stay outside IsSupportedOnDevice(): this is the one device entry point that takes them. A ScratchImage or
// DeviceScratchImage holds a planar texture as the reference lays it out (ComputePitch's pitches, one blob).
HRESULT ConvertToSinglePlane(Device& device, const Image& srcImage, ScratchImage& image) noexcept;
// array items x mips: every source goes up as the caller describes it, ONE batched submission, one download
HRESULT ConvertToSinglePlane(Device& device, const Image* srcImages, size_t nimages, const TexMetadata& metadata, ScratchImage& result) noexcept;
// resident: ONE batched submission on the Device's stream; the result can be handed to Convert, Resize, ... at once
HRESULT ConvertToSinglePlane(Device& device, const DeviceScratchImage& src, DeviceScratchImage& result) noexcept;
// ---- CopyRectangle and texassemble's steps (DirectXTexAMD_Assemble.cpp) -----------------------------------------------------------------
struct Rect
{
    size_t x = 0, y = 0, w = 0, h = 0;
    Rect() = default;
    Rect(size_t _x, size_t _y, size_t _w, size_t _h) noexcept : x(_x), y(_y), w(_w), h(_h) {}
};
// CopyRectangle (DirectXTex.h:1018-1020, DirectXTexMisc.cpp:275-381) with the device in front: host images, only the rectangle's rows travel
HRESULT CopyRectangle(Device& device, const Image& srcImage, const Rect& srcRect, const Image& dstImage, TEX_FILTER_FLAGS filter, size_t xOffset, size_t yOffset) noexcept;
// the same between images resident on the device (src and dst must differ or not overlap): queued on the Device's stream
HRESULT CopyRectangle(Device& device, const DeviceScratchImage& src, size_t srcMip, size_t srcItem, size_t srcSlice, const Rect& srcRect,
                      const DeviceScratchImage& dst, size_t dstMip, size_t dstItem, size_t dstSlice, TEX_FILTER_FLAGS filter, size_t xOffset, size_t yOffset) noexcept;
// texassemble's merge (Texassemble/texassemble.cpp:2236-2268): image 2 is converted to R32G32B32A32_FLOAT under `filter`, channel k of the
// result is channel permute[k] of image 1 (0..3) or of image 2 (4..7), then 0 where zero[k], then 1 where one[k]; the result has image 1's format
HRESULT MergeImages(Device& device, const Image& image1, const Image& image2, TEX_FILTER_FLAGS filter, const uint32_t permute[4], const bool zero[4],
                    const bool one[4], ScratchImage& result) noexcept;

// Where texassemble puts the six cube faces (+X -X +Y -Y +Z -Z) in a cross, tee or strip (texassemble.cpp:2040-2181): a grid of
// cols x rows faces and each face's cell. The tables are data: tests/golden/assemble_layouts.json holds the same numbers.
enum CROSS_KIND : uint32_t { CROSS_H_CROSS = 0, CROSS_V_CROSS, CROSS_H_TEE, CROSS_H_STRIP, CROSS_V_STRIP, CROSS_KIND_COUNT };
struct CrossLayout { const char* name; size_t cols, rows; size_t x[6], y[6]; };
const CrossLayout* GetCrossLayout(CROSS_KIND kind) noexcept;
// The assemble steps on resident images; every one is ONE copy_rect launch per 32 rectangles. Mip 0 only, as in texassemble.
// faces: at least six array items of one size -> a cols * w x rows * h image of their format, background zero
HRESULT AssembleCross(Device& device, CROSS_KIND kind, const DeviceScratchImage& faces, DeviceScratchImage& result) noexcept;
// the reverse (cube-from-hc ...): an image whose size is a whole number of cells -> a cubemap of six faces
HRESULT CubeFromCross(Device& device, CROSS_KIND kind, const DeviceScratchImage& image, DeviceScratchImage& cube) noexcept;
// The cross with a turned -Z face: what texassemble's v-cross-fnz and cube-from-vc-fnz do with TEX_FR_ROTATE180
// (texassemble.cpp:2134-2151, :2469-2487, :2532-2540). The five other faces stay the one copy_rect launch they are; the -Z face is one
// FlipRotate written straight into - or read straight out of - its cell of the cross through an image view on it: no temporary image, no
// second copy. negZ must be legal and must not exchange the face's width and height (E_INVALIDARG).
HRESULT AssembleCross(Device& device, CROSS_KIND kind, const DeviceScratchImage& faces, TEX_FR_FLAGS negZ, DeviceScratchImage& result) noexcept;
HRESULT CubeFromCross(Device& device, CROSS_KIND kind, const DeviceScratchImage& image, TEX_FR_FLAGS negZ, DeviceScratchImage& cube) noexcept;
// array-strip: the array items of `items` stacked top to bottom in one image
HRESULT AssembleStrip(Device& device, const DeviceScratchImage& items, DeviceScratchImage& result) noexcept;
// whole images, pairwise, between device-resident images (src[i] into dst[i] at (0, 0); sizes of a pair must agree, formats may differ)
HRESULT CopyImages(Device& device, const Image* srcDeviceImages, const Image* dstDeviceImages, size_t count, TEX_FILTER_FLAGS filter = TEX_FILTER_DEFAULT) noexcept;
// cube / array / cubearray: `count` device-resident images of one size and format as the items of one array (asCube: a cubemap, count a
// multiple of six); volume: as the slices of one volume
HRESULT StackArray(Device& device, const Image* deviceImages, size_t count, bool asCube, DeviceScratchImage& result) noexcept;
HRESULT StackVolume(Device& device, const Image* deviceImages, size_t count, DeviceScratchImage& result) noexcept;
// merge on resident images (image 0 of each side); image 2 is converted on the device
HRESULT MergeImages(Device& device, const DeviceScratchImage& image1, const DeviceScratchImage& image2, TEX_FILTER_FLAGS filter, const uint32_t permute[4],
                    const uint32_t zero[4], const uint32_t one[4], DeviceScratchImage& result) noexcept;
// texassemble's ParseSwizzleMask (texassemble.cpp:662-790): 1 to 4 of rgbaxyzw (image 1), RGBAXYZW (image 2), 0, 1; the last repeats
bool ParseMergeMask(const char* mask, uint32_t permute[4], uint32_t zero[4], uint32_t one[4]) noexcept;

// bytes moved between host and device for this Device since the last reset (see dxtex_ctx_transfer_bytes)
void GetTransferBytes(Device& device, uint64_t& hostToDevice, uint64_t& deviceToHost, bool reset = false) noexcept;
} // namespace DirectXTexAMD

// ---- DDS container: the on-disk format either side of the path ---------------------------------
// DirectXTexDDS.cpp's reader and writer: textures, arrays, cubemaps and volumes of every DXGI format; the whole legacy
// (Direct3D 9) pixel-format table incl. the expanding / swizzling conversions (24 bpp RGB, 3:3:2, palettes, luminance,
// bump-map formats, the D3DX 10:10:10:2 reversal), every DDS_FLAGS reader and writer option. File names are UTF-8.
namespace DirectXTexAMD
{
enum DDS_FLAGS : uint32_t
{
    DDS_FLAGS_NONE = 0x0,
    DDS_FLAGS_LEGACY_DWORD = 0x1,                // rows of a legacy file are DWORD aligned
    DDS_FLAGS_NO_LEGACY_EXPANSION = 0x2,         // fail instead of expanding a legacy format
    DDS_FLAGS_NO_R10B10G10A2_FIXUP = 0x4,        // trust the 10:10:10:2 masks instead of assuming D3DX's reversed ones
    DDS_FLAGS_FORCE_RGB = 0x8,                   // BGRA / BGRX -> RGBA
    DDS_FLAGS_NO_16BPP = 0x10,                   // 5:6:5, 5:5:5:1, 4:4:4:4 -> RGBA8
    DDS_FLAGS_EXPAND_LUMINANCE = 0x20,           // L8, A8L8, L16 -> RGBA (replicated) instead of R / RG
    DDS_FLAGS_BAD_DXTN_TAILS = 0x40,             // mips smaller than a block were not written properly
    DDS_FLAGS_PERMISSIVE = 0x80,                 // accept known header variants
    DDS_FLAGS_IGNORE_MIPS = 0x100,               // top level only (non-array files)
    DDS_FLAGS_FORCE_DX10_EXT = 0x10000, DDS_FLAGS_FORCE_DX10_EXT_MISC2 = 0x20000, DDS_FLAGS_FORCE_DX9_LEGACY = 0x40000,
    DDS_FLAGS_FORCE_DXT5_RXGB = 0x80000, DDS_FLAGS_FORCE_24BPP_RGB = 0x100000,
    DDS_FLAGS_ALLOW_LARGE_FILES = 0x1000000,
};
constexpr HRESULT HRESULT_E_INVALID_DATA = HRESULT(0x8007000D), HRESULT_E_HANDLE_EOF = HRESULT(0x80070026),
                  HRESULT_E_CANNOT_MAKE = HRESULT(0x80070052), HRESULT_E_FILE_TOO_LARGE = HRESULT(0x800700DF);

// the file's DDS_PIXELFORMAT as read (DirectXTex.h:297-307)
struct DDSMetaData { uint32_t size, flags, fourCC, RGBBitCount, RBitMask, GBitMask, BBitMask, ABitMask; };

class Blob
{
public:
    Blob() noexcept = default;
    ~Blob() { Release(); }
    Blob(const Blob&) = delete;
    Blob& operator=(const Blob&) = delete;
    HRESULT Initialize(size_t size) noexcept;
    HRESULT Trim(size_t size) noexcept;              // shortens the logical size, keeps the allocation
    void Release() noexcept;
    void Swap(Blob& o) noexcept { uint8_t* b = m_buffer; m_buffer = o.m_buffer; o.m_buffer = b; const size_t n = m_size; m_size = o.m_size; o.m_size = n; }
    uint8_t* GetBufferPointer() const noexcept { return m_buffer; }
    size_t GetBufferSize() const noexcept { return m_size; }
private:
    uint8_t* m_buffer = nullptr;
    size_t m_size = 0;
};

HRESULT GetMetadataFromDDSMemory(const void* pSource, size_t size, DDS_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT GetMetadataFromDDSMemoryEx(const void* pSource, size_t size, DDS_FLAGS flags, TexMetadata& metadata, DDSMetaData* ddPixelFormat) noexcept;
HRESULT GetMetadataFromDDSFile(const char* szFile, DDS_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT GetMetadataFromDDSFileEx(const char* szFile, DDS_FLAGS flags, TexMetadata& metadata, DDSMetaData* ddPixelFormat) noexcept;
HRESULT LoadFromDDSMemory(const void* pSource, size_t size, DDS_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT LoadFromDDSMemoryEx(const void* pSource, size_t size, DDS_FLAGS flags, TexMetadata* metadata, DDSMetaData* ddPixelFormat, ScratchImage& image) noexcept;
HRESULT LoadFromDDSFile(const char* szFile, DDS_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT LoadFromDDSFileEx(const char* szFile, DDS_FLAGS flags, TexMetadata* metadata, DDSMetaData* ddPixelFormat, ScratchImage& image) noexcept;
// required = header bytes; pDestination may be null to query (DirectXTexDDS.cpp:711-1033)
HRESULT EncodeDDSHeader(const TexMetadata& metadata, DDS_FLAGS flags, uint8_t* pDestination, size_t maxsize, size_t& required) noexcept;
HRESULT SaveToDDSMemory(const Image& image, DDS_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToDDSMemory(const Image* images, size_t nimages, const TexMetadata& metadata, DDS_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToDDSFile(const Image& image, DDS_FLAGS flags, const char* szFile) noexcept;
HRESULT SaveToDDSFile(const Image* images, size_t nimages, const TexMetadata& metadata, DDS_FLAGS flags, const char* szFile) noexcept;

// The byte-serial half of the reader, no device needed: the header, every refusal (the E_FAIL of a row conversion that does not exist for
// the result format included), the permissive cube fix and the size checks. What is left is per texel: image i of the texture (ScratchImage
// order) is `op` applied to the rows that start images[i].offset bytes into the payload, images[i].rowPitch apart - the file's pitch rule,
// DDS_FLAGS_LEGACY_DWORD and DDS_FLAGS_BAD_DXTN_TAILS applied. On failure `raw` is released: no payload pointer is handed out.
struct DDSRawImage
{
    struct Source { size_t offset, rowPitch, slicePitch; };
    TexMetadata metadata;
    uint32_t op = 0;                             // DXTEX_DDS_ROW_* (include/dxtex_amd.h)
    bool opaque = false;                         // alpha is forced (CONV_FLAGS_NOALPHA)
    bool paletted = false;
    uint32_t palette[256] = {};
    const uint8_t* payload = nullptr;            // into the caller's memory; LoadFromDDSFileRaw: into `storage`
    size_t payloadBytes = 0;                     // what the images need of it: the sum of the file's slice pitches
    std::vector<Source> images;
    bool direct = false;                         // a plain copy and every file pitch is the image's: the payload IS the image memory
    Blob storage;
    void Release() noexcept;
};
HRESULT LoadFromDDSMemoryRaw(const void* pSource, size_t size, DDS_FLAGS flags, DDSMetaData* ddPixelFormat, DDSRawImage& raw) noexcept;
HRESULT LoadFromDDSFileRaw(const char* szFile, DDS_FLAGS flags, DDSMetaData* ddPixelFormat, DDSRawImage& raw) noexcept;
// Resident forms: the payload crosses PCIe at the size it has in the file and the per-texel half runs on the device (dxtex_dds_unpack_device
// / dxtex_dds_pack24_device). HRESULTs, metadata, pixels and files are those of the host forms above. Load: raw.direct is ONE host -> device
// copy straight into the image's memory and no kernel; anything else is one upload of raw.payloadBytes and the unpack launches. The result
// is released on failure. Save: deviceImages' pixels are device pointers, as DeviceScratchImage::GetImages gives; images whose pitches are
// the file's come down straight behind the header (one copy per run of contiguous images), DDS_FLAGS_FORCE_24BPP_RGB packs on the device
// and comes down at 3 bytes a texel, anything else in one strided copy per image.
HRESULT LoadFromDDSMemory(Device& device, const void* pSource, size_t size, DDS_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
HRESULT LoadFromDDSMemoryEx(Device& device, const void* pSource, size_t size, DDS_FLAGS flags, TexMetadata* metadata, DDSMetaData* ddPixelFormat, DeviceScratchImage& image) noexcept;
HRESULT LoadFromDDSFile(Device& device, const char* szFile, DDS_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
HRESULT LoadFromDDSFileEx(Device& device, const char* szFile, DDS_FLAGS flags, TexMetadata* metadata, DDSMetaData* ddPixelFormat, DeviceScratchImage& image) noexcept;
// the second half of the resident load, for a caller that parsed the file before it had a device
HRESULT UploadDDSRaw(Device& device, const DDSRawImage& raw, DeviceScratchImage& image) noexcept;
HRESULT SaveToDDSMemory(Device& device, const Image& deviceImage, DDS_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToDDSMemory(Device& device, const Image* deviceImages, size_t nimages, const TexMetadata& metadata, DDS_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToDDSFile(Device& device, const Image& deviceImage, DDS_FLAGS flags, const char* szFile) noexcept;
HRESULT SaveToDDSFile(Device& device, const Image* deviceImages, size_t nimages, const TexMetadata& metadata, DDS_FLAGS flags, const char* szFile) noexcept;

// ---- Radiance RGBE (.hdr), DirectXTexHDR.cpp: loads to R32G32B32A32_FLOAT; saves RGBA32F / RGB32F / RGBA16F images ---------------
HRESULT GetMetadataFromHDRMemory(const void* pSource, size_t size, TexMetadata& metadata) noexcept;
HRESULT GetMetadataFromHDRFile(const char* szFile, TexMetadata& metadata) noexcept;
HRESULT LoadFromHDRMemory(const void* pSource, size_t size, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT LoadFromHDRFile(const char* szFile, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT SaveToHDRMemory(const Image& image, Blob& blob) noexcept;
HRESULT SaveToHDRFile(const Image& image, const char* szFile) noexcept;
// The header and the run-length expansion only: tight width * 4-byte rows of shared-exponent texels, and the file's exposure. Needs no device.
HRESULT LoadFromHDRMemoryRGBE(const void* pSource, size_t size, TexMetadata* metadata, float& exposure, Blob& rgbe) noexcept;
HRESULT LoadFromHDRFileRGBE(const char* szFile, TexMetadata* metadata, float& exposure, Blob& rgbe) noexcept;
// Resident forms: the texels cross PCIe as RGBE, 4 bytes each, and the float pass runs on the device (dxtex_rgbe_decode_device /
// dxtex_rgbe_encode_device). HRESULTs, metadata, pixels and files are those of the host forms above. Load: one upload of width * height * 4
// bytes, the result is released on failure. Save: deviceImage's pixels are a device pointer, as DeviceScratchImage::GetImage gives; one
// download of width * height * 4 bytes. A channel of +Inf is saved as a zero texel (include/dxtex_amd.h, dxtex_rgbe_encode).
HRESULT LoadFromHDRMemory(Device& device, const void* pSource, size_t size, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
// the second half of the resident load, for a caller that parsed the file before it had a device (LoadFrom...RGBE gave all three arguments)
HRESULT UploadHDRRows(Device& device, const TexMetadata& metadata, float exposure, const Blob& rgbe, DeviceScratchImage& image) noexcept;
HRESULT LoadFromHDRFile(Device& device, const char* szFile, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
HRESULT SaveToHDRMemory(Device& device, const Image& deviceImage, Blob& blob) noexcept;
HRESULT SaveToHDRFile(Device& device, const Image& deviceImage, const char* szFile) noexcept;

// ---- Truevision TGA, DirectXTexTGA.cpp: 8-bit grey -> R8, 16-bit -> B5G5R5A1, 24-bit -> RGBA8 (opaque), 32-bit -> RGBA8, colour-mapped
// (24-bit palette) -> RGBA8; raw or run-length encoded; TGA 2.0 extension area for alpha mode and gamma ------------------------------
enum TGA_FLAGS : uint32_t
{
    TGA_FLAGS_NONE = 0x0,
    TGA_FLAGS_BGR = 0x1,                       // keep BGR order: 24-bit -> B8G8R8X8, 32-bit -> B8G8R8A8
    TGA_FLAGS_ALLOW_ALL_ZERO_ALPHA = 0x2,      // an alpha channel of all zeros is meant (default: treated as opaque)
    TGA_FLAGS_IGNORE_SRGB = 0x10, TGA_FLAGS_FORCE_SRGB = 0x20, TGA_FLAGS_FORCE_LINEAR = 0x40, TGA_FLAGS_DEFAULT_SRGB = 0x80,
};
HRESULT GetMetadataFromTGAMemory(const void* pSource, size_t size, TGA_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT GetMetadataFromTGAFile(const char* szFile, TGA_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT LoadFromTGAMemory(const void* pSource, size_t size, TGA_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT LoadFromTGAFile(const char* szFile, TGA_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
// saves RGBA8 / BGRA8 (32-bit), BGRX8 (24-bit), R8 / A8 (grey), B5G5R5A1 (16-bit); metadata adds the TGA 2.0 extension area
HRESULT SaveToTGAMemory(const Image& image, TGA_FLAGS flags, Blob& blob, const TexMetadata* metadata = nullptr) noexcept;
HRESULT SaveToTGAFile(const Image& image, TGA_FLAGS flags, const char* szFile, const TexMetadata* metadata = nullptr) noexcept;
// The reader's byte-serial half, which needs no device: header, palette, the extension area's alpha mode and gamma, the size check of a raw
// file, the run-length packets undone. What comes back is the file's texels in the file's order, bytesPerTexel bytes each, and how to read
// them; `metadata` is the loader's except for the alpha rule, which needs the texels (an opaque image gets TEX_ALPHA_MODE_OPAQUE).
struct TGARawImage
{
    const uint8_t* texels = nullptr;             // width * height * bytesPerTexel bytes: inside the caller's buffer (a raw file: no copy) or in `storage`
    size_t texelBytes = 0;
    uint32_t bytesPerTexel = 0;                  // 1 (grey, or a palette index), 2, 3 or 4
    DXGI_FORMAT format = DXGI_FORMAT_UNKNOWN;    // the image's, before gamma relabels it sRGB
    bool paletted = false, rightToLeft = false, topDown = false;
    uint32_t palette[256] = {};                  // colour-mapped files: the words an index stands for, zero outside the file's map
    Blob storage;                                // a run-length file's texels; LoadFromTGAFileRaw: the file itself where `texels` points into it
    void Release() noexcept;
};
HRESULT LoadFromTGAMemoryRaw(const void* pSource, size_t size, TGA_FLAGS flags, TexMetadata* metadata, TGARawImage& raw) noexcept;
HRESULT LoadFromTGAFileRaw(const char* szFile, TGA_FLAGS flags, TexMetadata* metadata, TGARawImage& raw) noexcept;
// Resident forms: the texels cross PCIe as the file has them, 1 to 4 bytes each, and the per-texel pass runs on the device
// (dxtex_tga_unpack_device / dxtex_tga_pack_device). HRESULTs, metadata, pixels and files are those of the host forms above. Load: one upload
// of width * height * bytesPerTexel bytes and, for 16- and 32-bit files, a 4-byte read-back of the alpha answer; the result is released on
// failure. Save: deviceImage's pixels are a device pointer, as DeviceScratchImage::GetImage gives; one download of the file's rows.
HRESULT LoadFromTGAMemory(Device& device, const void* pSource, size_t size, TGA_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
// the second half of the resident load, for a caller that parsed the file before it had a device (LoadFromTGA...Raw gave metadata and raw,
// with the same flags); applies the alpha rule to `metadata`
HRESULT UploadTGARaw(Device& device, TexMetadata& metadata, TGA_FLAGS flags, const TGARawImage& raw, DeviceScratchImage& image) noexcept;
// the alpha rule's answer from the raw texels, on the host: one OR over their alpha bytes, for a caller that has to state the metadata
// before it has a device (UploadTGARaw finds the same answer on the device, where it also sets the alphas that need it)
void ApplyTGAAlphaRule(const TGARawImage& raw, TGA_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT LoadFromTGAFile(Device& device, const char* szFile, TGA_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
HRESULT SaveToTGAMemory(Device& device, const Image& deviceImage, TGA_FLAGS flags, Blob& blob, const TexMetadata* metadata = nullptr) noexcept;
HRESULT SaveToTGAFile(Device& device, const Image& deviceImage, TGA_FLAGS flags, const char* szFile, const TexMetadata* metadata = nullptr) noexcept;

// ---- Portable pixmaps, Texconv/PortablePixMap.cpp: .ppm (P3 ASCII and P6 binary -> R8G8B8A8_UNORM), .pfm (PF -> R32G32B32A32_FLOAT, Pf ->
// R32_FLOAT) and .phm (PH -> R16G16B16A16_FLOAT, Ph -> R16_FLOAT), either byte order. One loader takes all of them and tells them apart by
// the second byte, as texconv does by extension. The reference has the File forms only; the Memory forms are this project's. -----------------
HRESULT GetMetadataFromPortablePixMapMemory(const void* pSource, size_t size, TexMetadata& metadata) noexcept;
HRESULT GetMetadataFromPortablePixMapFile(const char* szFile, TexMetadata& metadata) noexcept;
HRESULT LoadFromPortablePixMapMemory(const void* pSource, size_t size, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT LoadFromPortablePixMapFile(const char* szFile, TexMetadata* metadata, ScratchImage& image) noexcept;
// SaveToPortablePixMap: a P6 file from R8G8B8A8 / B8G8R8A8 / B8G8R8X8_UNORM[_SRGB]. SaveToPortablePixMapHDR: a little-endian PF file from
// R32G32B32A32_FLOAT, R32G32B32_FLOAT or R16G16B16A16_FLOAT, a Pf file from R32_FLOAT. PH and Ph are never written, as in the reference.
HRESULT SaveToPortablePixMapMemory(const Image& image, Blob& blob) noexcept;
HRESULT SaveToPortablePixMapFile(const Image& image, const char* szFile) noexcept;
HRESULT SaveToPortablePixMapHDRMemory(const Image& image, Blob& blob) noexcept;
HRESULT SaveToPortablePixMapHDRFile(const Image& image, const char* szFile) noexcept;
// The reader's byte-serial half, which needs no device: the text header and every refusal. What comes back is where the samples lie and how
// to read them (dxtex_pnm_unpack's arguments). A P3 file's ASCII samples are byte-serial throughout: they are decoded here into
// R8G8B8A8_UNORM words (`ascii`; the payload is then those words, in `storage`). On failure `raw` is released.
struct PNMRawImage
{
    uint32_t kind = 0;                           // DXTEX_PNM_* (include/dxtex_amd.h)
    uint32_t maxval = 255;                       // P6: 1..255
    bool bigEndian = false;                      // float kinds: the scale line was >= 0
    bool ascii = false;                          // a P3 file: the payload is the finished image, width * height words
    const uint8_t* payload = nullptr;            // into the caller's memory; P3, and LoadFromPortablePixMapFileRaw: into `storage`
    size_t payloadOffset = 0;                    // of the payload in the file (P3: 0)
    size_t payloadBytes = 0;                     // width * height * bytes of a file texel
    Blob storage;
    void Release() noexcept;
};
HRESULT LoadFromPortablePixMapMemoryRaw(const void* pSource, size_t size, TexMetadata* metadata, PNMRawImage& raw) noexcept;
HRESULT LoadFromPortablePixMapFileRaw(const char* szFile, TexMetadata* metadata, PNMRawImage& raw) noexcept;
// Resident forms: the samples cross PCIe as the file has them - 3 bytes a texel for P6, 12 for PF, 6 for PH, 4 and 2 for the grey kinds - and
// the per-texel pass runs on the device (dxtex_pnm_unpack_device / dxtex_pnm_pack_device). HRESULTs, metadata, pixels and files are those of
// the host forms above. Load: one upload of payloadBytes (a P3 file: of the decoded words, straight into the image); the result is released
// on failure. Save: deviceImage's pixels are a device pointer, as DeviceScratchImage::GetImage gives; one download of the file's rows,
// straight behind the header.
HRESULT LoadFromPortablePixMapMemory(Device& device, const void* pSource, size_t size, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
HRESULT LoadFromPortablePixMapFile(Device& device, const char* szFile, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
// the second half of the resident load, for a caller that parsed the file before it had a device
HRESULT UploadPortablePixMapRaw(Device& device, const TexMetadata& metadata, const PNMRawImage& raw, DeviceScratchImage& image) noexcept;
HRESULT SaveToPortablePixMapMemory(Device& device, const Image& deviceImage, Blob& blob) noexcept;
HRESULT SaveToPortablePixMapFile(Device& device, const Image& deviceImage, const char* szFile) noexcept;
HRESULT SaveToPortablePixMapHDRMemory(Device& device, const Image& deviceImage, Blob& blob) noexcept;
HRESULT SaveToPortablePixMapHDRFile(Device& device, const Image& deviceImage, const char* szFile) noexcept;

// ---- PNG, Auxiliary/DirectXTexPNG.cpp (the reference's libpng codec): non-interlaced files of every colour type and depth in, grey 8 / 16,
// RGB 8 and RGBA 8 / 16 out. No library is linked: chunks, CRC-32, inflate (stored, fixed and dynamic blocks, Adler-32) and the five row
// filters are this file's own code. Formats, flags and metadata follow the reference (Update, GuessFormat, GetHeader, WriteImage); a missing
// file is HRESULT_ERROR_FILE_NOT_FOUND, an interlaced one HRESULT_E_NOT_SUPPORTED, every other defect E_FAIL. Four departures:
//   1. No alpha association and no gamma correction. The reference's png_set_alpha_mode(PNG_ALPHA_STANDARD, PNG_GAMMA_LINEAR) and, for a
//      gAMA that is not 1, png_set_gamma(2.2, gamma) make libpng premultiply and re-encode samples, against its own comment ("keep RGB
//      untouched"). Here every sample is the file's sample, as a WIC-built texconv delivers it; premultiplying and colour space are
//      -pmalpha's and -srgb*'s.
//   2. A grey file with a tRNS chunk is HRESULT_E_NOT_SUPPORTED (the reference expands it to two channels in a four-channel image).
//   3. The writer emits the colour chunks its code asks for, in front of IDAT: gAMA 100000 under PNG_FLAGS_FORCE_LINEAR, else sRGB
//      (intent 0) for an _SRGB format or under PNG_FLAGS_FORCE_SRGB; neither for grey. The reference sets them after png_write_info, where
//      libpng most likely no longer writes them.
//   4. The Memory forms are this project's; the reference has the File forms only.
// The writer stores: filter 0 on every row and stored deflate blocks, as the reference's compression level 0 asks for. The file's bytes are
// this project's own; its texels are the image's. ---------------------------------------------------------------------------------------------
constexpr HRESULT HRESULT_ERROR_FILE_NOT_FOUND = HRESULT(0x80070002);
enum PNG_FLAGS : uint32_t
{
    PNG_FLAGS_NONE = 0,
    PNG_FLAGS_BGR = 0x1,                 // 24bpp files are returned as BGRX; 32bpp files as BGRA
    PNG_FLAGS_IGNORE_SRGB = 0x2,         // ignores the sRGB chunk and gAMA: the format is the linear one
    PNG_FLAGS_DEFAULT_LINEAR = 0x4,      // a file that names no colour space is linear
    PNG_FLAGS_FORCE_SRGB = 0x20,         // the writer emits sRGB whatever the format
    PNG_FLAGS_FORCE_LINEAR = 0x40,       // the writer emits gAMA 1.0 whatever the format
};
inline PNG_FLAGS operator|(PNG_FLAGS a, PNG_FLAGS b) noexcept { return PNG_FLAGS(uint32_t(a) | uint32_t(b)); }
HRESULT GetMetadataFromPNGMemory(const void* pSource, size_t size, PNG_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT GetMetadataFromPNGFile(const char* szFile, PNG_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT LoadFromPNGMemory(const void* pSource, size_t size, PNG_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT LoadFromPNGFile(const char* szFile, PNG_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT SaveToPNGMemory(const Image& image, PNG_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToPNGFile(const Image& image, PNG_FLAGS flags, const char* szFile) noexcept;
// The reader's byte-serial half, which needs no device: signature, chunks and their CRCs, inflate, the row filters, every refusal. What comes
// back is the unfiltered rows - height rows of ceil(width * bits / 8) bytes, tight, no filter byte - and how to read them (dxtex_png_unpack's
// arguments). GetMetadata* stop behind the last chunk in front of IDAT and inflate nothing. On failure `raw` is released.
struct PNGRawImage
{
    uint32_t kind = 0;                           // DXTEX_PNG_* (include/dxtex_amd.h)
    uint32_t flags = 0;                          // DXTEX_PNG_BGR where PNG_FLAGS_BGR changes this kind's format
    uint32_t palette[256] = {};                  // palette kinds: R | G << 8 | B << 16 | A << 24, A from tRNS or 255
    uint32_t paletteCount = 0;
    size_t rowBytes = 0;                         // ceil(width * bits / 8)
    const uint8_t* rows = nullptr;               // into `storage`
    size_t rowsBytes = 0;                        // height * rowBytes
    Blob storage;
    void Release() noexcept;
};
HRESULT LoadFromPNGMemoryRaw(const void* pSource, size_t size, PNG_FLAGS flags, TexMetadata* metadata, PNGRawImage& raw) noexcept;
HRESULT LoadFromPNGFileRaw(const char* szFile, PNG_FLAGS flags, TexMetadata* metadata, PNGRawImage& raw) noexcept;
// Resident forms: the unfiltered rows cross PCIe as the file has them - 3 bytes a texel for RGB 8, one bit for grey 1 - and the per-texel
// pass runs on the device (dxtex_png_unpack_device / dxtex_png_pack_device). HRESULTs, metadata, pixels and files are those of the host forms
// above. Load: one upload of rowsBytes; a grey 8 or RGBA 8 file without PNG_FLAGS_BGR whose rows match the image's pitch goes straight into
// the image and no kernel runs; the result is released on failure. Save: deviceImage's pixels are a device pointer, as
// DeviceScratchImage::GetImage gives; one download of the file's rows.
HRESULT LoadFromPNGMemory(Device& device, const void* pSource, size_t size, PNG_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
HRESULT LoadFromPNGFile(Device& device, const char* szFile, PNG_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
// the second half of the resident load, for a caller that parsed the file before it had a device
HRESULT UploadPNGRaw(Device& device, const TexMetadata& metadata, const PNGRawImage& raw, DeviceScratchImage& image) noexcept;
HRESULT SaveToPNGMemory(Device& device, const Image& deviceImage, PNG_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToPNGFile(Device& device, const Image& deviceImage, PNG_FLAGS flags, const char* szFile) noexcept;

// ---- JPEG, Auxiliary/DirectXTexJPEG.cpp (the reference's libjpeg codec): baseline, extended and progressive Huffman files of one or three
// 8-bit components in, the reference's baseline files out (below). No library is linked: the marker walk, the Huffman decoder and the four
// progressive passes are this project's own code and end in the file's quantised coefficients; dequantisation, the inverse DCT, chroma
// upsampling and YCbCr -> RGB are csrc/dxtex_jpeg.h's, which follow libjpeg's defaults (JDCT_ISLOW, fancy upsampling) as the reference leaves
// them. Formats and metadata follow TranslateColor / GetMetadata: grey is R8_UNORM; colour is R8G8B8A8_UNORM_SRGB, or R8G8B8A8_UNORM under
// JPEG_FLAGS_DEFAULT_LINEAR, alpha 0xff, TEX_ALPHA_MODE_OPAQUE; 2-D, one item, one mip. The colour kind follows libjpeg's
// default_decompress_parms: one component is grey; of three, a JFIF marker means YCbCr; without one, Adobe transform 0 is RGB and any other
// YCbCr; with neither marker, component ids 'R', 'G', 'B' mean RGB and anything else YCbCr. Four components (CMYK, YCCK) are E_FAIL, as the
// reference throws for them. Null arguments are E_INVALIDARG, a missing file HRESULT_ERROR_FILE_NOT_FOUND, every defect in the bytes E_FAIL.
// Four departures:
//   1. The Memory forms are this project's; the reference has the File forms only.
//   2. HRESULT_E_NOT_SUPPORTED for: arithmetic coding (SOF9 to SOF15); lossless and hierarchical frames (SOF3, SOF5 to SOF7); 12-bit
//      precision; a DNL-defined height (height 0 in SOF); sampling other than luma 1x1, 2x1 or 2x2 over 1x1 chroma (grey with any factors
//      is 1x1); a progressive file whose scans end without bringing every coefficient of every component to Al = 0, whose blocks libjpeg
//      would smooth.
//   3. A truncated or corrupt entropy segment is E_FAIL, where libjpeg pads with zeros and warns: data that end before the last MCU, a bad
//      code, a wrong RSTn, a run past coefficient 63 (or past the band of a progressive scan), a missing EOI.
//   4. EXIF orientation, thumbnails and ICC profiles are ignored, as libjpeg ignores them.
// Out of scope: arithmetic coding, 12-bit samples, sampling other than 4:4:4 / 4:2:2 / 4:2:0, incomplete progressive files; in the writer,
// any quality but 100, any sampling but 4:2:0, optimised Huffman tables, progressive and RGB-coded files. -------------------------------------------------------------------------------------------------------------------------
enum JPEG_FLAGS : uint32_t
{
    JPEG_FLAGS_NONE = 0,
    JPEG_FLAGS_DEFAULT_LINEAR = 0x1,     // a colour file is R8G8B8A8_UNORM, not R8G8B8A8_UNORM_SRGB
};
inline JPEG_FLAGS operator|(JPEG_FLAGS a, JPEG_FLAGS b) noexcept { return JPEG_FLAGS(uint32_t(a) | uint32_t(b)); }
HRESULT GetMetadataFromJPEGMemory(const void* pSource, size_t size, JPEG_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT GetMetadataFromJPEGFile(const char* szFile, JPEG_FLAGS flags, TexMetadata& metadata) noexcept;
// without a device: the per-block and per-texel functions of csrc/dxtex_jpeg.h run serially
HRESULT LoadFromJPEGMemory(const void* pSource, size_t size, JPEG_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT LoadFromJPEGFile(const char* szFile, JPEG_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
// The reader's byte-serial half, which needs no device: markers, tables, the Huffman walk of every scan, every refusal. What comes back is the
// frame and its quantised coefficients (dxtex_jpeg_decode's arguments): int16, 64 a block in natural (row-major) order, blocks in raster
// order per component, one component after another, each component padded to whole MCUs - ceil(width / (8 hmax)) * h by
// ceil(height / (8 vmax)) * v blocks. GetMetadata* stop at the first scan. On failure `raw` is released.
struct JPEGRawImage
{
    struct Component
    {
        uint32_t h = 0, v = 0;                   // sampling factors (grey: 1 x 1 whatever the file says)
        uint32_t quant = 0;                      // which of `quant`
        uint32_t blocksPerRow = 0, blockRows = 0;
        size_t offset = 0;                       // of its first coefficient, in coefficients
    };
    uint32_t width = 0, height = 0, components = 0;
    uint32_t colour = 0;                         // DXTEX_JPEG_GREY / _YCBCR / _RGB (include/dxtex_amd.h)
    Component component[3];
    uint16_t quant[4][64] = {};                  // natural order
    const int16_t* coefficients = nullptr;       // into `storage`
    size_t coefficientCount = 0;
    Blob storage;
    void Release() noexcept;
};
HRESULT LoadFromJPEGMemoryRaw(const void* pSource, size_t size, JPEG_FLAGS flags, TexMetadata* metadata, JPEGRawImage& raw) noexcept;
HRESULT LoadFromJPEGFileRaw(const char* szFile, JPEG_FLAGS flags, TexMetadata* metadata, JPEGRawImage& raw) noexcept;
// Resident forms: the coefficients cross PCIe as the file has them - 2 bytes a texel for grey, 3 for 4:2:0, 4 for 4:2:2, 6 for 4:4:4 - and the
// inverse DCT, upsampling and colour run on the device (dxtex_jpeg_decode_device). HRESULTs, metadata and pixels are those of the host forms.
// One upload of the coefficients, no download; the result is released on failure.
HRESULT LoadFromJPEGMemory(Device& device, const void* pSource, size_t size, JPEG_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
HRESULT LoadFromJPEGFile(Device& device, const char* szFile, JPEG_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
// the second half of the resident load, for a caller that parsed the file before it had a device
HRESULT UploadJPEGRaw(Device& device, const TexMetadata& metadata, const JPEGRawImage& raw, DeviceScratchImage& image) noexcept;
// The writer, JPEGCompress::WriteImage: what libjpeg writes after jpeg_set_defaults and jpeg_set_quality(100), byte for byte. R8_UNORM gives a
// grey file of one 1 x 1 component; R8G8B8A8_UNORM[_SRGB], B8G8R8A8_UNORM[_SRGB] and B8G8R8X8_UNORM[_SRGB] give YCbCr at 4:2:0 in one interleaved
// scan, alpha or X ignored; every other format is HRESULT_E_NOT_SUPPORTED. JFIF 1.01, quantiser tables of ones, the standard Huffman tables,
// no restart intervals. A null file name is E_INVALIDARG, an image above 65535 texels a side E_INVALIDARG. `flags` changes nothing: _SRGB
// formats give the bytes of their plain twins. The Memory forms are this project's addition. On failure the blob is empty.
HRESULT SaveToJPEGMemory(const Image& image, JPEG_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToJPEGFile(const Image& image, JPEG_FLAGS flags, const char* szFile) noexcept;
// The writer's byte-serial half, which needs no device: the markers, the tables and factors the components name (DQT entries of 8 bits where
// all are at most 255, else 16 bits and SOF1), then baseline Huffman coding with the standard tables in MCU order - luma with tables 0,
// chroma with tables 1. Grey and YCbCr frames laid out as LoadFromJPEGMemoryRaw returns them; DXTEX_JPEG_RGB is HRESULT_E_NOT_SUPPORTED, a
// frame whose block counts or offsets are not its own or a quantiser entry of 0 E_INVALIDARG. E_FAIL where a DC difference needs more than 11
// bits or an AC coefficient more than 10 (libjpeg's JERR_BAD_DCT_COEF), which no 8-bit image reaches.
HRESULT SaveJPEGRaw(const JPEGRawImage& raw, Blob& blob) noexcept;
// Resident forms: colour transform, downsampling, forward DCT and quantisation run on the device (dxtex_jpeg_encode_device) and the image
// comes down as its coefficients - 2 bytes a texel for grey, 3 for colour - in one download; nothing goes up. Bytes and HRESULTs are
// those of the host forms.
HRESULT SaveToJPEGMemory(Device& device, const Image& deviceImage, JPEG_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToJPEGFile(Device& device, const Image& deviceImage, JPEG_FLAGS flags, const char* szFile) noexcept;

// ---- OpenEXR, Auxiliary/DirectXTexEXR.cpp (the reference's codec over the OpenEXR library's RgbaInputFile / RgbaOutputFile): single-part
// scanline files of compression NONE, RLE, ZIPS and ZIP in, NONE out. No library is linked: the header walk, the offset table, the RLE
// packets and - through DirectXTexAMD_Inflate.h - inflate are this project's own code; what happens to a chunk's bytes after that is
// csrc/dxtex_exr.h's. Metadata follow LoadFromEXRCommon / GetMetadataFromEXR*: R16G16B16A16_FLOAT, 2-D, one mip, the image is the data
// window; with an `envmap` attribute and width == height / 6 the height becomes the width and there are six array items. Channels follow
// RgbaInputFile: absent R, G, B read 0 and absent A 1.0; a file with Y and none of R, G, B reads R = G = B = Y; channels of other names,
// layer-prefixed ones included, are skipped; FLOAT and UINT samples become halves by the library's floatToHalf / uintToHalf (csrc/dxtex_exr.h).
// Null arguments are E_INVALIDARG, a missing file HRESULT_ERROR_FILE_NOT_FOUND, and E_FAIL is: bad magic, truncation, a malformed header
// or channel list, a missing needed attribute (channels, compression, dataWindow, displayWindow, lineOrder, pixelAspectRatio,
// screenWindowCenter, screenWindowWidth), an empty or overflowing window, an offset of zero or outside the file, a chunk whose y is not
// its table slot's, an expansion that does not give exactly the plain size. Departures:
//   1. HRESULT_E_NOT_SUPPORTED where the library would go on: tiled, deep and multipart files; PIZ, PXR24, B44, B44A, DWAA and DWAB;
//      RY / BY chroma channels; a channel among R, G, B, A, Y that is used and whose sampling is not 1.
//   2. Chunks are read through the offset table alone, so the line order needs no handling and an incomplete table is not reconstructed.
//   3. The writer stores compression NONE, one scanline a chunk, where the reference writes ZIP through zlib; the texels are the same:
//      channels A, B, G, R, all HALF, increasing Y, data window = display window = 0, 0, w-1, h-1, the eight needed attributes in name
//      order. R16G16B16A16_FLOAT moves as bits; R32G32B32A32_FLOAT and R32G32B32_FLOAT (alpha 1.0) become halves by XMConvertFloatToHalf,
//      as the reference's XMStoreHalf4 does; every other format is HRESULT_E_NOT_SUPPORTED.
//   4. The preview image and every attribute beyond those named are ignored.
// Out of scope: PIZ and the lossy codecs, tiled, deep and multipart files, luminance-chroma files, a deflating writer. -------------------------
HRESULT GetMetadataFromEXRMemory(const void* pSource, size_t size, TexMetadata& metadata) noexcept;
HRESULT GetMetadataFromEXRFile(const char* szFile, TexMetadata& metadata) noexcept;
HRESULT LoadFromEXRMemory(const void* pSource, size_t size, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT LoadFromEXRFile(const char* szFile, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT SaveToEXRMemory(const Image& image, Blob& blob) noexcept;
HRESULT SaveToEXRFile(const Image& image, const char* szFile) noexcept;
// The reader's byte-serial half, which needs no device: the header walk, every refusal, the offset table, inflate and the RLE packets. What
// comes back is ONE STREAM of the chunks' expanded bytes, coded or plain (csrc/dxtex_exr.h), and dxtex_exr_unpack's other arguments: a
// descriptor per chunk - consecutive plain chunks that follow one another in the stream and in the window share one - and where R, G, B
// and A lie in a scanline. A coded chunk starts on a multiple of 16 bytes of the stream. GetMetadata* stop behind the header. On failure
// `raw` is released.
struct EXRRawImage
{
    struct Chunk { uint64_t offset; uint32_t bytes, firstRow, rows, coded; };          // dxtex_exr_chunk's layout
    struct Channel { uint32_t offset, type; };                                          // dxtex_exr_channel's; type DXTEX_EXR_*
    uint32_t compression = 0;                    // the file's code: 0 NONE, 1 RLE, 2 ZIPS, 3 ZIP
    uint32_t scanlineBytes = 0;                  // of every channel of the file, skipped ones included
    Channel channel[4] = {};                     // R, G, B, A
    std::unique_ptr<Chunk[]> chunks;
    size_t chunkCount = 0;
    size_t deflatedBytes = 0;                    // of the file's chunks as stored
    const uint8_t* stream = nullptr;             // into `storage`
    size_t streamBytes = 0;
    Blob storage;
    void Release() noexcept;
};
HRESULT LoadFromEXRMemoryRaw(const void* pSource, size_t size, TexMetadata* metadata, EXRRawImage& raw) noexcept;
HRESULT LoadFromEXRFileRaw(const char* szFile, TexMetadata* metadata, EXRRawImage& raw) noexcept;
// Resident forms: the stream crosses PCIe as it leaves the inflater - 6 bytes a texel for RGB half - and the delta undo (a byte-wise prefix
// sum), the plane gather, the sample conversion and the channel fill run on the device (dxtex_exr_unpack_device). HRESULTs, metadata and
// pixels are those of the host forms. Load: one upload of streamBytes, no download; the result is released on failure. Save: deviceImage's
// pixels are a device pointer, as DeviceScratchImage::GetImage gives; the scanlines come down at 8 bytes a texel, straight behind the
// header and offset table and between the chunk headers the host wrote.
HRESULT LoadFromEXRMemory(Device& device, const void* pSource, size_t size, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
HRESULT LoadFromEXRFile(Device& device, const char* szFile, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
// the second half of the resident load, for a caller that parsed the file before it had a device
HRESULT UploadEXRRaw(Device& device, const TexMetadata& metadata, const EXRRawImage& raw, DeviceScratchImage& image) noexcept;
HRESULT SaveToEXRMemory(Device& device, const Image& deviceImage, Blob& blob) noexcept;
HRESULT SaveToEXRFile(Device& device, const Image& deviceImage, const char* szFile) noexcept;

// ---- TIFF, which the reference reads and writes through WIC (DirectXTexWIC.cpp: WIC_CODEC_TIFF; texconv's -ft tif). No library is
// linked: the header, the IFD walk, LZW, PackBits and - through DirectXTexAMD_Inflate.h - inflate are this project's own code; what
// happens to a strip's or a tile's bytes after that is csrc/dxtex_tiff.h's. Accepted: classic TIFF (magic 42), II and MM, the first IFD;
// strips (any RowsPerStrip) and tiles; PlanarConfiguration 1 and 2; Compression 1, 5 (LZW, MSB-first with the early code-width change), 8
// and 32946 (deflate), 32773 (PackBits); Predictor 1, 2 for 8- and 16-bit samples, 3 for 32-bit floats; SampleFormat 1 (4 reads as 1) for
// integers and 3 for 32 bits; FillOrder 1; the defaults of the TIFF 6.0 text. Kinds and formats follow g_WICFormats / g_WICConvert /
// DetermineFormat without WIC_FLAGS_ALLOW_MONO: bilevel, grey 4 and grey 8 are R8_UNORM (multiplied out, WhiteIsZero inverted), grey 16
// R16_UNORM, grey float R32_FLOAT, palette 1 / 4 / 8 R8G8B8A8_UNORM (entry >> 8, alpha 0xff), RGB 8 and RGBA 8 R8G8B8A8_UNORM, RGB 16 and
// RGBA 16 R16G16B16A16_UNORM, RGB float R32G32B32_FLOAT, RGBA float R32G32B32A32_FLOAT; a kind without alpha is TEX_ALPHA_MODE_OPAQUE. An
// 8-bit colour file is _SRGB when its Exif IFD (tag 34665) holds ColorSpace (40961) = 1, or under TIFF_FLAGS_DEFAULT_SRGB when it holds
// none; never under TIFF_FLAGS_IGNORE_SRGB. Null arguments are E_INVALIDARG, a missing file HRESULT_ERROR_FILE_NOT_FOUND, and E_FAIL is:
// a bad header, truncation, an offset or count outside the file, a missing needed tag, a segment that expands to fewer bytes than its rows
// need. Departures (WIC is not there to run against, so these are this project's rules; tests/tiff_ref.py restates them):
//   1. The Memory forms exist.
//   2. HRESULT_E_NOT_SUPPORTED for BigTIFF; JPEG, CCITT and any other compression; YCbCr, CMYK, CIELab and any other photometric; signed
//      integers, 16- and 64-bit floats; bits other than 1 / 4 / 8 / 16 / 32 or unequal across samples; grey plus alpha; more than one
//      extra sample; FillOrder 2; old-style LSB-first LZW; predictor 2 on 1-, 4- or 32-bit samples (and 3 on anything but 32-bit floats);
//      WhiteIsZero floats.
//   3. Associated alpha (ExtraSamples 1) keeps the file's samples and sets TEX_ALPHA_MODE_PREMULTIPLIED, where WIC would divide. An
//      unspecified fourth sample (ExtraSamples 0 or absent) reads as opaque: alpha forced to its maximum, TEX_ALPHA_MODE_OPAQUE.
//   4. Orientation and further IFDs are ignored, and so is Predictor where the compression is 1 or 32773: it belongs to the LZW and deflate
//      coders, and libtiff reads such files as they are.
//   5. The writer stores uncompressed: II, one IFD, one strip, chunky; ExtraSamples 2 for alpha, resolution 72 / 72 and Software
//      "DirectXTex" as the reference's EncodeImage / EncodeMetadata set; Exif ColorSpace 1 for an _SRGB format or under
//      TIFF_FLAGS_FORCE_SRGB, never under TIFF_FLAGS_FORCE_LINEAR. It takes R8_UNORM, R16_UNORM, R32_FLOAT, R8G8B8A8_UNORM[_SRGB],
//      R16G16B16A16_UNORM, R32G32B32_FLOAT, R32G32B32A32_FLOAT, B8G8R8A8_UNORM[_SRGB] (written RGBA) and B8G8R8X8_UNORM[_SRGB] (written
//      RGB, 3 bytes); every other format is HRESULT_E_NOT_SUPPORTED. ------------------------------------------------------------------------
enum TIFF_FLAGS : uint32_t
{
    TIFF_FLAGS_NONE = 0,
    TIFF_FLAGS_IGNORE_SRGB = 0x1,        // the Exif colour space does not choose the format: it is the linear one
    TIFF_FLAGS_DEFAULT_SRGB = 0x2,       // an 8-bit colour file that names no colour space is _SRGB
    TIFF_FLAGS_FORCE_SRGB = 0x20,        // the writer stores Exif ColorSpace 1 whatever the format
    TIFF_FLAGS_FORCE_LINEAR = 0x40,      // the writer stores no colour space whatever the format
};
inline TIFF_FLAGS operator|(TIFF_FLAGS a, TIFF_FLAGS b) noexcept { return TIFF_FLAGS(uint32_t(a) | uint32_t(b)); }
HRESULT GetMetadataFromTIFFMemory(const void* pSource, size_t size, TIFF_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT GetMetadataFromTIFFFile(const char* szFile, TIFF_FLAGS flags, TexMetadata& metadata) noexcept;
HRESULT LoadFromTIFFMemory(const void* pSource, size_t size, TIFF_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT LoadFromTIFFFile(const char* szFile, TIFF_FLAGS flags, TexMetadata* metadata, ScratchImage& image) noexcept;
HRESULT SaveToTIFFMemory(const Image& image, TIFF_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToTIFFFile(const Image& image, TIFF_FLAGS flags, const char* szFile) noexcept;
// The reader's byte-serial half, which needs no device: the header, the IFD walk, every refusal, LZW, PackBits and inflate. What comes
// back is ONE STREAM of the segments' expanded bytes - still predictor-coded, in the file's byte order, at the file's bits per sample -
// and dxtex_tiff_unpack's other arguments: a descriptor per segment (strips that follow one another in the stream and in the image share
// one; every other segment starts on a multiple of 16 bytes), the layout and the palette's 256 words. GetMetadata* stop behind the IFD. On
// failure `raw` is released.
struct TIFFRawImage
{
    struct Segment { uint64_t offset; uint32_t firstRow, rows, firstCol, cols, rowBytes, plane; };          // dxtex_tiff_segment's layout
    struct Layout { uint32_t width, height, bits, samples, kind, predictor, bigEndian, planar, whiteIsZero, opaque; };          // dxtex_tiff_layout's
    uint32_t compression = 0;                    // the file's code
    Layout layout = {};
    uint32_t palette[256] = {};                  // for the palette kinds: the words tiff_texels stores
    std::unique_ptr<Segment[]> segments;
    size_t segmentCount = 0;
    size_t storedBytes = 0;                      // of the file's segments as stored
    const uint8_t* stream = nullptr;             // into `storage`
    size_t streamBytes = 0;
    Blob storage;
    void Release() noexcept;
};
HRESULT LoadFromTIFFMemoryRaw(const void* pSource, size_t size, TIFF_FLAGS flags, TexMetadata* metadata, TIFFRawImage& raw) noexcept;
HRESULT LoadFromTIFFFileRaw(const char* szFile, TIFF_FLAGS flags, TexMetadata* metadata, TIFFRawImage& raw) noexcept;
// Resident forms: the stream crosses PCIe as it leaves the decoder - 3 bytes a texel for RGB 8, one bit for bilevel - and the predictor
// undo (a strided prefix sum along every row), the sample expansion, the palette, the alpha fill and the byte swaps run on the device
// (dxtex_tiff_unpack_device). HRESULTs, metadata and pixels are those of the host forms. Load: one upload of streamBytes, no download; a
// file that is its image already (csrc/dxtex_tiff.h's tiff_is_native) whose one segment matches the image's pitch goes straight into it,
// no kernel; the result is released on failure. Save: deviceImage's pixels are a device pointer, as DeviceScratchImage::GetImage gives;
// the file's rows come down straight behind the header the host wrote, and only the two BGR sources run a kernel.
HRESULT LoadFromTIFFMemory(Device& device, const void* pSource, size_t size, TIFF_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
HRESULT LoadFromTIFFFile(Device& device, const char* szFile, TIFF_FLAGS flags, TexMetadata* metadata, DeviceScratchImage& image) noexcept;
// the second half of the resident load, for a caller that parsed the file before it had a device
HRESULT UploadTIFFRaw(Device& device, const TexMetadata& metadata, const TIFFRawImage& raw, DeviceScratchImage& image) noexcept;
HRESULT SaveToTIFFMemory(Device& device, const Image& deviceImage, TIFF_FLAGS flags, Blob& blob) noexcept;
HRESULT SaveToTIFFFile(Device& device, const Image& deviceImage, TIFF_FLAGS flags, const char* szFile) noexcept;
} // namespace DirectXTexAMD
