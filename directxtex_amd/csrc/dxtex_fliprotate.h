// FlipRotate (DirectXTex.h:723-737, DirectXTexFlipRotate.cpp): what the host resolves per image, what the kernels in flip_rotate.hip
// receive, and which bytes each lane of them reads and writes. The kernels and the host check (tests/cpp/fliprotate_check.cpp) call the
// same index functions. Plain data and integer arithmetic only, __host__ __device__.
//
// THE RULE (this project's; tests/fliprotate_ref.py restates it in numpy): the source turned CLOCKWISE by the angle, then mirrored
// left-right if FLIP_HORIZONTAL is set, then mirrored top-bottom if FLIP_VERTICAL is set. The reference hands the flag word to WIC, whose
// documentation does not say whether a flip combined with a rotation comes before or after it, and neither of the reference's tools ever
// combines them, so this order is a stated departure nobody can check. It lives in fr_resolve() alone: turn it round there.
//
// The fifteen legal flag words are the eight symmetries of the rectangle, {transpose, mirrorX, mirrorY}; with W x H the result's size,
//   x1 = mirrorX ? W - 1 - xd : xd,   y1 = mirrorY ? H - 1 - yd : yd,   source texel = transpose ? (y1, x1) : (x1, y1).
// Texels move as bytes (1, 2, 4, 8, 12 or 16 of them), never through a float row.
//
// Routes, chosen per job by the host from the real addresses and pitches:
//   row wide     no transpose; a lane owns 16 bytes of a destination row. Taken when both first-row addresses, both pitches (with more than
//                one row) and the row's byte count are multiples of 16 and the texel is not 12 bytes. With mirrorX the lane reads the
//                mirrored 16 bytes - aligned as well, the row being whole 16-byte units - and reverses the texels inside them in registers.
//   row narrow   no transpose; a lane owns one destination texel, moved in `access`-byte pieces: the largest of 16 / 8 / 4 / 2 / 1 that
//                divides the texel and every row start of both sides.
//   tile         transpose; a workgroup owns a square tile of fr_tile_side() texels a side. Source rows of the tile go into LDS with
//                consecutive lanes on consecutive texels, one barrier, and LDS is read along its other axis so that consecutive lanes
//                are on consecutive texels of a destination row again. mirrorX / mirrorY move the tile's source position and turn the
//                LDS read's row / column index round. An LDS row is fr_tile_pitch() bytes: the texels plus one bank's worth of padding,
//                so that the column-order read walks the banks instead of standing on one. Edge tiles are guarded.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dxtex
{
constexpr uint32_t kFlipRotate90 = 1, kFlipRotate180 = 2, kFlipRotate270 = 3, kFlipHorizontal = 0x08, kFlipVertical = 0x10;

// TEX_FR_FLAGS that name an operation: fifteen values
__host__ __device__ inline bool fr_flags_legal(uint32_t flags) { return flags != 0 && (flags & ~0x1Bu) == 0; }

struct FlipOp { uint32_t transpose, mirrorX, mirrorY; };

// The one place that says what a flag word means (see THE RULE above). A clockwise quarter turn is the transpose mirrored left-right, a
// half turn both mirrors, three quarters the transpose mirrored top-bottom; the two flips come after and so toggle the same mirrors.
__host__ __device__ inline FlipOp fr_resolve(uint32_t flags)
{
    const uint32_t rot = flags & 3u;
    FlipOp op;
    op.transpose = rot & 1u;
    op.mirrorX = ((flags & kFlipHorizontal) ? 1u : 0u) ^ ((rot == 1u || rot == 2u) ? 1u : 0u);
    op.mirrorY = ((flags & kFlipVertical) ? 1u : 0u) ^ ((rot == 2u || rot == 3u) ? 1u : 0u);
    return op;
}

// the source texel of texel (xd, yd) of the W x H result
__host__ __device__ inline void fr_source_texel(const FlipOp& op, uint32_t W, uint32_t H, uint32_t xd, uint32_t yd, uint32_t* xs, uint32_t* ys)
{
    const uint32_t x1 = op.mirrorX ? W - 1u - xd : xd, y1 = op.mirrorY ? H - 1u - yd : yd;
    *xs = op.transpose ? y1 : x1;
    *ys = op.transpose ? x1 : y1;
}

enum FlipRoute : uint32_t { FR_ROW_WIDE = 0, FR_ROW_NARROW = 1, FR_TILE = 2 };

// One image. width x height is the RESULT's size in texels; src / dst point at the first byte of the first row.
struct FlipJob
{
    const uint8_t* src;
    uint8_t* dst;
    uint64_t srcPitch, dstPitch;
    uint32_t width, height;
    uint32_t texel;                 // bytes of a texel: 1, 2, 4, 8, 12, 16
    uint32_t mirrorX, mirrorY;
    uint32_t route;                 // FlipRoute
    uint32_t access;                // bytes of one global access of the narrow and tile routes; divides texel
    uint32_t pad;
};

// Jobs travel in the kernel's argument block like CopyBatch: a batch is ONE launch, more jobs are cut into several launches.
constexpr uint32_t kFlipBatchMax = 32;
struct FlipBatch
{
    FlipJob job[kFlipBatchMax];
    uint32_t count;
};
static_assert(sizeof(FlipBatch) <= 3072, "the batch must fit the kernel argument block next to nothing else");

constexpr uint32_t kFlipThreads = 256;
constexpr uint32_t kFlipRowsInFlight = 4;      // rows a lane of the row route loads before its first store, as copy_rect_move does

__host__ __device__ inline bool fr_texel_bytes_ok(uint32_t b) { return b == 1u || b == 2u || b == 4u || b == 8u || b == 12u || b == 16u; }

// the widest access (16, 8, 4, 2, 1) that divides the texel and that every row start of both sides is aligned to
__host__ __device__ inline uint32_t fr_access_bytes(uint32_t texel, uint64_t srcAddr, uint64_t dstAddr, uint64_t srcPitch, uint64_t dstPitch, uint32_t srcRows, uint32_t dstRows)
{
    uint64_t bits = srcAddr | dstAddr | texel;
    if (srcRows > 1u) bits |= srcPitch;
    if (dstRows > 1u) bits |= dstPitch;
    uint32_t v = 16;
    while (v > 1u && (bits & (v - 1u))) v >>= 1;
    return v;
}

// The route and access width of a job whose other fields are set.
__host__ __device__ inline void fr_choose_route(FlipJob* j, bool transpose)
{
    const uint64_t s = uint64_t(reinterpret_cast<uintptr_t>(j->src)), d = uint64_t(reinterpret_cast<uintptr_t>(j->dst));
    const uint32_t srcRows = transpose ? j->width : j->height;
    j->access = fr_access_bytes(j->texel, s, d, j->srcPitch, j->dstPitch, srcRows, j->height);
    if (transpose) { j->route = FR_TILE; return; }
    const uint64_t rowBytes = uint64_t(j->width) * j->texel;
    uint64_t bits = s | d | rowBytes;
    if (j->height > 1u) bits |= j->srcPitch | j->dstPitch;
    j->route = (j->texel != 12u && (bits & 15u) == 0) ? FR_ROW_WIDE : FR_ROW_NARROW;
}

// ---- the row route ------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline uint32_t fr_row_unit_bytes(const FlipJob& j) { return j.route == FR_ROW_WIDE ? 16u : j.texel; }
// lanes of a row: 16-byte units (wide) or texels (narrow)
__host__ __device__ inline uint32_t fr_row_units(const FlipJob& j)
{
    return j.route == FR_ROW_WIDE ? uint32_t(uint64_t(j.width) * j.texel / 16u) : j.width;
}
// where unit u of destination row y lies, and the unit that feeds it (from src / dst, in bytes)
__host__ __device__ inline void fr_row_unit(const FlipJob& j, uint32_t u, uint32_t y, uint64_t* srcByte, uint64_t* dstByte)
{
    const uint32_t ub = fr_row_unit_bytes(j), n = fr_row_units(j);
    const uint32_t su = j.mirrorX ? n - 1u - u : u, sy = j.mirrorY ? j.height - 1u - y : y;
    *srcByte = uint64_t(sy) * j.srcPitch + uint64_t(su) * ub;
    *dstByte = uint64_t(y) * j.dstPitch + uint64_t(u) * ub;
}

// the texels of 16 bytes (four dwords, lowest address first) in the opposite order; texel = 1, 2, 4, 8 or 16 bytes
__host__ __device__ inline void fr_reverse16(uint32_t (&v)[4], uint32_t texel)
{
    if (texel >= 16u) return;
    if (texel == 8u)
    {
        const uint32_t a = v[0], b = v[1];
        v[0] = v[2]; v[1] = v[3]; v[2] = a; v[3] = b;
        return;
    }
    const uint32_t a = v[0], b = v[1];
    v[0] = v[3]; v[1] = v[2]; v[2] = b; v[3] = a;
    if (texel == 4u) return;
#if defined(__clang__) || defined(__GNUC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k)
    {
        uint32_t w = (v[k] >> 16) | (v[k] << 16);
        if (texel == 1u) w = ((w & 0x00FF00FFu) << 8) | ((w >> 8) & 0x00FF00FFu);
        v[k] = w;
    }
}

// ---- the tile route -----------------------------------------------------------------------------------------------------------------
// A tile stays at or below 16 KiB of texels: 64 x 64 up to 4-byte texels, 32 x 32 for 8, 12 and 16 bytes.
__host__ __device__ inline uint32_t fr_tile_side(uint32_t texel) { return texel <= 4u ? 64u : 32u; }
// Bytes of a tile row in LDS. The LDS has 64 banks of 4 bytes; a pitch that is a multiple of 256 bytes (128 for the 32-bank accesses)
// would put a whole column on one bank. One dword more (one texel more for 8 and 16 bytes, whose accesses stay aligned that way) makes
// the pitch in dwords 17, 33, 65, 66, 97 and 132: lane i of a column read starts on bank i, 2i or 4i.
__host__ __device__ inline uint32_t fr_tile_pitch(uint32_t texel) { return fr_tile_side(texel) * texel + ((texel == 8u || texel == 16u) ? texel : 4u); }
constexpr uint32_t kFlipTileLdsBytes = 32u * (32u * 16u + 16u);       // the largest tile: 16-byte texels, 16.5 KiB
// passes of a workgroup over its tile: kFlipThreads lanes cover kFlipThreads / side rows at a time
__host__ __device__ inline uint32_t fr_tile_passes(uint32_t texel) { const uint32_t s = fr_tile_side(texel); return s / (kFlipThreads / s); }

// A destination tile and where its texels come from. The tile covers result texels [dx0, dx0 + tw) x [dy0, dy0 + th); its source is the
// th x tw (wide x high) block at (sx0, sy0), LDS row ly / column lx holding source texel (sx0 + lx, sy0 + ly).
struct FlipTile { uint32_t dx0, dy0, tw, th, sx0, sy0; };

__host__ __device__ inline bool fr_tile(const FlipJob& j, uint32_t bx, uint32_t by, FlipTile* t)
{
    const uint32_t side = fr_tile_side(j.texel);
    if (uint64_t(bx) * side >= j.width || uint64_t(by) * side >= j.height) return false;
    t->dx0 = bx * side; t->dy0 = by * side;
    t->tw = j.width - t->dx0 < side ? j.width - t->dx0 : side;
    t->th = j.height - t->dy0 < side ? j.height - t->dy0 : side;
    t->sx0 = j.mirrorY ? j.height - t->dy0 - t->th : t->dy0;
    t->sy0 = j.mirrorX ? j.width - t->dx0 - t->tw : t->dx0;
    return true;
}

// pass k of lane t, first half: the source texel it reads (bytes from src) and where it goes in LDS; false where the lane has none
__host__ __device__ inline bool fr_tile_load(const FlipJob& j, const FlipTile& t, uint32_t lane, uint32_t k, uint64_t* srcByte, uint32_t* ldsByte)
{
    const uint32_t side = fr_tile_side(j.texel);
    const uint32_t lx = lane % side, ly = lane / side + k * (kFlipThreads / side);
    if (lx >= t.th || ly >= t.tw) return false;
    *srcByte = uint64_t(t.sy0 + ly) * j.srcPitch + uint64_t(t.sx0 + lx) * j.texel;
    *ldsByte = ly * fr_tile_pitch(j.texel) + lx * j.texel;
    return true;
}

// second half, after the barrier: the LDS texel it reads and the destination texel it writes (bytes from dst)
__host__ __device__ inline bool fr_tile_store(const FlipJob& j, const FlipTile& t, uint32_t lane, uint32_t k, uint32_t* ldsByte, uint64_t* dstByte)
{
    const uint32_t side = fr_tile_side(j.texel);
    const uint32_t c = lane % side, r = lane / side + k * (kFlipThreads / side);
    if (c >= t.tw || r >= t.th) return false;
    const uint32_t row = j.mirrorX ? t.tw - 1u - c : c, col = j.mirrorY ? t.th - 1u - r : r;
    *ldsByte = row * fr_tile_pitch(j.texel) + col * j.texel;
    *dstByte = uint64_t(t.dy0 + r) * j.dstPitch + uint64_t(t.dx0 + c) * j.texel;
    return true;
}

// ---- launch geometry ------------------------------------------------------------------------------------------------------------------
// Row route: x over the units of the widest job, y over groups of kFlipRowsInFlight rows (a lane strides over more), z over jobs.
// Tile route: x, y over the tiles of the largest job (a workgroup strides over more tile rows), z over jobs.
// Workgroups outside their own job's extent leave at once.
__host__ __device__ inline void fr_grid(const FlipBatch& b, bool tiles, uint32_t* gx, uint32_t* gy)
{
    uint32_t x = 0, y = 0;
    for (uint32_t k = 0; k < b.count; ++k)
    {
        const FlipJob& j = b.job[k];
        const uint32_t side = fr_tile_side(j.texel);
        const uint32_t jx = tiles ? (j.width + side - 1u) / side : (fr_row_units(j) + kFlipThreads - 1u) / kFlipThreads;
        const uint32_t jy = tiles ? (j.height + side - 1u) / side : (j.height + kFlipRowsInFlight - 1u) / kFlipRowsInFlight;
        x = jx > x ? jx : x;
        y = jy > y ? jy : y;
    }
    *gx = x;
    if (!tiles)
    {
        // about 8192 workgroups over the batch, as copy_rect launches
        const uint32_t cap = x && b.count ? 8192u / (x * b.count) : 1u;
        if (y > (cap ? cap : 1u)) y = cap ? cap : 1u;
    }
    *gy = y < 65535u ? y : 65535u;
}
} // namespace dxtex
