// Host build of dxtex_fliprotate.h for tests/test_fliprotate_cpu.py: the flag rules, and what the kernels of flip_rotate.hip read and write,
// by visiting every (workgroup, lane, pass) their launch geometry visits and calling the index functions the kernels call.
//
//   fliprotate_check legal FLAGS...        one line per word: "FLAGS 0|1"
//   fliprotate_check classes               one line per legal word: "FLAGS transpose mirrorX mirrorY"
//   fliprotate_check coords W H            (W x H is the SOURCE) per legal word a line "FLAGS RW RH" and a line of RW * RH "xs ys" pairs, the
//                                          source texel of every texel of the result in row order
//   fliprotate_check walk W H TEXEL SRCPITCH DSTPITCH SRCSHIFT DSTSHIFT FLAGS OUT
//       One job as the C ABI resolves it, with first-row addresses SHIFT bytes after a 4096-byte boundary. Source byte i is
//       (i * 2654435761 >> 13) & 255, the destination starts as zero. The walk moves the bytes as the kernels do (the tile route through an
//       array that stands for the LDS) and fails (exit 1, a line on stderr) on an access that is not inside one row's texels, is not
//       aligned to its own width, an LDS offset outside the tile's array or misaligned, or an LDS read of a byte this tile did not write.
//       OUT receives the destination's RH * DSTPITCH bytes and then as many bytes holding how often each was written.
//       stdout: "route access gx gy"
#include "dxtex_fliprotate.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace dxtex;

namespace
{
[[noreturn]] void die(const char* what)
{
    fprintf(stderr, "fliprotate_check: %s\n", what);
    exit(1);
}

struct Side
{
    std::vector<uint8_t> bytes, count;
    uint64_t pitch, rowBytes, rows, base;
    // [at, at + n) lies inside one row's texels and is aligned to n where the job claims that alignment
    void touch(uint64_t at, uint32_t n, bool write)
    {
        const uint64_t row = at / pitch, in = at - row * pitch;
        if (row >= rows) die("an access beyond the last row");
        if (in + n > rowBytes) die("an access outside a row's texels");
        if ((base + at) % n) die("a misaligned access");
        if (write) for (uint32_t i = 0; i < n; ++i) ++count[size_t(at) + i];
    }
};

void move(Side& src, uint64_t from, Side& dst, uint64_t to, uint32_t n)
{
    src.touch(from, n, false);
    dst.touch(to, n, true);
    memcpy(&dst.bytes[size_t(to)], &src.bytes[size_t(from)], n);
}

int walk(int argc, char** argv)
{
    if (argc != 11) die("walk takes nine arguments");
    const uint64_t w = strtoull(argv[2], nullptr, 0), h = strtoull(argv[3], nullptr, 0);
    const uint32_t texel = uint32_t(strtoul(argv[4], nullptr, 0));
    const uint64_t srcPitch = strtoull(argv[5], nullptr, 0), dstPitch = strtoull(argv[6], nullptr, 0);
    const uint64_t srcShift = strtoull(argv[7], nullptr, 0), dstShift = strtoull(argv[8], nullptr, 0);
    const uint32_t flags = uint32_t(strtoul(argv[9], nullptr, 0));
    if (!fr_flags_legal(flags) || !fr_texel_bytes_ok(texel) || !w || !h) die("bad case");
    const FlipOp op = fr_resolve(flags);
    const uint64_t rw = op.transpose ? h : w, rh = op.transpose ? w : h;
    if (srcPitch < w * texel || dstPitch < rw * texel) die("a pitch below its row");

    Side src, dst;
    src.pitch = srcPitch; src.rowBytes = w * texel; src.rows = h; src.base = 4096 + srcShift;
    dst.pitch = dstPitch; dst.rowBytes = rw * texel; dst.rows = rh; dst.base = (1ull << 32) + 4096 + dstShift;
    src.bytes.resize(size_t(h * srcPitch)); src.count.assign(src.bytes.size(), 0);
    dst.bytes.assign(size_t(rh * dstPitch), 0); dst.count.assign(dst.bytes.size(), 0);
    for (size_t i = 0; i < src.bytes.size(); ++i) src.bytes[i] = uint8_t((uint32_t(i) * 2654435761u) >> 13);

    FlipBatch b = {};
    b.count = 1;
    FlipJob& j = b.job[0];
    j.src = reinterpret_cast<const uint8_t*>(uintptr_t(src.base)); j.dst = reinterpret_cast<uint8_t*>(uintptr_t(dst.base));     // addresses only: never dereferenced
    j.srcPitch = srcPitch; j.dstPitch = dstPitch;
    j.width = uint32_t(rw); j.height = uint32_t(rh);
    j.texel = texel; j.mirrorX = op.mirrorX; j.mirrorY = op.mirrorY;
    fr_choose_route(&j, op.transpose != 0);
    if (j.texel % j.access) die("the access width does not divide the texel");
    uint32_t gx = 0, gy = 0;
    fr_grid(b, j.route == FR_TILE, &gx, &gy);

    if (j.route != FR_TILE)
    {
        // flip_rows_kernel
        for (uint32_t by = 0; by < gy; ++by)
            for (uint32_t bx = 0; bx < gx; ++bx)
                for (uint32_t t = 0; t < kFlipThreads; ++t)
                {
                    const uint32_t u = bx * kFlipThreads + t;
                    if (u >= fr_row_units(j)) continue;
                    for (uint32_t y0 = by * kFlipRowsInFlight; y0 < j.height; y0 += gy * kFlipRowsInFlight)
                        for (uint32_t r = 0; r < kFlipRowsInFlight && y0 + r < j.height; ++r)
                        {
                            uint64_t from, to;
                            fr_row_unit(j, u, y0 + r, &from, &to);
                            if (j.route == FR_ROW_WIDE)
                            {
                                move(src, from, dst, to, 16);
                                uint32_t v[4];
                                memcpy(v, &dst.bytes[size_t(to)], 16);
                                if (j.mirrorX) fr_reverse16(v, j.texel);
                                memcpy(&dst.bytes[size_t(to)], v, 16);
                            }
                            else
                                for (uint32_t i = 0; i < j.texel; i += j.access) move(src, from + i, dst, to + i, j.access);
                        }
                }
    }
    else
    {
        // flip_transpose_kernel: all lanes load, the barrier, all lanes store
        std::vector<uint8_t> lds(kFlipTileLdsBytes);
        std::vector<uint32_t> stamp(kFlipTileLdsBytes, 0);
        const uint32_t align = texel == 12u ? 4u : texel;
        uint32_t tile = 0;
        for (uint32_t bx = 0; bx < gx; ++bx)
            for (uint32_t by0 = 0; by0 < gy; ++by0)
                for (uint32_t by = by0; ; by += gy)
                {
                    FlipTile t;
                    if (!fr_tile(j, bx, by, &t)) break;
                    ++tile;
                    for (uint32_t lane = 0; lane < kFlipThreads; ++lane)
                        for (uint32_t k = 0; k < fr_tile_passes(texel); ++k)
                        {
                            uint64_t from; uint32_t at;
                            if (!fr_tile_load(j, t, lane, k, &from, &at)) continue;
                            if (at % align || at + texel > kFlipTileLdsBytes) die("an LDS store outside the tile's array or misaligned");
                            for (uint32_t i = 0; i < texel; i += j.access) src.touch(from + i, j.access, false);
                            memcpy(&lds[at], &src.bytes[size_t(from)], texel);
                            for (uint32_t i = 0; i < texel; ++i) stamp[at + i] = tile;
                        }
                    for (uint32_t lane = 0; lane < kFlipThreads; ++lane)
                        for (uint32_t k = 0; k < fr_tile_passes(texel); ++k)
                        {
                            uint64_t to; uint32_t at;
                            if (!fr_tile_store(j, t, lane, k, &at, &to)) continue;
                            if (at % align || at + texel > kFlipTileLdsBytes) die("an LDS load outside the tile's array or misaligned");
                            for (uint32_t i = 0; i < texel; ++i) if (stamp[at + i] != tile) die("an LDS load of a byte this tile did not store");
                            for (uint32_t i = 0; i < texel; i += j.access) dst.touch(to + i, j.access, true);
                            memcpy(&dst.bytes[size_t(to)], &lds[at], texel);
                        }
                }
    }
    FILE* out = fopen(argv[10], "wb");
    if (!out) die("cannot open OUT");
    fwrite(dst.bytes.data(), 1, dst.bytes.size(), out);
    fwrite(dst.count.data(), 1, dst.count.size(), out);
    if (fclose(out) != 0) die("cannot write OUT");
    printf("%u %u %u %u\n", j.route, j.access, gx, gy);
    return 0;
}
}

int main(int argc, char** argv)
{
    if (argc >= 2 && !strcmp(argv[1], "legal"))
    {
        for (int i = 2; i < argc; ++i)
        {
            const uint32_t f = uint32_t(strtoul(argv[i], nullptr, 0));
            printf("%u %d\n", f, fr_flags_legal(f) ? 1 : 0);
        }
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "classes"))
    {
        for (uint32_t f = 0; f < 64; ++f)
        {
            if (!fr_flags_legal(f)) continue;
            const FlipOp op = fr_resolve(f);
            printf("%u %u %u %u\n", f, op.transpose, op.mirrorX, op.mirrorY);
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "coords"))
    {
        const uint32_t w = uint32_t(strtoul(argv[2], nullptr, 0)), h = uint32_t(strtoul(argv[3], nullptr, 0));
        for (uint32_t f = 0; f < 64; ++f)
        {
            if (!fr_flags_legal(f)) continue;
            const FlipOp op = fr_resolve(f);
            const uint32_t rw = op.transpose ? h : w, rh = op.transpose ? w : h;
            printf("%u %u %u\n", f, rw, rh);
            for (uint32_t y = 0; y < rh; ++y)
                for (uint32_t x = 0; x < rw; ++x)
                {
                    uint32_t xs, ys;
                    fr_source_texel(op, rw, rh, x, y, &xs, &ys);
                    printf("%u %u ", xs, ys);
                }
            printf("\n");
        }
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "walk")) return walk(argc, argv);
    fprintf(stderr, "usage: fliprotate_check legal FLAGS... | classes | coords W H | walk W H TEXEL SRCPITCH DSTPITCH SRCSHIFT DSTSHIFT FLAGS OUT\n");
    return 2;
}
