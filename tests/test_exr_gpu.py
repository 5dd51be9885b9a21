"""OpenEXR chunks on the GPU (dxtex_exr_unpack / dxtex_exr_pack and their _device forms) against tests/exr_ref.py: pixels and scanlines byte
for byte, the bytes around them untouched, every route of exr_undo, exr_texels and exr_pack asserted by profile mark."""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import exr_ref as R  # noqa: E402
from test_exr_cpu import CHANNEL_SETS, EDGE_FLOATS, SOURCE_BYTES, channels_of, make_samples, writer_pixels  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALIDARG, E_POINTER, E_NOT_SUPPORTED = 0x80070057 - (1 << 32), 0x80004003 - (1 << 32), 0x80070032 - (1 << 32)
FILL = 0xA5
TILE = dx.EXR_UNDO_TILE
RGBA16F = dx.DXGI_FORMAT_R16G16B16A16_FLOAT
ABSENT = (0, dx.EXR_ABSENT)
STREAM_MAX = 14 * TILE          # of the arena: three chunks of four tiles and a tail


def _marks(prof, prefix="exr_"):
    return {k: v[1] for k, v in prof.items() if k.startswith(prefix)}


def table_of(channels, w):
    """the channel table [(offset, type)] * 4 and the scanline's bytes of a file with these channels"""
    line, where = 0, {}
    for name, typ, _, _ in sorted(channels, key=lambda c: c[0].encode()):
        where[name] = (line, typ)
        line += w * R.TYPE_BYTES[typ]
    table = [where.get(n) for n in "RGBA"]
    if "Y" in where and table[:3] == [None] * 3:
        table[:3] = [where["Y"]] * 3
    return table, line


def expected(plain, table, scanline, w):
    """(rows, w, 4) halves of plain scanlines"""
    return R.texels(plain, dict(width=w, scanline=scanline, table=table), len(plain) // scanline)


def build_stream(plains, coded, align=16):
    """the chunks' plain bytes [(first row, rows, bytes)] -> (stream, descriptors): chunk i coded where coded(i), a coded chunk on a multiple
    of `align`"""
    stream, chunks = bytearray(), []
    for i, (first, rows, plain) in enumerate(plains):
        c = bool(coded(i))
        if c:
            stream += bytes(-len(stream) % align)
        chunks.append((len(stream), len(plain), first, rows, int(c)))
        stream += R.code(plain) if c else plain
    return np.frombuffer(bytes(stream), np.uint8), chunks


def file_chunks(channels, samples, h, lines):
    return [(y, min(lines, h - y), R.plain_chunk(channels, samples, y, min(lines, h - y))) for y in range(0, h, lines)]


class Arena:
    def __init__(self, ctx, stream_bytes, image_bytes):
        self.ctx = ctx
        self.s = ctx.device_alloc(stream_bytes + 256)
        self.d = ctx.device_alloc(image_bytes + 256)

    def close(self):
        self.ctx.device_free(self.s)
        self.ctx.device_free(self.d)


@pytest.fixture
def arena(ctx):
    a = Arena(ctx, STREAM_MAX, 1 << 20)
    yield a
    a.close()


def run_device(ctx, arena, stream, chunks, table, scanline, w, item_h, items, want, base=0, pad=0, seen=None, where=None):
    """the _device form: pixels, the bytes around them, the stream's plain chunks unchanged; returns the marks"""
    pitch = w * 8 + pad
    item_bytes = pitch * item_h
    assert base + stream.nbytes <= STREAM_MAX and item_bytes * items + 32 <= 1 << 20
    ctx.upload(arena.s + base, stream, sync=True)
    ctx.upload(arena.d, np.full(item_bytes * items + 32, FILL, np.uint8), sync=True)
    imgs = [dx.device_image(arena.d + i * item_bytes, w, item_h, RGBA16F, pitch, item_bytes) for i in range(items)]
    ctx.profile_begin()
    ctx.exr_unpack_device(arena.s + base, stream.nbytes, chunks, [ABSENT if e is None else e for e in table], scanline, imgs)
    prof = _marks(ctx.profile_end())
    got = np.zeros(item_bytes * items + 32, np.uint8)
    ctx.download(got, arena.d, sync=True)
    m = got[:item_bytes * items].reshape(items * item_h, pitch)
    assert np.array_equal(np.ascontiguousarray(m[:, :w * 8]).view("<u2").reshape(items * item_h, w, 4), want), where
    assert (m[:, w * 8:] == FILL).all() and (got[item_bytes * items:] == FILL).all(), ("bytes outside the rows were written", where)
    after = np.zeros(stream.nbytes, np.uint8)
    ctx.download(after, arena.s + base, sync=True)
    for off, n, _, _, c in chunks:
        if not c:
            assert np.array_equal(after[off:off + n], stream[off:off + n]), ("a plain chunk was written", where)
    any_coded = any(c[4] for c in chunks)
    wide = (arena.s + base) % 16 == 0 and all(c[0] % 16 == 0 for c in chunks if c[4])
    assert prof.get("exr_texels", 0) >= 1 and set(prof) <= {"exr_texels", "exr_undo_sums", "exr_undo<wide>", "exr_undo<narrow>"}, (prof, where)
    assert (("exr_undo<wide>" if wide else "exr_undo<narrow>") in prof) == any_coded and ("exr_undo<narrow>" if wide else "exr_undo<wide>") not in prof, (prof, where)
    assert ("exr_undo_sums" in prof) == any(c[4] and c[1] > TILE for c in chunks), (prof, where)
    if seen is not None:
        seen.update(prof)
    return prof


def test_zip_shaped_chunks_at_every_small_size(ctx, arena):
    """widths 1 .. 65 by heights 1 .. 33 in chunks of 16 rows, all coded: the last chunk is short, half the plain size is odd and even; the
    stream on and off the wide route's alignment, the image's pitch wider than the row and off its 8 bytes"""
    rng = np.random.default_rng(1)
    ch = channels_of("rgba_half")
    seen, n = set(), 0
    for w in (1, 2, 3, 5, 17, 64, 65):
        table, scanline = table_of(ch, w)
        for h in (1, 15, 16, 17, 33):
            samples = make_samples(ch, w, h, rng)
            plains = file_chunks(ch, samples, h, 16)
            want = expected(b"".join(p[2] for p in plains), table, scanline, w)
            assert np.array_equal(want, np.stack([samples[c] for c in "RGBA"], -1))          # halves move as bits
            for base, align, pad in ((0, 16, 0), (0, 16, 8), (1, 16, 0), (0, 2, 3), (16, 16, 24))[n % 2::2] + ((0, 16, 0),):
                stream, chunks = build_stream(plains, lambda i: True, align)
                run_device(ctx, arena, stream, chunks, table, scanline, w, h, 1, want, base, pad, seen, (w, h, base, align, pad))
            n += 1
    assert {"exr_undo<wide>", "exr_undo<narrow>", "exr_texels"} <= seen


@pytest.mark.parametrize("name", list(CHANNEL_SETS))
def test_every_channel_set_coded_and_plain_mixed(ctx, arena, name):
    """one-row and 16-row chunks, every other one coded, of every channel set: absent channels filled, Y spread, skipped channels skipped,
    FLOAT and UINT samples converted at the values where the conversion changes"""
    rng = np.random.default_rng(len(name))
    ch = channels_of(name)
    for w, h, lines in ((1, 1, 1), (3, 5, 1), (5, 33, 16), (65, 17, 16)):
        table, scanline = table_of(ch, w)
        samples = make_samples(ch, w, h, rng)
        plains = file_chunks(ch, samples, h, lines)
        want = expected(b"".join(p[2] for p in plains), table, scanline, w)
        for first_coded in (0, 1):
            stream, chunks = build_stream(plains, lambda i: i % 2 == first_coded)
            run_device(ctx, arena, stream, chunks, table, scanline, w, h, 1, want, where=(name, w, h, lines, first_coded))
    if name == "a_only":
        assert (want[..., :3] == 0).all()
    if name == "rgb_half":
        assert (want[..., 3] == 0x3C00).all()
    if name == "y_only":
        assert np.array_equal(want[..., 0], want[..., 1]) and np.array_equal(want[..., 0], want[..., 2])


def test_half_plane_boundaries(ctx, arena):
    """a chunk of two bytes (A only, width 1), and mixes of UINT, FLOAT and HALF whose plain size halves to an odd number: a sample then
    starts in one plane's tail and the planes meet off every alignment"""
    rng = np.random.default_rng(4)
    for name, w, rows in (("a_only", 1, 1), ("uint", 1, 1), ("uint", 3, 1), ("uint", 5, 3), ("rgb_half", 1, 1), ("a_half_rgb_float", 1, 1), ("a_half_rgb_float", 3, 5)):
        ch = channels_of(name)
        table, scanline = table_of(ch, w)
        n = scanline * rows
        assert name == "a_only" or (n // 2) % 2 == 1
        samples = make_samples(ch, w, rows, rng)
        plains = [(0, rows, R.plain_chunk(ch, samples, 0, rows))]
        stream, chunks = build_stream(plains, lambda i: True)
        run_device(ctx, arena, stream, chunks, table, scanline, w, rows, 1, expected(plains[0][2], table, scanline, w), where=(name, w, rows))


@pytest.mark.parametrize("extra", (0, 1, 4, TILE - 1, TILE + 5, 3 * TILE + 61))
def test_a_chunk_over_several_workgroups(ctx, arena, extra):
    """one coded chunk of the kernel's own tile plus `extra` bytes - exactly one tile, past it by one byte and by one dword, two and four
    tiles with tails - whose first and last bytes are read: exr_undo runs as partial sums and apply from one byte past the tile. The
    scanline is longer than its channels, as one with skipped channels is; an odd length puts A on odd bytes."""
    n = TILE + extra
    rng = np.random.default_rng(extra)
    w = 67
    plain = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    table = [(0, dx.EXR_HALF), (n // 2 - 33, dx.EXR_FLOAT), None, (n - 2 * w, dx.EXR_HALF)]
    want = expected(plain, table, n, w)
    seen = set()
    for base in (0, 3):
        stream, chunks = build_stream([(0, 1, plain)], lambda i: True)
        prof = run_device(ctx, arena, stream, chunks, table, n, w, 1, 1, want, base, 0, seen, (extra, base))
        assert ("exr_undo_sums" in prof) == (extra > 0)
    # behind a plain chunk and in front of a small coded one, all in one call
    other = rng.integers(0, 256, 2 * n, dtype=np.uint8).tobytes()
    plains = [(0, 1, other[:n]), (1, 1, plain), (2, 1, other[n:])]
    stream, chunks = build_stream(plains, lambda i: i > 0)
    run_device(ctx, arena, stream, chunks, table, n, w, 3, 1, expected(other[:n] + plain + other[n:], table, n, w), where=(extra, "mixed"))


def test_more_chunks_than_one_launch_takes(ctx, arena):
    """150 one-row chunks, coded and plain in turn and out of window order: three batches of descriptors"""
    rng = np.random.default_rng(8)
    ch = channels_of("rgb_half")
    w, h = 9, 150
    table, scanline = table_of(ch, w)
    samples = make_samples(ch, w, h, rng)
    plains = file_chunks(ch, samples, h, 1)
    want = expected(b"".join(p[2] for p in plains), table, scanline, w)
    order = [int(k) for k in rng.permutation(h)]
    stream, chunks = build_stream([plains[k] for k in order], lambda i: i % 3 != 0)
    prof = run_device(ctx, arena, stream, chunks, table, scanline, w, h, 1, want, where="150 chunks")
    assert prof["exr_texels"] == 3 and prof["exr_undo<wide>"] == 2          # 150 descriptors, 100 of them coded, 64 a launch


def test_six_items_of_an_environment_map(ctx, arena):
    rng = np.random.default_rng(6)
    ch = channels_of("rgba_half")
    w = 5
    table, scanline = table_of(ch, w)
    samples = make_samples(ch, w, 6 * w, rng)
    plains = file_chunks(ch, samples, 6 * w, 16)          # chunks cross the faces
    want = expected(b"".join(p[2] for p in plains), table, scanline, w)
    stream, chunks = build_stream(plains, lambda i: i != 1)
    run_device(ctx, arena, stream, chunks, table, scanline, w, w, 6, want, pad=16, where="envmap")
    # the host form: six images one behind another, through their pitch
    out = np.full((w * 8 + 16) * w * 6, FILL, np.uint8)
    ctx.transfer_bytes(reset=True)
    got = ctx.exr_unpack(stream, chunks, [ABSENT if e is None else e for e in table], scanline, w, w, items=6, row_pitch=w * 8 + 16, out=out)
    assert ctx.transfer_bytes() == (stream.nbytes, 6 * w * w * 8)
    m = got.reshape(6 * w, w * 8 + 16)
    assert np.array_equal(np.ascontiguousarray(m[:, :w * 8]).view("<u2").reshape(6 * w, w, 4), want) and (m[:, w * 8:] == FILL).all()
    assert np.array_equal(stream, build_stream(plains, lambda i: i != 1)[0])          # the caller's stream is not written


def test_host_form_matches_and_leaves_the_stream(ctx):
    rng = np.random.default_rng(10)
    ch = channels_of("a_half_rgb_float")
    for w, h in ((1, 1), (17, 33), (64, 16)):
        table, scanline = table_of(ch, w)
        samples = make_samples(ch, w, h, rng)
        plains = file_chunks(ch, samples, h, 16)
        stream, chunks = build_stream(plains, lambda i: i % 2 == 0)
        before = stream.copy()
        ctx.transfer_bytes(reset=True)
        got = ctx.exr_unpack(stream, chunks, [ABSENT if e is None else e for e in table], scanline, w, h)
        assert ctx.transfer_bytes() == (stream.nbytes, w * h * 8)
        assert np.array_equal(got.view("<u2").reshape(h, w, 4), expected(b"".join(p[2] for p in plains), table, scanline, w)), (w, h)
        assert np.array_equal(stream, before)


# ---- the writer's scanlines -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(SOURCE_BYTES))
def test_pack_matches_the_restatement_on_both_routes(ctx, arena, fmt):
    """NaNs, infinities, overflow and ties among the floats; R32G32B32's alpha is 1.0; the image on and off the wide route's alignment"""
    S = SOURCE_BYTES[fmt]
    rng = np.random.default_rng(fmt)
    seen = set()
    for w, h in ((1, 1), (3, 2), (4, 3), (5, 5), (64, 3), (65, 2), (260, 17)):
        for pad, base in ((0, 0), (16, 0), (4, 0), (0, 2)):
            pitch = w * S + pad
            px = writer_pixels(fmt, w, h, pitch, rng)
            tight = np.ascontiguousarray(px[:, :w * S])
            want = np.frombuffer(R.pack_rows(tight, w, h, fmt), np.uint8)
            ctx.upload(arena.d, px.reshape(-1), sync=True)
            ctx.upload(arena.s, np.full(want.size + base + 32, FILL, np.uint8), sync=True)
            ctx.profile_begin()
            ctx.exr_pack_device(dx.device_image(arena.d, w, h, fmt, pitch), arena.s + base, want.size)
            prof = _marks(ctx.profile_end())
            got = np.zeros(want.size + base + 32, np.uint8)
            ctx.download(got, arena.s, sync=True)
            assert np.array_equal(got[base:base + want.size], want), (fmt, w, h, pad, base)
            assert (got[:base] == FILL).all() and (got[base + want.size:] == FILL).all()
            wide = w % 4 == 0 and (arena.s + base) % 8 == 0 and arena.d % 16 == 0 and pitch % 16 == 0
            assert prof == {"exr_pack<wide>" if wide else "exr_pack<narrow>": 1}, (prof, fmt, w, h, pad, base)
            seen.update(prof)
        if fmt == R.RGB32F:
            assert (want.view("<u2").reshape(h, 4, w)[:, 0] == 0x3C00).all()          # the A plane
    assert seen == {"exr_pack<wide>", "exr_pack<narrow>"}
    # the host form, through a pitch: the rows up, 8 bytes a texel down, nothing behind them touched
    w, h = 65, 5
    px = writer_pixels(fmt, w, h, w * S + 8, rng)
    out = np.full(w * h * 8 + 16, FILL, np.uint8)
    ctx.transfer_bytes(reset=True)
    got = ctx.exr_pack(px, w, h, fmt, row_pitch=w * S + 8, out=out)
    assert ctx.transfer_bytes() == ((w * S + 8) * (h - 1) + w * S, w * h * 8)
    assert got[:w * h * 8].tobytes() == R.pack_rows(np.ascontiguousarray(px[:, :w * S]), w, h, fmt) and (got[w * h * 8:] == FILL).all()


def test_writer_fixture_holds_the_special_patterns():
    px = writer_pixels(R.RGBA32F, 260, 17, 260 * 16, np.random.default_rng(R.RGBA32F)).view("<u4")
    assert set(EDGE_FLOATS.tolist()) <= set(px.reshape(-1).tolist())


# ---- HRESULTs -------------------------------------------------------------------------------------------------------------------------------
def test_hresults_come_in_the_stated_order(ctx):
    lib, h = ctx._lib, ctx._h
    dev = ctx.device_alloc(8192)
    try:
        def image(w, hgt, fmt=RGBA16F, pitch=None, ptr=dev + 4096):
            pitch = w * 8 if pitch is None else pitch
            return dx.Image(w, hgt, fmt, pitch, pitch * max(hgt, 1), ptr)

        def unpack(stream, size, chunks, table, scanline, imgs, count=None, host=False):
            fn = lib.dxtex_exr_unpack if host else lib.dxtex_exr_unpack_device
            ch = None if chunks is None else (dx.ExrChunk * max(1, len(chunks)))(*[dx.ExrChunk(*c) for c in chunks])
            tab = None if table is None else (dx.ExrChannel * 4)(*[dx.ExrChannel(*c) for c in table])
            arr = None if imgs is None else (dx.Image * max(1, len(imgs)))(*imgs)
            return fn(h, stream, size, ch, 0 if chunks is None else len(chunks), tab, scanline, arr, (0 if imgs is None else len(imgs)) if count is None else count)

        def pack(img, stream, size, host=False):
            fn = lib.dxtex_exr_pack if host else lib.dxtex_exr_pack_device
            return fn(h, None if img is None else ctypes.byref(img), stream, size)

        HALF = dx.EXR_HALF
        table = [(0, HALF), (8, HALF), (16, HALF), (24, HALF)]          # a 4-wide scanline of 32 bytes
        good = [(0, 128, 0, 4, 1)]
        ctx.profile_begin()
        # E_POINTER beats everything
        assert unpack(None, 0, [], None, 0, None) == E_POINTER and unpack(dev, 0, None, None, 0, None) == E_POINTER
        assert unpack(dev, 0, [], None, 0, None) == E_POINTER and unpack(dev, 0, [], [(0, 9)] * 4, 0, None) == E_POINTER
        assert unpack(dev, 128, good, table, 32, [image(4, 4, ptr=None)]) == E_POINTER
        assert pack(None, dev, 0) == E_POINTER and pack(image(0, 4, 28, ptr=None), dev, 0) == E_POINTER and pack(image(0, 4, 28), None, 0) == E_POINTER
        # E_INVALIDARG for the arguments beats a format outside the table
        assert unpack(dev, 128, [], table, 32, [image(4, 4, 28)]) == E_INVALIDARG                      # no chunks
        assert unpack(dev, 128, good, table, 32, [image(4, 4, 28)], count=0) == E_INVALIDARG           # no items
        assert unpack(dev, 128, good, table, 32, [image(4, 4, 28)] * 7) == E_INVALIDARG                # more than six
        assert unpack(dev, 128, good, table, 32, [image(0, 4, 28)]) == E_INVALIDARG and unpack(dev, 128, good, table, 32, [image(4, 0, 28)]) == E_INVALIDARG
        assert unpack(dev, 128, good, [(0, HALF), (8, 4), (16, HALF), (24, HALF)], 32, [image(4, 4, 28)]) == E_INVALIDARG          # an unknown type
        assert unpack(dev, 128, good, table, 0, [image(4, 4, 28)]) == E_INVALIDARG
        assert pack(image(0, 4, 28), dev, 64) == E_INVALIDARG and pack(image(4, 0, 28), dev, 64) == E_INVALIDARG
        # NOT_SUPPORTED beats the sizes
        for fmt in (28, 2, 6, 11, 34, 0):
            assert unpack(dev, 1, [(0, 999, 9, 9, 7)], [(31, HALF)] * 4, 32, [image(4, 4, fmt, 1)]) == E_NOT_SUPPORTED, fmt
        for fmt in (28, 11, 41, 16, 95, 0):
            assert pack(image(4, 4, fmt, 1), dev, 1) == E_NOT_SUPPORTED, fmt
        # E_INVALIDARG: items of different sizes; an offset in the channel table that leaves a scanline
        assert unpack(dev, 128, good, table, 32, [image(4, 2), image(4, 3, ptr=dev + 6000)]) == E_INVALIDARG
        assert unpack(dev, 128, good, [(0, HALF), (8, HALF), (16, HALF), (25, HALF)], 32, [image(4, 4)]) == E_INVALIDARG
        assert unpack(dev, 128, good, [(0, HALF), (8, HALF), (16, HALF), (17, dx.EXR_FLOAT)], 32, [image(4, 4)]) == E_INVALIDARG
        assert unpack(dev, 128, good, [(0, HALF), (8, HALF), (16, HALF), (33, dx.EXR_UINT)], 32, [image(4, 4)]) == E_INVALIDARG
        assert unpack(dev, 128, good, [(0, HALF), (8, HALF), (16, HALF), (0xFFFFFFF8, HALF)], 32, [image(4, 4)]) == E_INVALIDARG
        assert unpack(dev, 128, good, [(0, HALF), (8, HALF), (16, HALF), (999, dx.EXR_ABSENT)], 32, [image(4, 4)]) == 0          # an absent channel's offset is not read
        # descriptors that leave the stream, are not rows * scanlineBytes long, name rows outside the window, overlap, or carry another flag
        for bad in ([(0, 128, 0, 4, 1)], [(1, 128, 0, 4, 0)], [(200, 32, 0, 1, 0)], [(2 ** 63, 32, 0, 1, 0)]):
            assert unpack(dev, 127 if bad[0][0] == 0 else 128, bad, table, 32, [image(4, 4)]) == E_INVALIDARG, bad
        for bad in ([(0, 96, 0, 4, 1)], [(0, 128, 0, 3, 1)], [(0, 0, 0, 0, 1)], [(0, 128, 1, 4, 1)], [(0, 32, 4, 1, 0)], [(0, 32, 0xFFFFFFFF, 1, 0)], [(0, 128, 0, 4, 2)],
                    [(0, 64, 0, 2, 1), (63, 64, 2, 2, 1)], [(64, 64, 2, 2, 0), (0, 64, 0, 2, 0)]):
            assert unpack(dev, 128, bad, table, 32, [image(4, 4)]) == E_INVALIDARG, bad
        # a pitch below the row; a chunk, or the stream, that overlaps an item
        assert unpack(dev, 128, good, table, 32, [image(4, 4, pitch=31)]) == E_INVALIDARG
        assert unpack(dev + 4096 - 100, 128, good, table, 32, [image(4, 4)]) == E_INVALIDARG
        assert unpack(dev + 4096 + 127, 128, good, table, 32, [image(4, 4)]) == E_INVALIDARG
        assert unpack(dev, 4097, good, table, 32, [image(4, 4)]) == E_INVALIDARG                      # the stream's tail, which no chunk names
        assert unpack(dev, 128, good, table, 32, [image(4, 2, ptr=dev + 4096), image(4, 2, ptr=dev + 64)]) == E_INVALIDARG          # the second item
        assert pack(image(4, 4), dev, 127) == E_INVALIDARG and pack(image(4, 4, pitch=31), dev, 128) == E_INVALIDARG
        assert pack(image(4, 4), dev + 4096 - 4, 128) == E_INVALIDARG and pack(image(4, 4), dev + 4096 + 127, 128) == E_INVALIDARG
        # the host forms check the same things in the same order
        buf, px = np.zeros(128, np.uint8), np.zeros(128, np.uint8)
        himg = dx.Image(4, 4, RGBA16F, 32, 128, px.ctypes.data)
        assert unpack(None, 128, good, table, 32, [himg], host=True) == E_POINTER and unpack(buf.ctypes.data, 128, [], table, 32, [himg], host=True) == E_INVALIDARG
        assert unpack(buf.ctypes.data, 127, good, table, 32, [himg], host=True) == E_INVALIDARG
        assert unpack(buf.ctypes.data, 128, good, table, 32, [dx.Image(4, 4, 28, 16, 64, px.ctypes.data)], host=True) == E_NOT_SUPPORTED
        assert pack(himg, buf.ctypes.data, 127, host=True) == E_INVALIDARG and pack(dx.Image(4, 4, 28, 16, 64, px.ctypes.data), buf.ctypes.data, 128, host=True) == E_NOT_SUPPORTED
        assert _marks(ctx.profile_end()) == {"exr_undo<wide>": 1, "exr_texels": 1}          # only the one call that was in order reached a kernel
        # and with everything in order: a stream longer than its chunks is fine
        assert unpack(dev, 4096, good, table, 32, [image(4, 4)]) == 0 and pack(image(4, 4), dev, 4096) == 0
        assert unpack(buf.ctypes.data, 128, good, table, 32, [himg], host=True) == 0 and pack(himg, buf.ctypes.data, 128, host=True) == 0
        ctx.synchronize()
    finally:
        ctx.device_free(dev)
