"""TIFF strips and tiles on the GPU (dxtex_tiff_unpack / dxtex_tiff_pack and their _device forms) against tests/tiff_ref.py: pixels and rows byte
for byte - nothing here rounds, and predictor 3 moves bits - the bytes around them untouched, both routes of tiff_undo, tiff_texels and
tiff_pack asserted by profile mark, and the no-kernel route by the absence of one."""
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tiff_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALIDARG, E_POINTER, E_NOT_SUPPORTED = 0x80070057 - (1 << 32), 0x80004003 - (1 << 32), 0x80070032 - (1 << 32)
FILL = 0xA5
TILE = dx.TIFF_UNDO_TILE
ARENA = 1 << 20
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 257)
# kind, predictor, big-endian: every bit depth, every sample count, all three predictors, both byte orders
KINDS = [(T.GREY1, 1, False), (T.GREY4, 1, True), (T.PAL1, 1, False), (T.PAL4, 1, False), (T.PAL8, 2, False), (T.GREY8, 2, False), (T.GREY16, 2, True), (T.GREY16, 1, True),
         (T.GREY32F, 3, False), (T.RGB8, 2, False), (T.RGBA8, 2, True), (T.RGB16, 2, True), (T.RGBA16, 2, False), (T.RGB16, 1, True), (T.RGB32F, 3, True), (T.RGBA32F, 3, False),
         (T.RGB32F, 1, True), (T.RGB8, 1, False)]


def _marks(prof, prefix="tiff_"):
    return {k: v[1] for k, v in prof.items() if k.startswith(prefix)}


def samples_of(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    bits, S, _, _ = T.KINDS[kind]
    if bits == 32:
        return rng.integers(0, 1 << 32, (h, w, S), dtype=np.uint32).view(np.float32)          # every bit pattern: nothing may round or quiet a NaN
    return rng.integers(0, 1 << bits, (h, w, S), dtype=np.uint16 if bits == 16 else np.uint8)


def case(kind, h, w, seed, predictor=1, **kw):
    """a file of this kind and layout -> (stream, segments, layout, palette words, format, the image's tight rows)"""
    bits = T.KINDS[kind][0]
    cm = [int(v) for v in np.random.default_rng(seed).integers(0, 65536, 3 << bits)] if kind in (T.PAL1, T.PAL4, T.PAL8) else None
    data = T.build(samples_of(kind, h, w, seed), kind, compression=T.DEFLATE, predictor=predictor, colormap=cm, **kw)
    hr, want = T.decode(data)
    assert hr == 0
    info = want["info"]
    stream, segs = T.segments(info)
    return np.frombuffer(stream, np.uint8), segs, T.layout_of(info), T.palette_of(info), want["format"], np.frombuffer(want["pixels"], np.uint8).reshape(h, -1)


class Arena:
    def __init__(self, ctx):
        self.ctx = ctx
        self.s = ctx.device_alloc(ARENA + 256)
        self.d = ctx.device_alloc(ARENA + 256)

    def close(self):
        self.ctx.device_free(self.s)
        self.ctx.device_free(self.d)


@pytest.fixture
def arena(ctx):
    a = Arena(ctx)
    yield a
    a.close()


def run_device(ctx, arena, c, base=0, pad=0):
    """the _device form: the pixels, and the bytes between and behind the rows untouched; returns the marks"""
    stream, segs, layout, palette, fmt, want = c
    h, row = want.shape
    pitch = row + pad
    assert base + stream.nbytes <= ARENA and pitch * h + 32 <= ARENA
    ctx.upload(arena.s + base, stream, sync=True)
    ctx.upload(arena.d, np.full(pitch * h + 32, FILL, np.uint8), sync=True)
    ctx.profile_begin()
    ctx.tiff_unpack_device(arena.s + base, stream.nbytes, segs, layout, dx.device_image(arena.d, layout[0], h, fmt, pitch), palette)
    prof = _marks(ctx.profile_end())
    got = np.zeros(pitch * h + 32, np.uint8)
    ctx.download(got, arena.d, sync=True)
    rows = got[:pitch * h].reshape(h, pitch)
    assert np.array_equal(rows[:, :row], want), (layout, segs[:3], base, pad)
    assert (rows[:-1, row:] == FILL).all() and (got[pitch * (h - 1) + row:] == FILL).all(), (layout, base, pad)
    return prof


@pytest.mark.parametrize("kind,predictor,be", KINDS)
def test_widths_heights_and_rows_per_strip(ctx, arena, kind, predictor, be):
    seed = 0
    for w in WIDTHS:
        for h in (1, 2, 5):
            for rps in sorted({1, 2, h}):
                seed += 1
                prof = run_device(ctx, arena, case(kind, h, w, seed, predictor, big_endian=be, rows_per_strip=rps))
                assert sum(v for k, v in prof.items() if k.startswith("tiff_texels")) == 1, prof          # strips that follow one another share a descriptor
                assert (sum(v for k, v in prof.items() if k.startswith("tiff_undo")) == 1) == (predictor != 1), prof


@pytest.mark.parametrize("kind,predictor,be", [k for k in KINDS if k[1] != 1])
def test_a_row_of_one_pass_and_one_texel_more(ctx, arena, kind, predictor, be):
    """a row of exactly what a workgroup scans in one pass (kTiffUndoTile bytes), and one texel more, which the carry reaches; then several passes"""
    bits, S, _, _ = T.KINDS[kind]
    texel = S * bits // 8
    assert TILE % texel == 0
    for w in (TILE // texel, TILE // texel + 1, 2 * TILE // texel + 5):
        run_device(ctx, arena, case(kind, 2, w, w, predictor, big_endian=be))
    if S > 1:          # separate planes: a row is one sample a pixel
        for w in (TILE * 8 // bits, TILE * 8 // bits + 1):
            run_device(ctx, arena, case(kind, 2, w, w, predictor, big_endian=be, planar=True))


@pytest.mark.parametrize("kind,predictor,be", KINDS)
def test_tiles_and_separate_planes(ctx, arena, kind, predictor, be):
    S = T.KINDS[kind][1]
    for (w, h) in ((1, 1), (16, 16), (20, 18)):
        for planar in ((False, True) if S > 1 else (False,)):
            prof = run_device(ctx, arena, case(kind, h, w, w + h, predictor, big_endian=be, tile=(16, 16), planar=planar))
            assert sum(prof.values()) == (1 if predictor == 1 else 2), prof          # every tile of every plane in one launch each
    if S > 1:
        for (w, h, rps) in ((5, 5, 2), (65, 2, 1), (257, 5, 5)):
            run_device(ctx, arena, case(kind, h, w, w, predictor, big_endian=be, planar=True, rows_per_strip=rps))


def test_more_segments_than_one_batch(ctx, arena):
    """9 x 9 tiles of 16 x 16 over three planes: 243 descriptors, four launches of each kernel"""
    prof = run_device(ctx, arena, case(T.RGB16, 130, 140, 1, 2, big_endian=True, tile=(16, 16), planar=True))
    assert prof == {"tiff_undo<wide>": 4, "tiff_texels<wide>": 4}, prof
    prof = run_device(ctx, arena, case(T.GREY8, 70, 9, 2, 2, tile=(16, 16)))
    assert sum(prof.values()) == 2, prof


@pytest.mark.parametrize("base", (0, 1, 4))
@pytest.mark.parametrize("pad", (0, 3, 4))
def test_stream_bases_pitch_pads_and_routes(ctx, arena, base, pad):
    """width 64: every row is a multiple of 16 bytes, so the routes follow the stream's base and the image's pitch alone"""
    for kind, predictor, be in KINDS:
        bits, S, _, ib = T.KINDS[kind]
        c = case(kind, 5, 64, base * 8 + pad, predictor, big_endian=be, rows_per_strip=2)
        prof = run_device(ctx, arena, c, base, pad)
        row_bytes = c[1][0][5]
        access = 4 if ib == 12 else ib
        assert ("tiff_texels<wide>" in prof) == (pad % access == 0) and ("tiff_texels<narrow>" in prof) == (pad % access != 0), (kind, prof)
        if predictor != 1:
            wide = base == 0 and row_bytes % 16 == 0
            assert ("tiff_undo<wide>" in prof) == wide and ("tiff_undo<narrow>" in prof) == (not wide), (kind, row_bytes, prof)
    # tiles, whose rows start on multiples of 16 whatever the image's width
    prof = run_device(ctx, arena, case(T.RGBA8, 18, 20, 3, 2, tile=(16, 16)), base, pad)
    assert ("tiff_undo<wide>" in prof) == (base == 0), prof


NATIVE = (T.GREY8, T.GREY16, T.GREY32F, T.RGBA8, T.RGBA16, T.RGBA32F, T.RGB32F)


@pytest.mark.parametrize("kind", NATIVE)
def test_a_file_that_is_its_image_runs_no_kernel(ctx, arena, kind):
    extra = 2 if T.KINDS[kind][1] == 4 else None
    for (w, h, rps, base, pad) in ((5, 5, 2, 0, 0), (65, 2, 1, 1, 3), (64, 5, 5, 4, 4)):
        c = case(kind, h, w, w, 1, rows_per_strip=rps, extra=extra, big_endian=(kind in (T.GREY8, T.RGBA8)))
        assert run_device(ctx, arena, c, base, pad) == {}, kind
    # the same kind takes the kernel as soon as something is left to do: tiles, the other byte order, an alpha to force
    assert run_device(ctx, arena, case(kind, 5, 5, 1, 1, tile=(16, 16), extra=extra)) == {"tiff_texels<wide>": 1}
    if kind not in (T.GREY8, T.RGBA8):
        assert run_device(ctx, arena, case(kind, 5, 5, 1, 1, big_endian=True, extra=extra)) == {"tiff_texels<wide>": 1}
    if extra:
        assert run_device(ctx, arena, case(kind, 5, 5, 1, 1, extra=0)) == {"tiff_texels<wide>": 1}
    if kind == T.GREY8:
        assert run_device(ctx, arena, case(kind, 5, 5, 1, 1, white_is_zero=True)) == {"tiff_texels<wide>": 1}


def test_white_is_zero_opaque_and_premultiplied(ctx, arena):
    for kind in (T.GREY1, T.GREY4, T.GREY8, T.GREY16):
        run_device(ctx, arena, case(kind, 5, 65, kind, 1, white_is_zero=True))
    for kind in (T.RGBA8, T.RGBA16, T.RGBA32F):
        for extra in (0, 1, 2, None):
            for planar in (False, True):
                run_device(ctx, arena, case(kind, 3, 17, kind, 1, extra=extra, planar=planar))


def test_the_stream_is_left_undone_and_little_endian(ctx, arena):
    c = case(T.GREY16, 3, 70, 1, 2, big_endian=True)
    run_device(ctx, arena, c)
    got = np.zeros(c[0].nbytes, np.uint8)
    ctx.download(got, arena.s, sync=True)
    assert np.array_equal(got, c[5].reshape(-1))          # grey 16: the undone little-endian stream is the image
    c = case(T.GREY32F, 2, 9, 2, 3)
    run_device(ctx, arena, c)
    ctx.download(got[:c[0].nbytes], arena.s, sync=True)
    planes = got[:c[0].nbytes].reshape(2, 4, 9)          # predictor 3: four byte planes a row, the most significant first, never regrouped
    assert np.array_equal(np.ascontiguousarray(planes[:, ::-1].transpose(0, 2, 1)).reshape(-1), c[5].reshape(-1))


def test_host_pointer_forms(ctx):
    for kind, predictor, be in KINDS:
        for (w, h, kw, pad) in ((65, 5, dict(rows_per_strip=2), 0), (20, 18, dict(tile=(16, 16)), 3)):
            stream, segs, layout, palette, fmt, want = case(kind, h, w, w, predictor, big_endian=be, **kw)
            before = stream.copy()
            row = want.shape[1]
            ctx.transfer_bytes(reset=True)
            out = ctx.tiff_unpack(stream, segs, layout, fmt, palette, row_pitch=row + pad, out=np.full((row + pad) * h, FILL, np.uint8))
            assert ctx.transfer_bytes() == (stream.nbytes, row * h)          # up goes exactly the stream, down exactly the rows' texels
            rows = out.reshape(h, row + pad)
            assert np.array_equal(rows[:, :row], want) and (rows[:, row:] == FILL).all() and np.array_equal(stream, before), (kind, kw)


PACK = [(T.R8_UNORM, False), (T.R16_UNORM, False), (T.R32_FLOAT, False), (T.R8G8B8A8_UNORM, False), (T.R8G8B8A8_UNORM_SRGB, False), (T.R16G16B16A16_UNORM, False),
        (T.R32G32B32_FLOAT, False), (T.R32G32B32A32_FLOAT, False), (T.B8G8R8A8_UNORM, True), (T.B8G8R8A8_UNORM_SRGB, True), (T.B8G8R8X8_UNORM, True), (T.B8G8R8X8_UNORM_SRGB, True)]


@pytest.mark.parametrize("fmt,kernel", PACK)
def test_pack(ctx, arena, fmt, kernel):
    rng = np.random.default_rng(fmt)
    ib, fb = T.SOURCES[fmt][3], T.SOURCES[fmt][4]
    for w in WIDTHS + (1024,):
        for (h, pad, base) in ((1, 0, 0), (2, 3, 1), (5, 16, 16), (5, 4, 4)):
            pitch = w * ib + pad
            px = rng.integers(0, 256, pitch * h, dtype=np.uint8)
            want = T.pack_rows(px.tobytes(), w, h, fmt, pitch).reshape(-1)
            ctx.upload(arena.d, px, sync=True)
            ctx.upload(arena.s, np.full(base + want.nbytes + 32, FILL, np.uint8), sync=True)
            ctx.profile_begin()
            ctx.tiff_pack_device(dx.device_image(arena.d, w, h, fmt, pitch), arena.s + base, want.nbytes)
            prof = _marks(ctx.profile_end())
            got = np.zeros(base + want.nbytes + 32, np.uint8)
            ctx.download(got, arena.s, sync=True)
            assert np.array_equal(got[base:base + want.nbytes], want), (fmt, w, h, pad, base)
            assert (got[:base] == FILL).all() and (got[base + want.nbytes:] == FILL).all()
            wide = w % 4 == 0 and pad % 16 == 0 and base % 16 == 0
            assert prof == ({("tiff_pack<wide>" if wide else "tiff_pack<narrow>"): 1} if kernel else {}), (fmt, w, pad, base, prof)
    px = rng.integers(0, 256, (65 * ib + 3) * 5, dtype=np.uint8)
    ctx.transfer_bytes(reset=True)
    out = ctx.tiff_pack(px, 65, 5, fmt, row_pitch=65 * ib + 3)
    assert np.array_equal(out[:65 * 5 * fb], T.pack_rows(px.tobytes(), 65, 5, fmt, 65 * ib + 3).reshape(-1))
    assert ctx.transfer_bytes() == ((65 * ib + 3) * 4 + 65 * ib, 65 * 5 * fb)


def test_argument_checks(ctx, arena):
    stream, segs, layout, palette, fmt, want = case(T.RGB8, 5, 9, 1, 2, rows_per_strip=2)
    ctx.upload(arena.s, stream, sync=True)
    img = dx.device_image(arena.d, 9, 5, fmt)

    def hr(segments=segs, lay=layout, image=img, pal=None, s=arena.s, n=stream.nbytes):
        with pytest.raises(dx.DxtexError) as e:
            ctx.tiff_unpack_device(s, n, segments, lay, image, pal)
        return e.value.hresult

    def with_(i, v):
        return layout[:i] + (v,) + layout[i + 1:]

    assert hr(s=None) == E_POINTER and hr(segments=None) == E_POINTER and hr(lay=None) == E_POINTER and hr(image=None) == E_POINTER
    assert hr(image=dx.device_image(None, 9, 5, fmt)) == E_POINTER
    assert hr(lay=with_(4, T.PAL8)) == E_POINTER          # a palette kind without a palette
    assert hr(segments=[]) == E_INVALIDARG and hr(lay=with_(0, 8)) == E_INVALIDARG and hr(lay=with_(4, 14)) == E_INVALIDARG
    assert hr(lay=with_(2, 16)) == E_INVALIDARG and hr(lay=with_(3, 4)) == E_INVALIDARG and hr(lay=with_(5, 0)) == E_INVALIDARG and hr(lay=with_(5, 4)) == E_INVALIDARG
    assert hr(lay=with_(5, 3)) == E_NOT_SUPPORTED and hr(image=dx.device_image(arena.d, 9, 5, dx.DXGI_FORMAT_B8G8R8A8_UNORM)) == E_NOT_SUPPORTED
    o, fr, rows, fc, cols, rb, plane = segs[0]
    for bad in ((o, fr, 0, fc, cols, rb, plane), (o, fr, 6, fc, cols, rb, plane), (o, 5, 1, fc, cols, rb, plane), (o, fr, rows, 1, cols, rb, plane), (o, fr, rows, fc, 10, rb, plane),
                (o, fr, rows, fc, cols, rb, 1), (o, fr, rows, fc, cols, rb - 1, plane), (stream.nbytes - rb * rows + 1, fr, rows, fc, cols, rb, plane), (1 << 40, fr, rows, fc, cols, rb, plane)):
        assert hr(segments=[bad]) == E_INVALIDARG, bad
    assert hr(segments=[segs[0], segs[0]]) == E_INVALIDARG          # overlap
    assert hr(image=dx.device_image(arena.d, 9, 5, fmt, 35)) == E_INVALIDARG          # a pitch smaller than the row
    assert hr(image=dx.device_image(arena.s + 8, 9, 5, fmt)) == E_INVALIDARG          # the stream overlaps the pixels
    with pytest.raises(dx.DxtexError) as e:
        ctx.tiff_pack_device(dx.device_image(arena.d, 4, 4, dx.DXGI_FORMAT_R16G16B16A16_FLOAT), arena.s, 4096)
    assert e.value.hresult == E_NOT_SUPPORTED
    with pytest.raises(dx.DxtexError) as e:
        ctx.tiff_pack_device(dx.device_image(arena.d, 4, 4, T.B8G8R8X8_UNORM), arena.s, 47)
    assert e.value.hresult == E_INVALIDARG
