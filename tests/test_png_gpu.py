"""PNG texels on the GPU (dxtex_png_unpack / dxtex_png_pack and their _device forms) against tests/png_ref.py, the restatement of
Auxiliary/DirectXTexPNG.cpp's per-texel rules: pixels and file rows byte for byte, the bytes around them untouched, on both routes of each
kernel, asserted by profile mark."""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALIDARG, E_POINTER, E_NOT_SUPPORTED = 0x80070057 - (1 << 32), 0x80004003 - (1 << 32), 0x80070032 - (1 << 32)
FILL = 0xA5
KINDS = sorted(R.TYPE_OF)
# where a byte of sub-byte texels, a group of four, a wave and a workgroup each have a tail
WIDTHS, HEIGHTS = (1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257), (1, 2, 5)
PITCH_PADS = (0, 4, 3)
PALETTE_LENGTHS = (1, 2, 16, 255, 256)


def span_align(dwords):
    return 16 if dwords % 4 == 0 else 8 if dwords % 2 == 0 else 4


def wide_rule(kind):
    """csrc/png.hip's rule for a kind: (texels a lane takes, the alignment asked of the stream's base, of the image's base and pitch)"""
    bits, D = R.file_bits(kind), R.IMAGE_BYTES[kind]
    if bits < 8:
        group = 8 // bits
        return group, 1, (group * D if group * D < 4 else span_align(group * D // 4))
    return 4, span_align(bits // 8), span_align(D)


def image_format(kind, bgr):
    ct, depth = R.TYPE_OF[kind]
    return R.metadata(ct, depth, (R.FLAGS_BGR if bgr else 0) | R.FLAGS_IGNORE_SRGB)[0]


def _marks(prof, prefix):
    return {k: v[1] for k, v in prof.items() if k.startswith(prefix)}


class Arena:
    """Two device allocations reused by every case of a test: the stream's and the image's."""
    def __init__(self, ctx, stream_bytes, image_bytes):
        self.ctx = ctx
        self.s = ctx.device_alloc(stream_bytes + 256)
        self.d = ctx.device_alloc(image_bytes + 256)

    def close(self):
        self.ctx.device_free(self.s)
        self.ctx.device_free(self.d)


@pytest.fixture
def arena(ctx):
    a = Arena(ctx, max(WIDTHS) * max(HEIGHTS) * 8, (max(WIDTHS) * 8 + 32) * max(HEIGHTS))
    yield a
    a.close()


_cases = {}


def _case(kind, w, h, bgr, entries):
    """(rows, palette words or None, the restatement's tight pixels (h, w * D)); computed once per case. Indices reach past a palette
    shorter than the kind's range: the rows are random bytes."""
    key = (kind, w, h, bgr, entries)
    if key not in _cases:
        rng = np.random.default_rng(kind * 7919 + w * 31 + h)
        rows = rng.integers(0, 256, R.row_bytes(kind, w) * h, dtype=np.uint8)
        pal = None
        if R.TYPE_OF[kind][0] == 3:
            pal = R.palette_words(rng.integers(0, 256, 3 * entries, dtype=np.uint8).tobytes(), rng.integers(0, 256, (entries + 1) // 2, dtype=np.uint8).tobytes())
        _cases[key] = (rows, pal, R.expand(rows.tobytes(), w, h, kind, bgr, pal))
    return _cases[key]


def _unpack_case(ctx, arena, kind, w, h, bgr, entries, base, pad, seen):
    D = R.IMAGE_BYTES[kind]
    rows, pal, want = _case(kind, w, h, bgr, entries)
    pitch = w * D + pad
    image_bytes = pitch * h
    ctx.upload(arena.s, np.full(rows.nbytes + 64, FILL, np.uint8), sync=True)
    ctx.upload(arena.s + base, rows, sync=True)
    ctx.upload(arena.d, np.full(image_bytes + 32, FILL, np.uint8), sync=True)
    ctx.profile_begin()
    ctx.png_unpack_device(arena.s + base, rows.nbytes, kind, dx.device_image(arena.d, w, h, image_format(kind, bgr), pitch), dx.PNG_BGR if bgr else 0, pal)
    prof = ctx.profile_end()
    got = np.zeros(image_bytes + 32, np.uint8)
    ctx.download(got, arena.d, sync=True)
    where = (kind, w, h, bgr, entries, base, pad)
    m = got[:image_bytes].reshape(h, pitch)
    assert np.array_equal(m[:, :w * D], want), where
    assert (m[:, w * D:] == FILL).all() and (got[image_bytes:] == FILL).all(), ("bytes outside the rows were written", where)
    back = np.zeros(rows.nbytes + 64, np.uint8)
    ctx.download(back, arena.s, sync=True)
    assert np.array_equal(back[base:base + rows.nbytes], rows) and (back[:base] == FILL).all() and (back[base + rows.nbytes:] == FILL).all(), ("the stream was written", where)
    group, stream_align, image_align = wide_rule(kind)
    wide = w % group == 0 and (arena.s + base) % stream_align == 0 and arena.d % image_align == 0 and pitch % image_align == 0
    mark = "png_unpack<wide>" if wide else "png_unpack<narrow>"
    assert _marks(prof, "png_") == {mark: 1}, (prof, where)
    seen.add(mark)


@pytest.mark.parametrize("bgr", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_unpack_matches_the_restatement(ctx, arena, kind, bgr):
    """Every size, stream base and destination pitch: pixels, the bytes around stream and image, and the route's profile mark. A palette
    kind takes its palette's length from PALETTE_LENGTHS in turn, so indices at and past its end occur."""
    seen, n = set(), 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for base in (0, 1, 2, 3):
                for pad in PITCH_PADS:
                    _unpack_case(ctx, arena, kind, w, h, bgr, PALETTE_LENGTHS[n % len(PALETTE_LENGTHS)], base, pad, seen)
                    n += 1
    assert seen == {"png_unpack<wide>", "png_unpack<narrow>"}          # both routes have run


@pytest.mark.parametrize("entries", PALETTE_LENGTHS)
def test_palette_lengths_and_indices_past_the_end(ctx, arena, entries):
    """every palette kind under every palette length on both routes; an index at or past the end gives opaque black"""
    seen = set()
    for kind in (R.P1, R.P2, R.P4, R.P8):
        for w, base in ((64, 0), (257, 0), (65, 1), (8, 0)):
            for bgr in (False, True):
                _unpack_case(ctx, arena, kind, w, 5, bgr, entries, base, 0, seen)
        rows, pal, want = _case(R.P8, 257, 5, False, entries)
        past = rows.reshape(5, 257) >= entries
        assert (want.reshape(5, 257, 4)[past] == (0, 0, 0, 255)).all() and (entries == 256 or past.any())
    assert seen == {"png_unpack<wide>", "png_unpack<narrow>"}


# ---- pack -----------------------------------------------------------------------------------------------------------------------------
def _pack_case(ctx, arena, fmt, w, h, pad, base, seen):
    ct, depth, S, F = R.WRITER[fmt]
    rng = np.random.default_rng(fmt * 1000 + w * 9 + h)
    px = rng.integers(0, 256, (h, w * S), dtype=np.uint8)
    want = R.pack_rows(px, w, h, fmt).reshape(-1)
    pitch = w * S + pad
    src = np.full((h, pitch), 0x5A, np.uint8)
    src[:, :w * S] = px
    ctx.upload(arena.d, src.reshape(-1), sync=True)
    ctx.upload(arena.s, np.full(want.size + 64, FILL, np.uint8), sync=True)
    ctx.profile_begin()
    ctx.png_pack_device(dx.device_image(arena.d, w, h, fmt, pitch), arena.s + base, want.size)
    prof = ctx.profile_end()
    got = np.zeros(want.size + 64, np.uint8)
    ctx.download(got, arena.s, sync=True)
    where = (fmt, w, h, pad, base)
    assert np.array_equal(got[base:base + want.size], want), where
    assert (got[:base] == FILL).all() and (got[base + want.size:] == FILL).all(), ("bytes outside the rows were written", where)
    image_align, stream_align = span_align(S), span_align(F)
    wide = w % 4 == 0 and (arena.s + base) % stream_align == 0 and arena.d % image_align == 0 and pitch % image_align == 0
    mark = "png_pack<wide>" if wide else "png_pack<narrow>"
    assert _marks(prof, "png_") == {mark: 1}, (prof, where)
    seen.add(mark)


@pytest.mark.parametrize("fmt", list(R.WRITER))
def test_pack_matches_the_writer(ctx, arena, fmt):
    seen = set()
    for w in WIDTHS:
        for h in HEIGHTS:
            for pad in (0, 16, 4, 3):          # padded source pitches that keep the rows' alignment, and two that do not
                for base in (0, 1, 2, 3):
                    _pack_case(ctx, arena, fmt, w, h, pad, base, seen)
    assert seen == {"png_pack<wide>", "png_pack<narrow>"}


# ---- host forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_host_unpack_gives_the_device_forms_bytes_and_moves_the_files_bytes(ctx, kind):
    D = R.IMAGE_BYTES[kind]
    for (w, h, bgr, pad, entries) in ((8, 2, False, 0, 256), (5, 5, True, 3, 2), (257, 2, True, 4, 16), (64, 5, False, 16, 255)):
        rows, pal, want = _case(kind, w, h, bgr, entries)          # what the device form was held to above
        pitch = w * D + pad
        out = np.full(pitch * h + 32, FILL, np.uint8)
        ctx.transfer_bytes(reset=True)
        ctx.profile_begin()
        # surplus bytes behind the image's rows are ignored and not moved
        got = ctx.png_unpack(np.concatenate([rows, np.full(7, 0x11, np.uint8)]), w, h, kind, image_format(kind, bgr), dx.PNG_BGR if bgr else 0, pal, row_pitch=pitch, out=out)
        prof = ctx.profile_end()
        up, down = ctx.transfer_bytes()
        m = got[:pitch * h].reshape(h, pitch)
        assert np.array_equal(m[:, :w * D], want), (kind, w, h)
        assert (m[:, w * D:] == FILL).all() and (got[pitch * h:] == FILL).all(), ("bytes outside the rows were written", kind, w, h)
        assert (up, down) == (rows.nbytes, w * h * D), (kind, w, h, up, down)          # the rows up, the rows' texels down
        assert _marks(prof, "png_") == {"png_unpack<wide>" if w % wide_rule(kind)[0] == 0 else "png_unpack<narrow>": 1}


@pytest.mark.parametrize("fmt", list(R.WRITER))
def test_host_pack_gives_the_device_forms_bytes(ctx, fmt):
    ct, depth, S, F = R.WRITER[fmt]
    for (w, h) in ((4, 2), (5, 5), (257, 2)):
        px = np.random.default_rng(fmt + w).integers(0, 256, (h, w * S), dtype=np.uint8)
        want = R.pack_rows(px, w, h, fmt).reshape(-1)
        out = np.full(want.size + 16, FILL, np.uint8)
        ctx.transfer_bytes(reset=True)
        got = ctx.png_pack(px, w, h, fmt, row_pitch=w * S, out=out)
        assert np.array_equal(got[:want.size], want) and (got[want.size:] == FILL).all(), (fmt, w, h)          # no byte behind the rows is touched
        assert ctx.transfer_bytes() == (w * h * S, want.size)


# ---- HRESULTs -------------------------------------------------------------------------------------------------------------------------
def test_hresults_come_in_the_stated_order(ctx):
    """E_POINTER, then E_INVALIDARG for the arguments, then NOT_SUPPORTED, then E_INVALIDARG for the sizes: each call carries every later
    error as well. None reaches a kernel."""
    lib, h = ctx._lib, ctx._h
    dev = ctx.device_alloc(4096)
    pal = np.zeros(256, np.uint32)
    try:
        def image(w, hgt, fmt, pitch, ptr=dev + 2048):
            return dx.device_image(ptr, w, hgt, fmt, pitch, pitch * max(hgt, 1))

        def unpack(stream, size, kind, img, flags=0, palette=None, count=0, host=False):
            fn = lib.dxtex_png_unpack if host else lib.dxtex_png_unpack_device
            return fn(h, stream, size, kind, flags, palette, count, None if img is None else ctypes.byref(img))

        def pack(img, stream, size, host=False):
            fn = lib.dxtex_png_pack if host else lib.dxtex_png_pack_device
            return fn(h, None if img is None else ctypes.byref(img), stream, size)

        P = pal.ctypes.data
        ctx.profile_begin()
        # E_POINTER beats an unknown kind, a mismatched format and a zero size
        assert unpack(None, 0, 99, image(0, 4, R.R32F, 0)) == E_POINTER and unpack(dev, 0, 99, None) == E_POINTER
        assert unpack(dev, 0, 99, image(0, 4, R.R32F, 0, ptr=None)) == E_POINTER
        assert pack(None, dev, 0) == E_POINTER and pack(image(0, 4, R.R32F, 0), None, 0) == E_POINTER and pack(image(0, 4, R.R32F, 0, ptr=None), dev, 0) == E_POINTER
        # E_INVALIDARG for the arguments beats a mismatched format: an unknown kind, unknown flag bits, a palette missing, unasked for or of a
        # wrong count, a zero size
        assert unpack(dev, 64, 15, image(4, 4, R.R32F, 16)) == E_INVALIDARG
        assert unpack(dev, 64, dx.PNG_RGB8, image(4, 4, R.R32F, 16), flags=2) == E_INVALIDARG and unpack(dev, 64, dx.PNG_RGB8, image(4, 4, R.R32F, 16), flags=0x80000001) == E_INVALIDARG
        assert unpack(dev, 64, dx.PNG_P8, image(4, 4, R.R32F, 16)) == E_INVALIDARG and unpack(dev, 64, dx.PNG_RGB8, image(4, 4, R.R32F, 16), palette=P, count=4) == E_INVALIDARG
        assert unpack(dev, 64, dx.PNG_P8, image(4, 4, R.R32F, 16), palette=P, count=0) == E_INVALIDARG and unpack(dev, 64, dx.PNG_P8, image(4, 4, R.R32F, 16), palette=P, count=257) == E_INVALIDARG
        for w, hgt, size in ((0, 4, 64), (4, 0, 64), (4, 4, 0)):
            assert unpack(dev, size, dx.PNG_RGB8, image(w, hgt, R.R32F, 16)) == E_INVALIDARG and pack(image(w, hgt, R.R32F, 16), dev, size) == E_INVALIDARG
        # NOT_SUPPORTED beats a short stream and a short pitch: every pair outside the tables
        for kind, flags, fmt in ((dx.PNG_G8, 0, R.RGBA8), (dx.PNG_G1, 0, R.R16), (dx.PNG_G16, 0, R.R8), (dx.PNG_GA8, 0, R.RGBA8_SRGB), (dx.PNG_GA8, 0, R.BGRA8), (dx.PNG_GA16, 0, R.RGBA8),
                                 (dx.PNG_RGB8, 0, R.BGRX8), (dx.PNG_RGB8, 1, R.RGBA8), (dx.PNG_RGB8, 1, R.BGRA8), (dx.PNG_RGBA8, 1, R.BGRX8), (dx.PNG_RGBA8, 0, R.BGRA8_SRGB),
                                 (dx.PNG_RGB16, 0, R.RGBA8), (dx.PNG_RGBA16, 1, R.BGRA8), (dx.PNG_RGBA8, 0, R.RGBA32F)):
            assert unpack(dev, 1, kind, image(4, 4, fmt, 1), flags=flags) == E_NOT_SUPPORTED, (kind, flags, fmt)
        assert unpack(dev, 1, dx.PNG_P4, image(4, 4, R.BGRA8, 1), flags=1, palette=P, count=16) == E_NOT_SUPPORTED
        for fmt in (R.RGBA32F, R.R32F, R.BC1, 10, 49):
            assert pack(image(4, 4, fmt, 1), dev, 1) == E_NOT_SUPPORTED, fmt
        # E_INVALIDARG: fewer bytes than the rows, a pitch below the row, overlap
        assert unpack(dev, 47, dx.PNG_RGB8, image(4, 4, R.RGBA8, 16)) == E_INVALIDARG and unpack(dev, 48, dx.PNG_RGB8, image(4, 4, R.RGBA8, 15)) == E_INVALIDARG
        assert unpack(dev, 3, dx.PNG_G1, image(4, 4, R.R8, 4)) == E_INVALIDARG and unpack(dev, 4, dx.PNG_G1, image(4, 4, R.R8, 3)) == E_INVALIDARG
        assert pack(image(4, 4, R.BGRX8, 16), dev, 47) == E_INVALIDARG and pack(image(4, 4, R.BGRX8, 15), dev, 48) == E_INVALIDARG
        assert unpack(dev + 2048 + 60, 48, dx.PNG_RGB8, image(4, 4, R.RGBA8, 16)) == E_INVALIDARG          # the rows start inside the image's last row
        assert pack(image(4, 4, R.BGRX8, 16), dev + 2048 - 4, 48) == E_INVALIDARG              # the last byte is the image's first
        # the host forms check the same things in the same order
        buf, px = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
        himg = dx.Image(4, 4, R.RGBA8, 16, 64, px.ctypes.data)
        assert unpack(buf.ctypes.data, 47, 15, himg, host=True) == E_INVALIDARG and unpack(buf.ctypes.data, 47, dx.PNG_G8, himg, host=True) == E_NOT_SUPPORTED
        assert unpack(buf.ctypes.data, 47, dx.PNG_RGB8, himg, host=True) == E_INVALIDARG and unpack(None, 48, dx.PNG_RGB8, himg, host=True) == E_POINTER
        assert pack(himg, buf.ctypes.data, 63, host=True) == E_INVALIDARG
        assert _marks(ctx.profile_end(), "png_") == {}          # no refusal reached a kernel
        # and with everything in order: a stream longer than the rows is fine
        assert unpack(dev, 64, dx.PNG_RGB8, image(4, 4, R.RGBA8, 16)) == 0 and pack(image(4, 4, R.RGBA8, 16), dev, 64) == 0
        assert unpack(dev, 64, dx.PNG_GA8, image(4, 4, R.BGRA8, 16), flags=1) == 0          # g, g, g, a is the same in either order
        assert unpack(buf.ctypes.data, 48, dx.PNG_RGB8, himg, host=True) == 0 and pack(himg, buf.ctypes.data, 64, host=True) == 0
        ctx.synchronize()
    finally:
        ctx.device_free(dev)
