"""Truevision TGA texels on the GPU (dxtex_tga_unpack / dxtex_tga_pack and their _device forms) against the reference's .tga reader and
writer (oracle): pixels, alpha answers and file rows byte for byte, on both routes of each kernel, asserted by profile mark."""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_hdr_tga_cpu import tga_header  # noqa: E402

pytestmark = pytest.mark.gpu

E_FAIL, E_INVALIDARG, E_POINTER = 0x80004005 - (1 << 32), 0x80070057 - (1 << 32), 0x80004003 - (1 << 32)
E_NOT_SUPPORTED = 0x80070032 - (1 << 32)
R8, A8, B5G5R5A1, RGBA8, RGBA8_SRGB, BGRA8, BGRA8_SRGB, BGRX8, BGRX8_SRGB = 61, 65, 86, 28, 29, 87, 91, 88, 93
FILL = 0xA5
OPAQUE = 3          # TEX_ALPHA_MODE_OPAQUE in the low three bits of miscFlags2
TGA_FLAGS_BGR, TGA_FLAGS_ALLOW_ALL_ZERO_ALPHA = 0x1, 0x2

# the reader's table (include/dxtex_amd.h): name -> (bytes per texel, destination format, palette, bytes of an image texel, alpha rule, the
# reader's TGA_FLAGS that select it, the file's image type and bits)
KINDS = {
    "grey": (1, R8, False, 1, False, 0, 3, 8),
    "5551": (2, B5G5R5A1, False, 2, True, 0, 2, 16),
    "rgb_rgba": (3, RGBA8, False, 4, False, 0, 2, 24),
    "rgb_bgrx": (3, BGRX8, False, 4, False, TGA_FLAGS_BGR, 2, 24),
    "bgra_rgba": (4, RGBA8, False, 4, True, 0, 2, 32),
    "bgra_bgra": (4, BGRA8, False, 4, True, TGA_FLAGS_BGR, 2, 32),
    "palette_rgba": (1, RGBA8, True, 4, False, 0, 1, 8),
    "palette_bgrx": (1, BGRX8, True, 4, False, TGA_FLAGS_BGR, 1, 8),
}
ORIENTATIONS = (0, dx.TGA_RIGHT_TO_LEFT, dx.TGA_TOP_DOWN, dx.TGA_RIGHT_TO_LEFT | dx.TGA_TOP_DOWN)
# where a group of four, a wave and a workgroup each have a tail, and where three-byte rows fall on and off dword alignment
WIDTHS, HEIGHTS = (1, 3, 4, 5, 63, 64, 65, 257), (1, 2, 5)
BASES = (0, 1, 4, 18 + 5)          # the stream's offset into its allocation: aligned, odd, a dword but no two, and behind a header with a five-byte ID field
PITCH_PADS = (0, 4, 3)
PALETTE_FIRST, PALETTE_LENGTH = 200, 56


def _palette(bgr):
    """(the file's colour-map bytes, the 256 words ReadPalette makes of them): entries 200 .. 255, zero words outside."""
    cmap = np.random.default_rng(77).integers(0, 256, (PALETTE_LENGTH, 3), dtype=np.uint8)
    words = np.zeros(256, np.uint32)
    c = cmap.astype(np.uint32)
    inside = (c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16)) if bgr else (c[:, 2] | (c[:, 1] << 8) | (c[:, 0] << 16))
    words[PALETTE_FIRST:PALETTE_FIRST + PALETTE_LENGTH] = inside | np.uint32(0xFF000000)
    return cmap.tobytes(), words


def _texels(kind, w, h, alpha):
    """The file-order texel stream, (w * h * B) uint8. alpha = 'zero', 'opaque' or 'mixed' for the kinds that carry one."""
    B = KINDS[kind][0]
    px = np.random.default_rng(w * 131 + h * 7 + B).integers(0, 256, (w * h, B), dtype=np.uint8)
    if B == 4:
        px[:, 3] = {"zero": 0, "opaque": 255}.get(alpha, px[:, 3])
    if B == 2:
        px[:, 1] = {"zero": px[:, 1] & 0x7F, "opaque": px[:, 1] | 0x80}.get(alpha, px[:, 1])
    if alpha == "mixed" and B in (2, 4) and w * h > 1:
        px[0, B - 1], px[-1, B - 1] = 0x00, 0xFF          # both kinds of alpha are there whatever the generator drew
    return px.reshape(-1)


_reference = {}


def _ref(oracle, kind, orient, w, h, alpha, allow):
    """(pixels (h, w * D), answer) of the reference loader for the stream as a .tga file; computed once per case."""
    key = (kind, orient, w, h, alpha, allow)
    if key not in _reference:
        B, fmt, paletted, D, rule, flags, itype, bits = KINDS[kind]
        desc = (0x10 if orient & dx.TGA_RIGHT_TO_LEFT else 0) | (0x20 if orient & dx.TGA_TOP_DOWN else 0) | (8 if bits == 32 else 0)
        if paletted:
            head = tga_header(1, w, h, 8, desc, cmap_type=1, cmap_first=PALETTE_FIRST, cmap_len=PALETTE_LENGTH, cmap_size=24) + _palette(bool(flags))[0]
        else:
            head = tga_header(itype, w, h, bits, desc)
        hr, meta, px = oracle.ref_load_tga(head + _texels(kind, w, h, alpha).tobytes(), flags | (TGA_FLAGS_ALLOW_ALL_ZERO_ALPHA if allow else 0))
        assert hr == 0 and (meta["width"], meta["height"], meta["format"]) == (w, h, fmt), (hr, meta)
        # the reference's S_FALSE shows as an opaque alpha mode. A colour-mapped file is the exception: it has no alpha rule (CopyPixels
        # returns S_OK for it), and its opaque mode comes from the header alone, so the texel pass answers 0
        answer = 0 if paletted else int((meta["miscFlags2"] & 7) == OPAQUE)
        _reference[key] = (px.reshape(h, w * D), answer)
    return _reference[key]


def _expected_unpack_mark(w, D, stream_ptr, dst_ptr, pitch):
    wide = w % 4 == 0 and stream_ptr % 4 == 0 and dst_ptr % (4 * D) == 0 and pitch % (4 * D) == 0
    return "tga_unpack<wide>" if wide else "tga_unpack<narrow>"


def _marks(prof, prefix):
    return {k: v[1] for k, v in prof.items() if k.startswith(prefix)}


class Arena:
    """Two device allocations reused by every case of a test: the stream's and the image's (+ a dword for the answer)."""
    def __init__(self, ctx, stream_bytes, image_bytes):
        self.ctx = ctx
        self.s = ctx.device_alloc(stream_bytes + 256)
        self.d = ctx.device_alloc(image_bytes + 256)

    def close(self):
        self.ctx.device_free(self.s)
        self.ctx.device_free(self.d)


@pytest.fixture
def arena(ctx):
    a = Arena(ctx, max(WIDTHS) * max(HEIGHTS) * 4, (max(WIDTHS) * 4 + 16) * max(HEIGHTS))
    yield a
    a.close()


def _unpack_case(ctx, oracle, arena, kind, orient, w, h, alpha, allow, base, pad, seen):
    B, fmt, paletted, D, rule, flags, _, _ = KINDS[kind]
    want, want_answer = _ref(oracle, kind, orient, w, h, alpha, allow)
    stream = _texels(kind, w, h, alpha)
    pitch = w * D + pad
    image_bytes = pitch * h
    answer_at = (image_bytes + 3) & ~3
    ctx.upload(arena.s + base, stream, sync=True)
    ctx.upload(arena.d, np.full(answer_at + 4, FILL, np.uint8), sync=True)
    how = orient | (dx.TGA_ALLOW_ALL_ZERO_ALPHA if allow else 0)
    ctx.profile_begin()
    ctx.tga_unpack_device(arena.s + base, stream.nbytes, B, dx.device_image(arena.d, w, h, fmt, pitch), how,
                          _palette(bool(flags))[1] if paletted else None, arena.d + answer_at)
    prof = ctx.profile_end()
    got = np.zeros(answer_at + 4, np.uint8)
    ctx.download(got, arena.d, sync=True)
    where = (kind, orient, w, h, alpha, allow, base, pad)
    m = got[:image_bytes].reshape(h, pitch)
    assert np.array_equal(m[:, :w * D], want), where
    assert (m[:, w * D:] == FILL).all() and (got[image_bytes:answer_at] == FILL).all(), ("bytes outside the rows were written", where)
    assert int(got[answer_at:].view(np.uint32)[0]) == want_answer, where
    mark = _expected_unpack_mark(w, D, arena.s + base, arena.d, pitch)
    assert _marks(prof, "tga_") == ({mark: 1, "tga_opaque": 1} if rule else {mark: 1}), (prof, where)
    seen.add(mark)


@pytest.mark.parametrize("orient", ORIENTATIONS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_unpack_matches_the_reference_reader(ctx, oracle, arena, kind, orient):
    """Every size, stream base and destination pitch; for the kinds with an alpha rule every alpha pattern with and without
    ALLOW_ALL_ZERO_ALPHA. Pixels, the bytes around them, the alpha answer and the route's profile mark."""
    rule = KINDS[kind][4]
    seen = set()
    for alpha, allow in ([(a, f) for a in ("zero", "opaque", "mixed") for f in (False, True)] if rule else [(None, False)]):
        for w in WIDTHS:
            for h in HEIGHTS:
                for base in BASES:
                    for pad in PITCH_PADS:
                        _unpack_case(ctx, oracle, arena, kind, orient, w, h, alpha, allow, base, pad, seen)
    assert seen == {"tga_unpack<wide>", "tga_unpack<narrow>"}          # both routes have run


def test_palette_indices_outside_the_map_are_zero_words(ctx, oracle, arena):
    """first = 200, length = 56: an index below 200 gives a zero word, as in the reference."""
    w, h = 64, 2
    stream = _texels("palette_rgba", w, h, None)
    assert (stream < PALETTE_FIRST).sum() > 20 and (stream >= PALETTE_FIRST).sum() > 5
    got, answer = ctx.tga_unpack(stream, w, h, 1, RGBA8, dx.TGA_TOP_DOWN, _palette(False)[1])
    want, _ = _ref(oracle, "palette_rgba", dx.TGA_TOP_DOWN, w, h, None, False)
    assert np.array_equal(got.reshape(h, w * 4), want) and answer == 0
    words = got.view(np.uint32)
    assert (words[stream < PALETTE_FIRST] == 0).all() and (words[stream >= PALETTE_FIRST] >> 24 == 0xFF).all()


# ---- pack -----------------------------------------------------------------------------------------------------------------------------
WRITER = ((RGBA8, 4, 4), (RGBA8_SRGB, 4, 4), (BGRA8, 4, 4), (BGRA8_SRGB, 4, 4), (BGRX8, 3, 4), (BGRX8_SRGB, 3, 4), (R8, 1, 1), (A8, 1, 1), (B5G5R5A1, 2, 2))
_rows = {}


def _ref_rows(oracle, fmt, B, D, w, h):
    """(the image's pixels (h, w * D), the reference writer's rows (w * h * B)); computed once per case."""
    key = (fmt, w, h)
    if key not in _rows:
        px = np.random.default_rng(fmt * 1000 + w * 9 + h).integers(0, 256, (h, w * D), dtype=np.uint8)
        hr, ref = oracle.ref_save_tga(px, w, h, fmt, w * D)
        assert hr == 0 and ref.size == 18 + w * h * B + 26 and ref[16] == 8 * B and ref[17] & 0x30 == 0x20          # top-down, left to right
        _rows[key] = (px, ref[18:18 + w * h * B])
    return _rows[key]


@pytest.mark.parametrize("fmt,B,D", WRITER)
def test_pack_matches_the_reference_writer(ctx, oracle, arena, fmt, B, D):
    seen = set()
    for w in WIDTHS:
        for h in HEIGHTS:
            px, want = _ref_rows(oracle, fmt, B, D, w, h)
            for pad in (16, 3):          # a padded source pitch that keeps the rows' alignment, and one that does not
                for base in (0, 1):      # the stream at an aligned and at an odd address
                    pitch = w * D + pad
                    src = np.full((h, pitch), 0x5A, np.uint8)
                    src[:, :w * D] = px
                    ctx.upload(arena.d, src.reshape(-1), sync=True)
                    ctx.upload(arena.s, np.full(want.size + 32, FILL, np.uint8), sync=True)
                    ctx.profile_begin()
                    ctx.tga_pack_device(dx.device_image(arena.d, w, h, fmt, pitch), B, arena.s + base, want.size)
                    prof = ctx.profile_end()
                    got = np.zeros(want.size + 32, np.uint8)
                    ctx.download(got, arena.s, sync=True)
                    where = (fmt, w, h, pad, base)
                    assert np.array_equal(got[base:base + want.size], want), where
                    assert (got[:base] == FILL).all() and (got[base + want.size:] == FILL).all(), ("bytes outside the stream were written", where)
                    wide = w % 4 == 0 and (arena.s + base) % 4 == 0 and arena.d % (4 * D) == 0 and pitch % (4 * D) == 0
                    mark = "tga_pack<wide>" if wide else "tga_pack<narrow>"
                    assert _marks(prof, "tga_") == {mark: 1}, (prof, where)
                    seen.add(mark)
    assert seen == {"tga_pack<wide>", "tga_pack<narrow>"}


# ---- host forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_host_unpack_gives_the_device_forms_bytes_and_moves_the_files_bytes(ctx, oracle, kind):
    B, fmt, paletted, D, rule, flags, _, _ = KINDS[kind]
    for (w, h, orient, alpha, pad) in ((4, 2, 0, "zero", 0), (5, 5, dx.TGA_RIGHT_TO_LEFT, "mixed", 3), (257, 2, dx.TGA_RIGHT_TO_LEFT | dx.TGA_TOP_DOWN, "opaque", 4)):
        alpha = alpha if rule else None
        want, want_answer = _ref(oracle, kind, orient, w, h, alpha, False)          # what the device form was held to above
        stream = _texels(kind, w, h, alpha)
        pitch = w * D + pad
        ctx.transfer_bytes(reset=True)
        got, answer = ctx.tga_unpack(stream, w, h, B, fmt, orient, _palette(bool(flags))[1] if paletted else None, row_pitch=pitch)
        up, down = ctx.transfer_bytes()
        assert np.array_equal(got.reshape(h, pitch)[:, :w * D], want) and answer == want_answer, (kind, w, h)
        # up: the stream as the file has it (the palette rides in the kernel's arguments); down: the image and, with an alpha rule, the answer
        assert (up, down) == (w * h * B, pitch * h + (4 if rule else 0)), (kind, w, h, up, down)


@pytest.mark.parametrize("fmt,B,D", WRITER)
def test_host_pack_gives_the_device_forms_bytes(ctx, oracle, fmt, B, D):
    for (w, h) in ((4, 2), (5, 5), (257, 2)):
        px, want = _ref_rows(oracle, fmt, B, D, w, h)
        ctx.transfer_bytes(reset=True)
        got = ctx.tga_pack(px, w, h, fmt, B, row_pitch=w * D)
        assert np.array_equal(got, want), (fmt, w, h)
        assert ctx.transfer_bytes() == (w * h * D, w * h * B)


# ---- HRESULTs -------------------------------------------------------------------------------------------------------------------------
def test_hresults_come_in_the_stated_order(ctx):
    """E_POINTER, then NOT_SUPPORTED, then E_INVALIDARG, then E_FAIL: each call carries every later error as well."""
    lib, h = ctx._lib, ctx._h
    dev = ctx.device_alloc(4096)
    try:
        def image(w, hgt, fmt, pitch, ptr=dev + 2048):
            return dx.device_image(ptr, w, hgt, fmt, pitch, pitch * max(hgt, 1))

        def unpack(stream, size, B, img, palette=None, host=False, answer=None):
            fn = lib.dxtex_tga_unpack if host else lib.dxtex_tga_unpack_device
            pal = None if palette is None else palette.ctypes.data
            return fn(h, stream, size, B, 0, pal, None if img is None else ctypes.byref(img), answer)

        def pack(img, B, stream, size, host=False):
            fn = lib.dxtex_tga_pack if host else lib.dxtex_tga_pack_device
            return fn(h, None if img is None else ctypes.byref(img), B, stream, size)

        answer = ctypes.c_uint32(0)
        # E_POINTER beats an unsupported pair, a zero width and a wrong size
        assert unpack(None, 1, 2, image(0, 4, RGBA8, 0)) == E_POINTER
        assert unpack(dev, 1, 2, None) == E_POINTER
        assert unpack(dev, 1, 2, image(0, 4, RGBA8, 0, ptr=None)) == E_POINTER
        assert unpack(dev, 1, 2, image(0, 4, RGBA8, 0), host=True, answer=None) == E_POINTER
        assert pack(None, 2, dev, 1) == E_POINTER and pack(image(0, 4, RGBA8, 0), 2, None, 1) == E_POINTER
        # NOT_SUPPORTED beats a zero width, a short pitch and a wrong size
        for B, fmt, pal in ((2, RGBA8, None), (3, BGRA8, None), (4, BGRX8, None), (1, RGBA8_SRGB, None), (4, 2, None), (2, RGBA8, np.zeros(256, np.uint32)),
                            (1, R8, np.zeros(256, np.uint32)), (5, RGBA8, None), (0, R8, None)):
            assert unpack(dev, 1, B, image(0, 4, fmt, 0), pal) == E_NOT_SUPPORTED, (B, fmt)
        for B, fmt in ((3, RGBA8), (4, BGRX8), (2, R8), (1, B5G5R5A1), (4, 2), (4, 30)):
            assert pack(image(0, 4, fmt, 0), B, dev, 1) == E_NOT_SUPPORTED, (B, fmt)
        # E_INVALIDARG beats a wrong size: extents, a pitch below the row, overlap
        for w, hgt, pitch in ((0, 4, 64), (4, 0, 64), (65536, 1, 65536 * 4), (1, 65536, 4), (4, 4, 15)):
            assert unpack(dev, 1, 4, image(w, hgt, RGBA8, pitch)) == E_INVALIDARG, (w, hgt, pitch)
            assert pack(image(w, hgt, RGBA8, pitch), 4, dev, 1) == E_INVALIDARG, (w, hgt, pitch)
        assert unpack(dev + 2048 + 60, 1, 4, image(4, 4, RGBA8, 16)) == E_INVALIDARG          # the stream starts inside the image's last row
        assert pack(image(4, 4, RGBA8, 16), 4, dev + 2048 - 4, 1) == E_INVALIDARG              # the stream's last texel is the image's first
        # E_FAIL: everything else is in order, the size is not width * height * B
        for size in (63, 65, 0):
            assert unpack(dev, size, 4, image(4, 4, RGBA8, 16)) == E_FAIL
            assert pack(image(4, 4, RGBA8, 16), 4, dev, size) == E_FAIL
        assert unpack(dev, 64, 4, image(4, 4, RGBA8, 16)) == 0 and pack(image(4, 4, RGBA8, 16), 4, dev, 64) == 0
        ctx.synchronize()
        # the host forms check the same things in the same order
        buf, px = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
        himg = dx.Image(4, 4, RGBA8, 16, 64, px.ctypes.data)
        assert unpack(buf.ctypes.data, 63, 2, himg, host=True, answer=ctypes.byref(answer)) == E_NOT_SUPPORTED
        assert unpack(buf.ctypes.data, 63, 4, dx.Image(4, 4, RGBA8, 15, 60, px.ctypes.data), host=True, answer=ctypes.byref(answer)) == E_INVALIDARG
        assert unpack(buf.ctypes.data, 63, 4, himg, host=True, answer=ctypes.byref(answer)) == E_FAIL
        assert pack(himg, 4, buf.ctypes.data, 63, host=True) == E_FAIL and pack(himg, 3, buf.ctypes.data, 63, host=True) == E_NOT_SUPPORTED
    finally:
        ctx.device_free(dev)
