"""JPEG coefficients on the GPU (dxtex_jpeg_encode and its _device form: jpeg_samples and jpeg_fdct of csrc/jpeg_encode.hip) against
tests/jpeg_write_ref.py, the numpy restatement of libjpeg in front of its Huffman coder, and against the files libjpeg-turbo wrote
(tests/golden/jpeg_write): coefficient for coefficient, the bytes around them untouched, the source unchanged, every route asserted by
profile mark. Uses numpy, the restatements and the committed fixtures only."""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref as R  # noqa: E402
import jpeg_write_ref as W  # noqa: E402
from test_jpeg_write_cpu import QUALITY_100, golden, source, texels  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALIDARG, E_POINTER, E_NOT_SUPPORTED = 0x80070057 - (1 << 32), 0x80004003 - (1 << 32), 0x80070032 - (1 << 32)
FILL = 0xA5
SIZES = ((1, 1), (2, 2), (3, 5), (4, 1), (5, 2), (6, 3), (7, 9), (16, 16), (17, 33), (33, 18), (40, 24), (65, 35))
SAMPLINGS = {"grey": None, "444": (1, 1), "422": (2, 1), "420": (2, 2)}
ORDERS = (R.RGBA8, W.B8G8R8A8, W.B8G8R8X8_SRGB)
MAX_W, MAX_H = 72, 48
ALL_ROUTES = {"jpeg_samples<wide>", "jpeg_samples<narrow>", "jpeg_fdct", "jpeg_fdct<unaligned>"}


def frame_for(w, h, sampling, quant=W.ONES, quant_of=(0, 1, 1)):
    return dx.jpeg_frame(w, h, R.GREY if sampling is None else R.YCBCR, sampling or (1, 1), quant, quant_of)


def _marks(prof, prefix="jpeg_"):
    return {k: v[1] for k, v in prof.items() if k.startswith(prefix)}


class Arena:
    """Two device allocations reused by every case of a test: the image's and the coefficients'."""
    def __init__(self, ctx):
        self.ctx = ctx
        self.s = ctx.device_alloc((MAX_W * 4 + 32) * MAX_H + 256)
        self.d = ctx.device_alloc(MAX_W * MAX_H * 3 * 2 + 4096)

    def close(self):
        self.ctx.device_free(self.s)
        self.ctx.device_free(self.d)


@pytest.fixture
def arena(ctx):
    a = Arena(ctx)
    yield a
    a.close()


def _device_case(ctx, arena, px, fmt, sampling, quant, quant_of, pad, base, seen, where, shift=0):
    """an image of pitch row + pad at arena.s + shift -> coefficients at arena.d + base: the restatement's, the bytes around them, the image
    and the bytes around it untouched, the marks"""
    h, w = px.shape[:2]
    frame = frame_for(w, h, sampling, quant, quant_of)
    want = R.coefficients(W.encode(px, sampling, quant, quant_of))
    assert want.size == dx.jpeg_coefficient_count(frame)
    rows, pitch = texels(px, fmt, pad, FILL)
    image = np.concatenate([np.full(shift, FILL, np.uint8), rows, np.full(32, FILL, np.uint8)])
    ctx.upload(arena.s, image, sync=True)
    ctx.upload(arena.d, np.full(want.nbytes + 64, FILL, np.uint8), sync=True)
    ctx.profile_begin()
    ctx.jpeg_encode_device(dx.device_image(arena.s + shift, w, h, fmt, pitch), frame, arena.d + base, want.nbytes)
    prof = ctx.profile_end()
    got = np.zeros(want.nbytes + 64, np.uint8)
    ctx.download(got, arena.d, sync=True)
    assert np.array_equal(got[base:base + want.nbytes].view("<i2"), want), where
    assert (got[:base] == FILL).all() and (got[base + want.nbytes:] == FILL).all(), ("bytes outside the coefficients were written", where)
    back = np.zeros(image.size, np.uint8)
    ctx.download(back, arena.s, sync=True)
    assert np.array_equal(back, image), ("the image was written", where)
    marks = {"jpeg_fdct" if (arena.d + base) % 16 == 0 else "jpeg_fdct<unaligned>": 1}
    if sampling is not None:
        wide = w % 4 == 0 and (arena.s + shift) % 16 == 0 and pitch % 16 == 0
        marks["jpeg_samples<wide>" if wide else "jpeg_samples<narrow>"] = 1
    assert _marks(prof) == marks, (prof, where)
    seen.update(marks)


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
def test_fixture_images_give_libjpegs_coefficients(ctx, arena):
    """the source pixels of every quality-100 fixture: the coefficients the reader's restatement parses out of libjpeg-turbo's file, through
    the device form and the host-pointer form; the host form moves the image's rows up and the coefficients down"""
    seen = set()
    for n, name in enumerate(QUALITY_100):
        px, info = source(name), R.decode(golden(name))
        grey = px.ndim == 2
        fmt = R.R8 if grey else ORDERS[n % 3]
        want = R.coefficients(info)
        assert np.array_equal(R.coefficients(W.encode(px, None if grey else (2, 2))), want), name
        _device_case(ctx, arena, px, fmt, None if grey else (2, 2), W.ONES, (0, 1, 1), 0, 0, seen, name)
        rows, pitch = texels(px, fmt)
        ctx.transfer_bytes(reset=True)
        got = ctx.jpeg_encode(rows, frame_for(px.shape[1], px.shape[0], None if grey else (2, 2)), fmt)
        assert np.array_equal(got, want), name
        assert ctx.transfer_bytes() == (rows.size, want.nbytes), name
    assert {"jpeg_fdct", "jpeg_samples<wide>", "jpeg_samples<narrow>"} <= seen          # 16x16, 24x24, 40x24 and 8x24 are whole quads across


@pytest.mark.parametrize("tables", ("ones", "random", "16-bit"))
@pytest.mark.parametrize("kind", list(SAMPLINGS))
def test_random_images_match_the_restatement_at_every_size(ctx, arena, kind, tables):
    """seeded noise at sizes of one texel, below one block, with dummy blocks right and below, whole MCUs and none; each on a tight and on a
    padded pitch - a pad of 3 takes the byte loads of the narrow route - into a coefficient base on 16 bytes and one 2 bytes off it; the
    three channel orders in turn"""
    rng = np.random.default_rng(len(kind) * 1000 + len(tables))
    sampling = SAMPLINGS[kind]
    seen = set()
    for n, (w, h) in enumerate(SIZES):
        px = rng.integers(0, 256, (h, w) if sampling is None else (h, w, 3), dtype=np.uint8)
        quant = W.ONES if tables == "ones" else rng.integers(1, 256 if tables == "random" else 65536, (4, 64)).astype(np.uint16)
        quant_of = (0, 1, 1) if tables == "ones" else (2, 0, 3)
        fmt = R.R8 if sampling is None else ORDERS[n % 3]
        for pad, base in ((0, 0), ((16, 3, 4)[n % 3], 2)):
            _device_case(ctx, arena, px, fmt, sampling, quant, quant_of, pad, base, seen, (kind, tables, w, h, fmt, pad, base))
    assert seen == ({"jpeg_fdct", "jpeg_fdct<unaligned>"} if kind == "grey" else ALL_ROUTES)


@pytest.mark.parametrize("kind", ("444", "422", "420"))
def test_both_routes_of_jpeg_samples_run(ctx, arena, kind):
    """an aligned image takes the wide route; a pitch that is no multiple of 16, a width that is no multiple of 4 and a base off 16 bytes
    each take the narrow one; the coefficients are the same. 40 texels across is a width of whole quads that ends inside a lane's eight"""
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (24, 40, 3), dtype=np.uint8)
    for pad, shift, wide in ((0, 0, True), (16, 0, True), (4, 0, False), (3, 0, False), (0, 4, False), (0, 16, True)):
        seen = set()
        _device_case(ctx, arena, px, R.RGBA8, SAMPLINGS[kind], W.ONES, (0, 1, 1), pad, 0, seen, (kind, pad, shift), shift)
        assert ("jpeg_samples<wide>" in seen) == wide and ("jpeg_samples<narrow>" in seen) != wide, (kind, pad, shift, seen)
    px = rng.integers(0, 256, (18, 33, 3), dtype=np.uint8)
    seen = set()
    _device_case(ctx, arena, px, W.B8G8R8A8, SAMPLINGS[kind], W.ONES, (0, 1, 1), 12, 0, seen, (kind, "a width of 33"))          # 33 * 4 + 12 = 144: the pitch alone would do
    assert "jpeg_samples<narrow>" in seen and "jpeg_samples<wide>" not in seen


def test_extreme_images_and_the_largest_size(ctx, arena):
    """all-0 / all-255 channels, whose coefficients are the largest an 8-bit image gives, and constant images at the arena's 72 x 48"""
    rng = np.random.default_rng(6)
    seen = set()
    for kind, sampling in SAMPLINGS.items():
        shape = (MAX_H, MAX_W) if sampling is None else (MAX_H, MAX_W, 3)
        for px in ((rng.integers(0, 2, shape) * 255).astype(np.uint8), np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)):
            _device_case(ctx, arena, px, R.R8 if sampling is None else W.B8G8R8X8, sampling, W.ONES, (0, 1, 1), 0, 0, seen, (kind, int(px.max())))


# ---- host form --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SAMPLINGS))
def test_host_form_gives_the_device_forms_coefficients_through_any_pitch(ctx, kind):
    rng = np.random.default_rng(8)
    sampling = SAMPLINGS[kind]
    quant = W.quality_tables(75)
    for (w, h), pad in zip(((5, 2), (17, 33), (40, 24), (65, 35)), (0, 3, 16, 4)):
        px = rng.integers(0, 256, (h, w) if sampling is None else (h, w, 3), dtype=np.uint8)
        fmt = R.R8 if sampling is None else W.B8G8R8A8_SRGB
        want = R.coefficients(W.encode(px, sampling, quant))          # what the device form was held to above
        rows, pitch = texels(px, fmt, pad)
        out = np.full(want.size + 16, 0x1111, np.int16)
        ctx.transfer_bytes(reset=True)
        ctx.profile_begin()
        got = ctx.jpeg_encode(rows, frame_for(w, h, sampling, quant), fmt, row_pitch=pitch, out=out)
        prof = ctx.profile_end()
        assert np.array_equal(got[:want.size], want), (kind, w, h)
        assert (got[want.size:] == 0x1111).all(), ("coefficients behind the frame's were written", kind, w, h)
        assert ctx.transfer_bytes() == (rows.size, want.nbytes), (kind, w, h)
        marks = _marks(prof)
        assert marks.pop("jpeg_fdct") == 1 and marks == ({} if kind == "grey" else {"jpeg_samples<wide>" if w % 4 == 0 and pitch % 16 == 0 else "jpeg_samples<narrow>": 1}), prof


# ---- HRESULTs -------------------------------------------------------------------------------------------------------------------------------
def test_hresults_come_in_the_stated_order(ctx):
    """E_POINTER, then E_INVALIDARG for the frame, then NOT_SUPPORTED for the colour, sampling and format, then E_INVALIDARG for the sizes:
    each call carries every later error as well. None reaches a kernel."""
    lib, h = ctx._lib, ctx._h
    dev = ctx.device_alloc(1 << 16)
    try:
        def image(w, hgt, fmt, pitch, ptr=dev + (1 << 15)):
            return dx.device_image(ptr, w, hgt, fmt, pitch, pitch * max(hgt, 1))

        def encode(img, frame, coef, size, host=False):
            fn = lib.dxtex_jpeg_encode if host else lib.dxtex_jpeg_encode_device
            return fn(h, None if img is None else ctypes.byref(img), None if frame is None else ctypes.byref(frame), coef, size)

        def frame(w=16, hgt=16, colour=R.YCBCR, sampling=(2, 2), zero=None, **edits):
            quant = np.ones((4, 64), np.uint16)
            if zero is not None:
                quant[zero] = 0
            f = dx.jpeg_frame(w, hgt, colour, sampling, quant)
            for key, value in edits.items():
                target, name = (f, key) if "_" not in key else (f.component[int(key.split("_")[1])], key.split("_")[0])
                setattr(target, name, value)
            return f

        good, need = frame(), 6 * 64 * 2
        ctx.profile_begin()
        # E_POINTER beats a bad frame, a mismatched format and a short buffer
        assert encode(image(16, 16, R.R8, 1), frame(colour=7), None, 0) == E_POINTER and encode(image(16, 16, R.R8, 1), None, dev, 0) == E_POINTER
        assert encode(None, frame(colour=7), dev, 0) == E_POINTER and encode(image(16, 16, R.R8, 1, ptr=None), frame(colour=7), dev, 0) == E_POINTER
        # E_INVALIDARG for the frame beats colour, sampling and format: an unknown colour, a component count that does not match it, a quantiser
        # index above 3, sizes of 0 or above 65535, an image of another size, an odd address
        bad_sampling = dict(h_0=1, v_0=2)
        assert encode(image(16, 16, R.R8, 1), frame(colour=3, **bad_sampling), dev, 1) == E_INVALIDARG
        assert encode(image(16, 16, R.R8, 1), frame(components=1, **bad_sampling), dev, 1) == E_INVALIDARG
        assert encode(image(16, 16, R.R8, 1), frame(colour=R.GREY, components=3), dev, 1) == E_INVALIDARG
        assert encode(image(16, 16, R.R8, 1), frame(quant_2=4, **bad_sampling), dev, 1) == E_INVALIDARG
        for w, hgt in ((0, 16), (16, 0), (65536, 16), (16, 65536)):
            assert encode(image(w, hgt, R.R8, 1), frame(width=w, height=hgt), dev, 1) == E_INVALIDARG, (w, hgt)
        assert encode(image(15, 16, R.R8, 1), good, dev, 1) == E_INVALIDARG and encode(image(16, 17, R.R8, 1), good, dev, 1) == E_INVALIDARG
        assert encode(image(16, 16, R.R8, 1), frame(colour=R.RGB, **bad_sampling), dev + 1, 1) == E_INVALIDARG
        # NOT_SUPPORTED beats wrong block counts, a zero quantiser entry, a short buffer and a short pitch: DXTEX_JPEG_RGB, sampling outside
        # the table, a format that does not pair
        assert encode(image(16, 16, R.RGBA8, 1), frame(colour=R.RGB, zero=0), dev, 1) == E_NOT_SUPPORTED
        for edits in (dict(h_0=1, v_0=2), dict(h_0=4, v_0=1), dict(h_0=2, v_0=4), dict(h_1=2), dict(v_2=2), dict(h_0=2, v_0=2, h_1=2, v_1=2, h_2=2, v_2=2)):
            assert encode(image(16, 16, R.RGBA8, 1), frame(zero=0, **edits), dev, 1) == E_NOT_SUPPORTED, edits
        assert encode(image(16, 16, R.R8, 1), frame(colour=R.GREY, sampling=(1, 1), h_0=2), dev, 1) == E_NOT_SUPPORTED
        for colour, fmt in ((R.YCBCR, R.R8), (R.GREY, R.RGBA8), (R.GREY, W.B8G8R8A8), (R.YCBCR, 31), (R.YCBCR, 2), (R.YCBCR, 24), (R.GREY, 65), (R.GREY, 56)):
            assert encode(image(16, 16, fmt, 1), frame(colour=colour, zero=0), dev, 1) == E_NOT_SUPPORTED, (colour, fmt)
        # E_INVALIDARG: block counts or offsets that are not the frame's, an entry of 0 in a table a component names, fewer bytes than the
        # coefficients, a pitch below the row, overlap
        for edits in (dict(blocksPerRow_0=3), dict(blockRows_1=2), dict(offset_1=0), dict(offset_2=64 * 6)):
            assert encode(image(16, 16, R.RGBA8, 64), frame(**edits), dev, need) == E_INVALIDARG, edits
        assert encode(image(16, 16, R.RGBA8, 64), frame(zero=(0, 63)), dev, need) == E_INVALIDARG and encode(image(16, 16, R.RGBA8, 64), frame(zero=(1, 0)), dev, need) == E_INVALIDARG
        assert encode(image(16, 16, R.RGBA8, 64), good, dev, need - 1) == E_INVALIDARG and encode(image(16, 16, R.RGBA8, 63), good, dev, need) == E_INVALIDARG
        assert encode(image(8, 8, R.R8, 8), frame(8, 8, R.GREY), dev, 127) == E_INVALIDARG
        assert encode(image(16, 16, R.RGBA8, 64), good, dev + (1 << 15) + 16 * 64 - 2, need) == E_INVALIDARG          # the coefficients start inside the image's last row
        assert encode(image(16, 16, R.RGBA8, 64), good, dev + (1 << 15) - need + 2, need) == E_INVALIDARG               # and end inside its first
        # the host form checks the same things in the same order
        buf, px = np.zeros(need // 2, np.int16), np.zeros(16 * 64, np.uint8)
        himg = dx.Image(16, 16, R.RGBA8, 64, 64 * 16, px.ctypes.data)
        assert encode(himg, frame(colour=3), buf.ctypes.data, need - 1, host=True) == E_INVALIDARG and encode(himg, frame(h_0=1, v_0=2), buf.ctypes.data, need - 1, host=True) == E_NOT_SUPPORTED
        assert encode(himg, good, buf.ctypes.data, need - 1, host=True) == E_INVALIDARG and encode(himg, good, None, need, host=True) == E_POINTER
        assert _marks(ctx.profile_end()) == {}          # no refusal reached a kernel
        # and with everything in order: more bytes than the coefficients is fine, a table no component names may hold zeros, every 32-bit
        # format of the table pairs with colour
        assert encode(image(16, 16, R.RGBA8, 64), frame(zero=2), dev, need + 64) == 0
        for fmt in (R.RGBA8_SRGB, W.B8G8R8A8, W.B8G8R8A8_SRGB, W.B8G8R8X8, W.B8G8R8X8_SRGB):
            assert encode(image(16, 16, fmt, 80), good, dev, need) == 0, fmt
        assert encode(image(8, 8, R.R8, 8), frame(8, 8, R.GREY, zero=1), dev, 128) == 0
        assert encode(himg, good, buf.ctypes.data, need, host=True) == 0
        ctx.synchronize()
    finally:
        ctx.device_free(dev)
