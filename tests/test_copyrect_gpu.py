"""dxtex_copy_rectangle / dxtex_copy_rectangles_device against the reference's own CopyRectangle (DirectXTexMisc.cpp:275-381), called
live in oracle/_ref/libdxtex_ref.so (tests/assemble_ref.py).

Every comparison is of the WHOLE destination buffer, which starts as a seeded random pattern: a byte written outside the rectangle, or
into row padding, shows.

Same format: one format per texel size (1, 2, 4, 8, 12, 16 bytes) and YUY2, whose "texel" CopyRectangle counts as a 4-byte element, so
that its rows run into the next row - there as here - and consecutive destination rows overlap: the later row must win, as after the
reference's row-by-row memcpy. Pitches are tight or padded by 3 bytes, which leaves no row but the first aligned
to anything: the mover's access width (16 / 8 / 4 / 2 / 1) must come from the real addresses. Byte equality.

Different formats: byte equality, except where an sRGB curve (powf on both sides) meets a source that is not 8-bit: DESIGN.md's rule for
those is 1 ulp on < 0.1 % of values, which in the 8-bit destinations of these cases is one code step on < 0.1 % of bytes.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx
from directxtex_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_ref as R  # noqa: E402
from test_scanline_routes_gpu import Device  # noqa: E402

pytestmark = pytest.mark.gpu

RGBA32F, RGB32F, RGBA16F, RGB10A2, RGBA8, RGBA8S, R32F, RG8, R8, B5G6R5, BGRA8, YUY2 = 2, 6, 10, 24, 28, 29, 41, 49, 61, 85, 87, 107
BC1, NV12, P8, R1, RGBA8_TYPELESS = 71, 103, 113, 66, 27
TEXEL_BYTES = {RGBA32F: 16, RGB32F: 12, RGBA16F: 8, RGB10A2: 4, RGBA8: 4, RGBA8S: 4, R32F: 4, RG8: 2, R8: 1, B5G6R5: 2, BGRA8: 4, YUY2: 4}
X2BIAS, DITHER, SRGB_IN, SRGB_OUT = 0x200, 0x10000, 0x1000000, 0x2000000
E_POINTER, E_INVALIDARG, E_FAIL, E_NOT_SUPPORTED = dx.E_POINTER, dx.E_INVALIDARG, dx.E_FAIL, dx.HRESULT_E_NOT_SUPPORTED

# (source size, rectangle, destination size, offset): 1 x 1; odd sizes at an odd corner; more than one workgroup column would need 4096
# bytes per row - 67 x 16 bytes is 1072: several accesses per lane row group, more rows (45) than one group of four, a tail group of one
SHAPES = [((1, 1), (0, 0, 1, 1), (1, 1), (0, 0)),
          ((7, 5), (1, 1, 5, 3), (7, 5), (1, 1)),
          ((97, 61), (13, 7, 67, 45), (131, 97), (31, 5))]


def _shape_id(s):
    return f"{s[1][2]}x{s[1][3]}"


def _signed(hr):
    hr &= 0xFFFFFFFF
    return hr - (1 << 32) if hr & 0x80000000 else hr


def _pitch(fmt, width, pad):
    return capi.compute_pitch(fmt, width, 1)[0] + pad


def _texels(rng, fmt, nbytes):
    """Random bytes; finite floats in [-0.25, 1.25) for the float formats (pitch padding then holds float bytes too, which is as good)."""
    if fmt in (RGBA32F, RGB32F, R32F):
        return (rng.random(nbytes // 4 + 1, dtype=np.float32) * 1.5 - 0.25).astype(np.float32).view(np.uint8)[:nbytes].copy()
    if fmt == RGBA16F:
        return (rng.random(nbytes // 2 + 1, dtype=np.float32) * 1.5 - 0.25).astype(np.float16).view(np.uint8)[:nbytes].copy()
    return rng.integers(0, 256, nbytes, dtype=np.uint8)


def _case(rng, sfmt, dfmt, shape, pad):
    (sw, sh), rect, (dw, dh), off = shape
    sp, dp = _pitch(sfmt, sw, pad), _pitch(dfmt, dw, pad)
    src, dst = _texels(rng, sfmt, sp * sh), rng.integers(0, 256, dp * dh, dtype=np.uint8)
    return src, (sw, sh, sfmt, sp), rect, dst, (dw, dh, dfmt, dp), off


def _device_copy(ctx, d, src, sdims, rect, dst, ddims, off, flt=0):
    ps, pd = d.put(src), d.put(dst)
    a = capi.device_image(ps, sdims[0], sdims[1], sdims[2], sdims[3])
    b = capi.device_image(pd, ddims[0], ddims[1], ddims[2], ddims[3])
    ctx.copy_rectangles_device([a], [rect], [b], [off[0]], [off[1]], flt)
    return d.get(pd, dst.nbytes)


# ---- same format: the byte mover ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 3], ids=["tight", "pad3"])
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("fmt", [R8, RG8, RGBA8, RGBA16F, RGB32F, RGBA32F, YUY2])
def test_same_format(ctx, oracle, fmt, shape, pad):
    src, sdims, rect, dst, ddims, off = _case(np.random.default_rng(fmt * 7 + rect_seed(shape) + pad), fmt, fmt, shape, pad)
    hr, want = R.copy_rectangle(oracle, src, sdims, rect, dst, ddims, 0, *off)
    assert hr == 0
    with Device(ctx) as d:
        got = _device_copy(ctx, d, src, sdims, rect, dst, ddims, off)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


@pytest.mark.parametrize("case", [(R8, 64, 37, 16), (R8, 64, 50, 16), (RGB32F, 16, 7, 16), (RGB32F, 16, 10, 16), (RG8, 32, 13, 16)],
                         ids=lambda c: f"{c[0]}-w{c[2]}")
def test_wide_accesses_and_byte_tail(ctx, oracle, case):
    """The mover's mixed route: aligned rows (x = 0, pitches a multiple of 16) whose byte count is no multiple of the access width, so
    that whole wide accesses are followed by a byte tail. case = (format, image width, rectangle width, the access width it leaves)."""
    fmt, width, w, vec = case
    pitch = width * TEXEL_BYTES[fmt]
    assert pitch % 16 == 0 and (w * TEXEL_BYTES[fmt]) % vec != 0 and w * TEXEL_BYTES[fmt] > vec
    shape = ((width, 9), (0, 2, w, 6), (width, 9), (0, 1))
    src, sdims, rect, dst, ddims, off = _case(np.random.default_rng(fmt + w), fmt, fmt, shape, 0)
    hr, want = R.copy_rectangle(oracle, src, sdims, rect, dst, ddims, 0, *off)
    assert hr == 0
    with Device(ctx) as d:
        got = _device_copy(ctx, d, src, sdims, rect, dst, ddims, off)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def rect_seed(shape):
    return shape[1][2] * 131 + shape[1][3]


# ---- different formats: LoadScanline -> ConvertScanline -> StoreScanline ------------------------------------------------------------------
PAIRS = [(RGBA8, RGBA16F), (RGBA16F, RGBA8), (BGRA8, RGBA8), (R32F, R8), (RGB10A2, RGBA8), (B5G6R5, RGBA8), (RGBA8S, RGBA32F), (RGBA32F, RGBA8S)]
EIGHT_BIT_SOURCES = {RGBA8, BGRA8, RGBA8S}


@pytest.mark.parametrize("flt", [0, SRGB_IN, SRGB_OUT, X2BIAS], ids=["default", "srgb_in", "srgb_out", "x2bias"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_converting(ctx, oracle, pair, flt):
    sfmt, dfmt = pair
    srgb = bool(flt & (SRGB_IN | SRGB_OUT)) or RGBA8S in pair
    for shape in SHAPES[1:]:
        src, sdims, rect, dst, ddims, off = _case(np.random.default_rng(sfmt * 17 + dfmt + (flt >> 9)), sfmt, dfmt, shape, 0)
        hr, want = R.copy_rectangle(oracle, src, sdims, rect, dst, ddims, flt, *off)
        assert hr == 0
        with Device(ctx) as d:
            got = _device_copy(ctx, d, src, sdims, rect, dst, ddims, off, flt)
            dithered = _device_copy(ctx, d, src, sdims, rect, dst, ddims, off, flt | DITHER)
        assert np.array_equal(dithered, got)        # CopyRectangle never dithers: the bit is ignored
        if not srgb or sfmt in EIGHT_BIT_SOURCES:
            assert np.array_equal(got, want), (shape, np.flatnonzero(got != want)[:8])
        else:
            step = np.abs(got.astype(np.int32) - want.astype(np.int32))
            rate = float((step != 0).mean())
            print(f"{sfmt}->{dfmt} filter {flt:#x}: max step {int(step.max())}, differing bytes {rate * 100:.4f} %")
            assert int(step.max()) <= 1 and rate < 0.001, (shape, int(step.max()), rate)


# ---- a batch is one launch ---------------------------------------------------------------------------------------------------------------
H_CROSS = [(2, 1), (0, 1), (1, 0), (1, 2), (1, 1), (3, 1)]      # +X -X +Y -Y +Z -Z in a 4 x 3 grid of faces


def _cross_jobs(rng, n_faces=6, face=16):
    faces = [rng.integers(0, 256, face * face * 4, dtype=np.uint8) for _ in range(n_faces)]
    return faces, [(x * face, y * face) for x, y in H_CROSS]


def test_batch_one_launch(ctx, oracle):
    """Six 16 x 16 faces into a 64 x 48 horizontal cross: one dxtex_copy_rectangles_device call, ONE copy_rect launch."""
    faces, at = _cross_jobs(np.random.default_rng(6))
    cross = np.zeros(64 * 48 * 4, np.uint8)
    want = cross
    for f, (x, y) in zip(faces, at):
        hr, want = R.copy_rectangle(oracle, f, (16, 16, RGBA8, 64), (0, 0, 16, 16), want, (64, 48, RGBA8, 256), 0, x, y)
        assert hr == 0
    with Device(ctx) as d:
        pc = d.put(cross)
        srcs = [capi.device_image(d.put(f), 16, 16, RGBA8) for f in faces]
        dsts = [capi.device_image(pc, 64, 48, RGBA8)] * 6
        ctx.profile_begin()
        try:
            ctx.copy_rectangles_device(srcs, [(0, 0, 16, 16)] * 6, dsts, [p[0] for p in at], [p[1] for p in at])
        finally:
            prof = ctx.profile_end()
        got = d.get(pc, cross.nbytes)
    assert set(prof) == {"copy_rect"} and prof["copy_rect"][1] == 1, prof
    assert np.array_equal(got, want)
    background = np.ones((48, 64), bool)
    for x, y in at:
        background[y:y + 16, x:x + 16] = False
    assert not got.reshape(48, 64, 4)[background].any()


def test_batch_beyond_the_limit(ctx, oracle):
    """40 rectangles of mixed routes and sizes: two launches (32 + 8), every rectangle where the reference puts it."""
    rng = np.random.default_rng(40)
    n, tile = 40, 9
    src = rng.integers(0, 256, 32 * 32 * 4, dtype=np.uint8)
    dst8, dst16 = np.zeros(8 * tile * 5 * tile * 4, np.uint8), np.zeros(8 * tile * 5 * tile * 8, np.uint8)
    dims8, dims16 = (8 * tile, 5 * tile, RGBA8, 8 * tile * 4), (8 * tile, 5 * tile, RGBA16F, 8 * tile * 8)
    rects = [(int(rng.integers(0, 20)), int(rng.integers(0, 20)), 1 + k % tile, 1 + (k * 5) % tile) for k in range(n)]
    at = [((k % 8) * tile, (k // 8) * tile) for k in range(n)]
    want8, want16 = dst8, dst16
    for k in range(n):
        if k % 2:
            hr, want16 = R.copy_rectangle(oracle, src, (32, 32, RGBA8, 128), rects[k], want16, dims16, 0, *at[k])
        else:
            hr, want8 = R.copy_rectangle(oracle, src, (32, 32, RGBA8, 128), rects[k], want8, dims8, 0, *at[k])
        assert hr == 0
    with Device(ctx) as d:
        ps, p8, p16 = d.put(src), d.put(dst8), d.put(dst16)
        a = capi.device_image(ps, 32, 32, RGBA8)
        b8, b16 = capi.device_image(p8, dims8[0], dims8[1], RGBA8), capi.device_image(p16, dims16[0], dims16[1], RGBA16F)
        ctx.profile_begin()
        try:
            ctx.copy_rectangles_device([a] * n, rects, [b16 if k % 2 else b8 for k in range(n)], [p[0] for p in at], [p[1] for p in at])
        finally:
            prof = ctx.profile_end()
        got8, got16 = d.get(p8, dst8.nbytes), d.get(p16, dst16.nbytes)
    assert prof["copy_rect"][1] == 2, prof
    assert np.array_equal(got8, want8) and np.array_equal(got16, want16)


# ---- HRESULTs ----------------------------------------------------------------------------------------------------------------------------
def _host_image(buf, dims):
    w, h, fmt, pitch = dims
    return capi.Image(w, h, fmt, pitch, pitch * h, None if buf is None else buf.ctypes.data)


def _hr(ctx, src, sdims, rect, dst, ddims, off, flt=0):
    try:
        ctx.copy_rectangle(_host_image(src, sdims), rect, _host_image(dst, ddims), flt, *off)
    except dx.DxtexError as e:
        return _signed(e.hresult & 0xFFFFFFFF)
    return 0


ERRORS = [
    # name, source (format, has pixels), destination (format, has pixels), rectangle, offset, expected, the reference defines it
    ("null source pixels", (RGBA8, False), (RGBA8, True), (1, 1, 5, 3), (1, 1), E_POINTER, True),
    ("null destination pixels", (RGBA8, True), (RGBA8, False), (1, 1, 5, 3), (1, 1), E_POINTER, True),
    ("null pixels before the format", (BC1, False), (RGBA8, True), (1, 1, 5, 3), (1, 1), E_POINTER, True),
    ("compressed source", (BC1, True), (RGBA8, True), (0, 0, 4, 4), (0, 0), E_NOT_SUPPORTED, True),
    ("compressed destination", (RGBA8, True), (BC1, True), (0, 0, 4, 4), (0, 0), E_NOT_SUPPORTED, True),
    ("planar", (NV12, True), (NV12, True), (0, 0, 2, 2), (0, 0), E_NOT_SUPPORTED, True),
    ("palettised", (RGBA8, True), (P8, True), (0, 0, 2, 2), (0, 0), E_NOT_SUPPORTED, True),
    ("unsupported before the rectangle", (BC1, True), (RGBA8, True), (0, 0, 0, 0), (0, 0), E_NOT_SUPPORTED, True),
    ("empty width", (RGBA8, True), (RGBA8, True), (1, 1, 0, 3), (1, 1), E_INVALIDARG, True),
    ("empty height", (RGBA8, True), (RGBA8, True), (1, 1, 5, 0), (1, 1), E_INVALIDARG, True),
    ("right of the source", (RGBA8, True), (RGBA8, True), (3, 1, 5, 3), (1, 1), E_INVALIDARG, True),
    ("below the source", (RGBA8, True), (RGBA8, True), (1, 3, 5, 3), (1, 1), E_INVALIDARG, True),
    ("right of the destination", (RGBA8, True), (RGBA8, True), (1, 1, 5, 3), (3, 1), E_INVALIDARG, True),
    ("below the destination", (RGBA8, True), (RGBA16F, True), (1, 1, 5, 3), (1, 3), E_INVALIDARG, True),
    ("no such format", (0, True), (0, True), (1, 1, 5, 3), (1, 1), E_INVALIDARG, True),
    ("monochrome", (R1, True), (R1, True), (0, 0, 5, 3), (0, 0), E_NOT_SUPPORTED, True),
    ("monochrome destination", (RGBA8, True), (R1, True), (0, 0, 5, 3), (0, 0), E_NOT_SUPPORTED, True),
    ("the rectangle before monochrome", (R1, True), (R1, True), (1, 1, 0, 3), (1, 1), E_INVALIDARG, True),
    # this project's additions
    ("typeless", (RGBA8_TYPELESS, True), (RGBA8_TYPELESS, True), (1, 1, 5, 3), (1, 1), E_NOT_SUPPORTED, False),
    ("packed pairs between formats", (YUY2, True), (RGBA8, True), (0, 0, 4, 3), (0, 0), E_NOT_SUPPORTED, False),
]


@pytest.mark.parametrize("case", ERRORS, ids=lambda c: c[0].replace(" ", "_"))
def test_hresults(ctx, oracle, case):
    _, (sfmt, spix), (dfmt, dpix), rect, off, expected, in_reference = case
    src = np.zeros(7 * 5 * 16, np.uint8) if spix else None
    dst = np.zeros(7 * 5 * 16, np.uint8) if dpix else None
    sdims, ddims = (7, 5, sfmt, 7 * TEXEL_BYTES.get(sfmt, 4)), (7, 5, dfmt, 7 * TEXEL_BYTES.get(dfmt, 4))
    got = _hr(ctx, src, sdims, rect, dst, ddims, off)
    assert got == _signed(expected), hex(got & 0xFFFFFFFF)
    if in_reference:
        hr, _ = R.copy_rectangle(oracle, src, sdims, rect, dst, ddims, 0, *off)
        assert got == hr, (hex(got & 0xFFFFFFFF), hex(hr & 0xFFFFFFFF))
    if dst is not None:
        assert not dst.any()            # a refused call writes nothing


def test_overlap_is_refused(ctx):
    """This project's convention: E_INVALIDARG where the bytes read and the bytes written intersect; disjoint rectangles of ONE image are fine."""
    buf = np.arange(16 * 16 * 4, dtype=np.uint32).view(np.uint8)[:16 * 16 * 4].copy()
    dims = (16, 16, RGBA8, 64)
    assert _hr(ctx, buf, dims, (0, 0, 8, 8), buf, dims, (4, 4)) == _signed(E_INVALIDARG)
    before = buf.copy()
    assert _hr(ctx, buf, dims, (0, 0, 8, 4), buf, dims, (8, 8)) == 0
    want = before.reshape(16, 64).copy()
    want[8:12, 32:64] = before.reshape(16, 64)[0:4, 0:32]
    assert np.array_equal(buf.reshape(16, 64), want)


def test_bytes_past_the_image_fail(ctx, oracle):
    """YUY2 counts 4 bytes per texel: a rectangle that ends in the image's last row runs past rowPitch * height. E_FAIL, as in the reference."""
    src, dst = np.zeros(8 * 4 * 2, np.uint8), np.zeros(8 * 4 * 2, np.uint8)
    dims = (8, 4, YUY2, 16)
    got = _hr(ctx, src, dims, (2, 1, 6, 3), dst, dims, (2, 1))
    hr, _ = R.copy_rectangle(oracle, src, dims, (2, 1, 6, 3), dst, dims, 0, 2, 1)
    assert got == _signed(E_FAIL) == hr


# ---- the host-pointer form moves the rectangle only ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(RGBA8, RGBA8), (RGBA8, RGBA16F), (RGB32F, RGB32F), (YUY2, YUY2)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_host_form_transfers(ctx, oracle, pair):
    sfmt, dfmt = pair
    src, sdims, rect, dst, ddims, off = _case(np.random.default_rng(sfmt + dfmt), sfmt, dfmt, SHAPES[2], 3 if sfmt == dfmt else 0)
    hr, want = R.copy_rectangle(oracle, src, sdims, rect, dst, ddims, 0, *off)
    assert hr == 0
    got = dst.copy()
    ctx.transfer_bytes(reset=True)
    ctx.copy_rectangle(_host_image(src, sdims), rect, _host_image(got, ddims), 0, *off)
    up, down = ctx.transfer_bytes()
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert up == rect[2] * rect[3] * TEXEL_BYTES[sfmt] and down == rect[2] * rect[3] * TEXEL_BYTES[dfmt], (up, down)
    assert ctypes.sizeof(capi.Rect) == 4 * ctypes.sizeof(ctypes.c_size_t)
