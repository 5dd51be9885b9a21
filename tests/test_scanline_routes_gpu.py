"""Every kernel route of the scanline launchers (launch_convert, launch_pack_group, launch_resize, launch_resize_tail, launch_mse in
scanline.hip) against the reference's own drivers, at the shapes, formats and flags that select each route.

The launchers pick a kernel from the shape, the formats and the alignment of the call. Each call here runs between profile_begin() and
profile_end(), whose kernel names (the marks the launchers record) prove which route ran; the output is then compared with the oracle:
byte-identical, or, where sRGB curves (powf) are involved, within one 8-bit step or one ulp of a float word on fewer than 1 % of words.

launch_resize_tail has two bodies, the generic tail and the LDS halving tail, and resize_tail_route() decides between them and the per-level
kernels for the C ABI and the launcher alike: a cubic chain that is no exact-halving RGBA8 clamp chain stays on resize_cubic /
resize_cubic_half_rgba8[_x2] (the CUBIC rows below), and a chain the predicate rejects is an error in launch_resize_tail.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_scanline_parity import _float_texels  # noqa: E402

pytestmark = pytest.mark.gpu

RGBA32F, RGBA32U, RGB32F, RGBA16F, RGBA16UN, RGBA8, RGBA8S, BGRA8, BGRX8, BGRA8S, R8 = 2, 3, 6, 10, 11, 28, 29, 87, 88, 91, 61
RG16F, RGB10A2, R11G11B10F, RGB9E5, B5G6R5, D32F, RGBG = 34, 24, 26, 67, 85, 40, 68
POINT, LINEAR, CUBIC, BOX, TRIANGLE = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
WRAP, MIRROR = 0x3, 0x30
X2BIAS, COPY_GREEN, COPY_ALPHA, DITHER, SRGB_IN, SRGB_OUT = 0x200, 0x2000, 0x8000, 0x10000, 0x1000000, 0x2000000
SRGB = SRGB_IN | SRGB_OUT

# DXTEX_QUAD_FORMATS (scanline.hip): every format whose texel is a whole number of dwords, with the bytes of a quad of four texels
QUAD_BYTES = {2: 64, 3: 64, 4: 64, 6: 48, 7: 48, 8: 48, 10: 32, 11: 32, 12: 32, 13: 32, 14: 32, 16: 32, 17: 32, 18: 32, 102: 32,
              24: 16, 25: 16, 26: 16, 28: 16, 29: 16, 30: 16, 31: 16, 32: 16, 34: 16, 35: 16, 36: 16, 37: 16, 38: 16, 41: 16, 42: 16,
              43: 16, 67: 16, 87: 16, 88: 16, 89: 16, 91: 16, 93: 16, 100: 16, 101: 16, 20: 32, 40: 16, 45: 16}
SRGB_FORMATS = {29, 91, 93}
EIGHT_BIT = {28, 29, 87, 88, 91, 93}                    # the 8-bit UNORM colour formats TEX_FILTER_SRGB_IN / OUT applies to
# the float channels of a format (dword or half-word elements) that must stay finite / carry the edge values
FLOAT32_WORDS = {2: 4, 6: 3, 16: 2, 41: 1, 40: 1}
FLOAT16_WORDS = {10: 4, 34: 2}


def _edges(rng, h, w, dtype):
    """_float_texels' values for an image of any width: its eight edge texels come first in row-major order."""
    return _float_texels(rng, h, max(w, 8), dtype).reshape(-1, 4)[:h * w].reshape(h, w, 4)


def _texels(oracle, rng, fmt, w, h):
    """Random bits for integer and packed formats; _float_texels' edge values for float channels; finite R11G11B10."""
    img = rng.integers(0, 256, oracle.image_bytes(fmt, w, h), dtype=np.uint8)
    if fmt in FLOAT32_WORDS:
        return np.ascontiguousarray(_edges(rng, h, w, np.float32)[..., :FLOAT32_WORDS[fmt]]).view(np.uint8).reshape(-1)
    if fmt in FLOAT16_WORDS:
        return np.ascontiguousarray(_edges(rng, h, w, np.float16)[..., :FLOAT16_WORDS[fmt]]).view(np.uint8).reshape(-1)
    if fmt == 20:              # D32_FLOAT_S8X24_UINT: a float depth, then stencil and padding bits
        d = img.view(np.uint32).reshape(h, w, 2).copy()
        d[..., 0] = _edges(rng, h, w, np.float32)[..., 0].view(np.uint32)
        return d.view(np.uint8).reshape(-1)
    if fmt == R11G11B10F:
        return (img.view(np.uint32) & np.uint32(~((1 << 10) | (1 << 21) | (1 << 31)) & 0xFFFFFFFF)).view(np.uint8)
    return img


def _smooth(oracle, rng, fmt, w, h):
    """Finite, filter-friendly texels for the mip / resize tests (no inf or NaN, whose payloads the filters need not agree on)."""
    if fmt in FLOAT32_WORDS:
        return (rng.random((h, w, FLOAT32_WORDS[fmt]), dtype=np.float32) * 4 - 0.5).astype(np.float32).view(np.uint8).reshape(-1)
    if fmt in FLOAT16_WORDS:
        return (rng.random((h, w, FLOAT16_WORDS[fmt]), dtype=np.float32) * 4 - 0.5).astype(np.float16).view(np.uint8).reshape(-1)
    if fmt == D32F:
        return rng.random((h, w), dtype=np.float32).view(np.uint8).reshape(-1)
    return _texels(oracle, rng, fmt, w, h)


def _profiled(ctx, fn):
    """-> (fn(), set of the kernel names the launchers marked while it ran)."""
    ctx.profile_begin()
    try:
        out = fn()
    finally:
        names = ctx.profile_end()
    return out, set(names)


def _diff(got, ref):
    return np.nonzero(got.reshape(-1) != ref.reshape(-1))[0][:8]


# The channels of the remaining formats, for _within_srgb_bar: whole-element channels by element type, and the bit fields (low bits first)
# of the packed ones. Float channels are compared as their words (one step = one ulp); D32_FLOAT_S8X24_UINT is a float word and a
# stencil word.
CHANNEL_WORDS = {np.uint32: (3, 7, 17, 42, 20), np.int32: (4, 8, 18, 43), np.uint16: (11, 12, 35, 36, 55, 56, 57, 102, 54),
                 np.int16: (13, 14, 37, 38, 58, 59), np.uint8: (30, 49, 50, 62, 65, 100), np.int8: (31, 32, 51, 52, 63, 64)}
CHANNEL_FIELDS = {24: (np.uint32, (10, 10, 10, 2)), 25: (np.uint32, (10, 10, 10, 2)), 89: (np.uint32, (10, 10, 10, 2)),
                  101: (np.uint32, (10, 10, 10, 2)), 26: (np.uint32, (11, 11, 10)), 45: (np.uint32, (24, 8)), 85: (np.uint16, (5, 6, 5)),
                  86: (np.uint16, (5, 5, 5, 1)), 115: (np.uint16, (4, 4, 4, 4)), 191: (np.uint16, (4, 4, 4, 4))}


def _channel_codes(raw, fmt):
    """-> [(int64 codes of one channel of every texel, bits of that channel)]"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    for word, formats in CHANNEL_WORDS.items():
        if fmt in formats:
            return [(raw.view(word).astype(np.int64), np.dtype(word).itemsize * 8)]
    word, fields = CHANNEL_FIELDS[fmt]
    v = raw.view(word).astype(np.int64)
    out, at = [], 0
    for bits in fields:
        out.append(((v >> at) & ((1 << bits) - 1), bits))
        at += bits
    return out


def _within_srgb_bar(got, ref, fmt):
    """sRGB curves go through powf on both sides: one 8-bit step for 8-bit UNORM, else at most one ulp of a float word on < 1 % of words.
    Every other format by its channels: at most one quantisation step of the channel (one ulp of a float channel), and channels wider
    than 8 bits differ on fewer than 1 % of their values."""
    if fmt in EIGHT_BIT or fmt == R8:
        return int(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max(initial=0)) <= 1
    if fmt in FLOAT32_WORDS or fmt in FLOAT16_WORDS:
        word = np.uint32 if fmt in FLOAT32_WORDS else np.uint16
        g = got.view(word).astype(np.int64); r = ref.view(word).astype(np.int64)
        return int(np.abs(g - r).max(initial=0)) <= 1 and float((g != r).mean()) < 0.01
    if fmt == RGB9E5:
        # mantissa * 2^exponent as integers: one step of the coarser of the two shared exponents
        g = np.ascontiguousarray(got).view(np.uint32).astype(np.int64); r = np.ascontiguousarray(ref).view(np.uint32).astype(np.int64)
        step = np.int64(1) << np.maximum(g >> 27, r >> 27)
        near = all((np.abs((((g >> s) & 511) << (g >> 27)) - (((r >> s) & 511) << (r >> 27))) <= step).all() for s in (0, 9, 18))
        return bool(near) and float((g != r).mean()) < 0.01
    wide_diff, wide_n = 0, 0
    for (g, bits), (r, _) in zip(_channel_codes(got, fmt), _channel_codes(ref, fmt)):
        if int(np.abs(g - r).max(initial=0)) > 1:
            return False
        if bits > 8:
            wide_diff += int((g != r).sum()); wide_n += g.size
    return wide_n == 0 or wide_diff / wide_n < 0.01


class Device:
    """Device buffers of the context, freed on exit."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, raw, nbytes=None):
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        p = self.ctx.device_alloc(max(1, nbytes or raw.nbytes), zero=True)
        self.ptrs.append(p)
        self.ctx.upload(p, raw, sync=True)
        return p

    def put_rows(self, raw, rows, row_bytes, pitch):
        """raw (tight rows) -> a device image whose rows are `pitch` bytes apart."""
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(rows, row_bytes)
        padded = np.zeros((rows, pitch), np.uint8)
        padded[:, :row_bytes] = raw
        return self.put(padded)

    def empty(self, nbytes):
        p = self.ctx.device_alloc(max(1, nbytes), zero=True)
        self.ptrs.append(p)
        return p

    def get(self, p, nbytes):
        self.ctx.synchronize()
        out = np.zeros(nbytes, np.uint8)
        self.ctx.download(out, p, sync=True)
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.synchronize()
        for p in self.ptrs:
            self.ctx.device_free(p)


# ---- a. the route table ---------------------------------------------------------------------------------------------------------
def _run_convert(ctx, oracle, src, dst, w, h, flags):
    img = _texels(oracle, np.random.default_rng(src * 131 + dst * 7 + flags % 97 + w), src, w, h)
    got, names = _profiled(ctx, lambda: ctx.convert(img, w, h, src, dst, flags, 0.5))
    return got, oracle.ref_convert(img, w, h, src, dst, flags, 0.5), names


def _run_resize(ctx, oracle, fmt, size, new_size, flt):
    (w, h), (nw, nh) = size, new_size
    img = _smooth(oracle, np.random.default_rng(fmt + w * 3 + nw), fmt, w, h)
    got, names = _profiled(ctx, lambda: ctx.resize(img, w, h, fmt, nw, nh, flt))
    return got, oracle.ref_resize(img, w, h, fmt, nw, nh, flt), names


def _run_mips(ctx, oracle, fmt, size, flt):
    w, h = size
    n = _levels(w, h)
    img = _smooth(oracle, np.random.default_rng(fmt * 5 + w + h), fmt, w, h)
    got, names = _profiled(ctx, lambda: ctx.generate_mips(img, w, h, fmt, n, flt))
    return np.concatenate(got), np.concatenate(oracle.ref_generate_mips(img, w, h, fmt, flt, n)), names


def _run_mse(ctx, oracle, fa, fb, w, h):
    rng = np.random.default_rng(fa * 17 + fb)
    a, b = _texels(oracle, rng, fa, w, h), _texels(oracle, rng, fb, w, h)
    with Device(ctx) as d:
        pa, pb = d.put(a), d.put(b)
        got, names = _profiled(ctx, lambda: ctx.compute_mse_device(pa, fa, pb, fb, w, h))
    return got, _mse64(oracle, a, fa, b, fb, w, h), names


def _levels(w, h):
    n = 1
    while w > 1 or h > 1:
        w, h = max(1, w >> 1), max(1, h >> 1); n += 1
    return n


Q = "convert_quad<{}>"
ROUTES = [
    # launch_convert: the nine quad instantiations <SQ, DQ, ROWS> (bytes of a source / destination quad; 0 = R32G32B32 or 64 -> 64)
    (Q.format("16,16,4"), ("convert", RGBA8, BGRA8, 64, 9, 0)),
    (Q.format("16,32,4"), ("convert", RGBA8, RGBA16F, 64, 9, 0)),
    (Q.format("16,64,4"), ("convert", RGBA8, RGBA32F, 64, 9, 0)),
    (Q.format("32,16,2"), ("convert", RGBA16F, RGBA8, 64, 9, 0)),
    (Q.format("32,32,2"), ("convert", RGBA16F, RGBA16UN, 64, 9, 0)),
    (Q.format("32,64,2"), ("convert", RGBA16F, RGBA32F, 64, 9, 0)),
    (Q.format("64,16,1"), ("convert", RGBA32F, RGBA8, 64, 9, 0)),
    (Q.format("64,32,1"), ("convert", RGBA32F, RGBA16F, 64, 9, 0)),
    (Q.format("0,0,1"), ("convert", RGBA32F, RGB32F, 64, 9, 0)),
    (Q.format("0,0,1"), ("convert", RGB32F, RGBA8, 64, 9, 0)),
    (Q.format("0,0,1"), ("convert", RGBA32F, RGBA32U, 64, 9, 0)),
    # ... and with ordered dithering, from float sources into dithered stores where the format has one
    (Q.format("16,16,4,dither"), ("convert", RG16F, RGBA8, 64, 9, DITHER)),
    (Q.format("16,32,4,dither"), ("convert", RG16F, RGBA16UN, 64, 9, DITHER)),
    (Q.format("16,64,4,dither"), ("convert", RG16F, RGBA32F, 64, 9, DITHER)),
    (Q.format("32,16,2,dither"), ("convert", RGBA16F, RGBA8, 64, 9, DITHER)),
    (Q.format("32,32,2,dither"), ("convert", RGBA16F, RGBA16UN, 64, 9, DITHER)),
    (Q.format("32,64,2,dither"), ("convert", RGBA16F, RGBA32F, 64, 9, DITHER)),
    (Q.format("64,16,1,dither"), ("convert", RGBA32F, RGB10A2, 64, 9, DITHER)),
    (Q.format("64,32,1,dither"), ("convert", RGBA32F, RGBA16UN, 64, 9, DITHER)),
    (Q.format("0,0,1,dither"), ("convert", RGB32F, RGBA8, 64, 9, DITHER)),
    # the one-texel kernel: a format that is not whole dwords, a width that is not a multiple of 4
    ("convert", ("convert", RGBA8, R8, 61, 19, 0)),
    ("convert", ("convert", RGBA16F, RGBA8, 61, 19, 0)),
    ("convert<dither>", ("convert", RGBA32F, R8, 61, 19, DITHER)),
    ("convert<dither>", ("convert", RGBA16F, RGBA8, 63, 9, DITHER)),
    # launch_pack_group: a destination whose element holds two texels, after Convert and after a mip level
    ("pack_group", ("convert", RGBA8, RGBG, 61, 19, 0)),
    ("pack_group", ("mips", RGBG, (160, 96), LINEAR)),
    # launch_resize
    ("resize_point", ("resize", RGBA16F, (64, 48), (32, 24), POINT)),
    ("resize_linear", ("resize", RGBA16F, (64, 48), (100, 31), LINEAR)),
    ("resize_cubic", ("resize", RGBA16F, (64, 48), (100, 31), CUBIC)),
    ("resize_cubic", ("resize", RGBA8, (64, 48), (32, 24), CUBIC | MIRROR)),
    ("resize_cubic_half_rgba8_x2", ("resize", RGBA8, (128, 64), (64, 32), CUBIC)),
    ("resize_cubic_half_rgba8", ("resize", RGBA8, (70, 40), (35, 20), CUBIC)),
    ("resize_box", ("resize", RGBA16F, (64, 64), (32, 32), BOX)),
    ("resize_box", ("resize", RGBA8, (256, 64), (128, 32), BOX)),
    ("resize_box_half_rgba8", ("resize", RGBA8, (1024, 8), (512, 4), BOX)),
    ("resize_box_half_rgba8", ("mips", RGBA8, (1024, 8), BOX)),
    ("resize_triangle", ("resize", RGBA16F, (64, 48), (100, 31), TRIANGLE)),
    # launch_resize_tail
    ("resize_tail", ("mips", RGBA16F, (64, 64), LINEAR)),
    ("resize_tail", ("mips", RGBA8, (64, 32), POINT)),
    ("resize_half_tail_rgba8<cubic>", ("mips", RGBA8, (64, 64), CUBIC)),
    ("resize_half_tail_rgba8<box>", ("mips", RGBA8, (64, 64), BOX)),
    # launch_mse
    ("mse", ("mse", RGBA8, BGRA8, 64, 32)),
    # launch_resize_tail, the box filter's stale tap on the W x 1 levels: the two-high level it reads is one the tail itself wrote (32 x 2),
    # the tail's own first source (64 x 2), or a level before the tail that the host hands in (256 x 2, two per-level launches first).
    # The W x 1 levels are no exact halvings, so RGBA8 takes the generic tail here too.
    ("resize_tail", ("mips", RGBA16F, (64, 4), BOX)),
    ("resize_tail", ("mips", RGBA8, (64, 4), BOX)),
    ("resize_tail", ("mips", RGBA16F, (128, 4), BOX)),
    ("resize_tail", ("mips", RGBA8, (128, 4), BOX)),
    ("resize_tail", ("mips", RGBA16F, (256, 2), BOX)),
    ("resize_tail", ("mips", RGBA8, (256, 2), BOX)),
]


@pytest.mark.parametrize("route,call", ROUTES, ids=[f"{r}-{i}" for i, (r, _) in enumerate(ROUTES)])
def test_route(ctx, oracle, route, call):
    kind, *args = call
    if kind == "convert":
        got, ref, names = _run_convert(ctx, oracle, *args)
    elif kind == "resize":
        got, ref, names = _run_resize(ctx, oracle, *args)
    elif kind == "mips":
        got, ref, names = _run_mips(ctx, oracle, *args)
    else:
        got, ref, names = _run_mse(ctx, oracle, *args)
    assert route in names, (route, sorted(names))
    if route == "resize_tail":
        assert "resize_half_tail_rgba8<box>" not in names, sorted(names)
    if kind == "mse":
        assert np.allclose(got, ref, rtol=1e-6, atol=0), (got, ref)
    else:
        assert np.array_equal(got, ref), (route, call, _diff(got, ref))


# ---- b. Convert on the quad domain -------------------------------------------------------------------------------------------------
SHAPES = [(68, 7), (4, 3), (64, 1), (1028, 5)]
FLAGS = [0, X2BIAS, COPY_GREEN, COPY_ALPHA, DITHER]


def _partners(fmt):
    """RGBA32F (R32G32B32_FLOAT for RGBA32F itself) and a format of another quad width."""
    other = {16: RGBA16F, 32: RGBA8, 48: RGBA16F, 64: RGBA8}[QUAD_BYTES[fmt]]
    return [RGB32F if fmt == RGBA32F else RGBA32F, other]


def _quad_name(src, dst, flags):
    sq, dq = QUAD_BYTES[src], QUAD_BYTES[dst]
    rows = {16: 4, 32: 2, 64: 1, 48: 1}[sq]
    if (sq, dq) not in {(a, b) for a in (16, 32, 64) for b in (16, 32, 64)} - {(64, 64)}:
        sq, dq, rows = 0, 0, 1
    return f"convert_quad<{sq},{dq},{rows}{',dither' if flags & DITHER else ''}>"


def _check_convert(ctx, oracle, img, w, h, src, dst, flags, route, fails, tag):
    try:
        ref = oracle.ref_convert(img, w, h, src, dst, flags, 0.5)
    except oracle.RefError as e:
        try:
            _profiled(ctx, lambda: ctx.convert(img, w, h, src, dst, flags, 0.5))
            fails.append((tag, src, dst, hex(flags), (w, h), f"the reference refuses ({e}) but the GPU path accepted"))
        except dx.DxtexError:
            pass
        return None
    got, names = _profiled(ctx, lambda: ctx.convert(img, w, h, src, dst, flags, 0.5))
    if route not in names:
        fails.append((tag, src, dst, hex(flags), (w, h), "route", route, sorted(names)))
    srgb = (flags & SRGB) or src in SRGB_FORMATS or dst in SRGB_FORMATS
    if not (np.array_equal(got, ref) or (srgb and _within_srgb_bar(got, ref, dst))):
        fails.append((tag, src, dst, hex(flags), (w, h), "bytes", _diff(got, ref)))
    return ref


def _convert_cases(fmt, role):
    cases = []
    for p in _partners(fmt):
        src, dst = (fmt, p) if role == "src" else (p, fmt)
        flags = list(FLAGS)
        if src in EIGHT_BIT or dst in EIGHT_BIT:
            flags += [SRGB_IN, SRGB_OUT, SRGB]
        cases += [(src, dst, f) for f in flags]
    return cases


@pytest.mark.parametrize("role", ["src", "dst"])
@pytest.mark.parametrize("fmt", sorted(QUAD_BYTES))
def test_convert_quad_domain(ctx, oracle, fmt, role):
    """Each quad format as source and as destination, against RGBA32F and a format of another quad width, under every Convert flag
    that changes the arithmetic; widths that are multiples of 4 with short last row groups, and 1028 (two workgroup columns). The same
    data again through the one-texel kernel: at width + 1, and through dxtex_convert_slice_device with a source pitch one texel longer."""
    fails = []
    for i, (src, dst, flags) in enumerate(_convert_cases(fmt, role)):
        w, h = SHAPES[i % len(SHAPES)]
        rng = np.random.default_rng(fmt * 1000 + src * 31 + dst * 7 + i)
        img = _texels(oracle, rng, src, w + 1, h)
        quad = np.ascontiguousarray(img.reshape(h, -1)[:, :oracle.image_bytes(src, w, 1)])
        ref = _check_convert(ctx, oracle, quad, w, h, src, dst, flags, _quad_name(src, dst, flags), fails, "quad")
        _check_convert(ctx, oracle, img, w + 1, h, src, dst, flags, "convert<dither>" if flags & DITHER else "convert", fails, "w+1")
        texel = QUAD_BYTES[src] // 4
        if ref is not None and flags == 0 and (w * texel + texel) % 16:
            row = w * texel
            with Device(ctx) as d:
                ps = d.put_rows(quad, h, row, row + texel)
                pd = d.empty(ref.nbytes)
                _, names = _profiled(ctx, lambda: ctx.convert_device(ps, w, h, src, pd, dst, flags, 0.5, 0, row + texel))
                got = d.get(pd, ref.nbytes)
            srgb = src in SRGB_FORMATS or dst in SRGB_FORMATS
            if "convert" not in names:
                fails.append(("pitch", src, dst, (w, h), "route", sorted(names)))
            if not (np.array_equal(got, ref) or (srgb and _within_srgb_bar(got, ref, dst))):
                fails.append(("pitch", src, dst, (w, h), "bytes", _diff(got, ref)))
    assert not fails, fails[:6]


@pytest.mark.parametrize("src,dst,w,h,flags", [
    (RGBA8, RGBA16F, 4, 32773, 0),              # ROWS = 4: 8194 row groups, more than one grid's 8192 rows
    (RGBA16F, RGBA8, 4, 16387, DITHER),         # ROWS = 2: 8194 row groups, with the dither row carried through the stride
    (RGBA32F, RGBA8, 4, 8195, DITHER),          # ROWS = 1: 8195 row groups
    (RGBA32F, RGBA8, 4, 8195, 0),
])
def test_convert_quad_y_stride(ctx, oracle, src, dst, w, h, flags):
    fails = []
    rng = np.random.default_rng(h)
    img = _texels(oracle, rng, src, w, h)
    _check_convert(ctx, oracle, img, w, h, src, dst, flags, _quad_name(src, dst, flags), fails, "stride")
    assert not fails, fails


# ---- c. GenerateMipMaps above the tail ---------------------------------------------------------------------------------------------
MIP_FORMATS = [RGBA16F, RGBA32F, R8, BGRA8, RGBA8S, RGB10A2, R11G11B10F, RGB9E5, B5G6R5, RGB32F, D32F, RGBG]
MIP_SIZES = [(160, 96), (256, 130), (512, 2), (1, 200), (256, 128)]
MIP_FILTERS = [POINT, LINEAR, BOX, CUBIC, TRIANGLE, LINEAR | WRAP, LINEAR | MIRROR, CUBIC | WRAP, CUBIC | MIRROR]
LEVEL_ROUTE = {POINT: "resize_point", LINEAR: "resize_linear", BOX: "resize_box"}


@pytest.mark.parametrize("size", MIP_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", MIP_FORMATS)
def test_generate_mips_above_tail(ctx, oracle, fmt, size):
    """Top levels wider or taller than 64 run the per-level kernels; point / linear / box chains then finish in resize_tail (grouped
    formats never take the tail). 512 x 2 under BOX reaches the stale-row tap of resize_box_kernel on a format other than RGBA8."""
    w, h = size
    pow2 = (w & (w - 1)) == 0 and (h & (h - 1)) == 0
    n = _levels(w, h)
    img = _smooth(oracle, np.random.default_rng(fmt * 3 + w + h), fmt, w, h)
    fails = []
    for flt in MIP_FILTERS:
        if (flt & 0xF00000) == BOX and not pow2:
            continue
        if size == (256, 128) and (flt & 0xF00000) != BOX:
            continue                                   # the power-of-two 2-D size is here for the box filter
        got, names = _profiled(ctx, lambda: ctx.generate_mips(img, w, h, fmt, n, flt))
        ref = oracle.ref_generate_mips(img, w, h, fmt, flt, n)
        srgb = fmt in SRGB_FORMATS
        for lvl in range(n):
            if srgb and lvl and (flt & 0xF00000) != BOX:     # powf on both sides: each level from the GPU's previous one, so steps do not compound
                pw, ph = oracle.mip_sizes(w, h, n)[lvl - 1]
                ref[lvl] = oracle.ref_generate_mips(got[lvl - 1], pw, ph, fmt, flt, 2)[1]
            if not (np.array_equal(got[lvl], ref[lvl]) or (srgb and _within_srgb_bar(got[lvl], ref[lvl], fmt))):
                fails.append((hex(flt), lvl, "bytes", _diff(got[lvl], ref[lvl])))
        mode = flt & 0xF00000
        if mode in LEVEL_ROUTE:
            want = {LEVEL_ROUTE[mode]} | ({"pack_group"} if fmt == RGBG else {"resize_tail"})
            if not want <= names:
                fails.append((hex(flt), "routes", sorted(want), sorted(names)))
            if fmt == RGBG and "resize_tail" in names:
                fails.append((hex(flt), "a grouped format took the tail", sorted(names)))
    assert not fails, fails[:6]


# ---- d. sRGB filtering at size -------------------------------------------------------------------------------------------------------
SRGB_CASES = [(RGBA8S, 0), (RGBA8, SRGB), (RGBA16F, SRGB)]


@pytest.mark.parametrize("flt,size", [(POINT, (160, 96)), (LINEAR, (160, 96)), (CUBIC, (160, 96)), (TRIANGLE, (160, 96)), (BOX, (256, 256)),
                                      (CUBIC, (128, 128)), (LINEAR | WRAP, (130, 70))])
@pytest.mark.parametrize("fmt,extra", SRGB_CASES)
def test_generate_mips_srgb_at_size(ctx, oracle, fmt, extra, flt, size):
    """Each level against the reference run from the GPU's previous level (levels=2), so that differences cannot compound down the chain:
    one 8-bit step, or one ulp on fewer than 1 % of half words. Square box sizes keep the chain off the W x 1 stale-row quirk."""
    w, h = size
    n = _levels(w, h)
    img = _smooth(oracle, np.random.default_rng(fmt + w), fmt, w, h)
    got = ctx.generate_mips(img, w, h, fmt, n, flt | extra)
    sizes = oracle.mip_sizes(w, h, n)
    for lvl in range(1, n):
        (pw, ph) = sizes[lvl - 1]
        ref = oracle.ref_generate_mips(got[lvl - 1], pw, ph, fmt, flt | extra, 2)[1]
        assert _within_srgb_bar(got[lvl], ref, fmt), (hex(flt | extra), lvl, _diff(got[lvl], ref))


@pytest.mark.parametrize("flt,dims", [(POINT, ((160, 96), (70, 50))), (LINEAR, ((160, 96), (70, 50))), (CUBIC, ((160, 96), (70, 50))),
                                      (TRIANGLE, ((160, 96), (70, 50))), (BOX, ((256, 128), (128, 64))), (CUBIC, ((256, 128), (128, 64)))])
@pytest.mark.parametrize("fmt,extra", SRGB_CASES)
def test_resize_srgb_at_size(ctx, oracle, fmt, extra, flt, dims):
    (w, h), (nw, nh) = dims
    img = _smooth(oracle, np.random.default_rng(fmt + nw), fmt, w, h)
    got = ctx.resize(img, w, h, fmt, nw, nh, flt | extra)
    ref = oracle.ref_resize(img, w, h, fmt, nw, nh, flt | extra)
    assert _within_srgb_bar(got, ref, fmt), (hex(flt | extra), _diff(got, ref))


# ---- e. Resize -------------------------------------------------------------------------------------------------------------------------
RESIZE_DIMS = [((160, 96), (70, 50)), ((64, 48), (100, 31)), ((70, 40), (35, 20)), ((1024, 8), (512, 4)), ((256, 128), (128, 64))]
RESIZE_FILTERS = [POINT, LINEAR, CUBIC, TRIANGLE, BOX, LINEAR | WRAP, CUBIC | MIRROR]


@pytest.mark.parametrize("dims", RESIZE_DIMS, ids=lambda d: f"{d[0][0]}x{d[0][1]}-{d[1][0]}x{d[1][1]}")
@pytest.mark.parametrize("fmt", [RGBA16F, R8, BGRA8, RGBA8S, RGB10A2, RGBA8])
def test_resize_formats(ctx, oracle, fmt, dims):
    (w, h), (nw, nh) = dims
    img = _smooth(oracle, np.random.default_rng(fmt * 7 + w + nw), fmt, w, h)
    fails = []
    for flt in RESIZE_FILTERS:
        if (flt & 0xF00000) == BOX and (w != 2 * nw or h != 2 * nh):
            continue
        got = ctx.resize(img, w, h, fmt, nw, nh, flt)
        ref = oracle.ref_resize(img, w, h, fmt, nw, nh, flt)
        if not (np.array_equal(got, ref) or (fmt in SRGB_FORMATS and _within_srgb_bar(got, ref, fmt))):
            fails.append((hex(flt), _diff(got, ref)))
    assert not fails, fails


@pytest.mark.parametrize("flt,dims,src_pad,dst_pad,route", [
    (CUBIC, ((128, 32), (64, 16)), 4, 0, "resize_cubic_half_rgba8"),      # source pitch not a multiple of 16: no pairs
    (CUBIC, ((128, 32), (64, 16)), 0, 4, "resize_cubic_half_rgba8"),      # destination pitch not a multiple of 8
    (CUBIC, ((128, 32), (64, 16)), 16, 8, "resize_cubic_half_rgba8_x2"),
    (BOX, ((1024, 8), (512, 4)), 4, 0, "resize_box"),                     # the 2:1 RGBA8 box needs 16-byte source rows
    (BOX, ((1024, 8), (512, 4)), 16, 8, "resize_box_half_rgba8"),
])
def test_resize_device_pitch(ctx, oracle, flt, dims, src_pad, dst_pad, route):
    """dxtex_resize_device with padded pitches: the RGBA8 2:1 kernels' admission rules, and the rows they then read and write."""
    (w, h), (nw, nh) = dims
    img = _smooth(oracle, np.random.default_rng(w + src_pad + dst_pad), RGBA8, w, h)
    ref = oracle.ref_resize(img, w, h, RGBA8, nw, nh, flt).reshape(nh, nw * 4)
    sp, dp = w * 4 + src_pad, nw * 4 + dst_pad
    with Device(ctx) as d:
        ps = d.put_rows(img, h, w * 4, sp)
        pd = d.empty(dp * nh)
        src = dx.Image(w, h, RGBA8, sp, sp * h, ps)
        dst = dx.Image(nw, nh, RGBA8, dp, dp * nh, pd)
        hr, names = _profiled(ctx, lambda: ctx._lib.dxtex_resize_device(ctx._h, ctypes.byref(src), ctypes.byref(dst), flt))
        assert hr == 0, hex(hr & 0xFFFFFFFF)
        got = d.get(pd, dp * nh).reshape(nh, dp)
    assert route in names, (route, sorted(names))
    assert np.array_equal(got[:, :nw * 4], ref), _diff(got[:, :nw * 4], ref)
    assert not got[:, nw * 4:].any()                                      # the padding is not written


# ---- f. ComputeMSE -----------------------------------------------------------------------------------------------------------------
def _mse64(oracle, a, fa, b, fb, w, h):
    """ComputeMSE (DirectXTexMisc.cpp:27-176) restated in float64 over LoadScanline's floats: sRGB images raised to g_Gamma22 =
    (2.2, 2.2, 2.2, 1) with powf, alpha ignored where either image is B8G8R8X8."""
    va, vb = oracle.load_image(a, w, h, fa), oracle.load_image(b, w, h, fb)
    for v, f in ((va, fa), (vb, fb)):
        if f in SRGB_FORMATS:
            v[..., :3] = np.power(v[..., :3], np.float32(2.2))
    d = va.astype(np.float64) - vb.astype(np.float64)
    if {fa, fb} & {BGRX8, 93}:
        d[..., 3] = 0
    return (d * d).reshape(-1, 4).mean(axis=0)


@pytest.mark.parametrize("size", [(1, 1), (257, 3), (300, 1500)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fa,fb", [(RGBA8, RGBA8S), (BGRA8S, BGRA8), (BGRX8, RGBA8), (RGBA16F, RGBA32F), (R8, RGBA8), (RGBG, RGBA8)])
def test_compute_mse_formats(ctx, oracle, fa, fb, size):
    """Random alpha: the sRGB exponent must leave alpha alone, B8G8R8X8 must drop it. 300 x 1500 runs mse_kernel's row stride."""
    w, h = size
    rng = np.random.default_rng(fa * 11 + fb + w)

    def image(f):
        if f in (RGBA16F, RGBA32F):
            v = rng.random((h, w, 4), dtype=np.float32)
            return v.astype(np.float16 if f == RGBA16F else np.float32).view(np.uint8).reshape(-1)
        return rng.integers(0, 256, oracle.image_bytes(f, w, h), dtype=np.uint8)

    a, b = image(fa), image(fb)
    with Device(ctx) as d:
        pa, pb = d.put(a), d.put(b)
        got, names = _profiled(ctx, lambda: ctx.compute_mse_device(pa, fa, pb, fb, w, h))
    assert "mse" in names
    want = _mse64(oracle, a, fa, b, fb, w, h)
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)
    ref32 = oracle.ref_compute_mse(a, fa, b, fb, w, h)
    assert np.allclose(got, ref32, rtol=2e-4, atol=0), (got, ref32)        # the reference accumulates in fp32, serially
