"""The four console formats - 116 R10G10B10_7E3_A2_FLOAT, 117 R10G10B10_6E4_A2_FLOAT, 189 R10G10B10_SNORM_A2_UNORM, 190 R4G4_UNORM -
through every scanline entry point, against the reference's own code (oracle/_ref). Byte equality unless a test says otherwise.
No NaN in any asserted input (tests/test_nonfinite_gpu.py); +-Inf, -0, negative values and fp32 denormals are asserted.

Where the existing suites check an operation against a numpy restatement (TransformImage, ComputeNormalMap, Analyze, Difference,
CopyRectangle, MergeImages), the formats are checked here by composition: the operation on format X must equal Convert X ->
R32G32B32A32_FLOAT, the same operation there, Convert back to X. Reading ConvertScanline (DirectXTexConvert.cpp:3453-3588) for these
Converts without flags: X -> RGBA32F reaches no branch for any of the four (the target is neither UNORM nor SNORM, and the
POS_ONLY branch needs TEX_FILTER_FLOAT_X2BIAS), so it is a pure load. RGBA32F -> 116 / 117 reaches none either: a pure store.
RGBA32F -> 189 clamps to [-1, 1] and RGBA32F -> 190 saturates; the stores of 189 and 190 clamp to the same or a narrower range
again, so without NaN those Converts store what a pure store would."""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx
from directxtex_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xbox_values as X  # noqa: E402
import nmap_ref  # noqa: E402
import oracle.dxtex_oracle as ox  # noqa: E402

pytestmark = pytest.mark.gpu

RGBA32F, RGBA16F, RGB10A2, R11G11B10F, RGBA8, RGBA8S, RG16UN, B5G6R5 = 2, 10, 24, 26, 28, 31, 35, 85
PARTNERS = [RGBA8, RGBA16F, RGB10A2, RGBA8S, R11G11B10F, RG16UN]
SRGB_IN, SRGB_OUT, X2BIAS, DITHER, DIFFUSION = 0x1000000, 0x2000000, 0x200, 0x10000, 0x20000
LINEAR, CUBIC, BOX, TRIANGLE = 0x200000, 0x300000, 0x400000, 0x500000
BC1, BC3, BC5U, BC5S, BC6HU, BC7 = 71, 77, 83, 84, 95, 98
ALPHA = (X.F7E3, X.F6E4, X.SN10)        # the three with an alpha field


def _diff(got, ref):
    return np.nonzero(np.asarray(got).reshape(-1) != np.asarray(ref).reshape(-1))[0][:8]


def _image(fmt, w, h, seed):
    """a source image of `fmt` without NaN: random bits where every pattern is a number, finite-or-infinite halves, finite R11G11B10"""
    rng = np.random.default_rng(seed)
    if fmt == RGBA16F or fmt == RGBA32F:
        v = (rng.random((h, w, 4), dtype=np.float32) * 3.0 - 1.0).astype(np.float32)
        v[rng.random((h, w, 4)) < 0.1] *= 300.0
        s = rng.random((h, w, 4))
        v[s < 0.01] = np.inf; v[(s >= 0.01) & (s < 0.02)] = -np.inf; v[(s >= 0.02) & (s < 0.04)] = -0.0
        v[(s >= 0.04) & (s < 0.05)] = 1e-41 if fmt == RGBA32F else 6e-8
        return v.astype(np.float16 if fmt == RGBA16F else np.float32).view(np.uint8).reshape(-1)
    raw = rng.integers(0, 256, ox.image_bytes(fmt, w, h), dtype=np.uint8)
    if fmt == R11G11B10F:
        return (raw.view(np.uint32) & np.uint32(~((1 << 10) | (1 << 21) | (1 << 31)) & 0xFFFFFFFF)).view(np.uint8)
    return raw


def _convert(ctx, raw, w, h, sf, df, flags=0, pitch=None, threshold=0.5):
    """dxtex_convert on host memory, the source rows `pitch` bytes apart"""
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    src = capi._host_image(raw, w, h, sf, pitch)
    rp, sp = dx.compute_pitch(df, w, h)
    out = np.zeros(sp, np.uint8)
    dst = dx.Image(w, h, df, rp, sp, out.ctypes.data)
    ctx._check(ctx._lib.dxtex_convert_slice(ctx._h, ctypes.byref(src), ctypes.byref(dst), flags, threshold, 0), "convert")
    return out


def _ref_convert(raw, w, h, sf, df, flags=0, pitch=0, threshold=0.5):
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    return ox._run(ox._load_ref().dxtex_ref_convert, ox.image_bytes(df, w, h), raw.ctypes.data, w, h, sf, pitch, df, flags, threshold)


def _padded(raw, w, h, fmt, pad):
    row = ox.image_bytes(fmt, w, 1)
    out = np.zeros((h, row + pad), np.uint8)
    out[:, :row] = np.asarray(raw).view(np.uint8).reshape(h, row)
    return out.reshape(-1), row + pad


def _hresult(fn):
    try:
        fn()
    except dx.DxtexError as e:
        return e.hresult & 0xFFFFFFFF
    except ox.RefError as e:
        return e.hresult & 0xFFFFFFFF
    return 0


# ---- 1. loads, exhaustive ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [X.F7E3, X.F6E4, X.SN10])
def test_load_every_code(ctx, oracle, fmt):
    w, h = 64, 48
    words = X.field_image(w * h)
    got = _convert(ctx, words, w, h, fmt, RGBA32F)
    assert np.array_equal(got, _ref_convert(words, w, h, fmt, RGBA32F)), _diff(got, _ref_convert(words, w, h, fmt, RGBA32F))


def test_load_every_byte_r4g4(ctx, oracle):
    px = np.arange(256, dtype=np.uint8)
    got = _convert(ctx, px, 16, 16, X.R4G4, RGBA32F)
    assert np.array_equal(got, _ref_convert(px, 16, 16, X.R4G4, RGBA32F))
    v = got.view(np.float32).reshape(256, 4)
    assert (v[:, 2] == 0).all() and (v[:, 3] == 1).all() and v[0x5A, 0] == np.float32(10) * np.float32(1 / 15) and v[0x5A, 1] == np.float32(5) * np.float32(1 / 15)


# ---- 2. stores, edges ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_image():
    """the value list of tests/test_xbox_formats_cpu.py plus k / 511 and k / 15 with neighbours and half-way points, 67 texels a row:
    an odd width, so the rows take the texel-per-lane kernel and every fourth row starts off a 16-byte boundary"""
    texels = X.store_texels(np.concatenate([X.small_float_values(), X.norm_values()]))
    img = X.as_image(texels, 67)
    assert not np.isnan(img).any()
    return np.ascontiguousarray(img)


@pytest.mark.parametrize("fmt", X.XBOX)
def test_store_edges(ctx, oracle, edge_image, fmt):
    h, w = edge_image.shape[:2]
    got = _convert(ctx, edge_image, w, h, RGBA32F, fmt)
    want = _ref_convert(edge_image, w, h, RGBA32F, fmt)
    assert np.array_equal(got, want), (fmt, _diff(got, want))


@pytest.mark.parametrize("fmt", X.XBOX)
def test_store_edges_quad_route(ctx, oracle, edge_image, fmt):
    """the same texels 64 wide with 16-byte aligned rows: the four-texels-per-lane kernel for the three 32-bit formats"""
    flat = edge_image.reshape(-1, 4)
    h = flat.shape[0] // 64
    img = np.ascontiguousarray(flat[:h * 64])
    got = _convert(ctx, img, 64, h, RGBA32F, fmt)
    want = _ref_convert(img, 64, h, RGBA32F, fmt)
    assert np.array_equal(got, want), (fmt, _diff(got, want))


# ---- 3. pairs ---------------------------------------------------------------------------------------------------------------------------
def _pair(ctx, sf, df, w=37, h=23, pad=12):
    raw = _image(sf, w, h, sf * 1000 + df)
    padded, pitch = _padded(raw, w, h, sf, pad)
    for flags in (0, SRGB_IN, SRGB_OUT, X2BIAS):
        got = _convert(ctx, padded, w, h, sf, df, flags, pitch)
        want = _ref_convert(padded, w, h, sf, df, flags, pitch)
        assert np.array_equal(got, want), (sf, df, hex(flags), _diff(got, want))


@pytest.mark.parametrize("partner", PARTNERS)
@pytest.mark.parametrize("fmt", X.XBOX)
def test_pairs_with_partners(ctx, oracle, fmt, partner):
    _pair(ctx, fmt, partner)
    _pair(ctx, partner, fmt)


@pytest.mark.parametrize("sf,df", [(a, b) for a in X.XBOX for b in X.XBOX if a != b])
def test_pairs_among_themselves(ctx, oracle, sf, df):
    _pair(ctx, sf, df)


def test_quad_route_pairs(ctx, oracle):
    """36 x 5 with 16-byte aligned rows: convert_quad, both directions, for the three 32-bit formats"""
    for fmt in ALPHA:
        for other in (RGBA8, RGBA16F, RGBA32F, RGB10A2):
            for sf, df in ((fmt, other), (other, fmt)):
                raw = _image(sf, 36, 5, sf * 7 + df)
                for flags in (0, X2BIAS, DITHER):
                    got, want = _convert(ctx, raw, 36, 5, sf, df, flags), _ref_convert(raw, 36, 5, sf, df, flags)
                    assert np.array_equal(got, want), (sf, df, hex(flags), _diff(got, want))


# ---- 4. dither ---------------------------------------------------------------------------------------------------------------------------
def _dither_source(sf, w, h, seed):
    if sf == RGBA8:
        return _image(RGBA8, w, h, seed)
    rng = np.random.default_rng(seed)
    v = (rng.random((h, w, 4), dtype=np.float32) * 2.6 - 1.3).astype(np.float32)
    ties = rng.random((h, w, 4)) < 0.2
    v[ties] = ((np.floor(v[ties] * np.float32(511)) + np.float32(0.5)) / np.float32(511)).astype(np.float32)
    s = rng.random((h, w, 4))
    v[s < 0.01] = np.inf; v[(s >= 0.01) & (s < 0.02)] = -np.inf; v[(s >= 0.02) & (s < 0.04)] = -0.0
    return v.view(np.uint8).reshape(-1)


@pytest.mark.parametrize("shape", [(37, 23), (4, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("flags", [DITHER, DIFFUSION], ids=["ordered", "diffusion"])
@pytest.mark.parametrize("sf", [RGBA32F, RGBA8])
@pytest.mark.parametrize("df", [X.SN10, X.R4G4])
def test_dithered_stores(ctx, oracle, df, sf, flags, shape):
    w, h = shape
    raw = _dither_source(sf, w, h, df + sf + w)
    got, want = _convert(ctx, raw, w, h, sf, df, flags), _ref_convert(raw, w, h, sf, df, flags)
    assert np.array_equal(got, want), (sf, df, hex(flags), shape, _diff(got, want))


@pytest.mark.parametrize("flags", [DITHER, DIFFUSION], ids=["ordered", "diffusion"])
@pytest.mark.parametrize("df", [X.F7E3, X.F6E4])
def test_small_floats_do_not_dither(ctx, oracle, df, flags):
    for sf in (RGBA32F, RGBA8):
        for w, h in ((37, 23), (4, 1)):
            raw = _dither_source(sf, w, h, df + sf + w)
            got = _convert(ctx, raw, w, h, sf, df, flags)
            assert np.array_equal(got, _ref_convert(raw, w, h, sf, df, flags)), (sf, df, hex(flags), w, h)
            assert np.array_equal(got, _convert(ctx, raw, w, h, sf, df, 0)), (sf, df, hex(flags), w, h)


# ---- 5. filters ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", X.XBOX)
def test_mip_chains(ctx, oracle, fmt):
    raw = X.random_packed(fmt, 32, 16, fmt)
    got, want = ctx.generate_mips(raw, 32, 16, fmt, 6, BOX), ox.ref_generate_mips(raw, 32, 16, fmt, BOX, 6)
    assert all(np.array_equal(g, r) for g, r in zip(got, want)), (fmt, "box")
    raw = X.random_packed(fmt, 37, 23, fmt + 1)
    for flt in (LINEAR, CUBIC, TRIANGLE):
        got, want = ctx.generate_mips(raw, 37, 23, fmt, 3, flt), ox.ref_generate_mips(raw, 37, 23, fmt, flt, 3)
        assert all(np.array_equal(g, r) for g, r in zip(got, want)), (fmt, hex(flt), [_diff(g, r) for g, r in zip(got, want)])


@pytest.mark.parametrize("fmt", X.XBOX)
def test_mip_chain_3d(ctx, oracle, fmt):
    raw = X.random_packed(fmt, 8, 8 * 4, fmt + 2)
    got, want = ctx.generate_mips3d(raw, 8, 8, 4, fmt, 4, BOX), ox.ref_generate_mips3d(raw, 8, 8, 4, fmt, BOX, 4)
    assert len(got) == len(want) == 4 and all(np.array_equal(g, r) for g, r in zip(got, want)), fmt


@pytest.mark.parametrize("fmt", X.XBOX)
def test_resize(ctx, oracle, fmt):
    raw = X.random_packed(fmt, 37, 23, fmt + 3)
    for flt in (LINEAR, CUBIC, LINEAR | dx.TEX_FILTER_WRAP, CUBIC | dx.TEX_FILTER_WRAP):
        got, want = ctx.resize(raw, 37, 23, fmt, 20, 31, flt), ox.ref_resize(raw, 37, 23, fmt, 20, 31, flt)
        assert np.array_equal(got, want), (fmt, hex(flt), _diff(got, want))


@pytest.mark.parametrize("fmt", X.XBOX)
def test_filters_drop_the_srgb_flags(ctx, oracle, fmt):
    """LoadScanlineLinear / StoreScanlineLinear keep TEX_FILTER_SRGB for the formats of DirectXTexConvert.cpp:2825-2849 only; the four are
    not among them, so Resize and GenerateMipMaps with the flags give the bytes they give without"""
    raw = X.random_packed(fmt, 37, 23, fmt + 4)
    for srgb in (SRGB_IN | SRGB_OUT, SRGB_IN, SRGB_OUT):
        got, want = ctx.resize(raw, 37, 23, fmt, 20, 31, CUBIC | srgb), ox.ref_resize(raw, 37, 23, fmt, 20, 31, CUBIC | srgb)
        assert np.array_equal(got, want), (fmt, hex(srgb), _diff(got, want))
        assert np.array_equal(want, ox.ref_resize(raw, 37, 23, fmt, 20, 31, CUBIC)), (fmt, hex(srgb))
        got, want = ctx.generate_mips(raw, 37, 23, fmt, 3, LINEAR | srgb), ox.ref_generate_mips(raw, 37, 23, fmt, LINEAR | srgb, 3)
        assert all(np.array_equal(g, r) for g, r in zip(got, want)), (fmt, hex(srgb))
        assert all(np.array_equal(a, b) for a, b in zip(want, ox.ref_generate_mips(raw, 37, 23, fmt, LINEAR, 3))), (fmt, hex(srgb))


def test_resize_and_mips_ignore_the_dither_bits(ctx, oracle):
    """texconv hands one filter word to Resize, Convert and GenerateMipMaps: only Convert may read the dither bits"""
    raw = _image(RGBA8, 40, 24, 5)
    for bit in (DITHER, DIFFUSION):
        want = ox.ref_resize(raw, 40, 24, RGBA8, 20, 12, BOX | bit)
        assert np.array_equal(want, ox.ref_resize(raw, 40, 24, RGBA8, 20, 12, BOX))
        assert np.array_equal(ctx.resize(raw, 40, 24, RGBA8, 20, 12, BOX | bit), want)
        want = ox.ref_resize(raw, 40, 24, RGBA8, 21, 13, LINEAR | bit)
        assert np.array_equal(ctx.resize(raw, 40, 24, RGBA8, 21, 13, LINEAR | bit), want)
        top = raw[:32 * 16 * 4]       # a power-of-two level 0: the box filter takes no other
        for flt in (BOX, LINEAR, CUBIC, TRIANGLE):
            got, want = ctx.generate_mips(top, 32, 16, RGBA8, 4, flt | bit), ox.ref_generate_mips(top, 32, 16, RGBA8, flt | bit, 4)
            assert all(np.array_equal(g, r) for g, r in zip(got, want)), (hex(flt), hex(bit))
            assert all(np.array_equal(a, b) for a, b in zip(want, ox.ref_generate_mips(top, 32, 16, RGBA8, flt, 4))), (hex(flt), hex(bit))


# ---- 6. Compress from / Decompress into ----------------------------------------------------------------------------------------------------
COMPRESS = [(f, bc) for f in ALPHA for bc in (BC1, BC3, BC7)] + [(X.F7E3, BC6HU), (X.F6E4, BC6HU), (X.SN10, BC5S), (X.R4G4, BC5U), (X.R4G4, BC1)]


@pytest.mark.parametrize("fmt,bc", COMPRESS)
def test_compress_from(ctx, oracle, fmt, bc):
    for w, h in ((36, 20), (37, 23)):
        raw = X.random_packed(fmt, w, h, fmt + bc + w)
        got, want = ctx.compress(raw, w, h, fmt, bc, 0, 0.5), ox.ref_compress_image(raw, w, h, fmt, bc, 0, 0.5)
        assert np.array_equal(got, want), (fmt, bc, w, h, _diff(got, want))


@pytest.mark.parametrize("fmt", X.XBOX)
def test_decompress_into(ctx, oracle, fmt):
    w, h = 37, 23
    bc1 = np.random.default_rng(fmt).integers(0, 256, ox.image_bytes(BC1, w, h), dtype=np.uint8)
    hdr = (np.random.default_rng(fmt + 1).random((h, w, 4), dtype=np.float32) * 40.0).astype(np.float16)
    bc6 = ctx.compress(hdr, w, h, RGBA16F, BC6HU, 0, 0.5)
    for bc, payload in ((BC1, bc1), (BC6HU, bc6)):
        ref_hr = _hresult(lambda: ox.ref_decompress_image(payload, w, h, bc, fmt))
        if ref_hr:
            assert _hresult(lambda: ctx.decompress(payload, w, h, bc, fmt)) == ref_hr, (fmt, bc, hex(ref_hr))
        else:
            got, want = ctx.decompress(payload, w, h, bc, fmt), ox.ref_decompress_image(payload, w, h, bc, fmt)
            assert np.array_equal(got, want), (fmt, bc, _diff(got, want))


# ---- 7. the other per-texel entry points ------------------------------------------------------------------------------------------------------
W, H = 24, 16


@pytest.mark.parametrize("fmt", X.XBOX)
def test_premultiply_alpha(ctx, oracle, fmt):
    raw = X.random_packed(fmt, W, H, fmt + 10)
    for flags in (0, 0x2):
        ref_hr = _hresult(lambda: ox.ref_premultiply_alpha(raw, W, H, fmt, flags))
        if ref_hr:          # no alpha channel: the reference refuses, and so must the library
            assert _hresult(lambda: ctx.premultiply_alpha(raw, W, H, fmt, flags)) == ref_hr, (fmt, hex(ref_hr))
        else:
            got, want = ctx.premultiply_alpha(raw, W, H, fmt, flags), ox.ref_premultiply_alpha(raw, W, H, fmt, flags)
            assert np.array_equal(got, want), (fmt, flags, _diff(got, want))


@pytest.mark.parametrize("fmt", X.XBOX)
def test_scale_mips_alpha_for_coverage(ctx, oracle, fmt):
    raw = X.random_packed(fmt, W, H, fmt + 11)
    levels = ox.ref_generate_mips(raw, W, H, fmt, LINEAR, 3)
    ref_hr = _hresult(lambda: ox.ref_scale_mips_alpha_for_coverage(levels, W, H, fmt, 0.5))
    if ref_hr:
        assert _hresult(lambda: ctx.scale_mips_alpha_for_coverage(levels, W, H, fmt, 0.5)) == ref_hr, (fmt, hex(ref_hr))
        return
    got, want = ctx.scale_mips_alpha_for_coverage(levels, W, H, fmt, 0.5), ox.ref_scale_mips_alpha_for_coverage(levels, W, H, fmt, 0.5)
    assert all(np.array_equal(g, r) for g, r in zip(got, want)), (fmt, [_diff(g, r) for g, r in zip(got, want)])


class _Device:
    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def put(self, raw):
        raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
        p = self.ctx.device_alloc(max(1, raw.nbytes), zero=True)
        self.ptrs.append(p)
        self.ctx.upload(p, raw, sync=True)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.synchronize()
        for p in self.ptrs:
            self.ctx.device_free(p)


@pytest.mark.parametrize("fmt", X.XBOX)
def test_compute_mse(ctx, oracle, fmt):
    """As tests/test_scanline_routes_gpu.py::test_compute_mse_formats holds mse_kernel: rtol 1e-6 against the fp64 mean over the loaded
    values (here the reference's own LoadScanline), 2e-4 against the reference's ComputeMSE, which accumulates serially in fp32."""
    a, b = X.random_packed(fmt, W, H, fmt + 12), _image(RGBA8, W, H, fmt + 13)
    with _Device(ctx) as d:
        got = ctx.compute_mse_device(d.put(a), fmt, d.put(b), RGBA8, W, H)
    va = X.ref_load(a, fmt, W * H).astype(np.float64)
    vb = b.reshape(-1, 4).astype(np.float32) * np.float32(1.0 / 255.0)
    want = ((va - vb.astype(np.float64)) ** 2).mean(axis=0)
    print(fmt, got, want)
    assert np.allclose(got, want, rtol=1e-6, atol=0), (got, want)
    assert np.allclose(got, ox.ref_compute_mse(a, fmt, b, RGBA8, W, H), rtol=2e-4, atol=0)


@pytest.mark.parametrize("fmt", [X.F7E3, X.SN10])
def test_alpha_all_opaque(ctx, oracle, fmt):
    words = (X.field_image(W * H) | np.uint32(0xC0000000)).astype(np.uint32)
    one = words.copy(); one[W * 7 + 5] = (one[W * 7 + 5] & np.uint32(0x3FFFFFFF)) | np.uint32(0x80000000)
    with _Device(ctx) as d:
        for img in (words, one):
            got = ctx.alpha_all_opaque_device([dx.device_image(d.put(img), W, H, fmt)])
            assert got == ox.ref_alpha_all_opaque([img], fmt, W, H), fmt
        assert ctx.alpha_all_opaque_device([dx.device_image(d.put(words), W, H, fmt)]) is True
        assert ctx.alpha_all_opaque_device([dx.device_image(d.put(one), W, H, fmt)]) is False


def _to_float(ctx, raw, fmt, w=W, h=H):
    return _convert(ctx, raw, w, h, fmt, RGBA32F)


def _from_float(ctx, f32, fmt, w=W, h=H):
    return _convert(ctx, f32, w, h, RGBA32F, fmt)


@pytest.mark.parametrize("fmt", X.XBOX)
def test_transform_swizzle_composes(ctx, oracle, fmt):
    raw = X.random_packed(fmt, W, H, fmt + 14)
    t = capi.make_transform(dx.TRANSFORM_SWIZZLE, swizzle=(1, 0, 3, 2), zero=(0, 0, 0, 0), one=(0, 0, 0, 0))
    got = ctx.transform_image(raw, W, H, fmt, t)
    want = _from_float(ctx, ctx.transform_image(_to_float(ctx, raw, fmt), W, H, RGBA32F, t), fmt)
    assert np.array_equal(got, want), (fmt, _diff(got, want))
    assert not np.array_equal(got, raw)


@pytest.mark.parametrize("fmt", X.XBOX)
def test_normal_map_composes(ctx, oracle, fmt):
    """source side for all four; destination side by composition for the three whose class gives the float intermediate's encoding. A
    UNORM target (190) is biased to [0, 1] by ComputeNormalMap itself, which an RGBA32F intermediate is not: it is checked against the
    numpy restatement (tests/nmap_ref.py) of the rows handed to StoreScanline, stored by the reference's Convert RGBA32F -> 190, which
    only saturates values that are in [0, 1] already."""
    raw = X.random_packed(fmt, W, H, fmt + 15)
    flags = dx.CNMAP_CHANNEL_LUMINANCE | dx.CNMAP_COMPUTE_OCCLUSION
    got = ctx.compute_normal_map(raw, W, H, fmt, RGBA32F, flags, 2.0)
    want = ctx.compute_normal_map(_to_float(ctx, raw, fmt), W, H, RGBA32F, RGBA32F, flags, 2.0)
    assert np.array_equal(got, want), (fmt, _diff(got, want))
    rows = nmap_ref.nmap_rows(X.ref_load(raw, fmt, W * H).reshape(H, W, 4), flags, 2.0, False)
    assert np.array_equal(got, rows.view(np.uint8).reshape(-1)), (fmt, "restatement fed with the loaded values")
    height = _image(RGBA8, W, H, fmt + 16)
    got = ctx.compute_normal_map(height, W, H, RGBA8, fmt, flags, 2.0)
    if fmt != X.R4G4:
        want = _from_float(ctx, ctx.compute_normal_map(height, W, H, RGBA8, RGBA32F, flags, 2.0), fmt)
    else:
        for fl in (flags, dx.CNMAP_CHANNEL_RED | dx.CNMAP_INVERT_SIGN | dx.CNMAP_MIRROR):
            rows = nmap_ref.nmap_rows(ox.load_image(height, W, H, RGBA8), fl, 2.0, True)
            assert not np.isnan(rows).any() and rows.min() >= 0 and rows.max() <= 1
            got, want = ctx.compute_normal_map(height, W, H, RGBA8, fmt, fl, 2.0), _ref_convert(rows, W, H, RGBA32F, fmt)
            assert np.array_equal(got, want), (fmt, hex(fl), _diff(got, want))
    assert np.array_equal(got, want), (fmt, _diff(got, want))


@pytest.mark.parametrize("fmt", X.XBOX)
def test_analyze_composes(ctx, oracle, fmt):
    """min / max exactly; the sums run over four texels a lane for both images, but over different lane counts where the quad route
    applies to one side only: rtol 1e-6, the bar tests/test_diag_gpu.py holds the fp64 sums to"""
    raw = X.random_packed(fmt, W, H, fmt + 17)
    got = ctx.analyze([(raw, W, H, fmt, None)])[0]
    want = ctx.analyze([(_to_float(ctx, raw, fmt), W, H, RGBA32F, None)])[0]
    loaded = X.ref_load(raw, fmt, W * H)
    assert np.array_equal(got["min"], loaded.min(axis=0)) and np.array_equal(got["max"], loaded.max(axis=0))
    assert np.array_equal(got["min"], want["min"]) and np.array_equal(got["max"], want["max"]) and np.array_equal(got["specials"], want["specials"])
    assert np.allclose(got["avg"], want["avg"], rtol=1e-6, atol=0) and np.allclose(got["variance"], want["variance"], rtol=1e-6, atol=0)
    assert np.allclose(got["avg"], loaded.astype(np.float64).mean(axis=0), rtol=1e-6, atol=0)


@pytest.mark.parametrize("fmt", X.XBOX)
def test_difference_and_merge_compose(ctx, oracle, fmt):
    raw = X.random_packed(fmt, W, H, fmt + 18)
    other = _image(RGBA32F, W, H, fmt + 19)
    f32 = _to_float(ctx, raw, fmt)
    got = ctx.difference(raw, other.view(np.float32), W, H, fmt, 0xFF00FF, 0.25)
    want = _from_float(ctx, ctx.difference(f32, other.view(np.float32), W, H, RGBA32F, 0xFF00FF, 0.25), fmt)
    assert np.array_equal(got, want), (fmt, "difference", _diff(got, want))
    permute = (4, 1, 6, 3)
    got = ctx.merge_image(raw, other.view(np.float32), W, H, fmt, permute)
    want = _from_float(ctx, ctx.merge_image(f32, other.view(np.float32), W, H, RGBA32F, permute), fmt)
    assert np.array_equal(got, want), (fmt, "merge", _diff(got, want))


@pytest.mark.parametrize("fmt", X.XBOX)
def test_copy_rectangle_composes(ctx, oracle, fmt):
    """a rectangle out of an image of the format into an RGBA32F image and back, at odd offsets: the converting route on both sides;
    and within the format: the mover"""
    raw = X.random_packed(fmt, W, H, fmt + 20)
    rect, at = (3, 2, 13, 9), (5, 4)

    def copy(src, sf, dst, df):
        dst = dst.copy()
        s, d = capi._host_image(src, W, H, sf), capi._host_image(dst, W, H, df)
        ctx.copy_rectangle(s, rect, d, 0, *at)
        return dst

    def paste(src_tight, dst_tight, bytes_per_texel):
        s = src_tight.reshape(H, W * bytes_per_texel); d = dst_tight.copy().reshape(H, W * bytes_per_texel)
        (x, y, w, h), (ox_, oy) = rect, at
        d[oy:oy + h, ox_ * bytes_per_texel:(ox_ + w) * bytes_per_texel] = s[y:y + h, x * bytes_per_texel:(x + w) * bytes_per_texel]
        return d.reshape(-1)

    bpt = X.BITS[fmt] // 8
    f32 = _to_float(ctx, raw, fmt)
    base32 = _image(RGBA32F, W, H, fmt + 21)
    assert np.array_equal(copy(raw, fmt, base32, RGBA32F), paste(f32, base32, 16)), (fmt, "load side")
    base = X.random_packed(fmt, W, H, fmt + 22)
    assert np.array_equal(copy(base32, RGBA32F, base, fmt), paste(_from_float(ctx, base32, fmt), base, bpt)), (fmt, "store side")
    assert np.array_equal(copy(raw, fmt, base, fmt), paste(raw, base, bpt)), (fmt, "mover")
