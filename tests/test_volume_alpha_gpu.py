"""GenerateMipMaps3D, PremultiplyAlpha, ScaleMipMapsAlphaForCoverage and IsAlphaAllOpaque on the GPU against the reference's own drivers,
at the sizes, formats, flags and pitches where their kernels (resize3d_*, pmalpha, alpha_coverage, scale_alpha, alpha_below in scanline.hip)
and the host logic around them (submit_mips3d, submit_coverage_chain, dxtex_alpha_all_opaque_device) branch.

Every call runs between profile_begin() and profile_end(); the marks the launchers record prove which kernel ran. Bar: byte identity with
the oracle; where sRGB curves (powf on both sides) are involved, test_scanline_routes_gpu's _within_srgb_bar, each mip level against the
reference re-run from the GPU's previous level so that steps do not compound.

Routes the C ABI cannot reach, and classes left out and why:
- TEX_FILTER_MIRROR_U / V / W with any filter, and TEX_FILTER_WRAP_U / V / W with the linear filter, in a mip chain: a level is never
  larger than its source, so a linear tap never leaves the source (linear_entry: isrcB < source whenever source >= dest) and a cubic tap
  leaves it by one texel at most, where mirroring and clamping give the same index (bounduvw). The reference's output under these flags
  equals its output without them (test_mips3d_axis_flags asserts exactly that, so the table stays honest); the calls still run for byte
  parity. The per-axis flags are pinned with the cubic and triangle filters under WRAP, where each axis changes the result.
- A W x 1 x D base volume under the box filter: the reference averages scanline buffers it never filled (test_scanline_parity keeps that
  skip); no case here starts from such a base. Box chains that reach W x 1 below a two-high level are run byte-exactly on the non-sRGB
  formats; sRGB box chains use shapes that never get there, since a re-based reference run has no stale buffer to agree with.
- NaN produced by PremultiplyAlpha's arithmetic (0 * Inf, Inf / Inf, NaN alpha): XMVectorMultiply / XMVectorDivide (DirectXTexPMAlpha.cpp
  :54, :141) leave the sign and payload of a generated NaN to the platform (x86 SSE returns the negative "real indefinite", gfx950 the
  positive one). In float formats a word that is NaN on both sides counts as equal; every other word, Inf included, is byte-exact.

The sRGB bar of PremultiplyAlpha on float formats is test_scanline_parity.test_premultiply_alpha's (fewer than 1 % of the words differ) with
a bound on the size of a difference added: two ulp. powf differs from libm's by one ulp on a few inputs; the multiplication or division by
alpha that follows rounds once more and can move the result into the binade below, where the same distance is two ulp. Measured on the
MI355X: at most 2 ulp, on 0.02 % of the words or fewer. 8-bit formats keep _within_srgb_bar.

scale_alpha_kernel's y stride needs a level 1 taller than 65535 rows, which the 3 x 65540 chain does not have: test_coverage_scale_alpha_y_stride
runs 3 x 131080.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_scanline_routes_gpu import (BGRA8, BGRA8S, BGRX8, B5G6R5, BOX, CUBIC, D32F, LINEAR, POINT,  # noqa: E402
                                      R8, R11G11B10F, RGB10A2, RGB32F, RGBA8, RGBA8S, RGBA16F, RGBA16UN, RGBA32F, RGBA32U, SRGB,
                                      SRGB_FORMATS, TRIANGLE, Device, _diff, _edges, _profiled, _smooth, _texels, _within_srgb_bar)

pytestmark = pytest.mark.gpu

RGBA16SN, RGBA8SN, B5G5R5A1, B4G4R4A4, A8 = 13, 31, 86, 115, 65
BC1, BC2, BC3, BC4, BC5, BC6H, BC7 = 71, 74, 77, 80, 83, 95, 98
WRAP_U, WRAP_V, WRAP_W, MIRROR_U, MIRROR_V, MIRROR_W = 0x1, 0x2, 0x4, 0x10, 0x20, 0x40
FILTER_NAME = {POINT: "point", LINEAR: "linear", CUBIC: "cubic", BOX: "box", TRIANGLE: "triangle"}
E_POINTER, E_FAIL, E_INVALIDARG = 0x80004003, 0x80004005, 0x80070057


def _hr(v):
    return v & 0xFFFFFFFF


# ---- a. GenerateMipMaps3D ------------------------------------------------------------------------------------------------------------
VOL_FORMATS = [RGBA16F, RGBA32F, R8, BGRA8, BGRX8, RGBA8S, RGB10A2, R11G11B10F, B5G6R5, RGB32F, D32F]
# two x workgroups; a deep cube; a tall slice; a deep stack; one column; depth-1 box chains that reach W x 1 below a two-high level of
# depth 1, and of depth 2; the stale tap inside the 3-D kernel at widths above 4 and in its second workgroup; sizes that are no power of two
VOL_DIMS = [(512, 4, 2), (64, 64, 64), (4, 512, 2), (2, 2, 256), (1, 8, 8), (32, 4, 1), (64, 2, 1), (64, 4, 4), (64, 2, 8), (2048, 2, 4),
            (320, 6, 5), (12, 10, 6)]
VOL_FILTERS = [0, POINT, LINEAR, CUBIC, BOX, TRIANGLE]


def _levels3(w, h, d):
    return 1 + int(np.floor(np.log2(max(w, h, d))))


def _pow2(dims):
    return all(v & (v - 1) == 0 for v in dims)


def _mode(flt, dims):
    return (flt & 0xF00000) or (BOX if _pow2(dims) else TRIANGLE)


def _reaches_stale_row(dims):
    """A box chain that gets to a W x 1 (W > 1) source level: the reference's never re-pointed fourth tap."""
    w, h, _ = dims
    return w > h


def _volume(oracle, rng, fmt, w, h, d):
    return np.concatenate([_smooth(oracle, rng, fmt, w, h) for _ in range(d)])


def _expected_marks(dims, n, mode):
    """submit_mips3d: the 3-D kernel while the source is more than one slice deep (always, for the triangle filter), else the 2-D launcher."""
    sizes, want3, want2 = [dims], False, False
    for _ in range(n - 1):
        sizes.append(tuple(max(1, v >> 1) for v in sizes[-1]))
    for s in sizes[:-1]:
        if s[2] > 1 or mode == TRIANGLE:
            want3 = True
        else:
            want2 = True
    return want3, want2


def _check_marks(names, dims, n, mode, fails, tag):
    want3, want2 = _expected_marks(dims, n, mode)
    has3 = {k for k in names if k.startswith("resize3d_")}
    has2 = {k for k in names if k.startswith("resize_")}
    ok2 = any(k.startswith("resize_" + FILTER_NAME[mode]) for k in has2) if want2 else not has2
    if has3 != ({"resize3d_" + FILTER_NAME[mode]} if want3 else set()) or not ok2:
        fails.append((tag, "marks", sorted(names), (want3, want2)))


def _check_volume_chain(ctx, oracle, vol, fmt, dims, flt, fails, srgb=False):
    w, h, d = dims
    n = _levels3(w, h, d)
    mode = _mode(flt, dims)
    got, names = _profiled(ctx, lambda: ctx.generate_mips3d(vol, w, h, d, fmt, n, flt))
    ref = oracle.ref_generate_mips3d(vol, w, h, d, fmt, flt, n)
    _check_marks(names, dims, n, mode, fails, hex(flt))
    sizes = oracle.mip_sizes3d(w, h, d, n)
    for lvl in range(n):
        if srgb and lvl:
            pw, ph, pd = sizes[lvl - 1]
            ref[lvl] = oracle.ref_generate_mips3d(got[lvl - 1], pw, ph, pd, fmt, flt, 2)[1]
        if not (np.array_equal(got[lvl], ref[lvl]) or (srgb and _within_srgb_bar(got[lvl], ref[lvl], fmt))):
            fails.append((hex(flt), lvl, "bytes", _diff(got[lvl], ref[lvl])))
    return got, ref


@pytest.mark.parametrize("dims", VOL_DIMS, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmt", VOL_FORMATS)
def test_mips3d_formats_at_size(ctx, oracle, fmt, dims):
    w, h, d = dims
    vol = _volume(oracle, np.random.default_rng(fmt * 11 + w + 3 * h + 7 * d), fmt, w, h, d)
    srgb = fmt in SRGB_FORMATS
    fails = []
    for flt in VOL_FILTERS:
        mode = _mode(flt, dims)
        if (flt & 0xF00000) == BOX and not _pow2(dims):
            continue                                   # E_FAIL on both sides (test_scanline_parity.test_generate_mips3d_errors)
        if srgb and mode == BOX and _reaches_stale_row(dims):
            continue                                   # see the docstring: run byte-exactly on the non-sRGB formats instead
        _check_volume_chain(ctx, oracle, vol, fmt, dims, flt, fails, srgb)
    assert not fails, fails[:6]


@pytest.mark.parametrize("dims", [(32, 32, 32), (4, 64, 8), (12, 10, 6), (320, 6, 5)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
def test_mips3d_srgb_flags(ctx, oracle, fmt, dims):
    """TEX_FILTER_SRGB_IN | SRGB_OUT on linear formats: srgbIn / srgbOut of every 3-D kernel by flag."""
    w, h, d = dims
    vol = _volume(oracle, np.random.default_rng(fmt + w + d), fmt, w, h, d)
    fails = []
    for flt in (POINT, LINEAR, CUBIC, BOX, TRIANGLE):
        if flt == BOX and not _pow2(dims):
            continue
        got, _ = _check_volume_chain(ctx, oracle, vol, fmt, dims, flt | SRGB, fails, srgb=True)
        if flt != POINT:
            plain = ctx.generate_mips3d(vol, w, h, d, fmt, _levels3(w, h, d), flt)
            assert not np.array_equal(got[1], plain[1]), (hex(flt), "the sRGB flags changed nothing")
    assert not fails, fails[:6]


AXIS_CASES = [(CUBIC, (WRAP_U, WRAP_V, WRAP_W), True), (TRIANGLE, (WRAP_U, WRAP_V, WRAP_W), True),
              (LINEAR, (WRAP_U, WRAP_V, WRAP_W), False), (CUBIC, (MIRROR_U, MIRROR_V, MIRROR_W), False)]


@pytest.mark.parametrize("dims", [(12, 10, 6), (320, 6, 5)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmt", [RGBA8, RGBA32F, RGB10A2, R8])
def test_mips3d_axis_flags(ctx, oracle, fmt, dims):
    """Each of the U, V and W flags alone, on a volume whose three dimensions and three axis contents differ. Where a flag can change the
    result (wrap under cubic and triangle) the reference's own outputs must differ from the unflagged run and between the axes, so a kernel
    that took one axis' flag from another's bit cannot pass; where it cannot (see the docstring) they must coincide."""
    w, h, d = dims
    vol = _volume(oracle, np.random.default_rng(fmt * 5 + w), fmt, w, h, d)
    n = _levels3(w, h, d)
    fails = []
    for flt, bits, discriminates in AXIS_CASES:
        base = np.concatenate(oracle.ref_generate_mips3d(vol, w, h, d, fmt, flt, n))
        refs = []
        for bit in bits:
            _, ref = _check_volume_chain(ctx, oracle, vol, fmt, dims, flt | bit, fails)
            refs.append(np.concatenate(ref))
        if discriminates:
            assert all(not np.array_equal(r, base) for r in refs), (hex(flt), "a single-axis flag left the reference's output unchanged")
            assert not any(np.array_equal(refs[i], refs[j]) for i in range(3) for j in range(i)), (hex(flt), "two axes' flags coincide")
        else:
            assert all(np.array_equal(r, base) for r in refs), (hex(flt), bits, "this flag does change a mip chain: move it to the discriminating cases")
    assert not fails, fails[:6]


def _triangle_matrix(oracle, source, dest):
    s, t, wbits = oracle.ref_triangle_filter(source, dest, False)
    m = np.zeros((dest, source), np.float64)
    np.add.at(m, (t, s), wbits.view(np.float32).astype(np.float64))
    return m


@pytest.mark.parametrize("dims", [(12, 10, 6), (64, 4, 4)], ids=lambda s: "x".join(map(str, s)))
def test_mips3d_triangle_r10g10b10a2_alpha_bias(ctx, oracle, dims):
    """The 3-D triangle filter adds 0.1 to the alpha of R10G10B10A2 (DirectXTexMipmaps.cpp:2767-2786). So that the case cannot go vacuous,
    the reference's level 1 alpha must differ somewhere from a plain float64 triangle filter of the alpha channel rounded to two bits."""
    w, h, d = dims
    rng = np.random.default_rng(w)
    vol = _volume(oracle, rng, RGB10A2, w, h, d)
    fails = []
    _, ref = _check_volume_chain(ctx, oracle, vol, RGB10A2, dims, TRIANGLE, fails)
    assert not fails, fails
    alpha = (vol.view(np.uint32).reshape(d, h, w) >> 30).astype(np.float64) / 3.0
    w1, h1, d1 = max(1, w >> 1), max(1, h >> 1), max(1, d >> 1)
    plain = np.einsum("zZ,yY,xX,ZYX->zyx", _triangle_matrix(oracle, d, d1), _triangle_matrix(oracle, h, h1), _triangle_matrix(oracle, w, w1), alpha)
    plain_code = np.floor(np.clip(plain, 0, 1) * 3.0 + 0.5).astype(np.uint32)
    ref_code = ref[1].view(np.uint32).reshape(d1, h1, w1) >> 30
    assert (plain_code != ref_code).any(), "the + 0.1 of the reference is invisible on this volume"


@pytest.mark.parametrize("row_pad,extra_rows", [(4, 0), (16, 0), (0, 1), (16, 1)])
@pytest.mark.parametrize("fmt,dims,flt", [(RGBA8, (64, 4, 4), BOX), (RGBA8, (12, 10, 6), TRIANGLE), (RGBA16F, (12, 10, 6), CUBIC), (RGBA8, (64, 2, 8), BOX)])
def test_mips3d_device_pitch(ctx, oracle, fmt, dims, flt, row_pad, extra_rows):
    """dxtex_generate_mips3d_device with padded rowPitch / slicePitch on every level: the tight result, and padding that stays zero."""
    w, h, d = dims
    n = _levels3(w, h, d)
    vol = _volume(oracle, np.random.default_rng(w + row_pad), fmt, w, h, d)
    ref = oracle.ref_generate_mips3d(vol, w, h, d, fmt, flt, n)
    sizes = oracle.mip_sizes3d(w, h, d, n)
    texel = oracle.BPP[fmt] // 8
    with Device(ctx) as dev:
        vols, ptrs = [], []
        for i, (lw, lh, ld) in enumerate(sizes):
            rp = lw * texel + row_pad
            sp = rp * (lh + extra_rows)
            host = np.zeros((ld, lh + extra_rows, rp), np.uint8)
            if i == 0:
                host[:, :lh, :lw * texel] = vol.reshape(ld, lh, lw * texel)
            p = dev.put(host)
            ptrs.append((p, host.shape))
            vols.append(dx.capi.Volume(lw, lh, ld, fmt, rp, sp, p))
        arr = (dx.capi.Volume * n)(*vols)
        hr, names = _profiled(ctx, lambda: ctx._lib.dxtex_generate_mips3d_device(ctx._h, arr, n, flt))
        assert hr == 0, hex(_hr(hr))
        for i, (lw, lh, ld) in enumerate(sizes[1:], 1):
            p, shape = ptrs[i]
            got = dev.get(p, int(np.prod(shape))).reshape(shape)
            assert np.array_equal(got[:, :lh, :lw * texel].reshape(-1), ref[i]), (i, _diff(got[:, :lh, :lw * texel], ref[i]))
            assert not got[:, :lh, lw * texel:].any() and not got[:, lh:, :].any(), (i, "padding was written")
    assert "resize3d_" + FILTER_NAME[flt] in names, sorted(names)


# ---- b. PremultiplyAlpha -------------------------------------------------------------------------------------------------------------
PM_FORMATS = [RGBA8, RGBA8S, BGRA8, BGRA8S, RGBA16UN, RGBA16SN, RGBA16F, RGBA32F, RGB10A2, B5G5R5A1, B4G4R4A4, A8]
PM_FLAGS = [0, 1, 2, 3, 0x1000000, 0x2000002]
PM_SHAPES = [(600, 5), (1, 1), (3, 65541)]           # three x workgroups; one texel; more rows than grid_rows()' 65535
SPECIAL_ALPHAS = [0.0, -0.0, -0.5, 1e9, 1.401298464324817e-45, np.nan, np.inf, -np.inf]


def _pm_texels(oracle, rng, fmt, w, h):
    """_texels' data; float formats also carry, from texel 8 on, the alphas the reverse path branches on: 0, -0.0, negative, huge, the
    smallest subnormal, and NaN / +-Inf."""
    img = _texels(oracle, rng, fmt, w, h)
    if fmt in (RGBA16F, RGBA32F) and w * h >= 8 + 2 * len(SPECIAL_ALPHAS):
        dtype = np.float16 if fmt == RGBA16F else np.float32
        v = img.view(dtype).reshape(-1, 4).copy()
        with np.errstate(over="ignore"):
            for i, a in enumerate(SPECIAL_ALPHAS):
                v[8 + 2 * i, 3] = dtype(a)
                v[9 + 2 * i] = [0.0, 0.25, -2.0, dtype(a)]
        img = v.view(np.uint8).reshape(-1)
    return img


def _pm_equal(got, ref, fmt, srgb_path):
    if np.array_equal(got, ref):
        return True
    if fmt in (RGBA16F, RGBA32F):
        dtype = np.float16 if fmt == RGBA16F else np.float32
        g, r = got.view(dtype), ref.view(dtype)
        nan = np.isnan(g) & np.isnan(r)                # a generated NaN's sign and payload are the platform's (see the docstring)
        word = np.uint16 if fmt == RGBA16F else np.uint32
        if np.array_equal(got.view(word)[~nan], ref.view(word)[~nan]):
            return True
        if srgb_path:
            keep = ~(np.isnan(g) | np.isnan(r))
            delta = np.abs(got.view(word)[keep].astype(np.int64) - ref.view(word)[keep].astype(np.int64))
            return bool((np.isnan(g) == np.isnan(r)).all()) and int(delta.max(initial=0)) <= 2 and float((delta != 0).mean()) < 0.01
        return False
    return bool(srgb_path) and _within_srgb_bar(got, ref, fmt)


def _pm_figures(got, ref, fmt):
    """For a failure message: where the bytes differ and, for float formats, by how many ulp and on what share of the words."""
    if fmt not in (RGBA16F, RGBA32F):
        return _diff(got, ref)
    word, dtype = (np.uint16, np.float16) if fmt == RGBA16F else (np.uint32, np.float32)
    keep = ~(np.isnan(got.view(dtype)) | np.isnan(ref.view(dtype)))
    delta = np.abs(got.view(word)[keep].astype(np.int64) - ref.view(word)[keep].astype(np.int64))
    return _diff(got, ref), f"largest difference {int(delta.max(initial=0))} ulp, {float((delta != 0).mean()):.5f} of the words differ"


@pytest.mark.parametrize("fmt", PM_FORMATS)
def test_premultiply_alpha_formats(ctx, oracle, fmt):
    fails = []
    fi = PM_FORMATS.index(fmt)
    for i, flags in enumerate(PM_FLAGS):
        for w, h in (PM_SHAPES[(i + fi) % 3], PM_SHAPES[(i + fi + 1) % 3]):
            img = _pm_texels(oracle, np.random.default_rng(fmt * 101 + flags % 13 + w), fmt, w, h)
            try:
                ref = oracle.ref_premultiply_alpha(img, w, h, fmt, flags)
            except oracle.RefError as e:
                try:
                    ctx.premultiply_alpha(img, w, h, fmt, flags)
                    fails.append((hex(flags), (w, h), f"the reference refuses ({e}) but the GPU path accepted"))
                except dx.DxtexError as g:
                    if _hr(g.hresult) != e.hresult:
                        fails.append((hex(flags), (w, h), "HRESULT", hex(_hr(g.hresult)), hex(e.hresult)))
                continue
            got, names = _profiled(ctx, lambda: ctx.premultiply_alpha(img, w, h, fmt, flags))
            if "pmalpha" not in names:
                fails.append((hex(flags), (w, h), "mark", sorted(names)))
            srgb_path = not (flags & 1) and (fmt in SRGB_FORMATS or flags & 0x3000000)
            if not _pm_equal(got, ref, fmt, srgb_path):
                fails.append((hex(flags), (w, h), "bytes", _pm_figures(got, ref, fmt)))
    assert not fails, fails[:6]


@pytest.mark.parametrize("flags", [0, 3, 0x2000002])
@pytest.mark.parametrize("fmt,src_pad,dst_pad", [(RGBA8, 4, 12), (RGBA16F, 8, 24), (RGBA32F, 16, 48), (B5G5R5A1, 2, 6), (A8, 3, 1)])
def test_premultiply_alpha_device_pitch(ctx, oracle, fmt, src_pad, dst_pad, flags):
    w, h = 600, 5
    img = _pm_texels(oracle, np.random.default_rng(fmt + flags % 11), fmt, w, h)
    ref = oracle.ref_premultiply_alpha(img, w, h, fmt, flags)
    row = oracle.image_bytes(fmt, w, 1)
    sp, dp = row + src_pad, row + dst_pad
    with Device(ctx) as d:
        ps = d.put_rows(img, h, row, sp)
        pd = d.empty(dp * h)
        src, dst = dx.Image(w, h, fmt, sp, sp * h, ps), dx.Image(w, h, fmt, dp, dp * h, pd)
        hr, names = _profiled(ctx, lambda: ctx._lib.dxtex_premultiply_alpha_device(ctx._h, ctypes.byref(src), ctypes.byref(dst), flags))
        assert hr == 0, hex(_hr(hr))
        got = d.get(pd, dp * h).reshape(h, dp)
    assert "pmalpha" in names, sorted(names)
    tight = np.ascontiguousarray(got[:, :row]).reshape(-1)
    assert _pm_equal(tight, ref, fmt, not (flags & 1) and bool(flags & 0x3000000)), _pm_figures(tight, ref, fmt)
    assert not got[:, row:].any()


# ---- c. ScaleMipMapsAlphaForCoverage -------------------------------------------------------------------------------------------------
COV_FORMATS = [RGBA8, BGRA8S, RGBA16UN, RGBA16F, RGBA32F, RGB10A2, B5G5R5A1, A8, R8]
COV_CHAINS = [((1024, 64), BOX, None), ((600, 300), CUBIC, None), ((64, 2), BOX, None), ((2, 64), BOX, None), ((3, 65540), POINT, 2)]
ALPHA_REFS = [0.0, 0.25, 0.5, 0.9, 1.0, 1.5, -0.1]


def _levels2(w, h):
    return 1 + int(np.floor(np.log2(max(w, h))))


def _alpha_image(oracle, rng, fmt, w, h, kind, ref_alpha=0.5):
    """An image of `fmt` whose alpha has structure: 'ramp' (smooth, two periods across, one down), 'noise' (uniform noise pushed towards
    the reference value, so that many quads straddle it), 'opaque', 'clear'. Colour is random."""
    v = rng.random((h, w, 4), dtype=np.float32)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    if kind == "ramp":
        v[..., 3] = 0.5 + 0.5 * np.sin(x * np.float32(4 * np.pi / max(w, 2)) + y * np.float32(2 * np.pi / max(h, 2)))
    elif kind == "noise":
        v[..., 3] = np.clip(np.float32(min(max(ref_alpha, 0.1), 0.9)) + (v[..., 3] - 0.5) * np.float32(0.6), 0, 1)
    else:
        v[..., 3] = 1.0 if kind == "opaque" else 0.0
    return v.reshape(-1).view(np.uint8) if fmt == RGBA32F else oracle.ref_convert(v, w, h, RGBA32F, fmt, 0, 0.5)


def _run_coverage(ctx, oracle, mips, w, h, fmt, ref_alpha, fails, tag):
    ref = oracle.ref_scale_mips_alpha_for_coverage(mips, w, h, fmt, ref_alpha)
    got, names = _profiled(ctx, lambda: ctx.scale_mips_alpha_for_coverage(mips, w, h, fmt, ref_alpha))
    want = ({"alpha_coverage"} if min(w, h) >= 2 else set()) | ({"scale_alpha"} if len(mips) > 1 else set())
    if not want <= names:
        fails.append((tag, "marks", sorted(names)))
    for lvl, (g, r) in enumerate(zip(got, ref)):
        if not np.array_equal(g, r):
            fails.append((tag, lvl, "bytes", _diff(g, r)))
    return ref


@pytest.mark.parametrize("chain", range(len(COV_CHAINS)), ids=[f"{c[0][0]}x{c[0][1]}" for c in COV_CHAINS])
@pytest.mark.parametrize("fmt", COV_FORMATS)
def test_coverage_chains(ctx, oracle, fmt, chain):
    (w, h), flt, levels = COV_CHAINS[chain]
    fi = COV_FORMATS.index(fmt)
    tall = h > 65535
    if tall and fi % 3:
        levels, h = None, 64                 # the 65540-row chain rotates over every third format; the others run 3 x 64 in full
    n = levels or _levels2(w, h)
    refs = [ALPHA_REFS[(chain * 3 + fi + k) % len(ALPHA_REFS)] for k in range(1 if tall else 3)]
    fails = []
    for k, ref_alpha in enumerate(refs):
        rng = np.random.default_rng(fmt * 7 + chain * 131 + k)
        base = _alpha_image(oracle, rng, fmt, w, h, "noise" if (fi + k) % 2 else "ramp", ref_alpha)
        mips = oracle.ref_generate_mips(base, w, h, fmt, flt, n)
        _run_coverage(ctx, oracle, mips, w, h, fmt, ref_alpha, fails, (ref_alpha, (w, h)))
    assert not fails, fails[:6]


@pytest.mark.parametrize("ref_alpha", ALPHA_REFS)
def test_coverage_every_alpha_reference(ctx, oracle, ref_alpha):
    """Every alphaReference, at and beyond 0 and 1 included, on the chain whose top levels span several workgroup columns."""
    w, h = 1024, 64
    fails = []
    for fmt in (RGBA8, RGBA32F):
        base = _alpha_image(oracle, np.random.default_rng(fmt), fmt, w, h, "noise", ref_alpha)
        mips = oracle.ref_generate_mips(base, w, h, fmt, BOX, _levels2(w, h))
        _run_coverage(ctx, oracle, mips, w, h, fmt, ref_alpha, fails, fmt)
    assert not fails, fails[:6]


def _alpha32(level):
    return level.view(np.float32).reshape(-1, 4)[:, 3]


def test_coverage_bisection_ends(ctx, oracle):
    """The three ways the bisection of a level ends, each shown on the reference's own output before the GPU is compared with it:
    a level rescaled by a factor other than 1; a level whose first probe already meets the target (output = input); a W x 1 level, whose
    coverage is 0 whatever the scale, so that `lo` walks up for all ten steps and the scale ends at 4 - 3 * 2^-10."""
    fails = []
    w, h = 1024, 64
    base = _alpha_image(oracle, np.random.default_rng(1), RGBA32F, w, h, "noise", 0.5)
    mips = oracle.ref_generate_mips(base, w, h, RGBA32F, BOX, _levels2(w, h))
    ref = _run_coverage(ctx, oracle, mips, w, h, RGBA32F, 0.5, fails, "rescaled")
    ratios = [float(_alpha32(r)[0] / _alpha32(m)[0]) for r, m in zip(ref[1:], mips[1:])]
    assert any(r != 1.0 and not np.array_equal(o, m) for r, o, m in zip(ratios, ref[1:], mips[1:])), ratios

    w, h = 64, 2
    base = _alpha_image(oracle, np.random.default_rng(2), RGBA32F, w, h, "ramp")
    mips = oracle.ref_generate_mips(base, w, h, RGBA32F, BOX, _levels2(w, h))
    ref = _run_coverage(ctx, oracle, mips, w, h, RGBA32F, 0.5, fails, "ten steps")
    limit = np.float32(4.0 - 3.0 * 2.0 ** -10)          # lo = 0, hi = 4, first probe at 1: ten times scale = (scale + 4) / 2
    assert all(np.array_equal(_alpha32(r), _alpha32(m) * limit) for r, m in zip(ref[1:], mips[1:])), "a W x 1 level did not end at the ten-step limit"
    assert (_alpha32(mips[1]) != 0).any()

    ref = _run_coverage(ctx, oracle, mips, w, h, RGBA32F, 1.0, fails, "first probe")       # nothing exceeds 1: the target is 0 and every probe equals it
    assert all(np.array_equal(r, m) for r, m in zip(ref, mips))
    assert not fails, fails


@pytest.mark.parametrize("kind", ["opaque", "clear", "single"])
@pytest.mark.parametrize("fmt", [RGBA8, RGBA32F, B5G5R5A1])
def test_coverage_uniform_and_single_level(ctx, oracle, fmt, kind):
    w, h = 64, 32
    base = _alpha_image(oracle, np.random.default_rng(fmt), fmt, w, h, "ramp" if kind == "single" else kind)
    mips = [base] if kind == "single" else oracle.ref_generate_mips(base, w, h, fmt, BOX, 6)
    fails = []
    for ref_alpha in (0.0, 0.5, 1.0):
        ref = _run_coverage(ctx, oracle, mips, w, h, fmt, ref_alpha, fails, ref_alpha)
        if kind == "opaque" and ref_alpha == 0.5:
            # every sub-sample of every quad is covered, at level 0 and below: the kernel's count makes the first probe of each level equal
            # the target, the bisection breaks there with scale 1, and levels of at least 2 x 2 (64 x 32 ... 4 x 2) come out as they went in
            assert all(np.array_equal(r, m) for r, m in zip(ref[:5], mips[:5])), "an opaque level did not end at its first probe"
    assert not fails, fails[:6]


@pytest.mark.parametrize("fmt", [RGBA8, RGBA32F])
def test_coverage_scale_alpha_y_stride(ctx, oracle, fmt):
    """3 x 131080, two levels: level 1 is 1 x 65540, so scale_alpha_kernel itself runs more rows than grid_rows()' 65535 (in the 3 x 65540
    chain only alpha_coverage does: level 0 is copied, level 1 is 32770 rows). A one-wide level has no quad, its coverage is 0, and the scale
    ends at the ten-step limit, so a row the stride missed would keep its unscaled alpha."""
    w, h = 3, 131080
    base = _alpha_image(oracle, np.random.default_rng(fmt + 9), fmt, w, h, "ramp")
    mips = oracle.ref_generate_mips(base, w, h, fmt, POINT, 2)
    fails = []
    ref = _run_coverage(ctx, oracle, mips, w, h, fmt, 0.5, fails, "tall")
    tail = oracle.image_bytes(fmt, 1, 65535)
    assert not np.array_equal(ref[1][tail:], mips[1][tail:]), "the rows past 65535 were not rescaled by the reference either"
    assert not fails, fails


@pytest.mark.parametrize("fmt,src_pad,dst_pad", [(RGBA8, 4, 12), (RGBA16F, 8, 16), (A8, 1, 3)])
def test_coverage_device_pitch(ctx, oracle, fmt, src_pad, dst_pad):
    w, h = 600, 40
    n = _levels2(w, h)
    base = _alpha_image(oracle, np.random.default_rng(fmt + 3), fmt, w, h, "noise", 0.5)
    mips = oracle.ref_generate_mips(base, w, h, fmt, CUBIC, n)
    ref = oracle.ref_scale_mips_alpha_for_coverage(mips, w, h, fmt, 0.5)
    assert any(not np.array_equal(r, m) for r, m in zip(ref, mips))
    with Device(ctx) as d:
        srcs, dsts, out = [], [], []
        for (lw, lh), m in zip(oracle.mip_sizes(w, h, n), mips):
            row = oracle.image_bytes(fmt, lw, 1)
            sp, dp = row + src_pad, row + dst_pad
            srcs.append(dx.Image(lw, lh, fmt, sp, sp * lh, d.put_rows(m, lh, row, sp)))
            pd = d.empty(dp * lh)
            dsts.append(dx.Image(lw, lh, fmt, dp, dp * lh, pd))
            out.append((pd, lh, row, dp))
        a, b = (dx.Image * n)(*srcs), (dx.Image * n)(*dsts)
        hr, names = _profiled(ctx, lambda: ctx._lib.dxtex_scale_mips_alpha_for_coverage_device(ctx._h, a, b, n, 0.5))
        assert hr == 0, hex(_hr(hr))
        for lvl, (pd, lh, row, dp) in enumerate(out):
            got = d.get(pd, dp * lh).reshape(lh, dp)
            assert np.array_equal(np.ascontiguousarray(got[:, :row]).reshape(-1), ref[lvl]), (lvl, _diff(got[:, :row], ref[lvl]))
            assert not got[:, row:].any(), (lvl, "padding was written")
    assert {"alpha_coverage", "scale_alpha"} <= names, sorted(names)


# ---- d. IsAlphaAllOpaque -------------------------------------------------------------------------------------------------------------
def _half_around(threshold):
    h = np.arange(0x3800, 0x3C01, dtype=np.uint16)
    f = h.view(np.float16).astype(np.float32)
    return int(h[f < np.float32(threshold)].max()), int(h[f >= np.float32(threshold)].min())


def _f32_bits(v):
    return int(np.float32(v).view(np.uint32))


# format -> (numpy word type of the alpha field's container, words per texel, word index, shift, bits, opaque code, the largest code below
# 0.997 and the smallest at or above it). From the formats' arithmetic: UNORM code / (2^bits - 1), SNORM code / (2^(bits-1) - 1), UINT as is.
ALPHA_FIELD = {
    RGBA8: (np.uint8, 4, 3, 0, 8, 255, 254, 255), RGBA8S: (np.uint8, 4, 3, 0, 8, 255, 254, 255), BGRA8: (np.uint8, 4, 3, 0, 8, 255, 254, 255),
    BGRA8S: (np.uint8, 4, 3, 0, 8, 255, 254, 255), A8: (np.uint8, 1, 0, 0, 8, 255, 254, 255), RGBA8SN: (np.uint8, 4, 3, 0, 8, 127, 126, 127),
    RGBA16UN: (np.uint16, 4, 3, 0, 16, 65535, 65338, 65339),             # 0.997 * 65535 = 65338.4
    RGBA16SN: (np.uint16, 4, 3, 0, 16, 32767, 32668, 32669),             # 0.997 * 32767 = 32668.7
    RGBA16F: (np.uint16, 4, 3, 0, 16, 0x3C00) + _half_around(0.997),
    RGBA32F: (np.uint32, 4, 3, 0, 32, _f32_bits(1.0), _f32_bits(np.nextafter(np.float32(0.997), np.float32(0))), _f32_bits(0.997)),
    RGBA32U: (np.uint32, 4, 3, 0, 32, 7, 0, 1),
    RGB10A2: (np.uint32, 1, 0, 30, 2, 3, 2, 3), B5G5R5A1: (np.uint16, 1, 0, 15, 1, 1, 0, 1), B4G4R4A4: (np.uint16, 1, 0, 12, 4, 15, 14, 15),
}
FLOAT_EXTRA = {RGBA16F: {"nan": 0x7E00, "-0.0": 0x8000}, RGBA32F: {"nan": 0x7FC00000, "-0.0": 0x80000000}}
OPAQUE_SHAPES = [((16400, 3), [(0, 0), (255, 0), (256, 1), (16383, 2), (16384, 0), (16399, 2)]),      # past 64 x 256 columns: the x stride
                 ((5, 4100), [(0, 0), (3, 2047), (1, 2048), (4, 4099)])]                               # past 2048 rows: the y stride


def _set_alpha(words, field, x, y, w, code):
    _, per, idx, shift, bits, *_ = field
    i = (y * w + x) * per + idx
    mask = ((1 << bits) - 1) << shift
    words[i] = (int(words[i]) & ~mask) | (code << shift)
    return i


def _opaque_image(oracle, rng, fmt, w, h):
    field = ALPHA_FIELD[fmt]
    dtype, per, idx, shift, bits, opaque = field[:6]
    words = rng.integers(0, 256, oracle.image_bytes(fmt, w, h), dtype=np.uint8).view(dtype).copy()
    if fmt in (RGBA16F, RGBA32F):
        words[:] = _edges(rng, h, w, np.float16 if fmt == RGBA16F else np.float32).reshape(-1).view(dtype)
    mask = dtype(((1 << bits) - 1) << shift)
    words[idx::per] = (words[idx::per] & ~mask) | dtype(opaque << shift)
    return words


@pytest.mark.parametrize("fmt", sorted(ALPHA_FIELD))
def test_alpha_all_opaque_thresholds_and_strides(ctx, oracle, fmt):
    """One texel just below and just at the 0.997 threshold, at the grid's corners and on either side of alpha_below_kernel's x and y
    strides. The image stays on the device; only the one texel is rewritten between calls."""
    field = ALPHA_FIELD[fmt]
    dtype, opaque, below, above = field[0], field[5], field[6], field[7]
    codes = {"below": below, "above": above, **FLOAT_EXTRA.get(fmt, {})}
    fails = []
    for (w, h), spots in OPAQUE_SHAPES:
        words = _opaque_image(oracle, np.random.default_rng(fmt + w), fmt, w, h)
        with Device(ctx) as d:
            p = d.put(words)
            image = [dx.device_image(p, w, h, fmt)]
            got, names = _profiled(ctx, lambda: ctx.alpha_all_opaque_device(image))
            want = oracle.ref_alpha_all_opaque([words], fmt, w, h)
            assert want is True and "alpha_below" in names, (want, sorted(names))
            if got != want:
                fails.append(((w, h), "opaque image", got))
            for x, y in spots:
                for name, code in codes.items():
                    i = _set_alpha(words, field, x, y, w, code)
                    ctx.upload(p + i * words.itemsize, words[i:i + 1], sync=True)
                    got, want = ctx.alpha_all_opaque_device(image), oracle.ref_alpha_all_opaque([words], fmt, w, h)
                    if name in ("below", "above", "nan", "-0.0"):
                        assert want == (name in ("above", "nan")), (fmt, name, want)      # what the formats' arithmetic says, before the GPU is asked
                    if got != want:
                        fails.append(((w, h), (x, y), name, got, want))
                    i = _set_alpha(words, field, x, y, w, opaque)
                    ctx.upload(p + i * words.itemsize, words[i:i + 1], sync=True)
    assert not fails, fails[:8]


def _rgba8_with_alpha(rng, w, h, alpha=255):
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = alpha
    return img


def _bc_opaque(ctx, payload, fmt, w, h):
    with Device(ctx) as d:
        p = d.put(payload)
        return _profiled(ctx, lambda: ctx.alpha_all_opaque_device([dx.device_image(p, w, h, fmt)]))


@pytest.mark.parametrize("size", [(64, 64), (61, 19), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", [BC1, BC2, BC3, BC7])
def test_alpha_all_opaque_bc(ctx, oracle, fmt, size):
    """Blocks encoded by the oracle: opaque; one texel at 253 / 255 (between the 0.99 of the block path and 0.997), at 252 / 255 and at 0,
    in the first and in the last texel; and a transparent texel that lies only in the padding of the last block."""
    w, h = size
    flags = 0x100000 if fmt == BC7 else 0                   # BC7_QUICK
    rng = np.random.default_rng(fmt + w)
    fails, seen = [], set()
    cases = [("opaque", None, 255)] + [(f"{a}@{pos}", pos, a) for a in (253, 252, 0) for pos in ((0, 0), (w - 1, h - 1))]
    for tag, pos, alpha in cases:
        img = _rgba8_with_alpha(rng, w, h)
        if pos:
            img[pos[1], pos[0], 3] = alpha
        payload = oracle.ref_compress_image(img, w, h, RGBA8, fmt, flags, 0.5)
        want = oracle.ref_alpha_all_opaque([payload], fmt, w, h)
        got, names = _bc_opaque(ctx, payload, fmt, w, h)
        seen.add(want)
        if got != want or "alpha_below" not in names:
            fails.append((tag, got, want, sorted(names)))
    assert seen == {True, False}
    # the padding: encode the image padded to whole blocks with its one transparent texel in the last column and row, declare the real size
    pw, ph = (w + 3) & ~3, (h + 3) & ~3
    if (pw, ph) != (w, h):
        img = _rgba8_with_alpha(rng, pw, ph)
        img[ph - 4:, pw - 4:, :3] = img[ph - 1, pw - 1, :3]       # one colour in the last block, so that every encoder keeps its other alphas at 1
        img[ph - 1, pw - 1, 3] = 0
        payload = oracle.ref_compress_image(img, pw, ph, RGBA8, fmt, flags, 0.5)
        assert payload.nbytes == oracle.image_bytes(fmt, w, h)
        assert not oracle.ref_alpha_all_opaque([payload], fmt, pw, ph) and oracle.ref_alpha_all_opaque([payload], fmt, w, h)
        for (dw, dh), want in (((pw, ph), False), ((w, h), True)):
            got, _ = _bc_opaque(ctx, payload, fmt, dw, dh)
            if got != want:
                fails.append(("padding", (dw, dh), got, want))
    assert not fails, fails


def test_alpha_all_opaque_bc3_between_thresholds(ctx, oracle):
    """Hand-built BC3 blocks whose decoded alpha is 253 / 255 (opaque for blocks, though below 0.997) and 252 / 255 (below 0.99)."""
    for alpha1, want in ((253, True), (252, False)):
        bits = sum(1 << (3 * i) for i in range(16))
        block = np.frombuffer(bytes([255, alpha1]) + bits.to_bytes(6, "little") + b"\xff\xff\xff\xff\x00\x00\x00\x00", np.uint8)
        payload = np.tile(block, 16 * 5)
        assert oracle.ref_alpha_all_opaque([payload], BC3, 61, 19) == want
        got, names = _bc_opaque(ctx, payload, BC3, 61, 19)
        assert got == want and "alpha_below" in names


@pytest.mark.parametrize("fmt", [BC4, BC5, BC6H, R8, BGRX8])
def test_alpha_all_opaque_without_alpha(ctx, oracle, fmt):
    """Formats that carry no alpha are opaque without a launch."""
    w, h = 16, 8
    payload = np.random.default_rng(fmt).integers(0, 256, oracle.image_bytes(fmt, w, h), dtype=np.uint8)
    assert oracle.ref_alpha_all_opaque([payload], fmt, w, h)
    got, names = _bc_opaque(ctx, payload, fmt, w, h)
    assert got is True and "alpha_below" not in names, (got, sorted(names))


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F, BC3])
def test_alpha_all_opaque_three_images(ctx, oracle, fmt):
    w, h = 61, 19
    rng = np.random.default_rng(fmt)
    imgs = [_rgba8_with_alpha(rng, w, h) for _ in range(3)]

    def payloads():
        if fmt == RGBA8:
            return [i.reshape(-1) for i in imgs]
        if fmt == RGBA16F:
            return [oracle.ref_convert(i, w, h, RGBA8, RGBA16F) for i in imgs]
        return [oracle.ref_compress_image(i, w, h, RGBA8, fmt, 0, 0.5) for i in imgs]

    for alpha, want in ((255, True), (0, False)):
        imgs[2][h - 1, w - 1, 3] = alpha
        data = payloads()
        assert oracle.ref_alpha_all_opaque(data, fmt, w, h) == want
        with Device(ctx) as d:
            images = [dx.device_image(d.put(p), w, h, fmt) for p in data]
            got, names = _profiled(ctx, lambda: ctx.alpha_all_opaque_device(images))
        assert got == want and "alpha_below" in names, (got, want, sorted(names))


def test_alpha_all_opaque_refusals(ctx):
    with Device(ctx) as d:
        p = d.empty(64 * 4)
        good = dx.device_image(p, 8, 8, RGBA8)
        for images, want in (([dx.Image(8, 8, RGBA8, 32, 256, None)], E_POINTER),
                             ([good, dx.device_image(p, 8, 8, BGRA8)], E_FAIL),
                             ([dx.Image(0, 8, RGBA8, 32, 256, p)], E_INVALIDARG), ([dx.Image(8, 0, RGBA8, 32, 256, p)], E_INVALIDARG)):
            with pytest.raises(dx.DxtexError) as e:
                ctx.alpha_all_opaque_device(images)
            assert _hr(e.value.hresult) == want, (hex(_hr(e.value.hresult)), hex(want))
        out = ctypes.c_int(5)
        assert _hr(ctx._lib.dxtex_alpha_all_opaque_device(ctx._h, None, 0, ctypes.byref(out))) == E_INVALIDARG and out.value == 0
