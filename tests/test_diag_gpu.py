"""texdiag's diagnostics on the GPU - dxtex_analyze*, dxtex_compute_mse_flags_device, dxtex_analyze_bc*, dxtex_difference* - against the
numpy restatement of the reference (tests/diag_ref.py) over the oracle's LoadScanline floats and its Convert store.

Every call runs between profile_begin() and profile_end(), whose kernel names prove that the launcher under test ran. Sizes: 1 x 1,
257 x 3 (odd, wider than a workgroup's 256 lanes, a quad tail) and 300 x 1500 (more rows than the reduction grid's 1024: the row stride).

Tolerances: minimum, maximum, luminance, special counts, histograms and the difference map are exact. avg, variance and the MSE are
fp64 sums of fp32 values in an order that differs from numpy's: rtol 1e-6, the bar test_compute_mse_formats holds mse_kernel to.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx
from directxtex_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import diag_ref as R  # noqa: E402
from test_scanline_routes_gpu import Device, _profiled  # noqa: E402

pytestmark = pytest.mark.gpu

RGBA32F, RGBA16F, RGBA8, RGBA8S, BGRA8, BGRX8, R8 = 2, 10, 28, 29, 87, 88, 61
BPP = {RGBA32F: 16, RGBA16F: 8, RGBA8: 4, RGBA8S: 4, BGRA8: 4, BGRX8: 4, R8: 1}
SIZES = [(1, 1), (257, 3), (300, 1500)]
E_POINTER, E_INVALIDARG, E_FAIL, E_NOT_SUPPORTED = dx.E_POINTER, dx.E_INVALIDARG, dx.E_FAIL, dx.HRESULT_E_NOT_SUPPORTED


def _size_id(s):
    return f"{s[0]}x{s[1]}"


def _image(rng, fmt, w, h):
    """Random texels: uniform [0, 1) for the float formats, random bytes otherwise."""
    if fmt in (RGBA16F, RGBA32F):
        v = rng.random((h, w, 4), dtype=np.float32)
        return v.astype(np.float16 if fmt == RGBA16F else np.float32).view(np.uint8).reshape(-1)
    return rng.integers(0, 256, w * h * BPP[fmt], dtype=np.uint8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_exact(got, want):
    assert np.array_equal(_bits(got["min"]), _bits(want["min"])), (got["min"], want["min"])
    assert np.array_equal(_bits(got["max"]), _bits(want["max"])), (got["max"], want["max"])
    assert _bits(got["luminance"]) == _bits(want["luminance"]), (got["luminance"], want["luminance"])
    assert np.array_equal(got["specials"], want["specials"]), (got["specials"], want["specials"])


def _analyze_device(ctx, d, raw, fmt, w, h):
    p = d.put(raw)
    (got,), names = _profiled(ctx, lambda: ctx.analyze_device([capi.device_image(p, w, h, fmt)]))
    assert {"analyze", "analyze_var"} <= names, names
    return got


# ---- Analyze ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=_size_id)
@pytest.mark.parametrize("fmt", [RGBA8, BGRX8, R8, RGBA16F, RGBA32F])
def test_analyze_formats(ctx, oracle, fmt, size):
    w, h = size
    raw = _image(np.random.default_rng(fmt * 13 + w), fmt, w, h)
    want = R.analyze(oracle.load_image(raw, w, h, fmt))
    with Device(ctx) as d:
        got = _analyze_device(ctx, d, raw, fmt, w, h)
    _assert_exact(got, want)
    if fmt == BGRX8:
        assert got["min"][3] == 1.0 and got["max"][3] == 1.0        # X loads as alpha 1
    assert np.allclose(got["avg"], want["avg"], rtol=1e-6, atol=0), (got["avg"], want["avg"])
    assert np.allclose(got["variance"], want["variance"], rtol=1e-6, atol=0), (got["variance"], want["variance"])


def test_analyze_host_pointers(ctx, oracle):
    """dxtex_analyze stages the image itself: the figures of the device form, and only the image goes up."""
    w, h = 257, 3
    raw = _image(np.random.default_rng(5), RGBA8, w, h)
    want = R.analyze(oracle.load_image(raw, w, h, RGBA8))
    ctx.transfer_bytes(reset=True)
    (got,), names = _profiled(ctx, lambda: ctx.analyze([(raw, w, h, RGBA8, None)]))
    up, down = ctx.transfer_bytes()
    assert {"analyze", "analyze_var"} <= names
    _assert_exact(got, want)
    assert np.allclose(got["avg"], want["avg"], rtol=1e-6, atol=0) and np.allclose(got["variance"], want["variance"], rtol=1e-6, atol=0)
    assert up == raw.nbytes and down == ctypes.sizeof(ctypes.c_double) * 17        # one upload, one 136-byte accumulator back


@pytest.mark.parametrize("fmt,value", [(RGBA32F, 0.5), (RGBA8, 255)])
def test_analyze_constant(ctx, oracle, fmt, value):
    """A flat image: avg is the value itself and the sum of squared deviations is exactly 0."""
    w, h = 300, 1500
    raw = (np.full((h, w, 4), value, np.float32) if fmt == RGBA32F else np.full((h, w, 4), value, np.uint8)).view(np.uint8).reshape(-1)
    texel = oracle.load_image(raw[:BPP[fmt]], 1, 1, fmt).reshape(4)
    with Device(ctx) as d:
        got = _analyze_device(ctx, d, raw, fmt, w, h)
    assert np.array_equal(got["variance"], np.zeros(4)), got["variance"]
    assert np.array_equal(got["avg"], texel.astype(np.float64)), (got["avg"], texel)
    assert np.array_equal(_bits(got["min"]), _bits(texel)) and np.array_equal(_bits(got["max"]), _bits(texel))


def test_analyze_specials(ctx, oracle):
    """NaN, +Inf and -Inf planted in known channels: exact counts; min and max skip the NaNs and keep the infinities."""
    w, h = 257, 3
    rng = np.random.default_rng(77)
    v = (rng.random((h, w, 4), dtype=np.float32) * 4 - 2).astype(np.float32)
    v[0, 0, 0] = np.nan; v[1, 200, 0] = np.nan; v[2, 256, 0] = -np.nan       # red: three NaNs (a quad lane, a tail texel)
    v[0, 5, 1] = np.inf; v[2, 100, 1] = np.nan                               # green: +Inf and a NaN
    v[1, 7, 2] = -np.inf                                                     # blue: -Inf
    v[0, 1, 3] = np.inf; v[0, 2, 3] = -np.inf                                # alpha: both
    want = R.analyze(v)
    assert list(want["specials"]) == [3, 2, 1, 2]
    assert want["max"][1] == np.inf and want["min"][2] == -np.inf and np.isfinite(want["min"][0]) and np.isfinite(want["max"][0])
    with Device(ctx) as d:
        got = _analyze_device(ctx, d, v.view(np.uint8).reshape(-1), RGBA32F, w, h)
    _assert_exact(got, want)


def test_analyze_batch(ctx, oracle):
    """Three images of different sizes and formats in one call: the exact fields of three single calls, one copy back."""
    shapes = [(RGBA8, 64, 64), (RGBA16F, 257, 3), (R8, 33, 17)]
    rng = np.random.default_rng(3)
    raws = [_image(rng, f, w, h) for f, w, h in shapes]
    with Device(ctx) as d:
        ims = [capi.device_image(d.put(r), w, h, f) for r, (f, w, h) in zip(raws, shapes)]
        singles = [ctx.analyze_device([im])[0] for im in ims]
        ctx.transfer_bytes(reset=True)
        batch, names = _profiled(ctx, lambda: ctx.analyze_device(ims))
        up, down = ctx.transfer_bytes()
    assert {"analyze", "analyze_var"} <= names
    assert up == 0 and down == 3 * 136
    for one, many, raw, (f, w, h) in zip(singles, batch, raws, shapes):
        _assert_exact(many, one)
        _assert_exact(many, R.analyze(oracle.load_image(raw, w, h, f)))
        assert np.allclose(many["avg"], one["avg"], rtol=1e-12) and np.allclose(many["variance"], one["variance"], rtol=1e-6)


def test_analyze_errors(ctx):
    with Device(ctx) as d:
        p = d.empty(64 * 64 * 4)
        out = (capi.ImageStats * 1)()
        ok = capi.device_image(p, 64, 64, RGBA8)
        call = ctx._lib.dxtex_analyze_device
        assert call(ctx._h, ctypes.byref(ok), 1, None) == E_POINTER
        assert call(ctx._h, None, 1, out) == E_INVALIDARG
        assert call(ctx._h, ctypes.byref(ok), 0, out) == E_INVALIDARG
        assert call(ctx._h, ctypes.byref(capi.Image(64, 64, RGBA8, 256, 256 * 64, None)), 1, out) == E_POINTER
        assert call(ctx._h, ctypes.byref(capi.device_image(p, 64, 64, 98)), 1, out) == E_NOT_SUPPORTED         # BC7: decompress first
        assert call(ctx._h, ctypes.byref(capi.Image(64, 64, 1, 1024, 65536, p)), 1, out) == E_NOT_SUPPORTED   # a typeless format
        assert call(ctx._h, ctypes.byref(ok), 1, out) == 0


# ---- ComputeMSE with flags ------------------------------------------------------------------------------------------------------------
MSE_FLAGS = [0, 0x1, 0x2, 0x10, 0x20, 0x40, 0x80, 0x100, 0x200, 0x1 | 0x200 | 0x20]


@pytest.mark.parametrize("size", [(1, 1), (300, 1500)], ids=_size_id)
@pytest.mark.parametrize("fa,fb", [(RGBA8, RGBA8S), (RGBA16F, RGBA32F), (BGRX8, RGBA8)])
def test_mse_flags(ctx, oracle, fa, fb, size):
    """Every CMSE_FLAGS bit alone and one combination; the formats' implied flags (sRGB image 2, B8G8R8X8's alpha) come on top."""
    w, h = size
    rng = np.random.default_rng(fa * 11 + fb + w)
    a, b = _image(rng, fa, w, h), _image(rng, fb, w, h)
    va, vb = oracle.load_image(a, w, h, fa), oracle.load_image(b, w, h, fb)
    ref32 = oracle.ref_compute_mse(a, fa, b, fb, w, h)
    with Device(ctx) as d:
        ia, ib = capi.device_image(d.put(a), w, h, fa), capi.device_image(d.put(b), w, h, fb)
        for flags in MSE_FLAGS:
            got, names = _profiled(ctx, lambda: ctx.compute_mse_flags_device(ia, ib, flags))
            assert "mse_flags" in names and "mse" not in names
            want = R.mse(va, fa, vb, fb, flags)
            print(f"flags {flags:#x}: got {got} want {want}")
            assert np.allclose(got, want, rtol=1e-6, atol=0), (hex(flags), got, want)
            for c in range(4):
                if (flags | R.mse_implied_flags(fa, fb)) & (0x10 << c):
                    assert got[c] == 0.0
            if flags == 0:
                assert np.allclose(got, ref32, rtol=2e-4, atol=0), (got, ref32)      # the reference accumulates in fp32, serially


def test_mse_flags_errors(ctx):
    with Device(ctx) as d:
        p = d.empty(64 * 64 * 16)
        a, b = capi.device_image(p, 64, 64, RGBA8), capi.device_image(p, 64, 64, RGBA32F)
        out = (ctypes.c_double * 4)()
        call = ctx._lib.dxtex_compute_mse_flags_device
        assert call(ctx._h, ctypes.byref(a), ctypes.byref(b), 0, None) == E_POINTER
        assert call(ctx._h, ctypes.byref(capi.Image(64, 64, RGBA8, 256, 256 * 64, None)), ctypes.byref(b), 0, out) == E_POINTER
        assert call(ctx._h, ctypes.byref(a), ctypes.byref(capi.device_image(p, 32, 64, RGBA32F)), 0, out) == E_INVALIDARG
        assert call(ctx._h, ctypes.byref(capi.device_image(p, 64, 64, 71)), ctypes.byref(b), 0, out) == E_NOT_SUPPORTED
        assert call(ctx._h, ctypes.byref(a), ctypes.byref(b), 0, out) == 0


# ---- AnalyzeBC -------------------------------------------------------------------------------------------------------------------------
BC_FORMATS = sorted(R.BC_BLOCK_BYTES)
# the bins a format's blocks can land in
BC_REACH = {71: [0, 1], 72: [0, 1], 74: [], 75: [], 77: [0, 1], 78: [0, 1], 80: [0, 1], 81: [0, 1], 83: [0, 1, 2, 3], 84: [0, 1, 2, 3],
            95: list(range(15)), 96: list(range(15)), 98: list(range(9)), 99: list(range(9))}


@pytest.mark.parametrize("size", [(4, 4), (5, 7), (256, 256)], ids=_size_id)
@pytest.mark.parametrize("fmt", BC_FORMATS)
def test_analyze_bc(ctx, fmt, size):
    """Blocks of uniformly random bytes reach every mode, the BC6H reserved prefixes and (about once in 256 blocks) BC7's zero mode byte."""
    w, h = size
    bw, bh = (w + 3) // 4, (h + 3) // 4
    payload = np.random.default_rng(fmt * 7 + w).integers(0, 256, bw * bh * R.BC_BLOCK_BYTES[fmt], dtype=np.uint8)
    want, nblocks = R.bc_hist(payload, fmt, w, h)
    assert nblocks == bw * bh and int(want.sum()) == nblocks * (len(BC_REACH[fmt]) > 0) * (2 if fmt in (83, 84) else 1)
    if size == (256, 256):
        assert all(want[b] > 0 for b in BC_REACH[fmt]), (fmt, want)          # the input really exercises every bin
    assert not any(want[b] for b in range(15) if b not in BC_REACH[fmt])
    with Device(ctx) as d:
        im = capi.device_image(d.put(payload), w, h, fmt)
        (got, blocks), names = _profiled(ctx, lambda: ctx.analyze_bc_device(im))
    assert "bc_hist" in names
    assert blocks == nblocks and np.array_equal(got, want), (got, want)
    got_host, blocks_host = ctx.analyze_bc(payload, w, h, fmt)
    assert blocks_host == nblocks and np.array_equal(got_host, want)


def test_analyze_bc_pitch(ctx):
    """A padded row pitch: only the ceil(w / 4) blocks of a row are counted."""
    w, h, fmt = 20, 12, 98
    pitch = 5 * 16 + 48
    payload = np.random.default_rng(9).integers(0, 256, pitch * 3, dtype=np.uint8)
    want, nblocks = R.bc_hist(payload, fmt, w, h, pitch)
    with Device(ctx) as d:
        got, blocks = ctx.analyze_bc_device(capi.device_image(d.put(payload), w, h, fmt, pitch))
    assert blocks == nblocks == 15 and np.array_equal(got, want)


def test_analyze_bc_errors(ctx):
    with Device(ctx) as d:
        p = d.empty(64 * 64 * 4)
        hist, blocks = (ctypes.c_uint64 * 15)(), ctypes.c_uint64()
        call = ctx._lib.dxtex_analyze_bc_device
        assert call(ctx._h, ctypes.byref(capi.device_image(p, 64, 64, RGBA8)), hist, ctypes.byref(blocks)) == E_NOT_SUPPORTED
        assert call(ctx._h, ctypes.byref(capi.device_image(p, 64, 64, 98)), None, ctypes.byref(blocks)) == E_POINTER
        assert call(ctx._h, ctypes.byref(capi.Image(64, 64, 98, 256, 4096, None)), hist, ctypes.byref(blocks)) == E_POINTER
        host = np.zeros(64 * 64 * 4, np.uint8)
        assert ctx._lib.dxtex_analyze_bc(ctx._h, ctypes.byref(capi._host_image(host, 64, 64, RGBA8)), hist, ctypes.byref(blocks)) == E_NOT_SUPPORTED


# ---- Difference -----------------------------------------------------------------------------------------------------------------------
def _difference_inputs(oracle, fmt, w, h):
    """a in fmt; b = a's floats plus noise of +-0.5 per channel, so that about (1/2)^3 .. 1/2 of the texels cross 0.25 on all three."""
    rng = np.random.default_rng(fmt * 3 + w)
    a = _image(rng, fmt, w, h)
    va = oracle.load_image(a, w, h, fmt)
    noise = (rng.random((h, w, 4), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
    big = rng.random((h, w)) < 0.5                       # half the texels: every channel at least 0.3 away
    noise[big] = (np.sign(noise[big]) * (np.abs(noise[big]) * np.float32(0.4) + np.float32(0.3))).astype(np.float32)
    vb = (va + noise).astype(np.float32)
    if w * h > 2:
        # texel 1: exactly two of three channels over the threshold - must not be coloured
        vb.reshape(-1, 4)[1, :3] = va.reshape(-1, 4)[1, :3] + np.array([0.5, 0.5, 0.125], np.float32)
    return a, va, vb


def _expected_map(oracle, fmt, va, vb, w, h, color, threshold):
    ref, hit = R.difference(va, vb, color, threshold)
    if fmt == RGBA32F:
        return ref.view(np.uint8).reshape(-1), hit
    return oracle.ref_convert(ref.view(np.uint8).reshape(-1), w, h, RGBA32F, fmt, 0, 0.0), hit


@pytest.mark.parametrize("color,threshold", [(0, 0.25), (0xFF00FF, 0.25), (0x0000FF, 0.0)], ids=["plain", "magenta", "blue-t0"])
@pytest.mark.parametrize("size", [(1, 1), (257, 3), (64, 64)], ids=_size_id)
@pytest.mark.parametrize("fmt", [RGBA8, BGRA8, RGBA16F, RGBA32F])
def test_difference(ctx, oracle, fmt, size, color, threshold):
    w, h = size
    a, va, vb = _difference_inputs(oracle, fmt, w, h)
    want, hit = _expected_map(oracle, fmt, va, vb, w, h, color, threshold)
    if w * h > 2 and color:
        if threshold > 0:
            assert hit.any() and not hit.all()                                   # both branches occur
            assert not hit.reshape(-1)[1]                                        # two of three channels over: the difference, not the colour
        else:
            assert hit.all()
    with Device(ctx) as d:
        ia = capi.device_image(d.put(a), w, h, fmt)
        ib = capi.device_image(d.put(vb), w, h, RGBA32F)
        pd = d.empty(want.nbytes)
        _, names = _profiled(ctx, lambda: ctx.difference_device(ia, ib, capi.device_image(pd, w, h, fmt), color, threshold))
        got = d.get(pd, want.nbytes)
    assert "difference" in names
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    if size == (257, 3):
        assert np.array_equal(ctx.difference(a, vb, w, h, fmt, color, threshold), want)       # the host-pointer form


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
def test_difference_padded_pitch(ctx, oracle, fmt):
    """Source and destination rows with padding (still 16-byte aligned: the quad route; and 4 bytes off it: the texel route): the
    padding of the destination stays as it was."""
    w, h = 64, 9
    a, va, vb = _difference_inputs(oracle, fmt, w, h)
    want, _ = _expected_map(oracle, fmt, va, vb, w, h, 0xFF00FF, 0.25)
    row = w * BPP[fmt]
    for pad in (32, 4):
        pitch = row + pad
        with Device(ctx) as d:
            ia = capi.device_image(d.put_rows(a, h, row, pitch), w, h, fmt, pitch)
            ib = capi.device_image(d.put(vb), w, h, RGBA32F)
            fill = np.full(pitch * h, 0xA5, np.uint8)
            pd = d.put(fill)
            ctx.difference_device(ia, ib, capi.device_image(pd, w, h, fmt, pitch), 0xFF00FF, 0.25)
            got = d.get(pd, pitch * h).reshape(h, pitch)
        assert np.array_equal(got[:, :row].reshape(-1), want), pad
        assert (got[:, row:] == 0xA5).all(), pad


def test_difference_errors(ctx):
    with Device(ctx) as d:
        p = d.empty(64 * 64 * 16)
        a, b, dst = capi.device_image(p, 64, 64, RGBA8), capi.device_image(p, 64, 64, RGBA32F), capi.device_image(p, 64, 64, RGBA8)

        def call(x, y, z):
            return ctx._lib.dxtex_difference_device(ctx._h, ctypes.byref(x), ctypes.byref(y), ctypes.byref(z), 0, 0.25)
        assert call(capi.Image(64, 64, RGBA8, 256, 256 * 64, None), b, dst) == E_POINTER
        assert call(a, capi.device_image(p, 64, 32, RGBA32F), dst) == E_FAIL
        assert call(a, capi.device_image(p, 64, 64, RGBA16F), dst) == E_NOT_SUPPORTED
        assert call(a, b, capi.device_image(p, 64, 64, BGRA8)) == E_NOT_SUPPORTED
        assert call(capi.device_image(p, 64, 64, 77), b, capi.device_image(p, 64, 64, 77)) == E_NOT_SUPPORTED
        assert call(a, b, dst) == 0


def test_difference_host_padding_and_pitch(ctx, oracle):
    """The host-pointer form leaves the row padding of the caller's destination as it was, and reports a second image whose rows are not
    16-byte multiples as E_INVALIDARG before anything runs."""
    w, h, fmt = 33, 5, RGBA8
    a, va, vb = _difference_inputs(oracle, fmt, w, h)
    want, _ = _expected_map(oracle, fmt, va, vb, w, h, 0xFF00FF, 0.25)
    row, pitch = w * 4, w * 4 + 12
    dst = np.full(pitch * h, 0x5A, np.uint8)
    ia, ib = capi._host_image(a, w, h, fmt), capi._host_image(np.ascontiguousarray(vb), w, h, RGBA32F)
    idst = capi.Image(w, h, fmt, pitch, pitch * h, dst.ctypes.data)
    assert ctx._lib.dxtex_difference(ctx._h, ctypes.byref(ia), ctypes.byref(ib), ctypes.byref(idst), 0xFF00FF, 0.25) == 0
    got = dst.reshape(h, pitch)
    assert np.array_equal(got[:, :row].reshape(-1), want) and (got[:, row:] == 0x5A).all()
    padded = np.zeros((w * 16 + 8) * h, np.uint8)
    bad = capi.Image(w, h, RGBA32F, w * 16 + 8, (w * 16 + 8) * h, padded.ctypes.data)
    assert ctx._lib.dxtex_difference(ctx._h, ctypes.byref(ia), ctypes.byref(bad), ctypes.byref(idst), 0, 0.25) == E_INVALIDARG
    assert b"multiple of 16" in ctx._lib.dxtex_ctx_last_error(ctx._h)
