"""dxtex_merge_image / dxtex_merge_image_device (texassemble's merge, Texassemble/texassemble.cpp:2236-2268) against the oracle's compiled
LoadScanline and StoreScanline around a numpy permute (tests/assemble_ref.py). Channels are moved, never computed, so every comparison is
byte equality - with NaN, infinity and -0 in both images where the destination is a float format, whose stores must keep their bits.

Sizes: 1 x 1 and 67 x 45 (odd, rows that are no multiple of anything, more rows than a workgroup column walks in one step is not
reachable below 8192 rows: the row stride is transform_kernel's, which tests/test_transform_gpu.py holds at size).
"""
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx
from directxtex_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_ref as R  # noqa: E402
from test_scanline_routes_gpu import Device, _profiled  # noqa: E402

pytestmark = pytest.mark.gpu

RGBA32F, RGBA16F, RGB10A2, RGBA8, BC1 = 2, 10, 24, 28, 71
BPP = {RGBA32F: 16, RGBA16F: 8, RGB10A2: 4, RGBA8: 4}
SIZES = [(1, 1), (67, 45)]
SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 65504.0, 1e-40], np.float32)

# all eight source indices, each in every output channel; then the zero / one masks (one wins where both are set)
PERMUTES = [((0, 1, 2, 3), (0, 0, 0, 0), (0, 0, 0, 0)),
            ((4, 5, 6, 7), (0, 0, 0, 0), (0, 0, 0, 0)),
            ((7, 2, 5, 0), (0, 0, 0, 0), (0, 0, 0, 0)),
            ((3, 6, 1, 4), (0, 0, 0, 0), (0, 0, 0, 0)),
            ((1, 0, 7, 6), (0, 0, 0, 0), (0, 0, 0, 0)),
            ((0, 1, 2, 4), (0, 0, 0, 0), (0, 0, 0, 0)),          # texassemble's default: rgb of image 1, alpha = red of image 2
            ((0, 5, 2, 7), (1, 0, 0, 1), (0, 0, 1, 0)),
            ((6, 6, 6, 6), (1, 1, 0, 0), (1, 0, 0, 1))]


def _first_image(rng, fmt, w, h):
    if fmt in (RGBA32F, RGBA16F):
        v = (rng.random((h, w, 4), dtype=np.float32) * 4 - 1).astype(np.float32)
        flat = v.reshape(-1)
        flat[:min(flat.size, SPECIALS.size)] = SPECIALS[:flat.size]
        return v.astype(np.float16 if fmt == RGBA16F else np.float32).view(np.uint8).reshape(-1)
    return rng.integers(0, 256, w * h * BPP[fmt], dtype=np.uint8)


def _second_image(rng, w, h, specials):
    """Finite floats in [-1, 3); with `specials` (float destinations, whose stores keep them) the special values too."""
    v = (rng.random((h, w, 4), dtype=np.float32) * 4 - 1).astype(np.float32)
    if specials:
        flat = v.reshape(-1)
        flat[-min(flat.size, SPECIALS.size):] = SPECIALS[:flat.size]
    return v


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F, RGB10A2, RGBA32F])
def test_merge_device(ctx, oracle, fmt, size):
    w, h = size
    rng = np.random.default_rng(fmt * 3 + w)
    a, b = _first_image(rng, fmt, w, h), _second_image(rng, w, h, fmt in (RGBA16F, RGBA32F))
    pitch = w * BPP[fmt]
    with Device(ctx) as d:
        pa, pb, pd = d.put(a), d.put(b), d.empty(pitch * h)
        ia, ib, idst = capi.device_image(pa, w, h, fmt), capi.device_image(pb, w, h, RGBA32F), capi.device_image(pd, w, h, fmt)
        for permute, zero, one in PERMUTES:
            want = R.merge(oracle, a, b, w, h, fmt, pitch, permute, zero, one)
            _, names = _profiled(ctx, lambda: ctx.merge_image_device(ia, ib, idst, permute, zero, one))
            assert names == {"merge"}, names
            got = d.get(pd, pitch * h)
            assert np.array_equal(got, want), (permute, zero, one, np.flatnonzero(got != want)[:8])


def test_merge_host_pointers(ctx, oracle):
    """dxtex_merge_image stages both images itself and brings the merged texels back: two uploads, one download of the image's bytes."""
    w, h = 67, 45
    rng = np.random.default_rng(9)
    a, b = _first_image(rng, RGBA8, w, h), _second_image(rng, w, h, False)
    permute, zero, one = PERMUTES[6]
    ctx.transfer_bytes(reset=True)
    got = ctx.merge_image(a, b, w, h, RGBA8, permute, zero, one)
    up, down = ctx.transfer_bytes()
    assert np.array_equal(got, R.merge(oracle, a, b, w, h, RGBA8, w * 4, permute, zero, one))
    assert up == a.nbytes + b.nbytes and down == a.nbytes, (up, down)


def test_merge_hresults(ctx):
    w, h = 4, 4
    with Device(ctx) as d:
        pa, pb, pd = d.empty(w * h * 16), d.empty(w * h * 16), d.empty(w * h * 16)
        a8, b32, d8 = capi.device_image(pa, w, h, RGBA8), capi.device_image(pb, w, h, RGBA32F), capi.device_image(pd, w, h, RGBA8)

        def hr(a, b, dst, permute=(0, 1, 2, 4)):
            try:
                ctx.merge_image_device(a, b, dst, permute)
            except dx.DxtexError as e:
                return e.hresult & 0xFFFFFFFF
            return 0
        assert hr(a8, b32, d8) == 0
        assert hr(a8, b32, d8, (0, 1, 2, 8)) == dx.E_INVALIDARG & 0xFFFFFFFF
        assert hr(a8, capi.device_image(pb, w, h, RGBA8), d8) == dx.HRESULT_E_NOT_SUPPORTED & 0xFFFFFFFF
        assert hr(a8, b32, capi.device_image(pd, w, h, RGBA16F)) == dx.HRESULT_E_NOT_SUPPORTED & 0xFFFFFFFF
        assert hr(capi.device_image(pa, w, h, BC1), b32, capi.device_image(pd, w, h, BC1)) == dx.HRESULT_E_NOT_SUPPORTED & 0xFFFFFFFF
        assert hr(a8, capi.device_image(pb, w, 3, RGBA32F), d8) == dx.E_FAIL & 0xFFFFFFFF
        assert hr(a8, b32, a8) == dx.E_INVALIDARG & 0xFFFFFFFF                                      # in place
        assert hr(a8, capi.device_image(pb + 4, w, h, RGBA32F), d8) == dx.E_INVALIDARG & 0xFFFFFFFF   # float4 rows need 16-byte alignment
        assert hr(capi.device_image(0, w, h, RGBA8), b32, d8) == dx.E_POINTER & 0xFFFFFFFF
    ctx.synchronize()
