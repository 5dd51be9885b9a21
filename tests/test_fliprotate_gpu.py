"""dxtex_flip_rotate / dxtex_flip_rotate_device against the numpy restatement (tests/fliprotate_ref.py).

Every comparison is of the WHOLE destination buffer, which starts as a seeded random pattern: a byte written into row padding, or outside a
cell of a larger image, shows. Byte equality: texels are moved, never computed.

One format per texel size (1, 2, 4, 8, 12, 16 bytes), all fifteen flag words, the two words of a class also against each other. Shapes:
1 x 1; 7 x 5; 131 x 97, which is at least two tiles and a ragged edge in both directions for both tile sides (64 and 32); 128 x 48, whose
tight rows are whole 16-byte units so that the wide form of the row route must run. Pitches tight, or padded by 3 bytes, which leaves
nothing aligned: the narrow form must run, a byte at a time. Which kernel ran is read from the profile marks."""
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx
from directxtex_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fliprotate_ref as R  # noqa: E402
from test_scanline_routes_gpu import Device  # noqa: E402

pytestmark = pytest.mark.gpu

RGBA32F, RGB32F, RGBA16F, RGBA8, RG8, R8 = 2, 6, 10, 28, 49, 61
TEXEL = {R8: 1, RG8: 2, RGBA8: 4, RGBA16F: 8, RGB32F: 12, RGBA32F: 16}
SHAPES = ((1, 1), (7, 5), (131, 97), (128, 48))
BC1, NV12, P8, R1, RGBA8_TYPELESS, YUY2, RG_BG, R32_UINT, D32S8 = 71, 103, 113, 66, 27, 107, 68, 42, 20


def _signed(hr):
    hr &= 0xFFFFFFFF
    return hr - (1 << 32) if hr & 0x80000000 else hr


def _out_size(w, h, flags):
    return (h, w) if R.transposes(flags) else (w, h)


def _expected_mark(w, h, texel, sp, dp, flags):
    """The route rule restated: addresses from the allocator are aligned, so only the pitches and the row's bytes decide."""
    if R.transposes(flags):
        return "flip_transpose"
    wide = texel != 12 and (w * texel) % 16 == 0 and (h == 1 or (sp % 16 == 0 and dp % 16 == 0))
    return "flip_rows<wide>" if wide else "flip_rows<narrow>"


def _run(ctx, d, src, w, h, fmt, sp, dst, dp, flags):
    W, H = _out_size(w, h, flags)
    ps, pd = d.put(src), d.put(dst)
    a = capi.device_image(ps, w, h, fmt, sp)
    b = capi.device_image(pd, W, H, fmt, dp)
    ctx.profile_begin()
    try:
        ctx.flip_rotate_device([a], [b], flags)
    finally:
        prof = ctx.profile_end()
    return d.get(pd, dst.nbytes), prof


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", sorted(TEXEL, reverse=True), ids=lambda f: f"fmt{f}")
def test_all_flags_equal_restatement(ctx, fmt, shape):
    w, h = shape
    texel = TEXEL[fmt]
    rng = np.random.default_rng(fmt * 1000 + w)
    for pad in (0, 3):
        sp = w * texel + pad
        src = rng.integers(0, 256, sp * h, dtype=np.uint8)
        results = {}
        with Device(ctx) as d:
            for f in R.LEGAL:
                W, H = _out_size(w, h, f)
                dp = W * texel + pad
                dst = rng.integers(0, 256, dp * H, dtype=np.uint8)
                got, prof = _run(ctx, d, src, w, h, fmt, sp, dst, dp, f)
                want = R.expected(dst, dp, src, w, h, texel, sp, f)
                assert np.array_equal(got, want), (fmt, shape, pad, f, np.flatnonzero(got != want)[:8])
                mark = _expected_mark(w, h, texel, sp, dp, f)
                assert set(prof) == {mark} and prof[mark][1] == 1, (fmt, shape, pad, f, prof)
                if pad == 3 and not R.transposes(f) and h > 1:
                    assert mark == "flip_rows<narrow>"
                if pad == 0 and shape == (128, 48) and not R.transposes(f):
                    assert mark == ("flip_rows<narrow>" if texel == 12 else "flip_rows<wide>")
                results[f] = R.texels(got, W, H, texel, dp)
        for cls in R.CLASSES:
            a = [results[f] for f in sorted(cls)]
            assert all(np.array_equal(a[0], x) for x in a), (fmt, shape, pad, cls)
        assert np.array_equal(results[26], R.texels(src, w, h, texel, sp))


def test_bits_are_kept_for_integer_and_depth_formats(ctx):
    """R32_UINT above 2^24 and D32_FLOAT_S8X24_UINT, which the reference would send through floats: here bits are kept."""
    rng = np.random.default_rng(5)
    for fmt, texel in ((R32_UINT, 4), (D32S8, 8)):
        w, h = 9, 6
        src = rng.integers(0, 256, w * h * texel, dtype=np.uint8)
        with Device(ctx) as d:
            for f in (R.ROTATE90, R.FLIP_HORIZONTAL):
                W, H = _out_size(w, h, f)
                dst = rng.integers(0, 256, W * H * texel, dtype=np.uint8)
                got, _ = _run(ctx, d, src, w, h, fmt, w * texel, dst, W * texel, f)
                assert np.array_equal(got, R.expected(dst, W * texel, src, w, h, texel, w * texel, f))


@pytest.mark.parametrize("flags", R.LEGAL)
def test_destination_is_a_cell_of_a_larger_image(ctx, flags):
    """A 16 x 16 face into the cell at (16, 16) of a 64 x 48 image: a pointer into it and its pitch. Nothing else of it changes."""
    rng = np.random.default_rng(flags)
    face = rng.integers(0, 256, 16 * 16 * 4, dtype=np.uint8)
    big = rng.integers(0, 256, 64 * 48 * 4, dtype=np.uint8)
    at = 16 * 256 + 16 * 4
    with Device(ctx) as d:
        pf, pb = d.put(face), d.put(big)
        ctx.flip_rotate_device([capi.device_image(pf, 16, 16, RGBA8)], [capi.device_image(pb + at, 16, 16, RGBA8, 256)], flags)
        got = d.get(pb, big.nbytes)
    assert np.array_equal(got, R.expected(big, 256, face, 16, 16, 4, 64, flags, at=at))


@pytest.mark.parametrize("flags", (R.FLIP_HORIZONTAL, R.FLIP_VERTICAL, R.ROTATE180, R.ROTATE90, R.ROTATE270 | R.FLIP_VERTICAL))
def test_batch_is_one_launch_per_route(ctx, flags):
    """A 16 x 8 texture with its full chain and two items, ten images in one call: one launch of the route the flags use."""
    rng = np.random.default_rng(11)
    sizes = [(16, 8), (8, 4), (4, 2), (2, 1), (1, 1)] * 2
    srcs = [rng.integers(0, 256, w * h * 4, dtype=np.uint8) for w, h in sizes]
    dsts = [rng.integers(0, 256, w * h * 4, dtype=np.uint8) for w, h in sizes]
    with Device(ctx) as d:
        ps, pd = [d.put(s) for s in srcs], [d.put(x) for x in dsts]
        a = [capi.device_image(p, w, h, RGBA8) for p, (w, h) in zip(ps, sizes)]
        b = [capi.device_image(p, *_out_size(w, h, flags), RGBA8) for p, (w, h) in zip(pd, sizes)]
        ctx.profile_begin()
        try:
            ctx.flip_rotate_device(a, b, flags)
        finally:
            prof = ctx.profile_end()
        got = [d.get(p, x.nbytes) for p, x in zip(pd, dsts)]
    assert len(prof) == 1 and list(prof.values())[0][1] == 1, prof
    # the chain's rows are 64, 32 and 16 bytes, then 8 and 4: both forms of the row route in the one launch
    assert set(prof) == ({"flip_transpose"} if R.transposes(flags) else {"flip_rows<mixed>"}), prof
    for g, s, x, (w, h) in zip(got, srcs, dsts, sizes):
        W, H = _out_size(w, h, flags)
        assert np.array_equal(g, R.expected(x, W * 4, s, w, h, 4, w * 4, flags))


def test_more_than_one_batch(ctx):
    """Forty images are two launches (32 + 8)."""
    rng = np.random.default_rng(12)
    srcs = [rng.integers(0, 256, 5 * 3 * 2, dtype=np.uint8) for _ in range(40)]
    with Device(ctx) as d:
        ps, pd = [d.put(s) for s in srcs], [d.empty(30) for _ in range(40)]
        ctx.profile_begin()
        try:
            ctx.flip_rotate_device([capi.device_image(p, 5, 3, RG8) for p in ps], [capi.device_image(p, 3, 5, RG8) for p in pd], R.ROTATE270)
        finally:
            prof = ctx.profile_end()
        got = [d.get(p, 30) for p in pd]
    assert prof == {"flip_transpose": (prof["flip_transpose"][0], 2)}, prof
    for g, s in zip(got, srcs):
        assert np.array_equal(g, R.flip_rotate(s.reshape(3, 5, 2), R.ROTATE270).reshape(-1))


def _hr(ctx, a, b, flags):
    try:
        ctx.flip_rotate_device(a, b, flags)
    except dx.DxtexError as e:
        return _signed(e.hresult)
    return 0


def test_hresults_in_order(ctx):
    with Device(ctx) as d:
        start = np.random.default_rng(3).integers(0, 256, 4096, dtype=np.uint8)
        ps, pd = d.put(start), d.put(start)

        def img(p, w=7, h=5, fmt=RGBA8, pitch=None):
            texel = TEXEL.get(fmt, 4)
            return capi.Image(w, h, fmt, pitch or w * texel, (pitch or w * texel) * h, p)

        ok_s, ok_d = img(ps), img(pd)
        assert _hr(ctx, [ok_s], [ok_d], R.FLIP_VERTICAL) == 0
        # 1. E_POINTER for null pixels - before the flags, the format and the sizes
        assert _hr(ctx, [img(0)], [ok_d], R.FLIP_VERTICAL) == R.E_POINTER
        assert _hr(ctx, [ok_s], [img(0)], R.FLIP_VERTICAL) == R.E_POINTER
        assert _hr(ctx, [img(0, fmt=BC1)], [img(pd, 3, 3)], 0) == R.E_POINTER
        # 2. E_INVALIDARG for illegal flags - before the format
        for f in R.ILLEGAL:
            assert _hr(ctx, [ok_s], [ok_d], f) == R.E_INVALIDARG
            assert _hr(ctx, [img(ps, fmt=BC1)], [img(pd, fmt=BC1)], f) == R.E_INVALIDARG
        # 3. DXTEX_E_NOT_SUPPORTED for compressed, planar, palettised, typeless, two-texel packed formats, R1_UNORM and no format - before
        #    the mismatch
        for fmt in (BC1, 98, NV12, P8, RGBA8_TYPELESS, YUY2, RG_BG, R1, 0, 200):
            assert _hr(ctx, [img(ps, 8, 4, fmt)], [img(pd, 8, 4, fmt)], R.ROTATE180) == R.E_NOT_SUPPORTED, fmt
            assert _hr(ctx, [img(ps, 8, 4, fmt)], [img(pd, 3, 3, RGBA8)], R.ROTATE180) == R.E_NOT_SUPPORTED, fmt
        # 4. E_FAIL for a format or size mismatch - before the overlap
        assert _hr(ctx, [ok_s], [img(pd, fmt=87)], R.FLIP_VERTICAL) == R.E_FAIL
        assert _hr(ctx, [ok_s], [img(pd, 5, 7)], R.FLIP_VERTICAL) == R.E_FAIL          # the swapped size, but no quarter turn
        assert _hr(ctx, [ok_s], [ok_d], R.ROTATE90) == R.E_FAIL                         # a quarter turn, but not the swapped size
        assert _hr(ctx, [ok_s], [img(ps, 5, 7)], R.FLIP_VERTICAL) == R.E_FAIL           # mismatch and overlap: the mismatch
        assert _hr(ctx, [ok_s], [img(pd, 5, 7)], R.ROTATE90) == 0
        # 5. E_INVALIDARG where the bytes read and the bytes written overlap, and for a pitch below the row
        assert _hr(ctx, [ok_s], [img(ps)], R.FLIP_VERTICAL) == R.E_INVALIDARG
        assert _hr(ctx, [ok_s], [img(ps + 7 * 4 * 4 + 27)], R.FLIP_VERTICAL) == R.E_INVALIDARG      # the last byte read is the first written
        assert _hr(ctx, [ok_s], [img(ps + 7 * 4 * 5)], R.FLIP_VERTICAL) == 0                          # the byte after it
        assert _hr(ctx, [ok_s], [img(pd, pitch=27)], R.FLIP_VERTICAL) == R.E_INVALIDARG
        # no images
        assert _hr(ctx, [], [], R.FLIP_VERTICAL) == R.E_INVALIDARG
        # all pairs are checked before anything is queued: the good first pair of a refused call has not run
        before = d.get(pd, 4096)
        assert _hr(ctx, [ok_s, ok_s], [ok_d, img(pd + 1024, 5, 7)], R.ROTATE180) == R.E_FAIL
        assert np.array_equal(d.get(pd, 4096), before)


@pytest.mark.parametrize("case", ((131, 97, RGB32F, R.ROTATE90, 3), (7, 5, R8, R.FLIP_HORIZONTAL, 0), (128, 48, RGBA8, R.ROTATE180 | R.FLIP_VERTICAL, 0)),
                         ids=lambda c: f"{c[0]}x{c[1]}_fmt{c[2]}_{c[3]}")
def test_host_pointer_form_moves_the_rows_only(ctx, case):
    w, h, fmt, flags, pad = case
    texel = TEXEL[fmt]
    sp = w * texel + pad
    src = np.random.default_rng(7).integers(0, 256, sp * h, dtype=np.uint8)
    ctx.transfer_bytes(reset=True)
    got = ctx.flip_rotate(src, w, h, fmt, flags, row_pitch=sp)
    up, down = ctx.transfer_bytes()
    W, H = _out_size(w, h, flags)
    assert np.array_equal(got.reshape(H, W, texel), R.flip_rotate(R.texels(src, w, h, texel, sp), flags))
    assert (up, down) == (w * h * texel, w * h * texel)


def test_host_pointer_form_leaves_padding_alone(ctx):
    """The caller's destination pitch is its own: only the rows' texels come down."""
    w, h, texel, flags = 7, 5, 4, R.ROTATE270
    rng = np.random.default_rng(8)
    src = rng.integers(0, 256, w * h * texel, dtype=np.uint8)
    dp = h * texel + 9
    dst = rng.integers(0, 256, dp * w, dtype=np.uint8)
    want = R.expected(dst, dp, src, w, h, texel, w * texel, flags)
    a = capi.Image(w, h, RGBA8, w * texel, w * texel * h, src.ctypes.data)
    b = capi.Image(h, w, RGBA8, dp, dp * w, dst.ctypes.data)
    import ctypes
    hr = ctx._lib.dxtex_flip_rotate(ctx._h, ctypes.byref(a), ctypes.byref(b), flags)
    assert hr == 0
    assert np.array_equal(dst, want)
