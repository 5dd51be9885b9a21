"""texconv's per-texel transforms on the GPU (dxtex_transform_image / dxtex_transform_images_device, TransformImage in the host layer,
dxtexconv -swizzle / -tonemap / -c / -inverty / -reconstructz) against the reference: its own LoadScanline / StoreScanline (oracle) around
the restated lambdas (tests/transform_ref.py), byte for byte."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import directxtex_amd as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import transform_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

E_FAIL, E_INVALIDARG, E_POINTER = 0x80004005 - (1 << 32), 0x80070057 - (1 << 32), 0x80004003 - (1 << 32)
E_NOT_SUPPORTED = 0x80070032 - (1 << 32)
RGBA8, RGBA8_SRGB, BGRA8, RGBA16F, RGBA16, RGBA16S, RGBA32F = 28, 29, 87, 10, 11, 13, 2
FORMATS = [RGBA8, RGBA8_SRGB, BGRA8, RGBA16F, RGBA16, RGBA16S, RGBA32F, 24, 26, 67, 85, 51, 61, 65, 45, 107, 66]
UNORM = {RGBA8, RGBA8_SRGB, BGRA8, RGBA16, 24, 85, 61, 65, 45, 107, 66}
KEY = 0x40C080
OPS = [("swizzle bgr1", R.SWIZZLE, "bgr1"), ("swizzle w0", R.SWIZZLE, "w0"), ("tonemap", R.TONEMAP, None), ("colorkey", R.COLOR_KEY, None),
       ("inverty", R.INVERT_Y, None), ("reconstructz", R.RECONSTRUCT_Z, None)]


def _hr(e):
    v = int(re.search(r"hr=(-?0x[0-9a-fA-F]+|-?\d+)", str(e)).group(1), 0)
    return v - (1 << 32) if v >= 1 << 31 else v


def _source(fmt, w, h, seed):
    """Random bytes of a tight image; float formats get NaNs (with payloads), infinities, signed zeros and denormals; UNORM texels near
    the colour key so that it matches somewhere."""
    rp, sp = dx.compute_pitch(fmt, w, h)
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, 256, sp, dtype=np.uint8)
    if fmt == RGBA32F:
        f = pix.view(np.uint32)
        special = np.array([0x7FC00001, 0xFF800000, 0x7F800000, 0x80000000, 0x00000001, 0xFFC12345, 0x3F800000, 0x3E800000], np.uint32)
        f[:] = np.where(rng.random(f.size) < 0.7, rng.uniform(-0.5, 2.0, f.size).astype(np.float32).view(np.uint32), f)
        f[rng.integers(0, f.size, max(1, f.size // 16))] = rng.choice(special, max(1, f.size // 16))
    elif fmt == RGBA16F:
        h16 = pix.view(np.uint16)
        h16[:] = np.where(rng.random(h16.size) < 0.7, rng.uniform(-0.5, 2.0, h16.size).astype(np.float16).view(np.uint16), h16)
        special = np.array([0x7E01, 0xFC00, 0x7C00, 0x8000, 0x0001, 0x3C00], np.uint16)
        h16[rng.integers(0, h16.size, max(1, h16.size // 16))] = rng.choice(special, max(1, h16.size // 16))
    elif fmt in (RGBA8, BGRA8) and w * h > 4:
        t = pix.reshape(-1, 4)
        k = np.array([(KEY >> 16) & 0xFF, (KEY >> 8) & 0xFF, KEY & 0xFF], np.uint8)
        if fmt == BGRA8:
            k = k[::-1]
        t[::5, :3] = k
    return pix, rp


HALF_FORMATS = (10, 34, 54)             # R16G16B16A16_FLOAT, R16G16_FLOAT, R16_FLOAT


def _want(oracle, pix, w, h, fmt, rp, op, mask, m=None, nan_texels=False):
    rows = R.load_rows(oracle, pix, w, h, fmt, rp)
    swz, zero, one = R.parse_swizzle_mask(mask) if mask else ((0, 1, 2, 3), (0,) * 4, (0,) * 4)
    if op == R.TONEMAP and m is None:
        m = R.max_luminance([rows])
    out = R.apply(rows, op, swz, zero, one, KEY, fmt in UNORM, m if m is not None else 0.0)
    want = R.store_rows(oracle, out, fmt, rp)
    return (want, np.isnan(out).any(axis=-1)) if nan_texels else want


def _assert_same(got, want, nan, fmt, w, h, rp, what):
    """Byte for byte. Where the op hands StoreScanline a NaN: R32G32B32A32_FLOAT stores the row as it is, so its NaNs are compared bit for
    bit; a half format stores a NaN half on both sides (store_half lets it through the clamp, as XMVectorClamp does), compared as "NaN in
    both" since a NaN half's sign and payload are the platform's; the other formats only have to store the texel somehow."""
    g, t = got.reshape(h, rp), want.reshape(h, rp)
    if fmt in HALF_FORMATS and nan.any():
        gh, th = g.view(np.float16), t.view(np.float16)
        same = (g.view(np.uint16) == t.view(np.uint16)) | (np.isnan(gh) & np.isnan(th))
        assert same.all(), (what, fmt, w, h, np.argwhere(~same)[:8])
        return
    if fmt != RGBA32F and nan.any() and fmt not in (107, 66):
        bpt = rp // w
        keep = np.ones((h, rp), bool)
        ys, xs = np.nonzero(nan)
        for k in range(bpt):
            keep[ys, xs * bpt + k] = False
        g, t = g[keep], t[keep]
    bad = np.nonzero(g.reshape(-1) != t.reshape(-1))[0]
    assert bad.size == 0, (what, fmt, w, h, bad[:8], g.reshape(-1)[bad[:8]], t.reshape(-1)[bad[:8]])


def _transform(op, mask):
    return dx.make_transform(op, mask if mask else (0, 1, 2, 3), color_key=KEY)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("w,h", [(1, 1), (67, 45)])
def test_every_op_matches_the_reference(ctx, oracle, fmt, w, h):
    pix, rp = _source(fmt, w, h, fmt * 131 + w)
    for name, op, mask in OPS:
        got = ctx.transform_image(pix, w, h, fmt, _transform(op, mask))
        want, nan = _want(oracle, pix, w, h, fmt, rp, op, mask, nan_texels=True)
        _assert_same(got, want, nan, fmt, w, h, rp, name)


@pytest.mark.parametrize("fmt", [RGBA8, RGBA16F])
def test_taller_than_the_grid(ctx, oracle, fmt):
    """3 x 70 000: the kernels stride past grid.y's 65 535 rows."""
    w, h = 3, 70000
    pix, rp = _source(fmt, w, h, 7)
    for name, op, mask in OPS:
        got = ctx.transform_image(pix, w, h, fmt, _transform(op, mask))
        want, nan = _want(oracle, pix, w, h, fmt, rp, op, mask, nan_texels=True)
        _assert_same(got, want, nan, fmt, w, h, rp, name)


def _upload(ctx, bufs):
    ptrs = []
    for b in bufs:
        p = ctx.device_alloc(b.nbytes)
        ctx.upload(p, b, sync=True)
        ptrs.append(p)
    return ptrs


@pytest.mark.parametrize("fmt", [RGBA16F, RGBA32F, RGBA8])
def test_tonemap_takes_the_maximum_over_every_image(ctx, oracle, fmt):
    """A 3-level mip chain of a 2-item array whose brightest texel sits in a small mip of the second item: the device call over all six
    images equals the restatement with the maximum over all of them, and each image differs from a tone map of that image alone."""
    sizes = [(40, 24), (20, 12), (10, 6)]
    imgs = []
    for item in range(2):
        for lvl, (w, h) in enumerate(sizes):
            pix, rp = _source(fmt, w, h, 100 + 10 * item + lvl)
            if fmt != RGBA8:
                rows = R.load_rows(oracle, pix, w, h, fmt, rp)
                rows = np.clip(np.nan_to_num(rows, nan=0.25, posinf=1.0, neginf=0.0), 0.0, 1.5)
                if item == 1 and lvl == 2:
                    rows[3, 4, :3] = 6.0
                pix = R.store_rows(oracle, rows, fmt, rp)
            elif item == 1 and lvl == 2:
                pix[(3 * w + 4) * 4:(3 * w + 4) * 4 + 3] = 255
            imgs.append((pix, w, h, rp))
    all_rows = [R.load_rows(oracle, p, w, h, fmt, rp) for p, w, h, rp in imgs]
    m = R.max_luminance(all_rows)
    srcs = _upload(ctx, [p for p, _, _, _ in imgs])
    dsts = [ctx.device_alloc(p.nbytes, zero=True) for p, _, _, _ in imgs]
    try:
        t = dx.make_transform(dx.TRANSFORM_TONEMAP)
        ctx.transform_images_device([dx.device_image(s, w, h, fmt) for s, (_, w, h, _) in zip(srcs, imgs)],
                                    [dx.device_image(d, w, h, fmt) for d, (_, w, h, _) in zip(dsts, imgs)], t)
        ctx.synchronize()
        differs = 0
        for d, (p, w, h, rp), rows in zip(dsts, imgs, all_rows):
            got = np.zeros(p.nbytes, np.uint8)
            ctx.download(got, d, sync=True)
            want = R.store_rows(oracle, R.tonemap(rows, m), fmt, rp)
            assert np.array_equal(got, want), (w, h)
            alone = ctx.transform_image(p, w, h, fmt, t)
            assert np.array_equal(alone, _want(oracle, p, w, h, fmt, rp, R.TONEMAP, None))      # the host form, one image
            differs += not np.array_equal(alone, got)
        assert differs >= 5
    finally:
        for p in srcs + dsts:
            ctx.device_free(p)


def test_hresults(ctx):
    w, h = 8, 8
    pix = np.zeros(w * h * 16, np.uint8)
    out = np.zeros(w * h * 16, np.uint8)
    t = dx.make_transform(dx.TRANSFORM_INVERT_Y)
    for fmt, want in ((71, E_NOT_SUPPORTED), (98, E_NOT_SUPPORTED), (27, E_NOT_SUPPORTED), (1, E_NOT_SUPPORTED), (103, E_NOT_SUPPORTED),
                      (104, E_NOT_SUPPORTED), (113, E_NOT_SUPPORTED), (118, E_NOT_SUPPORTED), (0, E_NOT_SUPPORTED), (RGBA8, 0)):
        s = dx.Image(w, h, fmt, w * 4, w * h * 4, pix.ctypes.data)
        d = dx.Image(w, h, fmt, w * 4, w * h * 4, out.ctypes.data)
        assert ctx._lib.dxtex_transform_image(ctx._h, s, d, t) == want, fmt
    s = dx.Image(w, h, RGBA8, w * 4, w * h * 4, pix.ctypes.data)
    assert ctx._lib.dxtex_transform_image(ctx._h, s, dx.Image(w, h, BGRA8, w * 4, w * h * 4, out.ctypes.data), t) == E_FAIL
    assert ctx._lib.dxtex_transform_image(ctx._h, s, dx.Image(w, h - 1, RGBA8, w * 4, w * h * 4, out.ctypes.data), t) == E_FAIL
    assert ctx._lib.dxtex_transform_image(ctx._h, s, dx.Image(w, h, RGBA8, w * 4, w * h * 4, None), t) == E_POINTER
    assert ctx._lib.dxtex_transform_image(ctx._h, s, dx.Image(w, h, RGBA8, w * 4, w * h * 4, out.ctypes.data), None) == E_POINTER
    assert ctx._lib.dxtex_transform_image(None, s, s, t) == E_POINTER
    assert ctx._lib.dxtex_transform_image(ctx._h, s, dx.Image(w, h, RGBA8, w * 4, w * h * 4, out.ctypes.data), dx.make_transform(9)) == E_INVALIDARG
    assert ctx._lib.dxtex_transform_image(ctx._h, s, dx.Image(w, h, RGBA8, w * 4, w * h * 4, out.ctypes.data), dx.make_transform(0, (0, 1, 4, 3))) == E_INVALIDARG
    big = dx.Image(1 << 32, 1, RGBA8, 1 << 34, 1 << 34, pix.ctypes.data)
    assert ctx._lib.dxtex_transform_image(ctx._h, big, big, t) == E_INVALIDARG
    # device form: a size mismatch in the second pair, overlapping pixels, no images
    d = ctx.device_alloc(8192, zero=True)
    try:
        a, b = dx.device_image(d, 8, 8, RGBA8), dx.device_image(d + 4096, 8, 8, RGBA8)
        srcs, dsts = (dx.Image * 2)(a, a), (dx.Image * 2)(b, dx.device_image(d + 4096, 8, 7, RGBA8))
        assert ctx._lib.dxtex_transform_images_device(ctx._h, srcs, dsts, 2, t) == E_FAIL
        over = (dx.Image * 1)(dx.device_image(d + 64, 8, 8, RGBA8))
        assert ctx._lib.dxtex_transform_images_device(ctx._h, (dx.Image * 1)(a), over, 1, t) == E_INVALIDARG
        assert ctx._lib.dxtex_transform_images_device(ctx._h, (dx.Image * 1)(a), (dx.Image * 1)(b), 0, t) == E_INVALIDARG
        assert ctx._lib.dxtex_transform_images_device(ctx._h, (dx.Image * 1)(a), (dx.Image * 1)(b), 1, t) == 0
        ctx.synchronize()
    finally:
        ctx.device_free(d)


def test_host_layer():
    exe = os.path.join(ROOT, "directxtex_amd", "lib", "transform_host_test")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} missing: run __graft_entry__.build()")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "transform host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


EXE = os.path.join(ROOT, "directxtex_amd", "lib", "dxtexconv")


def _conv(args):
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _pixels(oracle, path):
    meta, px = oracle.ref_load_dds(np.fromfile(path, np.uint8))
    return meta, px


def test_dxtexconv_bc5_reconstruct_z(tmp_path, oracle):
    """BC5 decodes to R8G8B8A8_UNORM when Z is rebuilt (texconv.cpp:2432-2443), the UNORM form of the op runs, nothing is converted."""
    w, h = 64, 32
    src_rgba = _source(RGBA8, w, h, 51)[0]
    bc = oracle.ref_compress_image(src_rgba, w, h, RGBA8, 83, 0, 0.5)
    src, out = tmp_path / "n.dds", tmp_path / "o.dds"
    oracle.ref_save_dds(bc, w, h, 83).tofile(src)
    txt = _conv(["-reconstructz", "-f", "R8G8B8A8_UNORM", "-m", "1", "-timing", "-overlap", "1", "-o", str(out), str(src)])
    dec = oracle.ref_decompress_image(bc, w, h, 83, RGBA8)
    want = _want(oracle, dec, w, h, RGBA8, w * 4, R.RECONSTRUCT_Z, None)
    meta, px = _pixels(oracle, out)
    assert meta["format"] == RGBA8 and np.array_equal(px, want)
    m = re.search(r"host -> device (\d+) bytes, device -> host (\d+) bytes", txt)
    # one upload of the blocks, one download of the texels (plus the 8-byte count of IsAlphaAllOpaque that picks the DDS alpha mode)
    assert m and int(m.group(1)) == bc.size and want.size <= int(m.group(2)) <= want.size + 8, txt


def test_dxtexconv_bc4_invert_y(tmp_path, oracle):
    """BC4_SNORM decodes to R8G8B8A8_SNORM when Y is inverted (:2398-2408) and is encoded back to BC4_SNORM."""
    w, h = 32, 16
    rng = np.random.default_rng(52)
    bc = oracle.ref_compress_image(rng.integers(0, 256, w * h * 4, dtype=np.uint8), w, h, 31, 81, 0, 0.5)
    src, out = tmp_path / "a.dds", tmp_path / "o.dds"
    oracle.ref_save_dds(bc, w, h, 81).tofile(src)
    _conv(["-inverty", "-m", "1", "-o", str(out), str(src)])
    dec = oracle.ref_decompress_image(bc, w, h, 81, 31)
    inv = _want(oracle, dec, w, h, 31, w * 4, R.INVERT_Y, None)
    want = oracle.ref_compress_image(inv, w, h, 31, 81, 0, 0.5)
    meta, px = _pixels(oracle, out)
    assert meta["format"] == 81 and np.array_equal(px, want)


def test_dxtexconv_hdr_tonemap(tmp_path, oracle):
    w, h = 48, 20
    rng = np.random.default_rng(53)
    rows = (rng.random((h, w, 4), dtype=np.float32) * 12.0).astype(np.float32)
    rows[..., 3] = 1.0
    hr, data = oracle.ref_save_hdr(rows, w, h, RGBA32F, w * 16)
    src, out = tmp_path / "sky.hdr", tmp_path / "o.dds"
    data.tofile(src)
    _conv(["-tonemap", "-f", "R8G8B8A8_UNORM", "-m", "1", "-o", str(out), str(src)])
    _, meta, px = oracle.ref_load_hdr(data)
    loaded = R.load_rows(oracle, px, w, h, RGBA32F, w * 16)
    tm = R.store_rows(oracle, R.tonemap(loaded, R.max_luminance([loaded])), RGBA32F, w * 16)
    want = oracle.ref_convert(tm, w, h, RGBA32F, RGBA8, 0, 0.5)
    meta, got = _pixels(oracle, out)
    assert meta["format"] == RGBA8 and np.array_equal(got, want)


@pytest.mark.parametrize("opts,op,mask", [(["-swizzle", "bgr1"], R.SWIZZLE, "bgr1"), (["-c", "40c080"], R.COLOR_KEY, None)])
def test_dxtexconv_tga(tmp_path, oracle, opts, op, mask):
    w, h = 30, 17
    pix = _source(RGBA8, w, h, 54)[0]
    hr, data = oracle.ref_save_tga(pix, w, h, RGBA8, w * 4)
    src, out = tmp_path / "s.tga", tmp_path / "o.dds"
    data.tofile(src)
    _conv(opts + ["-m", "1", "-o", str(out), str(src)])
    _, meta, loaded = oracle.ref_load_tga(data)
    want = _want(oracle, loaded, w, h, meta["format"], w * 4, op, mask)
    dmeta, got = _pixels(oracle, out)
    assert dmeta["format"] == meta["format"] and np.array_equal(got, want)
    if op == R.COLOR_KEY:
        assert (got.reshape(-1, 4)[:, 3] == 0).any() and (got.reshape(-1, 4)[:, 3] == 255).any()


def test_dxtexconv_identity_swizzle_hands_bc7_through(tmp_path, oracle):
    w, h = 32, 32
    bc = oracle.ref_compress_image(_source(RGBA8, w, h, 55)[0], w, h, RGBA8, 98, 0x100000, 0.5)      # BC7 quick
    src, out = tmp_path / "b.dds", tmp_path / "o.dds"
    oracle.ref_save_dds(bc, w, h, 98).tofile(src)
    _conv(["-swizzle", "rgba", "-f", "BC7_UNORM", "-m", "1", "-o", str(out), str(src)])
    meta, px = _pixels(oracle, out)
    assert meta["format"] == 98 and np.array_equal(px, bc)
