"""texconv's HDR colour rotation on the GPU (dxtex_rotate_color / dxtex_rotate_color_device) against the reference's own LoadScanline /
StoreScanline (oracle) around the restated lambdas (tests/rotate_ref.py), byte for byte, on both routes of rotate_color_kernel. The
sources hold the seeded fixture of rotate_ref.py as each format stores it; tests/test_rotate_cpu.py asserts that no pow evaluated on
them lies near an fp32 rounding boundary, so float64 pow is the exactly rounded powf here."""
import os
import re
import sys

import numpy as np
import pytest

import directxtex_amd as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rotate_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

E_FAIL, E_INVALIDARG, E_POINTER = 0x80004005 - (1 << 32), 0x80070057 - (1 << 32), 0x80004003 - (1 << 32)
E_NOT_SUPPORTED = 0x80070032 - (1 << 32)
RGBA32F, RGBA16F, RGB10A2, RGBA8, R11G11B10F, RGB32F, B5G6R5 = 2, 10, 24, 28, 26, 6, 85
BPT = {RGBA32F: 16, RGBA16F: 8, RGB10A2: 4, RGBA8: 4, R11G11B10F: 4, RGB32F: 12, B5G6R5: 2}
QUAD = {RGBA32F, RGBA16F, RGB10A2, RGBA8, R11G11B10F, RGB32F}
CURVE_MARK = {0: "", 1: ",st2084", 2: ",st2084_inverse"}
OPS = [(op, 200.0) for op in range(1, 9)]


def _mark(fmt, src_rp, dst_rp, op):
    """The profile mark launch_rotate_color gives the route it admits: quad for a whole-dword format with 16-byte aligned pitches (device
    allocations are aligned), else texel."""
    route = "quad" if fmt in QUAD and src_rp % 16 == 0 and dst_rp % 16 == 0 else "texel"
    return f"rotate_color<{route}{CURVE_MARK[R.PLAN[op][1]]}>"


def _source(oracle, domain, fmt, w, h, rp):
    """(bytes, rows) of a w x h image of row pitch rp: the fixture's texels as fmt holds them, repeated as far as needed."""
    q = R.quantised(oracle, domain, fmt).reshape(-1, 4)
    idx = np.arange(w * h) % q.shape[0]
    rows = q[idx].reshape(h, w, 4)
    return R.store_rows(oracle, rows, fmt, rp), rows


_cache = {}


def _case(oracle, domain, fmt, w, h, rp):
    """(source bytes, the rows LoadScanline makes of them), computed once and shared."""
    key = (domain, fmt, w, h, rp)
    if key not in _cache:
        pix, rows = _source(oracle, domain, fmt, w, h, rp)
        if w * h <= R.W * R.H:          # the source holds exactly the checked values (larger images repeat these texels)
            assert np.array_equal(R.load_rows(oracle, pix, w, h, fmt, rp).view(np.uint32), rows.view(np.uint32))
        _cache[key] = (pix, rows)
    return _cache[key]


def _assert_same(got, want, out_rows, fmt, w, h, rp, what):
    """Byte for byte, row padding included (never written: zero on both sides). A NaN channel of a float format is a NaN on both sides,
    of any payload."""
    g, t = got.reshape(h, rp), want.reshape(h, rp)
    ok = g == t
    nan = np.isnan(out_rows[..., :3])
    if nan.any() and fmt in (RGBA32F, RGB32F):
        n = BPT[fmt] // 4
        gf, tf = g[:, :w * n * 4].copy().view(np.float32), t[:, :w * n * 4].copy().view(np.float32)
        both = np.repeat(np.isnan(gf) & np.isnan(tf), 4, axis=1)
        ok[:, :w * n * 4] |= both
    elif nan.any() and fmt == RGBA16F:
        gh, th = g[:, :w * 8].copy().view(np.float16), t[:, :w * 8].copy().view(np.float16)
        ok[:, :w * 8] |= np.repeat(np.isnan(gh) & np.isnan(th), 2, axis=1)
    elif nan.any() and fmt == R11G11B10F:
        gu, tu = g[:, :w * 4].copy().view(np.uint32), t[:, :w * 4].copy().view(np.uint32)
        # 11-bit x and y: exponent 0x1F with a mantissa is the NaN; 10-bit z likewise
        fields = ((0, 0x7FF, 0x7C0, 0x3F), (11, 0x7FF, 0x7C0, 0x3F), (22, 0x3FF, 0x3E0, 0x1F))
        same = np.ones(gu.shape, bool)
        for k, (shift, mask, exp, man) in enumerate(fields):
            a, b = (gu >> shift) & mask, (tu >> shift) & mask
            isnan = lambda v: ((v & exp) == exp) & ((v & man) != 0)      # noqa: E731
            same &= (a == b) | (nan[..., k] & isnan(a) & isnan(b))
        ok[:, :w * 4] |= np.repeat(same, 4, axis=1)
    bad = np.argwhere(~ok)
    assert bad.size == 0, (what, fmt, w, h, rp, len(bad), bad[:6], g[~ok][:6], t[~ok][:6])


def _run_device(ctx, images, op, nits):
    """images: [(src bytes, w, h, fmt, src pitch, dst pitch)] -> ([dst bytes], profile) of one dxtex_rotate_color_device call."""
    srcs, dsts, outs = [], [], []
    try:
        for pix, w, h, fmt, srp, drp in images:
            s = ctx.device_alloc(max(pix.nbytes, 16))
            srcs.append(s)
            ctx.upload(s, pix, sync=True)
            dsts.append(ctx.device_alloc(max(drp * h, 16), zero=True))
        ctx.profile_begin()
        ctx.rotate_color_device([dx.device_image(s, w, h, fmt, srp) for s, (_, w, h, fmt, srp, _) in zip(srcs, images)],
                                [dx.device_image(d, w, h, fmt, drp) for d, (_, w, h, fmt, _, drp) in zip(dsts, images)], op, nits)
        prof = ctx.profile_end()
        for d, (_, w, h, fmt, _, drp) in zip(dsts, images):
            out = np.zeros(drp * h, np.uint8)
            ctx.download(out, d, sync=True)
            outs.append(out)
    finally:
        for p in srcs + dsts:
            ctx.device_free(p)
    return outs, prof


def _check(ctx, oracle, fmt, w, h, rp, ops=OPS):
    for op, nits in ops:
        pix, rows = _case(oracle, R.domain_of(op), fmt, w, h, rp)
        (got,), prof = _run_device(ctx, [(pix, w, h, fmt, rp, rp)], op, nits)
        out = R.apply(rows, op, nits)
        want = R.store_rows(oracle, out, fmt, rp)
        _assert_same(got, want, out, fmt, w, h, rp, op)
        names = [k for k in prof if k.startswith("rotate_color")]
        assert names == [_mark(fmt, rp, rp, op)] and prof[names[0]][1] == 1, (op, fmt, rp, prof)


def _tight(fmt, w):
    return w * BPT[fmt]


def _padded(fmt, w):
    """16-byte aligned with room to spare: the quad route's pitch."""
    return (_tight(fmt, w) + 15) // 16 * 16 + 16


def _unaligned(fmt, w):
    """A padded pitch that is no multiple of 16 (a multiple of the texel's own alignment): a quad format falls back to the texel route."""
    return (_tight(fmt, w) + 15) // 16 * 16 + min(BPT[fmt], 8) if BPT[fmt] != 12 else (_tight(fmt, w) + 15) // 16 * 16 + 4


@pytest.mark.parametrize("fmt", R.GPU_FORMATS)
def test_one_texel(ctx, oracle, fmt):
    _check(ctx, oracle, fmt, 1, 1, _tight(fmt, 1))


@pytest.mark.parametrize("fmt", R.GPU_FORMATS)
def test_quads_and_tail_on_a_padded_pitch(ctx, oracle, fmt):
    """67 x 45 on a 16-byte aligned padded pitch: 16 quads and a 3-texel tail per row for the whole-dword formats, texels for B5G6R5."""
    rp = _padded(fmt, R.W)
    assert rp % 16 == 0 and rp > _tight(fmt, R.W)
    _check(ctx, oracle, fmt, R.W, R.H, rp)


@pytest.mark.parametrize("fmt", R.GPU_FORMATS)
def test_unaligned_pitch_takes_the_texel_route(ctx, oracle, fmt):
    rp = _unaligned(fmt, R.W)
    assert rp % 16 != 0
    assert _mark(fmt, rp, rp, 3) == "rotate_color<texel>"
    _check(ctx, oracle, fmt, R.W, R.H, rp)


@pytest.mark.parametrize("fmt", [RGBA32F, RGBA8])
def test_tight_pitch(ctx, oracle, fmt):
    """67 x 45 tight: R32G32B32A32_FLOAT rows are 16-byte aligned as they are (quad route), R8G8B8A8 rows of 268 bytes are not."""
    _check(ctx, oracle, fmt, R.W, R.H, _tight(fmt, R.W), ops=[(1, 200.0), (2, 200.0), (7, 200.0)])


@pytest.mark.parametrize("nits", [80.0, 10000.0])
def test_paper_white_levels(ctx, oracle, nits):
    for fmt in (RGBA16F, RGB10A2):
        _check(ctx, oracle, fmt, R.W, R.H, _padded(fmt, R.W), ops=[(op, nits) for op in R.HDR10_OPS])


@pytest.mark.parametrize("rp,op", [(64, 3), (64, 1), (56, 5)])
def test_taller_than_the_grid(ctx, oracle, rp, op):
    """7 x 70 000 R16G16B16A16_FLOAT, sized as test_transform_gpu.py's: more rows than grid.y's 65 535 and than the about 8192 workgroups
    launched, so every lane strides. Pitch 64 takes the quad route (one quad and a 3-texel tail per row; two rows per lane and step
    without a curve, one with), the tight 56 the texel route."""
    _check(ctx, oracle, RGBA16F, 7, 70000, rp, ops=[(op, 200.0)])


def test_three_images_of_differing_sizes_in_one_device_call(ctx, oracle):
    fmt, op, nits = RGBA16F, 5, 200.0
    sizes = [(9, 5), (4, 2), (2, 1)]
    images, rows = [], []
    for w, h in sizes:
        rp = _padded(fmt, w)
        pix, r = _case(oracle, "linear", fmt, w, h, rp)
        images.append((pix, w, h, fmt, rp, rp))
        rows.append(r)
    outs, prof = _run_device(ctx, images, op, nits)
    for got, (pix, w, h, _, rp, _), r in zip(outs, images, rows):
        out = R.apply(r, op, nits)
        _assert_same(got, R.store_rows(oracle, out, fmt, rp), out, fmt, w, h, rp, (w, h))
    assert prof["rotate_color<quad,st2084>"][1] == 3, prof


def test_host_pointers_on_a_padded_image(ctx, oracle):
    """dxtex_rotate_color: a padded source through the context's staging, a tight destination."""
    fmt, w, h, op = RGBA32F, 13, 7, 2
    srp = _padded(fmt, w)
    pix, rows = _case(oracle, "hdr10", fmt, w, h, srp)
    got = ctx.rotate_color(pix, w, h, fmt, op, 200.0, row_pitch=srp)
    out = R.apply(rows, op, 200.0)
    _assert_same(got, R.store_rows(oracle, out, fmt, w * 16), out, fmt, w, h, w * 16, "host")
    assert not np.array_equal(got, R.store_rows(oracle, rows, fmt, w * 16))


def test_alpha_bits_survive(ctx, oracle):
    """Alpha is moved, never computed: NaN payloads, -0 and infinities in alpha come out as they went in."""
    w, h, fmt = 8, 1, RGBA32F
    rows = np.full((h, w, 4), 0.25, np.float32)
    rows[0, :, 3] = np.array([0x7FC12345, 0xFF800001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000, 0xFFC00000], np.uint32).view(np.float32)
    pix = np.ascontiguousarray(rows).view(np.uint8).reshape(-1)
    for op in (1, 2, 3):
        got = ctx.rotate_color(pix, w, h, fmt, op, 200.0).view(np.uint32).reshape(w, 4)
        assert np.array_equal(got[:, 3], rows[0, :, 3].view(np.uint32)), op


def test_hresults(ctx):
    w, h = 8, 8
    pix = np.zeros(w * h * 16, np.uint8)
    out = np.zeros(w * h * 16, np.uint8)
    call = ctx._lib.dxtex_rotate_color

    def img(fmt=RGBA8, width=w, height=h, buf=out):
        return dx.Image(width, height, fmt, w * 4, w * h * 4, buf.ctypes.data if buf is not None else None)
    for fmt in (71, 98, 27, 1, 103, 104, 113, 118, 0):          # compressed, typeless, planar, palettised, unknown
        assert call(ctx._h, img(fmt, buf=pix), img(fmt), 3, 200.0) == E_NOT_SUPPORTED, fmt
    s = img(buf=pix)
    assert call(ctx._h, s, img(), 3, 200.0) == 0
    for rotate in (0, 9, 0xFFFFFFFF):
        assert call(ctx._h, s, img(), rotate, 200.0) == E_INVALIDARG, rotate
    for nits in (0.0, -1.0, 10000.5, float("nan"), float("inf")):
        assert call(ctx._h, s, img(), 1, nits) == E_INVALIDARG, nits
        assert call(ctx._h, s, img(), 3, nits) == E_INVALIDARG, nits          # texconv checks -nits whatever the operation
    assert call(ctx._h, s, img(), 1, 10000.0) == 0
    big = dx.Image(1 << 32, 1, RGBA8, 1 << 34, 1 << 34, pix.ctypes.data)
    assert call(ctx._h, big, big, 3, 200.0) == E_INVALIDARG
    assert call(ctx._h, s, img(87), 3, 200.0) == E_FAIL                       # format mismatch
    assert call(ctx._h, s, img(height=h - 1), 3, 200.0) == E_FAIL             # size mismatch
    assert call(ctx._h, s, img(buf=None), 3, 200.0) == E_POINTER
    assert call(None, s, img(), 3, 200.0) == E_POINTER
    dev = ctx._lib.dxtex_rotate_color_device
    d = ctx.device_alloc(8192, zero=True)
    try:
        a, b = dx.device_image(d, 8, 8, RGBA8), dx.device_image(d + 4096, 8, 8, RGBA8)
        srcs, dsts = (dx.Image * 2)(a, a), (dx.Image * 2)(b, dx.device_image(d + 4096, 8, 7, RGBA8))
        assert dev(ctx._h, srcs, dsts, 2, 3, 200.0) == E_FAIL
        over = (dx.Image * 1)(dx.device_image(d + 64, 8, 8, RGBA8))
        assert dev(ctx._h, (dx.Image * 1)(a), over, 1, 3, 200.0) == E_INVALIDARG      # overlapping pixels
        assert dev(ctx._h, (dx.Image * 1)(a), (dx.Image * 1)(b), 0, 3, 200.0) == E_INVALIDARG
        assert dev(ctx._h, (dx.Image * 1)(a), (dx.Image * 1)(b), 1, 3, 200.0) == 0
        ctx.synchronize()
    finally:
        ctx.device_free(d)


def test_python_errors_carry_the_hresult(ctx):
    with pytest.raises(dx.DxtexError) as e:
        ctx.rotate_color(np.zeros(64, np.uint8), 4, 4, RGBA8, 9)
    assert re.search(r"rotate_color", str(e.value))
