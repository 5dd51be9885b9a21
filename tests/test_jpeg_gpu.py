"""JPEG samples on the GPU (dxtex_jpeg_decode and its _device form: jpeg_idct and jpeg_colour of csrc/jpeg.hip) against tests/jpeg_ref.py,
the numpy restatement of libjpeg's pixel stage, and against the files Pillow wrote and decoded (tests/golden/jpeg): pixels byte for byte,
the bytes around them untouched, both routes of jpeg_colour asserted by profile mark, nonsense coefficients as the host functions of
csrc/dxtex_jpeg.h give them. Uses numpy, the restatement and the committed fixtures only."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import directxtex_amd as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALIDARG, E_POINTER, E_NOT_SUPPORTED = 0x80070057 - (1 << 32), 0x80004003 - (1 << 32), 0x80070032 - (1 << 32)
FILL = 0xA5
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
CHECK = os.path.join(ROOT, "directxtex_amd", "lib", "jpeg_check")
SIZES = ((1, 1), (2, 2), (3, 5), (4, 1), (5, 2), (6, 3), (7, 9), (16, 16), (17, 33), (33, 18), (40, 24), (65, 35))
SAMPLINGS = {"grey": None, "444": (1, 1), "422": (2, 1), "420": (2, 2)}
MAX_W, MAX_H = 72, 48


def frame_of(info):
    """the dx.JpegFrame of a file the restatement decoded"""
    c0 = info["comps"][0]
    f = dx.jpeg_frame(info["width"], info["height"], info["colour"], (c0["h"], c0["v"]), [q if q is not None else np.zeros(64, np.uint16) for q in info["quant"]],
                      [c["tq"] for c in info["comps"]] + [0, 0])
    for k, c in enumerate(info["comps"]):
        assert (f.component[k].blocksPerRow, f.component[k].blockRows) == (c["bw"], c["bh"])
    return f


def image_format(colour):
    return R.R8 if colour == R.GREY else R.RGBA8


def _marks(prof, prefix="jpeg_"):
    return {k: v[1] for k, v in prof.items() if k.startswith(prefix)}


class Arena:
    """Two device allocations reused by every case of a test: the coefficients' and the image's."""
    def __init__(self, ctx):
        self.ctx = ctx
        self.s = ctx.device_alloc(MAX_W * MAX_H * 3 * 2 + 256)
        self.d = ctx.device_alloc((MAX_W * 4 + 32) * MAX_H + 256)

    def close(self):
        self.ctx.device_free(self.s)
        self.ctx.device_free(self.d)


@pytest.fixture
def arena(ctx):
    a = Arena(ctx)
    yield a
    a.close()


def _device_case(ctx, arena, frame, coef, want, pad, base, seen, where):
    """coefficients at arena.s + base -> an image of pitch row + pad: pixels, the bytes around them, the coefficients untouched, the marks"""
    w, h = frame.width, frame.height
    texel = 1 if frame.colour == R.GREY else 4
    pitch = w * texel + pad
    image_bytes = pitch * h
    coef = np.ascontiguousarray(coef, np.int16)
    ctx.upload(arena.s, np.full(coef.nbytes + 64, FILL, np.uint8), sync=True)
    ctx.upload(arena.s + base, coef.view(np.uint8), sync=True)
    ctx.upload(arena.d, np.full(image_bytes + 32, FILL, np.uint8), sync=True)
    ctx.profile_begin()
    ctx.jpeg_decode_device(arena.s + base, coef.nbytes, frame, dx.device_image(arena.d, w, h, image_format(frame.colour), pitch))
    prof = ctx.profile_end()
    got = np.zeros(image_bytes + 32, np.uint8)
    ctx.download(got, arena.d, sync=True)
    m = got[:image_bytes].reshape(h, pitch)
    assert np.array_equal(m[:, :w * texel], want.reshape(h, w * texel)), where
    assert (m[:, w * texel:] == FILL).all() and (got[image_bytes:] == FILL).all(), ("bytes outside the rows were written", where)
    back = np.zeros(coef.nbytes + 64, np.uint8)
    ctx.download(back, arena.s, sync=True)
    assert np.array_equal(back[base:base + coef.nbytes], coef.view(np.uint8)) and (back[:base] == FILL).all() and (back[base + coef.nbytes:] == FILL).all(), ("the coefficients were written", where)
    marks = {"jpeg_idct" if (arena.s + base) % 16 == 0 else "jpeg_idct<unaligned>": 1}
    if frame.colour != R.GREY:
        wide = w % 4 == 0 and arena.d % 16 == 0 and pitch % 16 == 0
        marks["jpeg_colour<wide>" if wide else "jpeg_colour<narrow>"] = 1
    assert _marks(prof) == marks, (prof, where)
    seen.update(marks)


_files = {}


def _own_file(kind, w, h):
    """a seeded random image through the restatement's writer and back through its parser: (frame, coefficients, the restatement's pixels);
    computed once"""
    key = (kind, w, h)
    if key not in _files:
        rng = np.random.default_rng(len(kind) * 7919 + w * 31 + h)
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        sampling = SAMPLINGS[kind]
        data = R.encode(px[..., 0], restart=2) if sampling is None else R.encode(px, sampling, quality_scale=0.3, restart=(w + h) % 3, jfif=w % 2 == 0, adobe=None if w % 2 == 0 else h % 2)
        info = R.decode(data)
        _files[key] = (frame_of(info), R.coefficients(info), R.pixels(info))
    return _files[key]


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
def golden_cases():
    return sorted(n[:-4] for n in os.listdir(GOLDEN) if n.endswith(".bin"))


def test_golden_files_decode_to_pillows_texels(ctx, arena):
    """the restatement parses the file, the device does the rest: Pillow's decode byte for byte, through the device and the host-pointer form;
    the host form moves the coefficients up and the image's texels down"""
    names = golden_cases()
    assert {"grey", "c444", "c422", "c420", "c420_wide", "c420_progressive", "c420_optimize", "c420_restart"} <= set(names)
    seen = set()
    for name in names:
        info = R.decode(open(os.path.join(GOLDEN, name + ".jpg"), "rb").read())
        want = np.fromfile(os.path.join(GOLDEN, name + ".bin"), np.uint8)
        frame, coef = frame_of(info), R.coefficients(info)
        texel = 1 if info["colour"] == R.GREY else 4
        assert want.size == info["width"] * info["height"] * texel and dx.jpeg_coefficient_count(frame) == coef.size
        _device_case(ctx, arena, frame, coef, want, 0, 0, seen, name)
        ctx.transfer_bytes(reset=True)
        got = ctx.jpeg_decode(coef, frame, image_format(info["colour"]))
        assert np.array_equal(got, want), name
        assert ctx.transfer_bytes() == (coef.nbytes, want.size), name
    assert {"jpeg_idct", "jpeg_colour<wide>", "jpeg_colour<narrow>"} <= seen          # c420_wide is 40 texels across


@pytest.mark.parametrize("kind", list(SAMPLINGS))
def test_random_images_match_the_restatement_at_every_size(ctx, arena, kind):
    """files of the restatement's own writer (YCbCr and RGB-coded, with restart intervals) at sizes around the dw <= 2 switch, the first
    and last column, one and several MCU rows and no multiple of the MCU; each on a tight and on a padded pitch, from a coefficient
    base on 16 bytes and from one 2 or 6 bytes off it"""
    seen = set()
    for n, (w, h) in enumerate(SIZES):
        frame, coef, want = _own_file(kind, w, h)
        for pad, base in ((0, 0), ((16, 3, 4)[n % 3], (0, 2, 6)[n % 3])):
            _device_case(ctx, arena, frame, coef, want, pad, base, seen, (kind, w, h, pad, base))
    assert {"jpeg_idct", "jpeg_idct<unaligned>"} <= seen
    if kind != "grey":
        assert {"jpeg_colour<wide>", "jpeg_colour<narrow>"} <= seen


@pytest.mark.parametrize("kind", ("444", "422", "420"))
def test_both_routes_of_jpeg_colour_run(ctx, arena, kind):
    """an aligned destination takes the wide route; a pitch that is no multiple of 16, a width that is no multiple of 4 and a base off 16
    bytes each take the narrow one; the pixels are the same"""
    frame, coef, want = _own_file(kind, 40, 24)
    for pad, wide in ((0, True), (16, True), (4, False), (3, False)):
        seen = set()
        _device_case(ctx, arena, frame, coef, want, pad, 0, seen, (kind, pad))
        assert ("jpeg_colour<wide>" in seen) == wide and ("jpeg_colour<narrow>" in seen) != wide, (kind, pad, seen)
    frame, coef, want = _own_file(kind, 33, 18)
    seen = set()
    _device_case(ctx, arena, frame, coef, want, 12, 0, seen, (kind, "a width of 33"))          # 33 * 4 + 12 = 144: the pitch alone would do
    assert "jpeg_colour<narrow>" in seen and "jpeg_colour<wide>" not in seen
    # the image's base 4 bytes in
    frame, coef, want = _own_file(kind, 40, 24)
    w, h = 40, 24
    ctx.upload(arena.s, coef.view(np.uint8), sync=True)
    ctx.upload(arena.d, np.full(w * h * 4 + 64, FILL, np.uint8), sync=True)
    ctx.profile_begin()
    ctx.jpeg_decode_device(arena.s, coef.nbytes, frame, dx.device_image(arena.d + 4, w, h, R.RGBA8_SRGB, w * 4))
    assert _marks(ctx.profile_end()) == {"jpeg_idct": 1, "jpeg_colour<narrow>": 1}
    got = np.zeros(w * h * 4 + 64, np.uint8)
    ctx.download(got, arena.d, sync=True)
    assert np.array_equal(got[4:4 + w * h * 4], want.reshape(-1)) and (got[:4] == FILL).all() and (got[4 + w * h * 4:] == FILL).all()


# ---- nonsense coefficients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SAMPLINGS))
def test_any_int16_times_any_uint16_gives_the_host_functions_bytes(ctx, arena, tmp_path, kind):
    """random int16 coefficients with random 16-bit quantiser tables, far outside what an encoder writes: 32-bit wraparound in both passes and
    the wrap of the range limit. The device gives what csrc/dxtex_jpeg.h gives on the host (jpeg_check) and what the restatement gives."""
    rng = np.random.default_rng(77 + len(kind))
    sampling = SAMPLINGS[kind]
    seen = set()
    for w, h in ((7, 9), (40, 24), (65, 35)):
        for spread in (2048, 32768):
            colour = R.GREY if sampling is None else (R.YCBCR if spread == 2048 else R.RGB)
            quant = rng.integers(0, 65536 if spread == 32768 else 256, (4, 64)).astype(np.uint16)
            frame = dx.jpeg_frame(w, h, colour, sampling or (1, 1), quant, (0, 1, 2))
            coef = rng.integers(-spread, spread, dx.jpeg_coefficient_count(frame)).astype(np.int16)
            comps, at = [], 0
            for k in range(frame.components):
                c = frame.component[k]
                n = c.blocksPerRow * c.blockRows * 64
                comps.append(dict(h=c.h, v=c.v, tq=c.quant, bw=c.blocksPerRow, bh=c.blockRows, dw=R.ceil_div(w * c.h, frame.component[0].h),
                                  dh=R.ceil_div(h * c.v, frame.component[0].v), coef=coef[at:at + n].reshape(c.blockRows, c.blocksPerRow, 64)))
                at += n
            want = R.pixels_from(w, h, colour, comps, quant)
            quant.astype("<u2").tofile(tmp_path / "q")
            coef.astype("<i2").tofile(tmp_path / "c")
            hmax, vmax = sampling or (1, 1)
            r = subprocess.run([CHECK, "pixels", str(w), str(h), str(colour), str(hmax), str(vmax), str(tmp_path / "q"), str(tmp_path / "c"), str(tmp_path / "o")], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert np.array_equal(np.fromfile(tmp_path / "o", np.uint8), want.reshape(-1)), (kind, w, h, spread)
            _device_case(ctx, arena, frame, coef, want, 0, 0, seen, (kind, w, h, spread))


# ---- host form --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SAMPLINGS))
def test_host_form_gives_the_device_forms_bytes_through_any_pitch(ctx, kind):
    for (w, h), pad in zip(((5, 2), (17, 33), (40, 24), (65, 35)), (0, 3, 16, 4)):
        frame, coef, want = _own_file(kind, w, h)          # what the device form was held to above
        texel = 1 if kind == "grey" else 4
        pitch = w * texel + pad
        out = np.full(pitch * h + 32, FILL, np.uint8)
        ctx.transfer_bytes(reset=True)
        ctx.profile_begin()
        # surplus coefficients behind the frame's are ignored and not moved
        got = ctx.jpeg_decode(np.concatenate([coef, np.full(9, 0x1111, np.int16)]), frame, image_format(frame.colour), row_pitch=pitch, out=out)
        prof = ctx.profile_end()
        m = got[:pitch * h].reshape(h, pitch)
        assert np.array_equal(m[:, :w * texel], want.reshape(h, w * texel)), (kind, w, h)
        assert (m[:, w * texel:] == FILL).all() and (got[pitch * h:] == FILL).all(), ("bytes outside the rows were written", kind, w, h)
        assert ctx.transfer_bytes() == (coef.nbytes, w * h * texel), (kind, w, h)
        marks = _marks(prof)
        assert marks.pop("jpeg_idct") == 1 and marks == ({} if kind == "grey" else {"jpeg_colour<wide>" if w % 4 == 0 else "jpeg_colour<narrow>": 1}), prof


# ---- HRESULTs -------------------------------------------------------------------------------------------------------------------------------
def test_hresults_come_in_the_stated_order(ctx):
    """E_POINTER, then E_INVALIDARG for the frame, then NOT_SUPPORTED for sampling and format, then E_INVALIDARG for the sizes: each call
    carries every later error as well. None reaches a kernel."""
    lib, h = ctx._lib, ctx._h
    dev = ctx.device_alloc(1 << 16)
    try:
        def image(w, hgt, fmt, pitch, ptr=dev + (1 << 15)):
            return dx.device_image(ptr, w, hgt, fmt, pitch, pitch * max(hgt, 1))

        def decode(coef, size, frame, img, host=False):
            fn = lib.dxtex_jpeg_decode if host else lib.dxtex_jpeg_decode_device
            return fn(h, coef, size, None if frame is None else ctypes.byref(frame), None if img is None else ctypes.byref(img))

        def frame(w=16, hgt=16, colour=R.YCBCR, sampling=(2, 2), **edits):
            f = dx.jpeg_frame(w, hgt, colour, sampling, np.ones((4, 64), np.uint16))
            for key, value in edits.items():
                target, name = (f, key) if "_" not in key else (f.component[int(key.split("_")[1])], key.split("_")[0])
                setattr(target, name, value)
            return f

        good, need = frame(), 6 * 64 * 2
        ctx.profile_begin()
        # E_POINTER beats a bad frame, a mismatched format and a short buffer
        assert decode(None, 0, frame(colour=7), image(16, 16, R.R8, 1)) == E_POINTER and decode(dev, 0, None, image(16, 16, R.R8, 1)) == E_POINTER
        assert decode(dev, 0, frame(colour=7), None) == E_POINTER and decode(dev, 0, frame(colour=7), image(16, 16, R.R8, 1, ptr=None)) == E_POINTER
        # E_INVALIDARG for the frame beats sampling and format: an unknown colour, a component count that does not match it, a quantiser index
        # above 3, sizes of 0 or above 65535, an image of another size, an odd address, block counts or offsets that are not the frame's
        bad_sampling = dict(h_0=1, v_0=2)
        assert decode(dev, 1, frame(colour=3, **bad_sampling), image(16, 16, R.R8, 1)) == E_INVALIDARG
        assert decode(dev, 1, frame(components=1, **bad_sampling), image(16, 16, R.R8, 1)) == E_INVALIDARG
        assert decode(dev, 1, frame(colour=R.GREY, components=3), image(16, 16, R.R8, 1)) == E_INVALIDARG
        assert decode(dev, 1, frame(quant_2=4, **bad_sampling), image(16, 16, R.R8, 1)) == E_INVALIDARG
        for w, hgt in ((0, 16), (16, 0), (65536, 16), (16, 65536)):
            assert decode(dev, 1, frame(width=w, height=hgt), image(w, hgt, R.R8, 1)) == E_INVALIDARG, (w, hgt)
        assert decode(dev, 1, good, image(15, 16, R.R8, 1)) == E_INVALIDARG and decode(dev, 1, good, image(16, 17, R.R8, 1)) == E_INVALIDARG
        assert decode(dev + 1, 1, frame(**bad_sampling), image(16, 16, R.R8, 1)) == E_INVALIDARG
        # NOT_SUPPORTED beats wrong block counts, a short buffer and a short pitch: sampling outside the table, a format that does not pair
        for edits in (dict(h_0=1, v_0=2), dict(h_0=4, v_0=1), dict(h_0=2, v_0=4), dict(h_1=2), dict(v_2=2), dict(h_0=2, v_0=2, h_1=2, v_1=2, h_2=2, v_2=2)):
            assert decode(dev, 1, frame(**edits), image(16, 16, R.RGBA8, 1)) == E_NOT_SUPPORTED, edits
        assert decode(dev, 1, frame(colour=R.GREY, sampling=(1, 1), h_0=2), image(16, 16, R.R8, 1)) == E_NOT_SUPPORTED
        for colour, fmt in ((R.YCBCR, R.R8), (R.RGB, R.R8), (R.GREY, R.RGBA8), (R.GREY, R.RGBA8_SRGB), (R.YCBCR, 87), (R.YCBCR, 2), (R.GREY, 65)):
            assert decode(dev, 1, frame(colour=colour), image(16, 16, fmt, 1)) == E_NOT_SUPPORTED, (colour, fmt)
        # E_INVALIDARG: block counts or offsets that are not the frame's, fewer bytes than the coefficients, a pitch below the row, overlap
        for edits in (dict(blocksPerRow_0=3), dict(blockRows_1=2), dict(offset_1=0), dict(offset_2=64 * 6)):
            assert decode(dev, need, frame(**edits), image(16, 16, R.RGBA8, 64)) == E_INVALIDARG, edits
        assert decode(dev, need - 1, good, image(16, 16, R.RGBA8, 64)) == E_INVALIDARG and decode(dev, need, good, image(16, 16, R.RGBA8, 63)) == E_INVALIDARG
        assert decode(dev, 127, frame(8, 8, R.GREY), image(8, 8, R.R8, 8)) == E_INVALIDARG
        assert decode(dev + (1 << 15) + 16 * 64 - 2, need, good, image(16, 16, R.RGBA8, 64)) == E_INVALIDARG          # the coefficients start inside the image's last row
        # the host form checks the same things in the same order
        buf, px = np.zeros(need // 2, np.int16), np.zeros(16 * 64, np.uint8)
        himg = dx.Image(16, 16, R.RGBA8, 64, 64 * 16, px.ctypes.data)
        assert decode(buf.ctypes.data, need - 1, frame(colour=3), himg, host=True) == E_INVALIDARG and decode(buf.ctypes.data, need - 1, frame(h_0=1, v_0=2), himg, host=True) == E_NOT_SUPPORTED
        assert decode(buf.ctypes.data, need - 1, good, himg, host=True) == E_INVALIDARG and decode(None, need, good, himg, host=True) == E_POINTER
        assert _marks(ctx.profile_end()) == {}          # no refusal reached a kernel
        # and with everything in order: more bytes than the coefficients is fine, either 8-bit RGBA format pairs with colour
        assert decode(dev, need + 64, good, image(16, 16, R.RGBA8, 64)) == 0 and decode(dev, need, good, image(16, 16, R.RGBA8_SRGB, 80)) == 0
        assert decode(dev, 128, frame(8, 8, R.GREY), image(8, 8, R.R8, 8)) == 0
        assert decode(buf.ctypes.data, need, good, himg, host=True) == 0
        ctx.synchronize()
    finally:
        ctx.device_free(dev)
