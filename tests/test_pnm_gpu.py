"""Portable pixmap texels on the GPU (dxtex_pnm_unpack / dxtex_pnm_pack and their _device forms) against tests/pnm_ref.py, the restatement
of Texconv/PortablePixMap.cpp, and for the writer's half-to-float and BGRA-to-RGBA step against the live oracle's Convert: pixels and file
rows byte for byte, the bytes around them untouched, on both routes of each kernel, asserted by profile mark."""
import ctypes
import os
import sys

import numpy as np
import pytest

import directxtex_amd as dx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnm_ref as R  # noqa: E402
from test_pnm_cpu import SPECIAL16, SPECIAL32, samples  # noqa: E402

pytestmark = pytest.mark.gpu

E_INVALIDARG, E_POINTER, E_NOT_SUPPORTED = 0x80070057 - (1 << 32), 0x80004003 - (1 << 32), 0x80070032 - (1 << 32)
FILL = 0xA5
KINDS = {"P6": dx.PNM_P6, "PF": dx.PNM_PF, "Pf": dx.PNM_Pf, "PH": dx.PNM_PH, "Ph": dx.PNM_Ph}
# where a group of four, a wave and a workgroup each have a tail, and where 3- and 6-byte rows fall on and off dword alignment
WIDTHS, HEIGHTS = (1, 3, 4, 5, 63, 64, 65, 257), (1, 2, 5)
PITCH_PADS = (0, 4, 3)
MAXVALS = (255, 254, 100, 16, 2, 1)
# csrc/pnm.hip's span_align: the alignment the wide route asks of the stream's base / of the image's base and pitch, by kind
STREAM_ALIGN = {dx.PNM_P6: 4, dx.PNM_PF: 16, dx.PNM_Pf: 16, dx.PNM_PH: 8, dx.PNM_Ph: 8}
IMAGE_ALIGN = {dx.PNM_P6: 16, dx.PNM_PF: 16, dx.PNM_Pf: 16, dx.PNM_PH: 16, dx.PNM_Ph: 8}


def header_length(kind, w, h):
    """the length of the file's real header: where the samples of such a file start"""
    return len(b"P6\n%d %d\n255\n" % (w, h)) if kind == dx.PNM_P6 else len(b"PF\n%d %d\n-1.000000\n" % (w, h))


def _marks(prof, prefix):
    return {k: v[1] for k, v in prof.items() if k.startswith(prefix)}


class Arena:
    """Two device allocations reused by every case of a test: the stream's and the image's."""
    def __init__(self, ctx, stream_bytes, image_bytes):
        self.ctx = ctx
        self.s = ctx.device_alloc(stream_bytes + 256)
        self.d = ctx.device_alloc(image_bytes + 256)

    def close(self):
        self.ctx.device_free(self.s)
        self.ctx.device_free(self.d)


@pytest.fixture
def arena(ctx):
    a = Arena(ctx, max(WIDTHS) * max(HEIGHTS) * 16, (max(WIDTHS) * 16 + 32) * max(HEIGHTS))
    yield a
    a.close()


_cases = {}


def _case(kind, big, w, h, maxval):
    """(samples, the restatement's tight pixels (h, w * D)); computed once per case"""
    key = (kind, big, w, h, maxval)
    if key not in _cases:
        data = samples(kind, w, h, np.random.default_rng(kind * 7919 + w * 31 + h + int(big)), big)
        if kind == dx.PNM_P6 and w * h >= 2:          # whatever the generator drew, a sample above every maxval of MAXVALS but 255 is there
            data = bytes([255, 254, 101, 17, 3, 2]) + data[6:]
        _cases[key] = (np.frombuffer(data, np.uint8), R.unpack(data, kind, w, h, maxval, big).reshape(h, w * R.IMAGE_BYTES[kind]))
    return _cases[key]


def _unpack_case(ctx, arena, kind, big, w, h, maxval, base, pad, seen):
    D = R.IMAGE_BYTES[kind]
    stream, want = _case(kind, big, w, h, maxval)
    pitch = w * D + pad
    image_bytes = pitch * h
    ctx.upload(arena.s + base, stream, sync=True)
    ctx.upload(arena.d, np.full(image_bytes + 32, FILL, np.uint8), sync=True)
    ctx.profile_begin()
    ctx.pnm_unpack_device(arena.s + base, stream.nbytes, kind, dx.device_image(arena.d, w, h, R.KIND_FORMAT[kind], pitch), maxval, dx.PNM_BIG_ENDIAN if big else 0)
    prof = ctx.profile_end()
    got = np.zeros(image_bytes + 32, np.uint8)
    ctx.download(got, arena.d, sync=True)
    where = (kind, big, w, h, maxval, base, pad)
    m = got[:image_bytes].reshape(h, pitch)
    assert np.array_equal(m[:, :w * D], want), where
    assert (m[:, w * D:] == FILL).all() and (got[image_bytes:] == FILL).all(), ("bytes outside the rows were written", where)
    wide = w % 4 == 0 and (arena.s + base) % STREAM_ALIGN[kind] == 0 and arena.d % IMAGE_ALIGN[kind] == 0 and pitch % IMAGE_ALIGN[kind] == 0
    mark = "pnm_unpack<wide>" if wide else "pnm_unpack<narrow>"
    assert _marks(prof, "pnm_") == {mark: 1}, (prof, where)
    seen.add(mark)


@pytest.mark.parametrize("big", (False, True))
@pytest.mark.parametrize("kind", list(KINDS))
def test_unpack_matches_the_restatement(ctx, arena, kind, big):
    """Every size, stream base and destination pitch: pixels, the bytes around them and the route's profile mark. The float kinds' samples
    hold +-0, denormals, +-Inf and quiet and signalling NaNs with payloads. PNM_P6 (which has no byte order: its second run is the same
    sweep with the list of maxvals walked from the other end) takes its maxval from MAXVALS in turn."""
    kind = KINDS[kind]
    seen, n = set(), 0
    for w in WIDTHS:
        for h in HEIGHTS:
            for base in (0, 1, 2, header_length(kind, w, h)):
                for pad in PITCH_PADS:
                    maxval = (MAXVALS[::-1] if big else MAXVALS)[n % len(MAXVALS)] if kind == dx.PNM_P6 else 255
                    _unpack_case(ctx, arena, kind, big and kind != dx.PNM_P6, w, h, maxval, base, pad, seen)
                    n += 1
    assert seen == {"pnm_unpack<wide>", "pnm_unpack<narrow>"}          # both routes have run


def test_float_fixtures_hold_the_special_patterns():
    """what the sweep above feeds the float kinds: every special pattern is among the samples and comes out of the restatement unchanged"""
    for kind, special in ((dx.PNM_PF, SPECIAL32), (dx.PNM_Pf, SPECIAL32), (dx.PNM_PH, SPECIAL16), (dx.PNM_Ph, SPECIAL16)):
        for big in (False, True):
            stream, want = _case(kind, big, 257, 5, 255)
            e = stream.view((">" if big else "<") + ("u4" if special is SPECIAL32 else "u2"))
            assert set(special.tolist()) <= set(e.tolist()) and set(special.tolist()) <= set(want.reshape(-1).view(special.dtype).tolist())


@pytest.mark.parametrize("maxval", MAXVALS)
def test_p6_maxval_spills_like_the_reference(ctx, arena, maxval):
    """random bytes 0..255 under every maxval of the list, on both routes: a sample above maxval spills into the next channel"""
    seen = set()
    for w, h, base in ((64, 5, 0), (257, 2, 0), (64, 2, 1), (4, 1, 0), (5, 5, 0)):
        _unpack_case(ctx, arena, dx.PNM_P6, False, w, h, maxval, base, 0, seen)
        stream, want = _case(dx.PNM_P6, False, w, h, maxval)
        if maxval < 255:
            assert (stream > maxval).any() and (want.reshape(-1).view(np.uint32) >> 24 == 0xFF).all()
    assert seen == {"pnm_unpack<wide>", "pnm_unpack<narrow>"}
    # the identity: maxval 255 leaves the three bytes as they are
    stream, want = _case(dx.PNM_P6, False, 64, 5, 255)
    assert np.array_equal(want.reshape(-1, 4)[:, :3].reshape(-1), stream)


# ---- pack -----------------------------------------------------------------------------------------------------------------------------
# source format -> (kind, bytes of an image texel, the alignment the wide route asks of the image / of the stream)
WRITER = {R.RGBA8: (dx.PNM_P6, 4, 16, 4), R.RGBA8_SRGB: (dx.PNM_P6, 4, 16, 4), R.BGRA8: (dx.PNM_P6, 4, 16, 4), R.BGRA8_SRGB: (dx.PNM_P6, 4, 16, 4),
          R.BGRX8: (dx.PNM_P6, 4, 16, 4), R.BGRX8_SRGB: (dx.PNM_P6, 4, 16, 4), R.RGBA32F: (dx.PNM_PF, 16, 16, 16), R.RGB32F: (dx.PNM_PF, 12, 16, 16),
          R.RGBA16F: (dx.PNM_PF, 8, 16, 16), R.R32F: (dx.PNM_Pf, 4, 16, 16)}
_rows = {}


def _widen(oracle):
    def widen(halves):
        h, w = halves.shape[:2]
        rgba = np.zeros((h, w, 4), np.uint16)
        rgba[..., :3] = halves
        return oracle.ref_convert(rgba, w, h, R.RGBA16F, R.RGB32F).view(np.uint32).reshape(h, w, 3)
    return widen


def _ref_rows(oracle, fmt, w, h):
    """(the image's pixels (h, w * S) as bytes, the writer's samples): the restatement's file behind its header, whose one arithmetic
    step comes from the live oracle (Convert to R32G32B32_FLOAT; to R8G8B8A8_UNORM); computed once per case."""
    key = (fmt, w, h)
    if key not in _rows:
        rng = np.random.default_rng(fmt * 1000 + w * 9 + h)
        kind, S = WRITER[fmt][:2]
        if kind == dx.PNM_P6:
            px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            file = R.save_ppm(px, fmt)
            rgba = px if fmt in (R.RGBA8, R.RGBA8_SRGB) else oracle.ref_convert(px, w, h, fmt, R.RGBA8_SRGB if fmt in (R.BGRA8_SRGB, R.BGRX8_SRGB) else R.RGBA8).reshape(h, w, 4)
            assert file.endswith(np.ascontiguousarray(rgba[..., :3]).tobytes())
        else:
            dt = np.uint16 if fmt == R.RGBA16F else np.uint32
            px = rng.integers(0, np.iinfo(dt).max + 1, (h, w, S // dt().itemsize), dtype=dt)
            special = SPECIAL16 if fmt == R.RGBA16F else SPECIAL32
            px.reshape(-1)[::7] = special[rng.integers(0, len(special), len(px.reshape(-1)[::7]))]
            file = R.save_pfm(px, fmt, _widen(oracle))
        n = w * h * R.FILE_BYTES[kind]
        _rows[key] = (px.view(np.uint8).reshape(h, w * S), np.frombuffer(file[len(file) - n:], np.uint8))
    return _rows[key]


def _pack_case(ctx, arena, fmt, px, want, w, h, pad, base, seen):
    kind, S, image_align, stream_align = WRITER[fmt]
    pitch = w * S + pad
    src = np.full((h, pitch), 0x5A, np.uint8)
    src[:, :w * S] = px
    ctx.upload(arena.d, src.reshape(-1), sync=True)
    ctx.upload(arena.s, np.full(want.size + 64, FILL, np.uint8), sync=True)
    ctx.profile_begin()
    ctx.pnm_pack_device(dx.device_image(arena.d, w, h, fmt, pitch), kind, arena.s + base, want.size)
    prof = ctx.profile_end()
    got = np.zeros(want.size + 64, np.uint8)
    ctx.download(got, arena.s, sync=True)
    where = (fmt, w, h, pad, base)
    assert np.array_equal(got[base:base + want.size], want), where
    assert (got[:base] == FILL).all() and (got[base + want.size:] == FILL).all(), ("bytes outside the samples were written", where)
    wide = w % 4 == 0 and (arena.s + base) % stream_align == 0 and arena.d % image_align == 0 and pitch % image_align == 0
    mark = "pnm_pack<wide>" if wide else "pnm_pack<narrow>"
    assert _marks(prof, "pnm_") == {mark: 1}, (prof, where)
    seen.add(mark)


@pytest.mark.parametrize("fmt", list(WRITER))
def test_pack_matches_the_writer(ctx, oracle, arena, fmt):
    seen = set()
    for w in WIDTHS:
        for h in HEIGHTS:
            px, want = _ref_rows(oracle, fmt, w, h)
            for pad in (0, 16, 4, 3):          # padded source pitches that keep the rows' alignment, and two that do not
                for base in (0, 1, 2, header_length(WRITER[fmt][0], w, h)):
                    _pack_case(ctx, arena, fmt, px, want, w, h, pad, base, seen)
    assert seen == {"pnm_pack<wide>", "pnm_pack<narrow>"}


def test_every_half_is_widened_like_the_oracle(ctx, oracle):
    """256 x 256 holds each of the 65 536 half patterns in every colour channel; the .pfm payload is the oracle's Convert, flipped"""
    halves = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    px = np.stack([halves, halves[::-1], halves.T, np.full((256, 256), 0x3C00, np.uint16)], axis=2)
    want = oracle.ref_convert(px, 256, 256, R.RGBA16F, R.RGB32F).view(np.uint32).reshape(256, 256, 3)[::-1]
    out = np.full(256 * 256 * 12 + 64, FILL, np.uint8)
    ctx.profile_begin()
    got = ctx.pnm_pack(px, 256, 256, R.RGBA16F, dx.PNM_PF, out=out)
    prof = ctx.profile_end()
    assert np.array_equal(got[:256 * 256 * 12].view(np.uint32).reshape(256, 256, 3), want)
    assert (got[256 * 256 * 12:] == FILL).all() and _marks(prof, "pnm_") == {"pnm_pack<wide>": 1}
    # and one column less, on the narrow route
    got = ctx.pnm_pack(np.ascontiguousarray(px[:, :255]), 255, 256, R.RGBA16F, dx.PNM_PF)
    assert np.array_equal(got.view(np.uint32).reshape(256, 255, 3), want[:, :255])


# ---- host forms -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_host_unpack_gives_the_device_forms_bytes_and_moves_the_files_bytes(ctx, kind):
    kind = KINDS[kind]
    D, B = R.IMAGE_BYTES[kind], R.FILE_BYTES[kind]
    for (w, h, big, pad, maxval) in ((4, 2, False, 0, 255), (5, 5, True, 3, 100), (257, 2, True, 4, 16), (64, 5, False, 16, 2)):
        big = big and kind != dx.PNM_P6
        maxval = maxval if kind == dx.PNM_P6 else 255
        stream, want = _case(kind, big, w, h, maxval)          # what the device form was held to above
        pitch = w * D + pad
        out = np.full(pitch * h + 32, FILL, np.uint8)
        ctx.transfer_bytes(reset=True)
        ctx.profile_begin()
        # surplus samples behind the image's are ignored and not moved
        got = ctx.pnm_unpack(np.concatenate([stream, np.full(7, 0x11, np.uint8)]), w, h, kind, R.KIND_FORMAT[kind], maxval, dx.PNM_BIG_ENDIAN if big else 0, row_pitch=pitch, out=out)
        prof = ctx.profile_end()
        up, down = ctx.transfer_bytes()
        m = got[:pitch * h].reshape(h, pitch)
        assert np.array_equal(m[:, :w * D], want), (kind, w, h)
        assert (m[:, w * D:] == FILL).all() and (got[pitch * h:] == FILL).all(), ("bytes outside the rows were written", kind, w, h)
        assert (up, down) == (w * h * B, w * h * D), (kind, w, h, up, down)          # the samples up, the rows' texels down
        assert _marks(prof, "pnm_") == {"pnm_unpack<wide>" if w % 4 == 0 else "pnm_unpack<narrow>": 1}


@pytest.mark.parametrize("fmt", list(WRITER))
def test_host_pack_gives_the_device_forms_bytes(ctx, oracle, fmt):
    kind, S = WRITER[fmt][:2]
    for (w, h) in ((4, 2), (5, 5), (257, 2)):
        px, want = _ref_rows(oracle, fmt, w, h)
        out = np.full(want.size + 16, FILL, np.uint8)
        ctx.transfer_bytes(reset=True)
        got = ctx.pnm_pack(px, w, h, fmt, kind, row_pitch=w * S, out=out)
        assert np.array_equal(got[:want.size], want) and (got[want.size:] == FILL).all(), (fmt, w, h)          # no byte behind the samples is touched
        assert ctx.transfer_bytes() == (w * h * S, want.size)


# ---- HRESULTs -------------------------------------------------------------------------------------------------------------------------
def test_hresults_come_in_the_stated_order(ctx):
    """E_POINTER, then E_INVALIDARG for the arguments, then NOT_SUPPORTED, then E_INVALIDARG for the sizes: each call carries every later
    error as well. None reaches a kernel."""
    lib, h = ctx._lib, ctx._h
    dev = ctx.device_alloc(4096)
    try:
        def image(w, hgt, fmt, pitch, ptr=dev + 2048):
            return dx.device_image(ptr, w, hgt, fmt, pitch, pitch * max(hgt, 1))

        def unpack(stream, size, kind, img, maxval=255, flags=0, host=False):
            fn = lib.dxtex_pnm_unpack if host else lib.dxtex_pnm_unpack_device
            return fn(h, stream, size, kind, maxval, flags, None if img is None else ctypes.byref(img))

        def pack(img, kind, stream, size, host=False):
            fn = lib.dxtex_pnm_pack if host else lib.dxtex_pnm_pack_device
            return fn(h, None if img is None else ctypes.byref(img), kind, stream, size)

        P6, PF, Pf, PH, Ph = dx.PNM_P6, dx.PNM_PF, dx.PNM_Pf, dx.PNM_PH, dx.PNM_Ph
        ctx.profile_begin()
        # E_POINTER beats an unknown kind, a mismatched format and a zero size
        assert unpack(None, 0, 9, image(0, 4, R.R16F, 0)) == E_POINTER
        assert unpack(dev, 0, 9, None) == E_POINTER
        assert unpack(dev, 0, 9, image(0, 4, R.R16F, 0, ptr=None)) == E_POINTER
        assert pack(None, 9, dev, 0) == E_POINTER and pack(image(0, 4, R.R16F, 0), 9, None, 0) == E_POINTER and pack(image(0, 4, R.R16F, 0, ptr=None), 9, dev, 0) == E_POINTER
        # E_INVALIDARG for the arguments beats a mismatched format: an unknown kind, maxval outside 1..255 with P6, unknown flag bits, a zero size
        assert unpack(dev, 64, 5, image(4, 4, R.R16F, 16)) == E_INVALIDARG and pack(image(4, 4, R.R16F, 16), 5, dev, 64) == E_INVALIDARG
        assert unpack(dev, 64, P6, image(4, 4, R.R16F, 16), maxval=0) == E_INVALIDARG and unpack(dev, 64, P6, image(4, 4, R.R16F, 16), maxval=256) == E_INVALIDARG
        assert unpack(dev, 64, PF, image(4, 4, R.R16F, 16), flags=2) == E_INVALIDARG and unpack(dev, 64, PF, image(4, 4, R.R16F, 16), flags=0x80000001) == E_INVALIDARG
        for w, hgt, size in ((0, 4, 64), (4, 0, 64), (4, 4, 0)):
            assert unpack(dev, size, PF, image(w, hgt, R.R16F, 16)) == E_INVALIDARG and pack(image(w, hgt, R.R16F, 16), PF, dev, size) == E_INVALIDARG
        # NOT_SUPPORTED beats a short stream and a short pitch: every pair outside the tables
        for kind, fmt in ((P6, R.RGBA8_SRGB), (P6, R.BGRA8), (P6, R.RGBA32F), (PF, R.RGB32F), (PF, R.RGBA16F), (Pf, R.RGBA32F), (PH, R.RGBA32F), (PH, R.R16F), (Ph, R.RGBA16F), (Ph, 56)):
            assert unpack(dev, 1, kind, image(4, 4, fmt, 1)) == E_NOT_SUPPORTED, (kind, fmt)
        for kind, fmt in ((P6, R.RGBA32F), (P6, 61), (PF, R.RGBA8), (PF, R.R32F), (Pf, R.RGBA32F), (Pf, R.R16F), (PH, R.RGBA16F), (Ph, R.R16F), (PH, R.RGBA32F)):
            assert pack(image(4, 4, fmt, 1), kind, dev, 1) == E_NOT_SUPPORTED, (kind, fmt)
        # E_INVALIDARG: fewer samples than the image, a pitch below the row, overlap
        assert unpack(dev, 47, P6, image(4, 4, R.RGBA8, 16)) == E_INVALIDARG and unpack(dev, 48, P6, image(4, 4, R.RGBA8, 15)) == E_INVALIDARG
        assert pack(image(4, 4, R.RGBA8, 16), P6, dev, 47) == E_INVALIDARG and pack(image(4, 4, R.RGBA8, 15), P6, dev, 48) == E_INVALIDARG
        assert unpack(dev, 191, PF, image(4, 4, R.RGBA32F, 64)) == E_INVALIDARG and pack(image(4, 4, R.RGB32F, 47), PF, dev, 192) == E_INVALIDARG
        assert unpack(dev + 2048 + 60, 48, P6, image(4, 4, R.RGBA8, 16)) == E_INVALIDARG          # the samples start inside the image's last row
        assert pack(image(4, 4, R.RGBA8, 16), P6, dev + 2048 - 4, 48) == E_INVALIDARG              # the last sample is the image's first byte
        # the host forms check the same things in the same order
        buf, px = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
        himg = dx.Image(4, 4, R.RGBA8, 16, 64, px.ctypes.data)
        assert unpack(buf.ctypes.data, 47, 7, himg, host=True) == E_INVALIDARG and unpack(buf.ctypes.data, 47, PF, himg, host=True) == E_NOT_SUPPORTED
        assert unpack(buf.ctypes.data, 47, P6, himg, host=True) == E_INVALIDARG and unpack(None, 48, P6, himg, host=True) == E_POINTER
        assert pack(himg, P6, buf.ctypes.data, 47, host=True) == E_INVALIDARG and pack(himg, PF, buf.ctypes.data, 64, host=True) == E_NOT_SUPPORTED
        assert _marks(ctx.profile_end(), "pnm_") == {}          # no refusal reached a kernel
        # and with everything in order: a stream longer than the image is fine
        assert unpack(dev, 64, P6, image(4, 4, R.RGBA8, 16)) == 0 and pack(image(4, 4, R.RGBA8, 16), P6, dev, 64) == 0
        assert unpack(buf.ctypes.data, 48, P6, himg, host=True) == 0 and pack(himg, P6, buf.ctypes.data, 48, host=True) == 0
        ctx.synchronize()
    finally:
        ctx.device_free(dev)
