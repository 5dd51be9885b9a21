"""ConvertToSinglePlane on the GPU: dxtex_convert_to_single_plane_device and the host-pointer form against the reference's own
ConvertToSinglePlane (called live, tests/plane_ref.py), byte for byte, over the matrix tests/test_single_plane_cpu.py runs on the host
build. Every comparison is of the WHOLE destination buffer, which starts as a seeded random pattern: bytes outside the written elements
(row padding, elements the end guard leaves out) must be unchanged."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _expected(oracle, c, src, start):
    hr, dfmt, pitch, rows = R.convert(oracle, src, c["w"], c["h"], c["fmt"], c["row_pitch"], c["slice_pitch"])
    assert hr == R.S_OK and dfmt == R.planar_to_single(c["fmt"])
    return R.expected(start, rows, R.written_mask(c["w"], c["h"], c["fmt"], c["row_pitch"], c["slice_pitch"], c["dst_pitch"]))


class Arena:
    """One device allocation cut into 256-byte aligned pieces (plus a shift), filled by one upload and read back by one download."""

    def __init__(self, ctx):
        self.ctx, self.parts, self.size = ctx, [], 0

    def add(self, data, shift=0):
        at = self.size + shift
        self.parts.append((at, np.ascontiguousarray(data, np.uint8).reshape(-1)))
        self.size = (at + len(self.parts[-1][1]) + 255) & ~255
        return at

    def upload(self):
        host = np.zeros(max(self.size, 256), np.uint8)
        for at, data in self.parts:
            host[at:at + len(data)] = data
        self.base = self.ctx.device_alloc(host.nbytes)
        assert self.base % 256 == 0
        self.ctx.upload(self.base, host, sync=True)
        return self.base

    def download(self):
        host = np.zeros(max(self.size, 256), np.uint8)
        self.ctx.download(host, self.base, sync=True)
        return host

    def free(self):
        self.ctx.device_free(self.base)


@pytest.fixture(scope="module")
def dx():
    import directxtex_amd
    return directxtex_amd


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_device_matrix_equals_reference(ctx, oracle, dx, fmt):
    """Every case of the format in ONE call (launches of 32 jobs): wide and element routes, padded pitches, truncated slicePitch. The
    matrix is the CPU test's, which asserts that it reaches the wide route with tails, several units and cut groups."""
    cases = R.matrix(fmt)
    arena, want, at = Arena(ctx), [], []
    for i, c in enumerate(cases):
        src = R.source(c["fmt"], c["w"], c["h"], c["row_pitch"], c["slice_pitch"], c["seed"])
        start = np.random.default_rng(c["seed"] + 7).integers(1, 256, (c["h"], c["dst_pitch"]), dtype=np.uint8)
        want.append(_expected(oracle, c, src, start))
        at.append((arena.add(src, c["src_shift"]), arena.add(start, c["dst_shift"])))      # an image off the 16-byte grid never takes the wide route
    base = arena.upload()
    srcs = [dx.device_image(base + s, c["w"], c["h"], fmt, c["row_pitch"], c["slice_pitch"]) for c, (s, _) in zip(cases, at)]
    dsts = [dx.device_image(base + d, c["w"], c["h"], R.planar_to_single(fmt), c["dst_pitch"], c["dst_pitch"] * c["h"]) for c, (_, d) in zip(cases, at)]
    try:
        ctx.convert_to_single_plane_device(srcs, dsts)
        ctx.synchronize()
        back = arena.download()
    finally:
        arena.free()
    for c, (_, d), exp in zip(cases, at, want):
        assert np.array_equal(back[d:d + exp.size].reshape(exp.shape), exp), c
    # nothing but the sources and destinations changed either: the arena's gaps are still zero, the sources as uploaded
    for off, data in arena.parts[::2]:
        assert np.array_equal(back[off:off + len(data)], data)


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_host_pointer_form_equals_reference(ctx, oracle, dx, fmt):
    """The host-pointer form, on padded and pre-filled destinations: only the written elements come back."""
    for c in R.matrix(fmt)[::3]:
        src = R.source(c["fmt"], c["w"], c["h"], c["row_pitch"], c["slice_pitch"], c["seed"])
        start = np.random.default_rng(c["seed"] + 7).integers(1, 256, (c["h"], c["dst_pitch"]), dtype=np.uint8)
        exp = _expected(oracle, c, src, start)
        dst = start.copy()
        s = dx.Image(c["w"], c["h"], fmt, c["row_pitch"], c["slice_pitch"], src.ctypes.data)
        d = dx.Image(c["w"], c["h"], R.planar_to_single(fmt), c["dst_pitch"], dst.nbytes, dst.ctypes.data)
        hr = ctx._lib.dxtex_convert_to_single_plane(ctx._h, ctypes.byref(s), ctypes.byref(d))
        assert hr == 0, (c, ctx._lib.dxtex_ctx_last_error(ctx._h))
        assert np.array_equal(dst, exp), c


@pytest.mark.parametrize("fmt", R.FORMATS)
def test_python_binding_defaults(ctx, oracle, dx, fmt):
    """Context.convert_to_single_plane with ComputePitch's layout -> the reference's tight rows; planar_to_single."""
    w, h = R.shapes(fmt)[2]
    rp, sp = R.natural(fmt, w, h)
    assert dx.planar_to_single(fmt) == R.planar_to_single(fmt)
    src = R.source(fmt, w, h, rp, sp, 77)
    _, _, _, rows = R.convert(oracle, src, w, h, fmt, rp, sp)
    assert np.array_equal(ctx.convert_to_single_plane(src, w, h, fmt), rows.reshape(-1))
    assert [dx.planar_to_single(f) for f in (106, 107, 130, 28, 0)] == [0, 0, 0, 0, 0]


def test_batch_is_one_launch(ctx, oracle, dx):
    """An NV12 8 x 8 array of two items with three mips - six jobs, levels 8 x 8, 4 x 4 and 2 x 2 - as one call: one launch of
    single_plane_kernel, the six results those of the reference's array overload."""
    levels = [(8, 8), (4, 4), (2, 2)]
    images, arena, at = [], Arena(ctx), []
    for item in range(2):
        for (w, h) in levels:
            rp, sp = R.natural(R.NV12, w, h)
            images.append((R.source(R.NV12, w, h, rp, sp, 300 + len(images)), w, h, rp, sp))
    hr, ref = R.convert_array(oracle, images, 8, 8, 2, 3, R.NV12)
    assert hr == R.S_OK and len(ref) == 6
    for (buf, w, h, rp, sp), (dfmt, pitch, rows) in zip(images, ref):
        assert dfmt == R.YUY2
        at.append((arena.add(buf), arena.add(np.zeros(rows.size, np.uint8))))
    base = arena.upload()
    srcs = [dx.device_image(base + s, w, h, R.NV12, rp, sp) for (_, w, h, rp, sp), (s, _) in zip(images, at)]
    dsts = [dx.device_image(base + d, w, h, R.YUY2) for (_, w, h, _, _), (_, d) in zip(images, at)]
    try:
        ctx.profile_begin()
        ctx.convert_to_single_plane_device(srcs, dsts)
        prof = ctx.profile_end()
        back = arena.download()
    finally:
        arena.free()
    assert set(prof) == {"single_plane_kernel"} and prof["single_plane_kernel"][1] == 1, prof
    for (_, d), (_, _, rows) in zip(at, ref):
        assert np.array_equal(back[d:d + rows.size], rows.reshape(-1))


def test_hresults_leave_the_destination_untouched(ctx, dx):
    """Every HRESULT of the table, through both forms; a refused call writes nothing."""
    for (name, sf, sshift, df, dshift, flags, want) in R.HRESULT_TABLE:
        src = np.full(sf[4] + 16, 0x55, np.uint8)
        start = np.random.default_rng(5).integers(1, 256, df[2] * df[3] + 16, dtype=np.uint8)
        arena = Arena(ctx)
        s_at, d_at = arena.add(src, sshift), arena.add(start, dshift)
        base = arena.upload()
        try:
            for form in ("device", "host"):
                if form == "device":
                    sp, dp = base + s_at, base + d_at
                else:
                    # numpy buffers start 16-byte aligned or better; the shift puts the image where the case wants it
                    hs, hd = np.zeros(src.size + 32, np.uint8), np.zeros(start.size + 32, np.uint8)
                    so = (-hs.ctypes.data) % 16 + sshift
                    do = (-hd.ctypes.data) % 16 + dshift
                    hs[so:so + src.size] = src
                    hd[do:do + start.size] = start
                    sp, dp = hs.ctypes.data + so, hd.ctypes.data + do
                sp = None if flags & 1 else sp
                dp = None if flags & 2 else (sp if flags & 4 else dp)
                s = dx.Image(sf[1], sf[2], sf[0], sf[3], sf[4], sp)
                d = dx.Image(df[1], df[2], df[0], df[3], df[3] * df[2], dp)
                if form == "device":
                    hr = ctx._lib.dxtex_convert_to_single_plane_device(ctx._h, ctypes.byref(s), ctypes.byref(d), 1)
                else:
                    hr = ctx._lib.dxtex_convert_to_single_plane(ctx._h, ctypes.byref(s), ctypes.byref(d))
                assert hr == want, f"{name} ({form}): got {hr & 0xFFFFFFFF:08X}, want {want & 0xFFFFFFFF:08X}"
                if want != 0 and form == "host":
                    assert np.array_equal(hd[do:do + start.size], start) and np.array_equal(hs[so:so + src.size], src), name
            ctx.synchronize()
            back = arena.download()
        finally:
            arena.free()
        if want != 0:
            assert np.array_equal(back[d_at:d_at + start.size], start) and np.array_equal(back[s_at:s_at + src.size], src), name
    # the device form's own arguments: no images
    one = dx.Image(4, 2, R.NV12, 4, 12, None)
    assert ctx._lib.dxtex_convert_to_single_plane_device(ctx._h, ctypes.byref(one), ctypes.byref(one), 0) == R.E_INVALIDARG


@pytest.mark.parametrize("fmt,w,h", [(R.NV12, 34, 6), (R.P010, 34, 6), (R.NV11, 36, 5), (R.NV12, 2056, 2)])
def test_truncated_slice_in_an_allocation_of_exactly_that_size(ctx, oracle, dx, fmt, w, h):
    """slicePitch short of the chroma data by 5 samples, and the device allocation holds exactly slicePitch bytes: the result is the
    reference's, with the elements the end guard leaves out still zero."""
    rp = R.natural(fmt, w, h)[0]
    sp = R.data_end(fmt, w, h, rp) - 5 * R.sample_bytes(fmt)
    src = R.source(fmt, w, h, rp, sp, 900 + w)
    hr, dfmt, pitch, rows = R.convert(oracle, src, w, h, fmt, rp, sp)
    assert hr == R.S_OK and not rows.all()              # something was left out
    sptr, dptr = ctx.device_alloc(sp), ctx.device_alloc(rows.size, zero=True)
    try:
        ctx.upload(sptr, src, sync=True)
        ctx.convert_to_single_plane_device([dx.device_image(sptr, w, h, fmt, rp, sp)], [dx.device_image(dptr, w, h, dfmt)])
        got = np.zeros(rows.size, np.uint8)
        ctx.synchronize()
        ctx.download(got, dptr, sync=True)
    finally:
        ctx.device_free(sptr)
        ctx.device_free(dptr)
    assert np.array_equal(got, rows.reshape(-1))
