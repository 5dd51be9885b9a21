"""Dithered Convert on the GPU against the reference's own ConvertCustom (DirectXTexConvert.cpp compiled in place into oracle/_ref):
ordered dithering (TEX_FILTER_DITHER) in the Convert kernels, error diffusion (TEX_FILTER_DITHER_DIFFUSION) in its one-workgroup kernel,
for every destination format with a dithered store, the formats without one, the slice phase of volumes, the device entry point and the
C++ host layer. Bar: byte identity, except sRGB conversions from sources off the 8-bit grid (powf on both sides; one step per channel)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ORDERED, DIFFUSION, X2BIAS, SRGB_IN, SRGB_OUT = 0x10000, 0x20000, 0x200, 0x1000000, 0x2000000
RGBA32F, RGBA16F, RGBA8, RGBA8S = 2, 10, 28, 31
# StoreScanlineDither's cases (:4127-4557) other than the two Xbox-only formats
DITHER_FORMATS = [11, 12, 13, 14, 24, 25, 89, 28, 29, 30, 31, 32, 35, 36, 37, 38, 45, 49, 50, 51, 52, 55, 56, 57, 58, 59,
                  61, 62, 63, 64, 65, 85, 86, 87, 91, 88, 93, 115, 191]
SRGB_FORMATS = (29, 91, 93)
BYTE_CHANNELS = (28, 29, 87, 88, 91, 93, 61, 49, 65)        # one byte per channel: a step is one byte
SOURCES = [RGBA32F, RGBA16F, RGBA8, RGBA8S]
PAIRS = [(s, d) for d in DITHER_FORMATS for s in SOURCES if s != d]      # Convert refuses the same format on both sides


def _float_image(rng, w, h, kind, dtype):
    if kind == "noise":
        v = rng.random((h, w, 4), dtype=np.float32) * 1.6 - 0.3
    elif kind == "gradient":
        x = np.linspace(-0.05, 1.05, w, dtype=np.float32)[None, :, None]
        v = np.broadcast_to(x * np.array([1.0, 0.8, 0.6, 0.4], np.float32) + np.linspace(0, 0.2, h, dtype=np.float32)[:, None, None], (h, w, 4)).copy()
    elif kind == "flat":
        v = np.full((h, w, 4), 0.4123, np.float32)
        v[:, :, 3] = 1.0
    elif kind == "ties":
        k = rng.integers(0, 64, (h, w, 4)).astype(np.float32)
        v = (k + 0.5) / np.float32(63.0) * np.where(rng.random((h, w, 4)) < 0.5, np.float32(1.0), np.float32(63.0 / 255.0))
    else:   # nonfinite: out of range, negatives, -0.0, NaN, +-Inf
        v = rng.random((h, w, 4), dtype=np.float32) * 6 - 3
        r = rng.random((h, w, 4))
        v[r < 0.03] = np.nan
        v[(r >= 0.03) & (r < 0.06)] = np.inf
        v[(r >= 0.06) & (r < 0.09)] = -np.inf
        v[(r >= 0.09) & (r < 0.12)] = -0.0
        v[(r >= 0.12) & (r < 0.2)] *= 40000.0
    return v.astype(dtype)


def _image(src, w, h, kind, seed):
    rng = np.random.default_rng(seed)
    if src == RGBA32F:
        return _float_image(rng, w, h, kind, np.float32)
    if src == RGBA16F:
        return _float_image(rng, w, h, kind, np.float32).astype(np.float16)
    if kind == "flat":
        return np.full((h, w, 4), 105, np.uint8)
    if kind == "gradient":
        return np.broadcast_to(np.linspace(0, 255, w).astype(np.uint8)[None, :, None], (h, w, 4)).copy()
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def _tolerant(src, dst, flags):
    return (dst in SRGB_FORMATS or flags & (SRGB_IN | SRGB_OUT)) and src != RGBA8


def _compare(got, ref, src, dst, flags, what):
    if _tolerant(src, dst, flags) and dst in BYTE_CHANNELS:
        d = np.abs(got.astype(np.int16) - ref.astype(np.int16))
        share = float((d != 0).mean())
        print(f"{what}: {share * 100:.3f} % of the bytes one step off (sRGB through powf)")
        assert int(d.max(initial=0)) <= 1, (what, np.nonzero(d > 1)[0][:8])
    else:
        assert np.array_equal(got, ref), (what, np.nonzero(got != ref)[0][:8])


def _filters(dst):
    out = [ORDERED, ORDERED | X2BIAS]
    if dst in BYTE_CHANNELS:
        out += [ORDERED | SRGB_IN, ORDERED | SRGB_OUT]
    return out


@pytest.mark.parametrize("src,dst", PAIRS)
def test_ordered_parity(ctx, oracle, src, dst):
    for flags in _filters(dst):
        for w, h in [(1, 1), (3, 5), (61, 19), (64, 8)]:
            for kind in ("noise", "ties", "nonfinite"):
                img = _image(src, w, h, kind, seed=dst * 7 + w + h)
                got = ctx.convert(img, w, h, src, dst, flags, 0.5)
                ref = oracle.ref_convert(img, w, h, src, dst, flags, 0.5)
                _compare(got, ref, src, dst, flags, (src, dst, hex(flags), w, h, kind))


DIFFUSION_SIZES = [(1, 1), (1, 37), (37, 1), (2, 2), (65, 7), (257, 33)]


@pytest.mark.parametrize("src,dst", PAIRS)
def test_diffusion_parity(ctx, oracle, src, dst):
    for kind in ("noise", "gradient", "flat", "ties", "nonfinite"):
        sizes = DIFFUSION_SIZES + ([(4096, 4), (600, 600)] if kind in ("noise", "flat") and dst in (28, 85, 12, 61, 89) else [])
        for w, h in sizes:
            img = _image(src, w, h, kind, seed=dst * 11 + w * 3 + h)
            got = ctx.convert(img, w, h, src, dst, DIFFUSION, 0.5)
            ref = oracle.ref_convert(img, w, h, src, dst, DIFFUSION, 0.5)
            _compare(got, ref, src, dst, DIFFUSION, (src, dst, w, h, kind))


@pytest.mark.parametrize("dst", [28, 85, 86, 89, 45, 12, 65])
def test_both_bits_run_diffusion(ctx, oracle, dst):
    w, h = 45, 13
    img = _image(RGBA32F, w, h, "noise", seed=dst)
    both = ctx.convert(img, w, h, RGBA32F, dst, ORDERED | DIFFUSION, 0.5)
    assert np.array_equal(both, ctx.convert(img, w, h, RGBA32F, dst, DIFFUSION, 0.5))
    assert np.array_equal(both, oracle.ref_convert(img, w, h, RGBA32F, dst, ORDERED | DIFFUSION, 0.5))


@pytest.mark.parametrize("dst", [RGBA16F, RGBA32F, 26, 67, 68])
def test_fall_through_formats(ctx, oracle, dst):
    """No dithered store: diffusion still adds the zero error row first (-0.0 becomes +0.0), ordered dithering changes nothing."""
    w, h = 38, 6
    src = RGBA16F if dst == RGBA32F else RGBA32F
    img = _image(src, w, h, "noise", seed=dst)
    img.reshape(-1)[::5] = -0.0
    plain = ctx.convert(img, w, h, src, dst, 0, 0.5)
    assert np.array_equal(ctx.convert(img, w, h, src, dst, ORDERED, 0.5), plain)
    assert np.array_equal(plain, oracle.ref_convert(img, w, h, src, dst, ORDERED, 0.5))
    got = ctx.convert(img, w, h, src, dst, DIFFUSION, 0.5)
    assert np.array_equal(got, oracle.ref_convert(img, w, h, src, dst, DIFFUSION, 0.5))
    if dst in (RGBA16F, RGBA32F):
        assert not np.array_equal(got, plain)      # the -0.0 texels are +0.0 now


@pytest.mark.parametrize("dst,bpt", [(28, 4), (85, 2), (12, 8), (61, 1)])
def test_volume_slice_phase(ctx, oracle, dst, bpt):
    """g_Dither's 8-wide rows repeat a 4-wide row, so slice z equals the 2-D result of the slice shifted right by z & 3 columns."""
    w, h = 29, 11
    img = _image(RGBA32F, w, h, "noise", seed=dst)
    for z in (0, 1, 2, 3, 5):
        pad = z & 3
        padded = np.concatenate([np.zeros((h, pad, 4), np.float32), img], axis=1)
        ref = oracle.ref_convert(padded, w + pad, h, RGBA32F, dst, ORDERED, 0.5).reshape(h, (w + pad) * bpt)[:, pad * bpt:].reshape(-1)
        got = ctx.convert(img, w, h, RGBA32F, dst, ORDERED, 0.5, z=z)
        assert np.array_equal(got, ref), (dst, z)


@pytest.mark.parametrize("flags", [ORDERED, DIFFUSION])
def test_device_path_moves_no_bytes(ctx, flags):
    import torch
    w, h, dst = 300, 70, 85
    img = _image(RGBA32F, w, h, "noise", seed=5)
    want = ctx.convert(img, w, h, RGBA32F, dst, flags, 0.5)
    d_src = torch.from_numpy(img.reshape(-1).view(np.uint8).copy()).cuda()
    d_dst = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.transfer_bytes(reset=True)
    ctx.convert_device(d_src.data_ptr(), w, h, RGBA32F, d_dst.data_ptr(), dst, flags, 0.5)
    ctx.synchronize()
    assert ctx.transfer_bytes() == (0, 0)
    assert np.array_equal(d_dst.cpu().numpy(), want)


def test_diffusion_stats(ctx):
    before = ctx.convert_dither_stats()
    w, h = 512, 16
    ctx.convert(_image(RGBA32F, w, h, "noise", seed=9), w, h, RGBA32F, 28, DIFFUSION, 0.5)
    rerun, total = ctx.convert_dither_stats()
    assert total - before[1] == w * h
    assert 0 <= rerun - before[0] <= 64 * w * h
    print(f"merge re-ran {(rerun - before[0]) / (w * h) * 100:.1f} % of the texels")


def test_host_layer():
    exe = os.path.join(ROOT, "directxtex_amd", "lib", "dither_host_test")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} missing: run __graft_entry__.build()")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "dither host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
