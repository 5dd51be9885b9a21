"""dxtexconv --rotate-color end to end against the oracle's Convert / Compress / Decompress around the restated lambdas
(tests/rotate_ref.py): the step's place in the pipeline (after the swizzle, before the tone map), the half-float convert in front of
HDR10to709, what that does to the convert step, the end of a BC hand-through, and the transfer counts."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rotate_ref as R  # noqa: E402
import transform_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "dxtexconv")
RGBA32F, RGBA16F, RGB10A2, RGBA8, BC7 = 2, 10, 24, 28, 98
W, H = R.W, R.H


def _conv(args, ok=True):
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout + r.stderr


def _pixels(oracle, path):
    return oracle.ref_load_dds(np.fromfile(path, np.uint8))


def _rotated(oracle, pix, w, h, fmt, op, nits=200.0):
    """The checker on an image: LoadScanline -> lambda -> StoreScanline, tight pitch."""
    rp = pix.size // h
    return T.store_rows(oracle, R.apply(T.load_rows(oracle, pix, w, h, fmt, rp), op, nits), fmt, rp)


def test_709_to_hdr10_into_r10g10b10a2(tmp_path, oracle):
    """A linear R16G16B16A16_FLOAT texture becomes an HDR10 R10G10B10A2_UNORM one: rotate on the halves, then the convert step. One
    upload of the file's texels, one download of the result."""
    src_px = T.store_rows(oracle, R.quantised(oracle, "linear", RGBA16F), RGBA16F, W * 8)
    src, out = tmp_path / "lin.dds", tmp_path / "hdr10.dds"
    oracle.ref_save_dds(src_px, W, H, RGBA16F).tofile(src)
    txt = _conv(["--rotate-color", "709toHDR10", "--paper-white-nits", "200", "-f", "R10G10B10A2_UNORM", "-m", "1", "-timing", "-overlap", "1", "-o", out, src])
    want = oracle.ref_convert(_rotated(oracle, src_px, W, H, RGBA16F, 1, 200.0), W, H, RGBA16F, RGB10A2, 0, 0.5)
    meta, px = _pixels(oracle, out)
    assert meta["format"] == RGB10A2 and np.array_equal(px, want)
    m = re.search(r"host -> device (\d+) bytes, device -> host (\d+) bytes", txt)
    # (plus the 8-byte count of IsAlphaAllOpaque that picks the DDS alpha mode)
    assert m and int(m.group(1)) == src_px.size and want.size <= int(m.group(2)) <= want.size + 8, txt
    # the default paper-white level is 200 nits; another level gives another file
    _conv(["-rotate-color", "709tohdr10", "-f", "R10G10B10A2_UNORM", "-m", "1", "-y", "-o", out, src])
    assert np.array_equal(_pixels(oracle, out)[1], want)
    _conv(["--rotate-color", "709toHDR10", "--paper-white-nits", "80", "-f", "R10G10B10A2_UNORM", "-m", "1", "-y", "-o", out, src])
    assert np.array_equal(_pixels(oracle, out)[1], oracle.ref_convert(_rotated(oracle, src_px, W, H, RGBA16F, 1, 80.0), W, H, RGBA16F, RGB10A2, 0, 0.5))


def test_hdr10_to_709_from_r10g10b10a2(tmp_path, oracle):
    """texconv converts to R16G16B16A16_FLOAT in front of HDR10to709 (texconv.cpp:2699-2733) and rotates the halves. The target format was
    fixed before that (:2314): with -f R16G16B16A16_FLOAT the rotated halves are the output; without -f the target is still the input's
    R10G10B10A2_UNORM, and the convert step (:3100) goes back to it, as texconv's does."""
    src_px = T.store_rows(oracle, R.quantised(oracle, "hdr10", RGB10A2), RGB10A2, W * 4)
    src, out = tmp_path / "hdr10.dds", tmp_path / "lin.dds"
    oracle.ref_save_dds(src_px, W, H, RGB10A2).tofile(src)
    half = oracle.ref_convert(src_px, W, H, RGB10A2, RGBA16F, 0, 0.5)
    want = _rotated(oracle, half, W, H, RGBA16F, 2, 200.0)
    _conv(["--rotate-color", "HDR10to709", "-f", "R16G16B16A16_FLOAT", "-m", "1", "-o", out, src])
    meta, px = _pixels(oracle, out)
    assert meta["format"] == RGBA16F and np.array_equal(px, want)
    _conv(["--rotate-color", "HDR10to709", "-m", "1", "-y", "-o", out, src])
    meta, px = _pixels(oracle, out)
    assert meta["format"] == RGB10A2 and np.array_equal(px, oracle.ref_convert(want, W, H, RGBA16F, RGB10A2, 0, 0.5))


def test_half_float_input_to_709_fails_as_in_texconv(tmp_path, oracle):
    """P3D65to709 on a texture that already is R16G16B16A16_FLOAT: texconv's unconditional Convert refuses the same format (E_INVALIDARG)."""
    src_px = T.store_rows(oracle, R.quantised(oracle, "linear", RGBA16F), RGBA16F, W * 8)
    src, out = tmp_path / "h.dds", tmp_path / "o.dds"
    oracle.ref_save_dds(src_px, W, H, RGBA16F).tofile(src)
    txt = _conv(["--rotate-color", "P3D65to709", "-m", "1", "-o", out, src], ok=False)
    assert "FAILED [convert] (80070057)" in txt and not out.exists()


def test_rotate_runs_before_the_tone_map(tmp_path, oracle):
    rows = np.ascontiguousarray(R.quantised(oracle, "linear", RGBA32F)[1:])          # without the specials' row: every value is finite
    h = rows.shape[0]
    src_px = T.store_rows(oracle, rows, RGBA32F, W * 16)
    src, out = tmp_path / "s.dds", tmp_path / "o.dds"
    oracle.ref_save_dds(src_px, W, h, RGBA32F).tofile(src)
    _conv(["--rotate-color", "709to2020", "-tonemap", "-m", "1", "-o", out, src])
    rotated = R.apply(rows, 3)
    want = T.store_rows(oracle, T.tonemap(rotated, T.max_luminance([rotated])), RGBA32F, W * 16)
    other = T.store_rows(oracle, R.apply(T.tonemap(rows, T.max_luminance([rows])), 3), RGBA32F, W * 16)
    meta, px = _pixels(oracle, out)
    assert meta["format"] == RGBA32F and np.array_equal(px, want) and not np.array_equal(px, other)


def test_rotate_ends_the_bc7_hand_through(tmp_path, oracle):
    """A BC7 file with -f BC7_UNORM is handed through block for block unless a step touches the texels; the rotation does. BC7 decodes to
    R8G8B8A8_UNORM (the decompress-first condition, texconv.cpp:2394-2448, does not name the rotation), is rotated and encoded again."""
    w, h = 32, 32
    rgba = np.random.default_rng(61).integers(0, 256, w * h * 4, dtype=np.uint8)
    bc = oracle.ref_compress_image(rgba, w, h, RGBA8, BC7, 0x100000, 0.5)          # BC7 quick
    src, out = tmp_path / "b.dds", tmp_path / "o.dds"
    oracle.ref_save_dds(bc, w, h, BC7).tofile(src)
    _conv(["--rotate-color", "709toP3D65", "-f", "BC7_UNORM", "-m", "1", "-o", out, src])
    dec = oracle.ref_decompress_image(bc, w, h, BC7, RGBA8)
    want = oracle.ref_compress_image(_rotated(oracle, dec, w, h, RGBA8, 7), w, h, RGBA8, BC7, 0, 0.5)
    meta, px = _pixels(oracle, out)
    assert meta["format"] == BC7 and np.array_equal(px, want) and not np.array_equal(px, bc)
