"""texconv's per-texel transforms without a GPU: the host build of dxtex_transform.h (directxtex_amd/lib/transform_check) against the
numpy restatement (tests/transform_ref.py) bit for bit, texconv's swizzle-mask rules in the host layer and the Python binding, and
dxtexconv's parsing of -swizzle, -c, -tonemap, -inverty, -reconstructz and their long names."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from directxtex_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import transform_ref as R  # noqa: E402
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK = os.path.join(LIB, "transform_check")
EXE = os.path.join(LIB, "dxtexconv")

EDGE_BITS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF812345, 0x7FC0BEEF, 0x00000001,
             0x807FFFFF, 0x00400000, 0x3F800000, 0xBF800000, 0x3F7FFFFF, 0x3F000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3E4CCCCD, 0x40000000]


def _edge_rows():
    """Every pair of the edge values in (r, g), with b and a from the list too: NaN payloads, signed zeros, infinities, denormals."""
    e = np.array(EDGE_BITS, np.uint32)
    n = len(e)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    rows = np.stack([e[i.ravel()], e[j.ravel()], e[(i.ravel() + 3) % n], e[(j.ravel() + 7) % n]], -1)
    return rows.view(np.float32)


def _key_rows(key):
    """Texels at, just inside and just outside the colour key's 0.2 tolerance (51/255 away) on every channel."""
    k = R.color_key_value(key)
    s = np.float32(1.0) / np.float32(255.0)
    base = np.array(list(k) + [np.float32(0.5)], np.float32)
    out = [base]
    for c in range(3):
        ch = (key >> (16 - 8 * c)) & 0xFF
        for d in (-52, -51, -50, 50, 51, 52):
            v = base.copy()
            v[c] = np.float32(ch + d) * s
            out.append(v)
            for step in (np.inf, -np.inf):
                w = v.copy()
                w[c] = np.nextafter(v[c], np.float32(step))
                out.append(w)
            w = v.copy(); w[c] = np.float32(0.2) + k[c]; out.append(w)
            w = v.copy(); w[c] = k[c] - np.float32(0.2); out.append(w)
    return np.stack(out).astype(np.float32)


def _random_rows(seed, n=20000):
    rng = np.random.default_rng(seed)
    a = rng.uniform(-2.0, 3.0, (n, 4)).astype(np.float32)
    a[: n // 4] = rng.uniform(0.0, 1.0, (n // 4, 4)).astype(np.float32)
    raw = rng.integers(0, 2**32, (n // 8, 4), dtype=np.uint64).astype(np.uint32)
    a[n // 2: n // 2 + n // 8] = raw.view(np.float32)             # any bit pattern
    return a


def _apply_host(tmp_path, rows, op, swz=(0, 1, 2, 3), zero=(0, 0, 0, 0), one=(0, 0, 0, 0), key=0, unorm=False, m_bits=0):
    if not os.path.exists(CHECK):
        pytest.fail("directxtex_amd/lib/transform_check is missing: run build()")
    src, dst = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    np.ascontiguousarray(rows, np.float32).tofile(src)
    zm = sum(1 << k for k in range(4) if zero[k])
    om = sum(1 << k for k in range(4) if one[k])
    args = [CHECK, "apply", str(op)] + [str(s) for s in swz] + [str(zm), str(om), f"{key:x}", str(int(unorm)), f"{m_bits:x}", src, dst]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(dst, np.float32).reshape(-1, 4)


def _same_bits(got, want):
    g, w = np.asarray(got, np.float32).view(np.uint32), np.asarray(want, np.float32).view(np.uint32)
    bad = np.nonzero((g != w).any(axis=-1))[0]
    assert bad.size == 0, f"{bad.size} texels differ, first {bad[:4]}: got {g[bad[:4]]}, want {w[bad[:4]]}"


def _inputs(seed):
    return np.concatenate([_edge_rows(), _random_rows(seed)])


@pytest.mark.parametrize("mask", ["bgr1", "rrrg", "w0", "1", "0", "a", "xyzw", "g01", "rgba", "BgRa", "z"])
def test_swizzle_header_equals_restatement(tmp_path, mask):
    swz, zero, one = R.parse_swizzle_mask(mask)
    rows = _inputs(len(mask))
    _same_bits(_apply_host(tmp_path, rows, R.SWIZZLE, swz, zero, one), R.swizzle(rows, swz, zero, one))


@pytest.mark.parametrize("m_bits", [0x00000000, 0x3F800000, 0x40490FDB, 0x7F800000, 0x7FC00000, 0x00000001, 0x5F000000, 0x3DCCCCCD])
def test_tonemap_header_equals_restatement(tmp_path, m_bits):
    rows = _inputs(7)
    m = np.array(m_bits, np.uint32).view(np.float32)
    _same_bits(_apply_host(tmp_path, rows, R.TONEMAP, m_bits=m_bits), R.tonemap(rows, m))


def test_tonemap_maximum_equals_restatement(tmp_path):
    for seed, rows in enumerate((_random_rows(3), _edge_rows(), np.full((5, 4), -1.0, np.float32), np.full((3, 4), np.nan, np.float32))):
        src = str(tmp_path / f"lum{seed}.f32")
        rows.tofile(src)
        r = subprocess.run([CHECK, "maxlum", src], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0
        assert int(r.stdout, 16) == int(np.array(R.max_luminance([rows]), np.float32).view(np.uint32)), seed


@pytest.mark.parametrize("key", [0x00FF00, 0xFF00FF, 0x000000, 0xFFFFFF, 0x336699, 0x7F80FF])
def test_color_key_header_equals_restatement(tmp_path, key):
    rows = np.concatenate([_key_rows(key), _inputs(key & 0xFF)])
    got = _apply_host(tmp_path, rows, R.COLOR_KEY, key=key)
    want = R.color_key(rows, key)
    _same_bits(got, want)
    kr = _key_rows(key)
    hits = R.color_key(kr, key)[:, 3] == 0
    assert hits.any() and (~hits).any()                 # the boundary rows fall on both sides


def test_color_key_ignores_the_high_byte(tmp_path):
    rows = _key_rows(0x123456)
    _same_bits(_apply_host(tmp_path, rows, R.COLOR_KEY, key=0xAB123456), R.color_key(rows, 0x123456))


def test_invert_y_header_equals_restatement(tmp_path):
    rows = _inputs(11)
    _same_bits(_apply_host(tmp_path, rows, R.INVERT_Y), R.invert_y(rows))


@pytest.mark.parametrize("unorm", [True, False])
def test_reconstruct_z_header_equals_restatement(tmp_path, unorm):
    rng = np.random.default_rng(5)
    outside = rng.uniform(-1.5, 1.5, (4096, 4)).astype(np.float32)         # x^2 + y^2 > 1 for many of these: sqrt of a negative
    rows = np.concatenate([_inputs(13), outside, np.array([[1, 1, 0, 1], [0, 0, 0, 0], [0.5, 0.5, 0, 0], [-0.0, 0, 0, 0]], np.float32)])
    got = _apply_host(tmp_path, rows, R.RECONSTRUCT_Z, unorm=unorm)
    _same_bits(got, R.reconstruct_z(rows, unorm))
    assert np.isnan(got[:, 2]).any() and np.isfinite(got[:, 2]).any()


MASKS = ["r", "g", "b", "a", "x", "y", "z", "w", "R", "G", "B", "A", "X", "Y", "Z", "W", "0", "1", "rg", "bgr", "bgr1", "rgba", "abgr",
         "r0", "g1", "01", "10", "w0", "1r", "rrrg", "xyzw", "XyZw", "0000", "1111", "a1", "r0g", "",
         "q", "rgq", "rgbaa", "rgbar", "rg ", "2", "-", "rgb?", "ab!"]


@pytest.mark.parametrize("mask", MASKS)
def test_swizzle_mask_parsing(mask):
    want = R.parse_swizzle_mask(mask)
    assert capi.parse_swizzle_mask(mask) == want
    if mask:
        r = subprocess.run([CHECK, "mask", mask], capture_output=True, text=True, timeout=30)
        assert r.returncode == 0
        got = r.stdout.split()
        if want is None:
            assert got == ["bad"]
        else:
            assert [int(v) for v in got] == want[0] + want[1] + want[2]


def _run(args):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def dds(tmp_path_factory):
    d = tmp_path_factory.mktemp("xf")
    rng = np.random.default_rng(2)
    path = str(d / "a.dds")
    oracle.ref_save_dds(rng.integers(0, 256, 8 * 4 * 4, dtype=np.uint8), 8, 4, 28).tofile(path)
    return path


@pytest.mark.parametrize("opts", [["-swizzle", "bgr1"], ["--swizzle", "rrrg"], ["-swizzle", "1"], ["-swizzle", "XyZw"], ["-tonemap"], ["--tonemap"],
                                  ["-inverty"], ["--invert-y"], ["-reconstructz"], ["--reconstruct-z"], ["-c", "00ff00"], ["-c", "0xFF00FF"],
                                  ["--color-key", "123456"], ["-c", "ABCDEF12"],
                                  ["-swizzle", "w0", "-tonemap", "-c", "ff", "-inverty", "-reconstructz"]])
def test_transform_options_are_accepted(dds, opts):
    r = _run(opts + ["-info", dds])
    assert r.returncode == 0, (opts, r.stderr)


@pytest.mark.parametrize("opts", [["-swizzle", "rgbaa"], ["-swizzle", "q"], ["--swizzle", "rg2"], ["-swizzle", ""], ["-swizzle"], ["-c", "zz"], ["-c"],
                                  ["--color-key", "xyz"], ["-rotatecolor", "709to2020"], ["-nits", "200"], ["-dxt5nm"], ["-dxt5rxgb"], ["-vflip"],
                                  ["-hflip"], ["-inverty:1"]])
def test_transform_option_errors(dds, opts):
    r = _run(opts + ["-o", "x.dds", dds])
    assert r.returncode == 1 and "usage: dxtexconv" in r.stderr, (opts, r.stderr)
