"""The three tools on JPEG files, end to end: dxtexconv decodes a golden .jpg to the texels Pillow gave for it, -ignoresrgb changes only the
format, -info prints the metadata without a device, -timing counts the coefficient bytes; dxtexassemble builds an array from .jpg items and
dxtexdiag analyzes one as it does a DDS of the same texels; -ft jpg and -o x.jpg stay usage errors."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")


def _tool(name, args, ok=True):
    r = subprocess.run([os.path.join(LIB, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout + r.stderr


def _golden(name):
    jpg = os.path.join(GOLDEN, name + ".jpg")
    fmt, misc2, w, h = map(int, open(os.path.join(GOLDEN, name + ".txt")).read().split())
    return jpg, np.fromfile(os.path.join(GOLDEN, name + ".bin"), np.uint8), fmt, misc2, w, h


@pytest.mark.parametrize("name", ("c420", "c422", "c444", "c420_progressive", "c420_restart", "c420_wide"))
def test_dxtexconv_decodes_a_golden_jpg_to_pillows_texels(tmp_path, oracle, name):
    """-f R8G8B8A8_UNORM under -ignoresrgb (so that no sRGB conversion runs): the DDS holds Pillow's decode; the coefficients went up and
    nothing else; without -ignoresrgb the file loads as R8G8B8A8_UNORM_SRGB, and only the format differs"""
    jpg, want, fmt, misc2, w, h = _golden(name)
    out = tmp_path / "o.dds"
    txt = _tool("dxtexconv", ["-nologo", "-timing", "-ignoresrgb", "-m", "1", "-f", "R8G8B8A8_UNORM", "-o", out, jpg])
    meta, px = oracle.ref_load_dds(np.fromfile(out, np.uint8))
    assert (meta["width"], meta["height"], meta["format"]) == (w, h, R.RGBA8)
    assert np.array_equal(np.asarray(px, np.uint8).reshape(-1)[:want.size], want)
    assert f"format {R.RGBA8})" in txt.splitlines()[0], txt
    up = int(re.search(r"host -> device (\d+) bytes", txt).group(1))
    assert up == R.coefficients(R.decode(open(jpg, "rb").read())).nbytes, txt
    srgb = tmp_path / "s.dds"
    txt = _tool("dxtexconv", ["-nologo", "-m", "1", "-f", "R8G8B8A8_UNORM_SRGB", "-o", srgb, jpg])
    assert f"format {R.RGBA8_SRGB})" in txt.splitlines()[0] and fmt == R.RGBA8_SRGB, txt
    meta, px = oracle.ref_load_dds(np.fromfile(srgb, np.uint8))
    assert meta["format"] == R.RGBA8_SRGB and np.array_equal(np.asarray(px, np.uint8).reshape(-1)[:want.size], want)


def test_dxtexconv_decodes_a_grey_jpg(tmp_path, oracle):
    jpg, want, fmt, misc2, w, h = _golden("grey")
    out = tmp_path / "g.dds"
    txt = _tool("dxtexconv", ["-nologo", "-m", "1", "-f", "R8_UNORM", "-o", out, jpg])
    meta, px = oracle.ref_load_dds(np.fromfile(out, np.uint8))
    assert (meta["width"], meta["height"], meta["format"]) == (w, h, R.R8) and np.array_equal(np.asarray(px, np.uint8).reshape(-1)[:want.size], want)
    assert f"format {R.R8})" in txt.splitlines()[0], txt


def test_info_prints_a_jpgs_metadata(tmp_path):
    for name in ("grey", "c420", "c420_progressive"):
        jpg, want, fmt, misc2, w, h = _golden(name)
        info = _tool("dxtexconv", ["-nologo", "-info", jpg])
        assert f"{w}x{h}" in info and f"format {fmt} " in info and "mips 1 items 1" in info and ("alpha opaque" in info) == (misc2 == 3), info
        assert (" sRGB" in info) == (fmt == R.RGBA8_SRGB), info
    info = _tool("dxtexconv", ["-nologo", "-info", "-ignoresrgb", _golden("c420")[0]])
    assert f"format {R.RGBA8} " in info and " sRGB" not in info, info
    info = _tool("dxtexconv", ["-nologo", "-info", os.path.join(GOLDEN, "cmyk.jpg")], ok=False)
    assert "80004005" in info, info


def test_jpeg_output_is_a_usage_error(tmp_path):
    jpg = _golden("c420")[0]
    for args in (["-ft", "jpg", "-o", tmp_path, jpg], ["-ft", "JPEG", "-o", tmp_path, jpg], ["-o", tmp_path / "x.jpg", jpg], ["-o", tmp_path / "x.jpeg", jpg]):
        r = subprocess.run([os.path.join(LIB, "dxtexconv"), "-nologo"] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "usage: dxtexconv" in r.stderr and "JPEG output is not written yet" in r.stderr, (args, r.stderr)
    assert not os.path.exists(tmp_path / "x.jpg")


def _figures(report):
    """the lines of an analyze report that hold the texels' statistics"""
    return [line.split() for line in report.splitlines() if any(k in line for k in ("Minimum", "Average", "Maximum", "Variance", "Luminance"))]


def test_dxtexassemble_array_and_dxtexdiag_analyze_take_a_jpg(tmp_path, oracle):
    """two .jpg items give the array that the same texels stored as DDS give; analyze reports the figures it reports for that DDS"""
    items, same = [], []
    for name in ("c420", "c444"):
        jpg, want, fmt, misc2, w, h = _golden(name)
        items.append(jpg)
        same.append(tmp_path / f"{name}.dds")
        oracle.ref_save_dds(want.reshape(h, w * 4), w, h, R.RGBA8_SRGB).tofile(same[-1])
    a, b = tmp_path / "a.dds", tmp_path / "b.dds"
    _tool("dxtexassemble", ["array", "-nologo", "-y", "-o", a, *items])
    _tool("dxtexassemble", ["array", "-nologo", "-y", "-o", b, *same])
    ma, pa = oracle.ref_load_dds(np.fromfile(a, np.uint8))
    mb, pb = oracle.ref_load_dds(np.fromfile(b, np.uint8))
    assert (ma["width"], ma["height"], ma["format"], ma["arraySize"]) == (21, 13, R.RGBA8_SRGB, 2) == (mb["width"], mb["height"], mb["format"], mb["arraySize"])
    assert np.array_equal(pa, pb)
    wants = np.concatenate([_golden(n)[1] for n in ("c420", "c444")])
    assert np.array_equal(np.asarray(pa, np.uint8).reshape(-1)[:wants.size], wants)
    x = _figures(_tool("dxtexdiag", ["analyze", "-nologo", items[0]]))
    y = _figures(_tool("dxtexdiag", ["analyze", "-nologo", same[0]]))
    assert len(x) >= 4 and x == y, (x, y)
