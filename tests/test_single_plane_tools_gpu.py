"""Planar DDS inputs (NV12, P010, NV11, written with the oracle's DDS writer) through dxtexconv, dxtexdiag and dxtexassemble: each tool
converts them to their single-plane form on the device first, as the reference's tools do, so their output equals what they make of the
pre-converted file (the reference's own ConvertToSinglePlane, tests/plane_ref.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
RGBA8, RGBA16 = 28, 11
W, H = 40, 6          # a multiple of four wide (NV11), even (4:2:0); a file's tight pitches (40 or 80 -> 80 or 160) take the wide route,
                      # whole 16-byte groups over three row pairs (a tight layout that goes wide has no tail: the matrix tests cover tails)


def _tool(name, *args, ok=True):
    r = subprocess.run([os.path.join(LIB, name), *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout + r.stderr


def _dds(oracle, px, w, h, fmt):
    """The reference's SaveToDDSMemory of one 2-D image (the general writer entry: the short one sizes its input by a table without planar formats)."""
    hr, data = oracle.ref_save_dds_ex(px, w, h, 1, fmt, 1, 1, 0, 0, 3, 0)
    assert hr == 0 and data is not None
    return bytes(data)


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    """Per format: the planar file, the reference's single-plane rows and their file."""
    d = tmp_path_factory.mktemp("planar")
    out = {}
    for fmt, name in ((R.NV12, "nv12"), (R.P010, "p010"), (R.NV11, "nv11")):
        rp, sp = R.natural(fmt, W, H)
        src = np.random.default_rng(fmt).integers(1, 256, sp, dtype=np.uint8)
        hr, dfmt, pitch, rows = R.convert(oracle, src, W, H, fmt, rp, sp)
        assert hr == R.S_OK
        planar, single = d / f"{name}.dds", d / f"{name}_single.dds"
        planar.write_bytes(_dds(oracle, src, W, H, fmt))
        single.write_bytes(_dds(oracle, rows.reshape(-1), W, H, dfmt))
        out[fmt] = dict(dir=d, planar=planar, single=single, rows=rows.reshape(-1), dfmt=dfmt, name=name)
    return out


def _payload(oracle, path, fmt):
    meta, px = oracle.ref_load_dds(np.frombuffer(path.read_bytes(), np.uint8))
    assert (meta["width"], meta["height"], meta["format"], meta["arraySize"], meta["mipLevels"]) == (W, H, fmt, 1, 1)
    return px


@pytest.mark.parametrize("fmt", [R.NV12, R.P010, R.NV11])
def test_dxtexconv_converts_planar_inputs(oracle, files, fmt):
    f = files[fmt]
    for target, tname in ((RGBA8, "R8G8B8A8_UNORM"),) + (((RGBA16, "R16G16B16A16_UNORM"),) if fmt == R.P010 else ()):
        out = f["dir"] / f"{f['name']}_{tname}.dds"
        log = _tool("dxtexconv", "-nologo", "-y", "-timing", "-m", "1", "-f", tname, "-o", out, f["planar"])
        want = oracle.ref_convert(f["rows"], W, H, f["dfmt"], target).view(np.uint8).reshape(-1)
        assert np.array_equal(_payload(oracle, out, target), want)
        # one upload, of the planar bytes
        up = re.search(r"host -> device (\d+) bytes", log)
        assert up and int(up.group(1)) == R.natural(fmt, W, H)[1], log
    out = f["dir"] / f"{f['name']}_plain.dds"
    _tool("dxtexconv", "-nologo", "-y", "-m", "1", "-o", out, f["planar"])
    assert np.array_equal(_payload(oracle, out, f["dfmt"]), f["rows"])


def test_dxtexconv_info_is_unchanged(files):
    log = _tool("dxtexconv", "-info", files[R.NV12]["planar"])
    assert "(container only: no GPU path for this format)" in log


def test_dxtexconv_reports_a_failed_conversion(oracle, files, tmp_path):
    """NV11 with a width that is no multiple of four: the step fails under texconv's name and the file counts as failed."""
    rp, sp = R.natural(R.NV11, 6, 2)
    bad = tmp_path / "bad.dds"
    bad.write_bytes(_dds(oracle, np.full(sp, 7, np.uint8), 6, 2, R.NV11))
    log = _tool("dxtexconv", "-nologo", "-y", "-m", "1", "-f", "R8G8B8A8_UNORM", "-o", tmp_path / "out.dds", bad, ok=False)
    assert "FAILED [converttosingleplane] (80070057)" in log


def _without_names(text, *paths):
    """The tool's output without the lines that name a file or a format."""
    keep = []
    for line in text.splitlines():
        if any(os.path.basename(str(p)) in line for p in paths) or re.search(r"format|NV12|P010|NV11|YUY2|Y210", line):
            continue
        keep.append(line)
    return keep


@pytest.mark.parametrize("fmt", [R.NV12, R.P010, R.NV11])
def test_dxtexdiag_on_planar_equals_preconverted(files, fmt):
    f = files[fmt]
    a = _tool("dxtexdiag", "analyze", "-nologo", f["planar"])
    b = _tool("dxtexdiag", "analyze", "-nologo", f["single"])
    assert _without_names(a, f["planar"], f["single"]) == _without_names(b, f["planar"], f["single"]) and "Minimum" in a
    a = _tool("dxtexdiag", "compare", "-nologo", f["planar"], f["single"])
    b = _tool("dxtexdiag", "compare", "-nologo", f["single"], f["single"])
    assert _without_names(a, f["planar"], f["single"]) == _without_names(b, f["planar"], f["single"]) and "Result: 0.000000" in a


def test_dxtexassemble_takes_a_planar_input(oracle, files):
    f = files[R.NV12]
    rgba = f["dir"] / "rgba.dds"
    rgba.write_bytes(bytes(oracle.ref_save_dds(np.random.default_rng(3).integers(1, 256, W * H * 4, dtype=np.uint8), W, H, RGBA8)))
    a, b = f["dir"] / "array_planar.dds", f["dir"] / "array_single.dds"
    _tool("dxtexassemble", "array", "-nologo", "-y", "-f", "R8G8B8A8_UNORM", "-o", a, f["planar"], rgba)
    _tool("dxtexassemble", "array", "-nologo", "-y", "-f", "R8G8B8A8_UNORM", "-o", b, f["single"], rgba)
    assert a.read_bytes() == b.read_bytes()
    meta, px = oracle.ref_load_dds(np.frombuffer(a.read_bytes(), np.uint8))
    assert (meta["width"], meta["height"], meta["format"], meta["arraySize"]) == (W, H, RGBA8, 2)
    assert np.array_equal(px[:W * H * 4], oracle.ref_convert(f["rows"], W, H, f["dfmt"], RGBA8).view(np.uint8).reshape(-1))
