"""The tools on JPEG output, end to end: dxtexassemble h-strip -o x.jpg and dxtexdiag diff -o x.jpg write, through the resident saver, the
file the host saver writes from the texels of their -o x.dds; dxtexconv -info reads it back; a format the writer refuses fails with its
HRESULT; dxtexconv's own -ft jpg stays the usage error it was."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref as R  # noqa: E402
import jpeg_write_ref as W  # noqa: E402
from test_jpeg_write_cpu import HOST, save_many  # noqa: E402

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "directxtex_amd", "lib")


def _tool(name, args, ok=True):
    r = subprocess.run([os.path.join(LIB, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout + r.stderr


def _faces(tmp_path, oracle, n):
    files = []
    for k in range(6):
        px = np.random.default_rng(60 + k).integers(0, 256, (n, n, 4), dtype=np.uint8)
        files.append(tmp_path / f"face{k}.dds")
        oracle.ref_save_dds(px.reshape(n, n * 4), n, n, R.RGBA8_SRGB).tofile(files[-1])
    return files


def _same_as_the_host_saver(tmp_path, oracle, jpg, dds, name):
    """the .jpg is the host saver's file of the .dds's texels, and -info gives its size and what the reader makes of it"""
    meta, px = oracle.ref_load_dds(np.fromfile(dds, np.uint8))
    w, h, fmt = meta["width"], meta["height"], meta["format"]
    rows = np.asarray(px, np.uint8).reshape(-1)[:w * h * 4].reshape(h, w, 4)
    rgb = rows[..., :3] if fmt in (R.RGBA8, R.RGBA8_SRGB) else rows[..., 2::-1]
    _, files = save_many(HOST, str(tmp_path), [(fmt, rgb, 0)], name=name)
    data = open(jpg, "rb").read()
    assert data == files[0], (name, len(data), len(files[0]))
    info = R.decode(data)
    assert np.array_equal(R.coefficients(info), R.coefficients(W.encode(rgb, (2, 2))))
    txt = _tool("dxtexconv", ["-nologo", "-info", jpg])
    assert f"{w}x{h}" in txt and f"format {R.RGBA8_SRGB} " in txt and "mips 1 items 1" in txt, txt
    return w, h


def test_dxtexassemble_h_strip_as_jpg(tmp_path, oracle):
    n = 12
    cube = tmp_path / "cube.dds"
    _tool("dxtexassemble", ["cube", "-nologo", "-y", "-o", cube, *_faces(tmp_path, oracle, n)])
    xj, xe, xd = tmp_path / "x.jpg", tmp_path / "X.JPEG", tmp_path / "x.dds"
    _tool("dxtexassemble", ["h-strip", "-nologo", "-y", "-o", xj, cube])
    _tool("dxtexassemble", ["h-strip", "-nologo", "-y", "-o", xe, cube])
    _tool("dxtexassemble", ["h-strip", "-nologo", "-y", "-o", xd, cube])
    assert _same_as_the_host_saver(tmp_path, oracle, xj, xd, "strip") == (6 * n, n)
    assert open(xe, "rb").read() == open(xj, "rb").read()


def test_dxtexdiag_diff_as_jpg(tmp_path, oracle):
    faces = _faces(tmp_path, oracle, 21)
    dj, dd = tmp_path / "d.jpg", tmp_path / "d.dds"
    _tool("dxtexdiag", ["diff", "-nologo", faces[0], faces[1], "-o", dj])
    _tool("dxtexdiag", ["diff", "-nologo", faces[0], faces[1], "-o", dd])
    assert _same_as_the_host_saver(tmp_path, oracle, dj, dd, "diff") == (21, 21)


def test_a_format_the_writer_refuses_fails_with_its_hresult(tmp_path, oracle):
    faces = _faces(tmp_path, oracle, 8)
    txt = _tool("dxtexdiag", ["diff", "-nologo", "-f", "R32G32B32A32_FLOAT", faces[0], faces[1], "-o", tmp_path / "d.jpg"], ok=False)
    assert "80070032" in txt.lower() and not os.path.exists(tmp_path / "d.jpg"), txt
    cube = tmp_path / "cube.dds"
    _tool("dxtexassemble", ["cube", "-nologo", "-y", "-o", cube, *faces])
    txt = _tool("dxtexassemble", ["h-strip", "-nologo", "-y", "-f", "R16G16B16A16_UNORM", "-o", tmp_path / "x.jpg", cube], ok=False)
    assert "80070032" in txt.lower() and not os.path.exists(tmp_path / "x.jpg"), txt
    txt = _tool("dxtexassemble", ["array", "-nologo", "-y", "-o", tmp_path / "a.jpg", *faces[:2]], ok=False)
    assert "the output file must be .dds" in txt, txt


def test_dxtexconv_still_writes_no_jpg(tmp_path, oracle):
    src = _faces(tmp_path, oracle, 8)[0]
    for args in (["-ft", "jpg", "-o", tmp_path, src], ["-o", tmp_path / "x.jpg", src]):
        r = subprocess.run([os.path.join(LIB, "dxtexconv"), "-nologo"] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 1 and "usage: dxtexconv" in r.stderr and "JPEG output is not written yet" in r.stderr, (args, r.stderr)
    assert not os.path.exists(tmp_path / "x.jpg")
