"""The tools on .tga files, end to end against the reference's reader and writer (oracle): dxtexconv sends a .tga input up as the file's own
bytes a texel and brings an -ft tga output down as the file's rows (the -timing line counts the bytes), dxtexassemble builds a cube from
.tga faces, dxtexdiag analyses a .tga as it analyses the same pixels in a DDS."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_hdr_tga_cpu import TGA_STAMP, tga_header, tga_rle  # noqa: E402

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
RGBA8, BGRX8 = 28, 88
CUBE = 0x4          # TEX_MISC_TEXTURECUBE


def _tool(name, args):
    r = subprocess.run([os.path.join(LIB, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout + r.stderr


def _moved(txt):
    m = re.search(r"host -> device (\d+) bytes, device -> host (\d+) bytes", txt)
    assert m, txt
    return int(m.group(1)), int(m.group(2))


def _tga(seed, w, h, bits, descriptor=0, rle=False):
    """a true-colour file: 24 or 32 bits, raw or run-length encoded, alpha in use"""
    rng = np.random.default_rng(seed)
    px = rng.integers(0, 256, (w * h, bits // 8), dtype=np.uint8)
    body = tga_rle(rng, px, bits // 8, w) if rle else px.tobytes()
    return tga_header(10 if rle else 2, w, h, bits, descriptor | (8 if bits == 32 else 0)) + body


@pytest.mark.parametrize("w,h,bits,descriptor,rle", [(130, 3, 24, 0x00, False), (65, 5, 32, 0x10, True)])
def test_dxtexconv_uploads_a_tga_file_at_its_own_bytes(tmp_path, oracle, w, h, bits, descriptor, rle):
    """A 24-bit bottom-up file and a 32-bit run-length right-to-left one: the DDS holds the reference loader's pixels, and width * height *
    3 (4) bytes went up."""
    src, out = tmp_path / "in.tga", tmp_path / "out.dds"
    data = _tga(bits + w, w, h, bits, descriptor, rle)
    with open(src, "wb") as f:
        f.write(data)
    txt = _tool("dxtexconv", ["-timing", "-m", "1", "-f", "R8G8B8A8_UNORM", "-o", out, src])
    hr, meta, want = oracle.ref_load_tga(data, 0)
    assert hr == 0 and meta["format"] == RGBA8
    dmeta, px = oracle.ref_load_dds(np.fromfile(out, np.uint8))
    assert (dmeta["width"], dmeta["height"], dmeta["format"], dmeta["mipLevels"]) == (w, h, RGBA8, 1)
    assert np.array_equal(np.asarray(px, np.uint8)[:want.size], want) and px.size == want.size
    assert _moved(txt)[0] == w * h * bits // 8, txt


def test_dxtexconv_downloads_a_tga_output_as_the_files_rows(tmp_path, oracle):
    """-ft tga -tga20 from a B8G8R8X8 DDS: the reference writer's file outside the time stamp, and width * height * 3 bytes came down."""
    w, h = 52, 9
    src, out = tmp_path / "in.dds", tmp_path / "in.tga"
    px = np.random.default_rng(5).integers(0, 256, (h, w * 4), dtype=np.uint8)
    oracle.ref_save_dds(px, w, h, BGRX8).tofile(src)
    txt = _tool("dxtexconv", ["-timing", "-m", "1", "-ft", "tga", "-tga20", "-o", tmp_path, src])
    rhr, ref = oracle.ref_save_tga(px, w, h, BGRX8, w * 4, 0, 0)
    assert rhr == 0
    got, ref = np.fromfile(out, np.uint8), ref.copy()
    assert got.size == ref.size == 18 + w * h * 3 + 495 + 26
    at = ref.size - 26 - 495
    got[at + TGA_STAMP.start:at + TGA_STAMP.stop] = 0
    ref[at + TGA_STAMP.start:at + TGA_STAMP.stop] = 0
    assert np.array_equal(got, ref)
    assert _moved(txt)[1] == w * h * 3, txt


def test_dxtexassemble_cube_from_tga_faces(tmp_path, oracle):
    """Six small .tga faces (a 32-bit run-length one and a right-to-left one among 24-bit ones) give the DDS that the same faces stored as
    DDS give."""
    n = 20
    tgas, ddss = [], []
    for k in range(6):
        data = _tga(40 + k, n, n, 32, (0x00, 0x10, 0x20, 0x30)[k % 4], rle=(k % 2 == 1))
        hr, meta, px = oracle.ref_load_tga(data, 0)
        assert hr == 0 and meta["format"] == RGBA8
        tgas.append(tmp_path / f"face{k}.tga")
        with open(tgas[-1], "wb") as f:
            f.write(data)
        ddss.append(tmp_path / f"face{k}.dds")
        oracle.ref_save_dds(px, n, n, RGBA8).tofile(ddss[-1])
    a, b = tmp_path / "a.dds", tmp_path / "b.dds"
    _tool("dxtexassemble", ["cube", "-nologo", "-y", "-o", a, *tgas])
    _tool("dxtexassemble", ["cube", "-nologo", "-y", "-o", b, *ddss])
    got, want = np.fromfile(a, np.uint8), np.fromfile(b, np.uint8)
    meta, _ = oracle.ref_load_dds(got)
    assert (meta["width"], meta["height"], meta["format"], meta["arraySize"], meta["miscFlags"] & CUBE) == (n, n, RGBA8, 6, CUBE)
    assert np.array_equal(got, want)


def test_dxtexdiag_analyze_of_a_tga_file(tmp_path, oracle):
    """analyze loads a .tga with the resident loader: its report is that of a DDS holding the reference reader's pixels."""
    w, h = 37, 6
    src, dds = tmp_path / "a.tga", tmp_path / "a.dds"
    data = _tga(9, w, h, 24, 0x10)
    with open(src, "wb") as f:
        f.write(data)
    hr, meta, px = oracle.ref_load_tga(data, 0)
    assert hr == 0
    oracle.ref_save_dds(px, w, h, RGBA8).tofile(dds)
    a = _tool("dxtexdiag", ["analyze", "-nologo", src]).replace(str(src), "FILE")
    b = _tool("dxtexdiag", ["analyze", "-nologo", dds]).replace(str(dds), "FILE")
    assert "Minimum" in a, a
    assert a == b


def test_dxtexdiag_compare_and_diff_of_tga_files(tmp_path, oracle):
    """compare and diff load a .tga resident and diff writes its .tga through the resident saver: the printed lines and the difference map
    are those of the same pixels in DDS files, and the .tga map is the reference writer's file of the DDS map's pixels."""
    w, h = 37, 6
    names = {}
    for k, (bits, desc, rle) in enumerate(((32, 0x20, True), (24, 0x00, False))):
        data = _tga(20 + k, w, h, bits, desc, rle)
        hr, meta, px = oracle.ref_load_tga(data, 0)
        assert hr == 0 and meta["format"] == RGBA8
        names[k] = (tmp_path / f"i{k}.tga", tmp_path / f"i{k}.dds")
        with open(names[k][0], "wb") as f:
            f.write(data)
        oracle.ref_save_dds(px, w, h, RGBA8).tofile(names[k][1])
    a = _tool("dxtexdiag", ["compare", "-nologo", names[0][0], names[1][0]])
    b = _tool("dxtexdiag", ["compare", "-nologo", names[0][1], names[1][1]])
    assert a == b and "Result:" in a, (a, b)
    outs = [tmp_path / "t.tga", tmp_path / "d.tga", tmp_path / "d.dds"]
    _tool("dxtexdiag", ["diff", "-nologo", names[0][0], names[1][1], "-o", outs[0]])          # a .tga and a .dds in
    _tool("dxtexdiag", ["diff", "-nologo", names[0][1], names[1][1], "-o", outs[1]])
    _tool("dxtexdiag", ["diff", "-nologo", names[0][1], names[1][1], "-o", outs[2]])
    t, d = np.fromfile(outs[0], np.uint8), np.fromfile(outs[1], np.uint8)
    assert np.array_equal(t, d)
    meta, px = oracle.ref_load_dds(np.fromfile(outs[2], np.uint8))
    rhr, ref = oracle.ref_save_tga(np.asarray(px, np.uint8), w, h, meta["format"], w * 4)
    assert rhr == 0 and np.array_equal(t, ref)
