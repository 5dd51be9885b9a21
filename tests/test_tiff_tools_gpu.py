"""The three tools on TIFF files, end to end: dxtexconv takes a .tif as it takes the same texels in a DDS (a 16-bit height map to BC4_UNORM, RGB 8
to BC7_UNORM) and writes -ft tif files that tests/tiff_ref.py reads back as the image; dxtexassemble and dxtexdiag read one each and write .tif."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tiff_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
W, H = 68, 36


def _tool(name, args, ok=True):
    r = subprocess.run([os.path.join(LIB, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout + r.stderr


def _moved(txt):
    m = re.search(r"host -> device (\d+) bytes, device -> host (\d+) bytes", txt)
    assert m, txt
    return int(m.group(1)), int(m.group(2))


def _smooth(kind, seed):
    bits, S, _, _ = T.KINDS[kind]
    top = (1 << bits) - 1
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    planes = [((np.sin(x / (4.0 + k) + seed) + 1) * (np.cos(y / (6.0 + k)) + 1) / 4 * top + rng.integers(0, max(2, top // 200), (H, W))).clip(0, top) for k in range(S)]
    return np.stack(planes, 2).astype(np.uint16 if bits == 16 else np.uint8)


def test_height16_tif_to_bc4_is_the_dds_routes_file(tmp_path, oracle):
    """dxtexconv -f BC4_UNORM -o out/ height16.tif: the file the DDS route produces from the same texels, byte for byte; 2 bytes a texel went up"""
    tif, dds = tmp_path / "height16.tif", tmp_path / "same" / "height16.dds"
    os.makedirs(tmp_path / "same"); os.makedirs(tmp_path / "out"); os.makedirs(tmp_path / "out2")
    a = _smooth(T.GREY16, 1)
    tif.write_bytes(T.build(a, T.GREY16, compression=T.ADOBE_DEFLATE, predictor=2, rows_per_strip=8))
    oracle.ref_save_dds(np.ascontiguousarray(a.reshape(H, W)).view(np.uint8), W, H, T.R16_UNORM).tofile(dds)
    txt = _tool("dxtexconv", ["-nologo", "-timing", "-f", "BC4_UNORM", "-o", tmp_path / "out", tif])
    _tool("dxtexconv", ["-nologo", "-f", "BC4_UNORM", "-o", tmp_path / "out2", dds])
    assert np.array_equal(np.fromfile(tmp_path / "out" / "height16.dds", np.uint8), np.fromfile(tmp_path / "out2" / "height16.dds", np.uint8))
    assert _moved(txt)[0] == W * H * 2, txt


def test_rgb8_tiff_to_bc7_and_back_to_tif(tmp_path, oracle):
    tif, dds = tmp_path / "colour.tiff", tmp_path / "colour.dds"
    a = _smooth(T.RGB8, 2)
    tif.write_bytes(T.build(a, T.RGB8, compression=T.LZW, predictor=2, tile=(16, 16), big_endian=True, planar=True))
    rgba = np.frombuffer(T.texels(a, T.RGB8).tobytes(), np.uint8).reshape(H, W * 4)
    oracle.ref_save_dds(rgba, W, H, T.R8G8B8A8_UNORM).tofile(dds)
    x, y = tmp_path / "x.dds", tmp_path / "y.dds"
    txt = _tool("dxtexconv", ["-nologo", "-timing", "-f", "BC7_UNORM", "-o", x, tif])
    _tool("dxtexconv", ["-nologo", "-f", "BC7_UNORM", "-o", y, dds])
    assert np.array_equal(np.fromfile(x, np.uint8), np.fromfile(y, np.uint8))
    assert _moved(txt)[0] == len(T.segments(T.parse(tif.read_bytes()))[0]), txt
    # -ft tif: the file tiff_ref.save makes of the image, and -o as a .tif / .tiff name or a directory
    out = tmp_path / "back.tif"
    _tool("dxtexconv", ["-nologo", "-m", "1", "-ft", "tif", "-o", out, tif])
    assert out.read_bytes() == T.save(rgba.tobytes(), W, H, T.R8G8B8A8_UNORM)[1]
    _tool("dxtexconv", ["-nologo", "-ft", "tiff", "-f", "R16_UNORM", "-o", tmp_path, dds])
    hr, d = T.decode((tmp_path / "colour.tif").read_bytes())          # a directory receives <name>.tif
    assert hr == 0 and d["format"] == T.R16_UNORM and (d["width"], d["height"]) == (W, H)
    assert "-ft tif writes a .tif" in _tool("dxtexconv", ["-nologo", "-ft", "tif", "-o", tmp_path / "wrong.png", tif], ok=False)


def test_dxtexassemble_and_dxtexdiag_read_and_write_tif(tmp_path):
    a, b = tmp_path / "a.tif", tmp_path / "b.tif"
    pa, pb = _smooth(T.RGBA8, 3), _smooth(T.RGBA8, 3)
    pb[5, 7, 1] ^= 0x40
    a.write_bytes(T.build(pa, T.RGBA8, compression=T.PACKBITS, extra=2))
    b.write_bytes(T.build(pb, T.RGBA8, compression=T.DEFLATE, predictor=2, extra=2, rows_per_strip=5))
    # dxtexdiag: the two files differ in one texel; the difference map is written as a .tif the restatement reads
    m = re.search(r"Result: ([0-9.eE+-]+)", _tool("dxtexdiag", ["compare", "-nologo", a, b]))
    assert m and float(m.group(1)) > 0.0
    m = re.search(r"Result: ([0-9.eE+-]+)", _tool("dxtexdiag", ["compare", "-nologo", a, a]))
    assert m and float(m.group(1)) == 0.0
    _tool("dxtexdiag", ["diff", "-nologo", "-f", "R8G8B8A8_UNORM", a, b, "-o", tmp_path / "diff.tif"])
    hr, d = T.decode((tmp_path / "diff.tif").read_bytes())
    assert hr == 0 and (d["width"], d["height"]) == (W, H)
    txt = _tool("dxtexdiag", ["analyze", "-nologo", a])
    assert "a.tif" in txt, txt
    # dxtexassemble: merge takes two .tif inputs and writes a .tif
    out = tmp_path / "merged.tif"
    _tool("dxtexassemble", ["merge", "-nologo", "-y", "-o", out, a, b])
    hr, d = T.decode(out.read_bytes())
    assert hr == 0 and (d["width"], d["height"]) == (W, H)
    # and an array of both as a .dds
    _tool("dxtexassemble", ["array", "-nologo", "-y", "-o", tmp_path / "array.dds", a, b])
    assert (tmp_path / "array.dds").stat().st_size >= 2 * W * H * 4
