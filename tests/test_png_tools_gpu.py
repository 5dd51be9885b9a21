"""The three tools on PNG files, end to end: dxtexconv takes a .png as it takes the same texels in a .ppm or a .dds and writes -ft png files
that any PNG reader (tests/png_ref.py over zlib) reads back as the image; -ignoresrgb and a BGR -f change the loaded format as in texconv;
-info prints the metadata; dxtexassemble builds a cube from six .png faces and writes a cross as .png; dxtexdiag analyzes and diffs them."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
W, H = 65, 5
CUBE = 0x4


def _tool(name, args, ok=True):
    r = subprocess.run([os.path.join(LIB, name)] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout + r.stderr


def _moved(txt):
    m = re.search(r"host -> device (\d+) bytes, device -> host (\d+) bytes", txt)
    assert m, txt
    return int(m.group(1)), int(m.group(2))


def _png(path, kind, w, h, seed, **kw):
    """a .png of random texels with adaptive filters at level 6 -> (its bytes, its unfiltered rows)"""
    rng = np.random.default_rng(seed)
    ct, depth = R.TYPE_OF[kind]
    rows = [rng.integers(0, 256, R.row_bytes(kind, w), dtype=np.uint8).tobytes() for _ in range(h)]
    data = R.encode(w, h, ct, depth, rows, filters=tuple(int(v) for v in rng.integers(0, 5, h)), **kw)
    with open(path, "wb") as f:
        f.write(data)
    return data, b"".join(rows)


def test_dxtexconv_takes_a_png_like_the_same_texels_in_a_ppm(tmp_path):
    """RGB 8 -> BC1_UNORM with the full chain: the DDS of the .ppm that holds the same bytes, and 3 bytes a texel went up"""
    png, ppm = tmp_path / "in.png", tmp_path / "in.ppm"
    data, rows = _png(png, R.RGB8, W, H, 1)
    with open(ppm, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (W, H) + rows)
    a, b = tmp_path / "a.dds", tmp_path / "b.dds"
    txt = _tool("dxtexconv", ["-nologo", "-timing", "-ignoresrgb", "-m", "0", "-f", "BC1_UNORM", "-o", a, png])
    _tool("dxtexconv", ["-nologo", "-m", "0", "-f", "BC1_UNORM", "-o", b, ppm])
    assert np.array_equal(np.fromfile(a, np.uint8), np.fromfile(b, np.uint8))
    assert _moved(txt)[0] == W * H * 3, txt


@pytest.mark.parametrize("kind", (R.G4, R.G16, R.GA8, R.RGBA8K, R.RGBA16K, R.P2))
def test_dxtexconv_takes_a_png_like_the_equivalent_dds(tmp_path, oracle, kind):
    """other kinds against the DDS that holds the restatement's texels in the restatement's format; the unfiltered rows went up"""
    rng = np.random.default_rng(kind)
    plte = rng.integers(0, 256, 9, dtype=np.uint8).tobytes() if kind == R.P2 else None          # three entries: index 3 is past the end
    png, dds = tmp_path / "in.png", tmp_path / "same.dds"
    data, rows = _png(png, kind, W, H, 10 + kind, plte=plte, trns=b"\x80" if plte else None)
    ct, depth = R.TYPE_OF[kind]
    fmt, misc2 = R.metadata(ct, depth)
    px = R.expand(rows, W, H, kind, False, R.palette_words(plte, b"\x80") if plte else None)
    oracle.ref_save_dds(px, W, H, fmt).tofile(dds)
    target = "R16G16B16A16_UNORM" if depth == 16 else "R8G8B8A8_UNORM"
    a, b = tmp_path / "a.dds", tmp_path / "b.dds"
    txt = _tool("dxtexconv", ["-nologo", "-timing", "-m", "1", "-f", target, "-o", a, png])
    _tool("dxtexconv", ["-nologo", "-m", "1", "-f", target, "-o", b, dds])
    ma, pa = oracle.ref_load_dds(np.fromfile(a, np.uint8))
    mb, pb = oracle.ref_load_dds(np.fromfile(b, np.uint8))
    assert (ma["width"], ma["height"], ma["format"]) == (mb["width"], mb["height"], mb["format"]) and np.array_equal(pa, pb)
    assert _moved(txt)[0] == R.row_bytes(kind, W) * H, txt
    assert f"format {fmt})" in txt.splitlines()[0], txt
    info = _tool("dxtexconv", ["-nologo", "-info", png])
    assert f"{W}x{H}" in info and f"format {fmt} " in info and "mips 1 items 1" in info and ("alpha opaque" in info) == (misc2 == 3), info


def test_ignoresrgb_and_a_bgr_format_change_the_loaded_format(tmp_path):
    """texconv.cpp:2213-2217: PNG_FLAGS_BGR when -f names a BGR format, PNG_FLAGS_IGNORE_SRGB under -ignoresrgb; the "reading" line shows it"""
    rgba, rgb = tmp_path / "rgba.png", tmp_path / "rgb.png"
    _png(rgba, R.RGBA8K, W, H, 2, srgb=0)
    _png(rgb, R.RGB8, W, H, 3)
    out = tmp_path / "o.dds"

    def loaded(args, src):
        return int(re.search(r"format (\d+)\)", _tool("dxtexconv", ["-nologo", "-y", "-m", "1", *args, "-o", out, src]).splitlines()[0]).group(1))

    assert loaded([], rgba) == R.RGBA8_SRGB and loaded(["-ignoresrgb"], rgba) == R.RGBA8
    assert loaded(["-f", "B8G8R8A8_UNORM"], rgba) == R.BGRA8_SRGB and loaded(["-f", "B8G8R8A8_UNORM", "-ignoresrgb"], rgba) == R.BGRA8
    assert loaded(["-f", "B8G8R8X8_UNORM"], rgb) == R.BGRX8_SRGB and loaded(["-f", "B8G8R8A8_UNORM_SRGB", "-ignoresrgb"], rgb) == R.BGRX8
    assert loaded(["-f", "R8G8B8A8_UNORM"], rgb) == R.RGBA8_SRGB
    info = _tool("dxtexconv", ["-nologo", "-info", "-ignoresrgb", rgba])
    assert f"format {R.RGBA8} " in info, info


@pytest.mark.parametrize("fmt", (R.R8, R.R16, R.RGBA8, R.BGRA8_SRGB, R.RGBA16, R.BGRX8))
def test_dxtexconv_writes_png_files_that_read_back_as_the_image(tmp_path, oracle, fmt):
    """-ft png of a DDS: any PNG reader gets the image's texels, this project's reader gets the same DDS back, the file's rows came down"""
    ct, depth, S, F = R.WRITER[fmt]
    px = np.random.default_rng(fmt).integers(0, 256, (H, W * S), dtype=np.uint8)
    src = tmp_path / "in.dds"
    oracle.ref_save_dds(px, W, H, fmt).tofile(src)
    txt = _tool("dxtexconv", ["-nologo", "-timing", "-m", "1", "-ft", "png", "-o", tmp_path, src])
    data = open(tmp_path / "in.png", "rb").read()
    info = R.decode(data)
    assert (info["width"], info["height"], info["ct"], info["depth"]) == (W, H, ct, depth)
    assert info["rows"] == R.pack_rows(px, W, H, fmt).tobytes()
    assert [(t, b) for t, b in R.chunks(data)[1:] if t not in (b"IDAT", b"IEND")] == R.writer_chunks(fmt)
    # down: the file's rows, and for a format with alpha the 8-byte count of the tool's alpha-mode reduction (texconv.cpp:3738-3766)
    assert _moved(txt)[1] in (W * H * F, W * H * F + 8), txt
    # and back: the same texels (X reads as 0xff)
    back = tmp_path / "back.dds"
    names = {R.R8: "R8_UNORM", R.R16: "R16_UNORM", R.RGBA8: "R8G8B8A8_UNORM", R.BGRA8_SRGB: "B8G8R8A8_UNORM_SRGB", R.RGBA16: "R16G16B16A16_UNORM", R.BGRX8: "B8G8R8X8_UNORM"}
    _tool("dxtexconv", ["-nologo", "-m", "1", "-ignoresrgb" if fmt in (R.RGBA8, R.BGRX8) else "-nologo", "-f", names[fmt], "-o", back, tmp_path / "in.png"])
    meta, got = oracle.ref_load_dds(np.fromfile(back, np.uint8))
    want = px.copy()
    if fmt == R.BGRX8:
        want[:, 3::4] = 255
    assert meta["format"] == fmt and np.array_equal(np.asarray(got, np.uint8).reshape(-1)[:want.size], want.reshape(-1))


def test_dxtexconv_refuses_what_the_writer_refuses(tmp_path, oracle):
    src = tmp_path / "in.dds"
    oracle.ref_save_dds(np.zeros((H, W, 4), np.float32), W, H, R.RGBA32F).tofile(src)
    txt = _tool("dxtexconv", ["-nologo", "-m", "1", "-ft", "png", "-o", tmp_path, src], ok=False)
    assert "80070032" in txt.lower(), txt


def _faces(tmp_path, oracle, n=20):
    pngs, ddss = [], []
    for k in range(6):
        kind = (R.RGBA8K, R.RGBA8K, R.RGBA8K)[k % 3]
        pngs.append(tmp_path / f"face{k}.png")
        data, rows = _png(pngs[-1], kind, n, n, 40 + k, every=(None, 7)[k % 2], srgb=0)
        ddss.append(tmp_path / f"face{k}.dds")
        oracle.ref_save_dds(R.expand(rows, n, n, kind), n, n, R.RGBA8_SRGB).tofile(ddss[-1])
    return pngs, ddss


def test_dxtexassemble_cube_from_png_faces_and_a_cross_as_png(tmp_path, oracle):
    """six .png faces give the DDS that the same faces stored as DDS give; h-cross -o x.png holds the texels of h-cross -o x.dds"""
    n = 20
    pngs, ddss = _faces(tmp_path, oracle, n)
    a, b = tmp_path / "a.dds", tmp_path / "b.dds"
    _tool("dxtexassemble", ["cube", "-nologo", "-y", "-o", a, *pngs])
    _tool("dxtexassemble", ["cube", "-nologo", "-y", "-o", b, *ddss])
    got, want = np.fromfile(a, np.uint8), np.fromfile(b, np.uint8)
    meta, _ = oracle.ref_load_dds(got)
    assert (meta["width"], meta["height"], meta["format"], meta["arraySize"], meta["miscFlags"] & CUBE) == (n, n, R.RGBA8_SRGB, 6, CUBE)
    assert np.array_equal(got, want)
    xp, xd = tmp_path / "x.png", tmp_path / "x.dds"
    _tool("dxtexassemble", ["h-cross", "-nologo", "-y", "-o", xp, a])
    _tool("dxtexassemble", ["h-cross", "-nologo", "-y", "-o", xd, a])
    meta, px = oracle.ref_load_dds(np.fromfile(xd, np.uint8))
    info = R.decode(open(xp, "rb").read())
    assert (info["width"], info["height"]) == (meta["width"], meta["height"]) == (4 * n, 3 * n)
    assert info["rows"] == R.pack_rows(np.asarray(px, np.uint8)[:4 * n * 3 * n * 4], 4 * n, 3 * n, meta["format"]).tobytes()


def test_dxtexdiag_analyze_and_diff_of_png_files(tmp_path, oracle):
    """analyze and compare load a .png resident: their reports are those of a DDS holding the same texels; diff -o x.png holds the texels of
    diff -o x.dds"""
    pngs, ddss = _faces(tmp_path, oracle)
    a = _tool("dxtexdiag", ["analyze", "-nologo", pngs[0]]).replace(str(pngs[0]), "FILE")
    b = _tool("dxtexdiag", ["analyze", "-nologo", ddss[0]]).replace(str(ddss[0]), "FILE")
    assert "Minimum" in a and a == b, (a, b)
    a = _tool("dxtexdiag", ["compare", "-nologo", pngs[0], pngs[1]])
    b = _tool("dxtexdiag", ["compare", "-nologo", ddss[0], ddss[1]])
    assert a == b and "Result:" in a, (a, b)
    op, od = tmp_path / "d.png", tmp_path / "d.dds"
    _tool("dxtexdiag", ["diff", "-nologo", pngs[0], ddss[1], "-o", op])
    _tool("dxtexdiag", ["diff", "-nologo", ddss[0], ddss[1], "-o", od])
    meta, px = oracle.ref_load_dds(np.fromfile(od, np.uint8))
    info = R.decode(open(op, "rb").read())
    w, h = meta["width"], meta["height"]
    assert (info["width"], info["height"]) == (w, h)
    assert info["rows"] == R.pack_rows(np.asarray(px, np.uint8)[:w * h * R.WRITER[meta["format"]][2]], w, h, meta["format"]).tobytes()
