"""dxtexconv on portable pixmaps, end to end: a .ppm / .pfm / .phm input goes up as the file's own bytes a texel and gives the DDS the same
pipeline makes of the equivalent DDS (the pixels tests/pnm_ref.py, the restatement of the reference's reader, reads from the file);
-ft ppm / pfm outputs are the restatement's files and come down as the file's rows; -info prints the metadata."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnm_ref as R  # noqa: E402
from test_pnm_cpu import p3_file, pnm_file  # noqa: E402

pytestmark = pytest.mark.gpu
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
W, H = 65, 5


def _tool(args):
    r = subprocess.run([os.path.join(LIB, "dxtexconv")] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout + r.stderr


def _moved(txt):
    m = re.search(r"host -> device (\d+) bytes, device -> host (\d+) bytes", txt)
    assert m, txt
    return int(m.group(1)), int(m.group(2))


def _finite(data, kind, big):
    """a float file's samples made finite and moderate, so that the block encoder downstream has defined input"""
    head = len(data) - W * H * R.FILE_BYTES[kind]
    n = W * H * (3 if kind in (R.PF, R.PH) else 1)
    v = np.random.default_rng(kind).random(n) * 4
    body = v.astype(np.float32).astype(">f4" if big else "<f4") if kind in (R.PF, R.Pf) else v.astype(np.float16).astype(">f2" if big else "<f2")
    return data[:head] + body.tobytes()


CASES = {
    "ppm": (lambda rng: pnm_file(R.P6, W, H, rng, comment=b"# a comment\n"), "BC1_UNORM", 3),
    "ppm_maxval": (lambda rng: pnm_file(R.P6, W, H, rng, maxval=100), "BC1_UNORM", 3),
    "ppm_ascii": (lambda rng: p3_file(W, H, rng), "BC1_UNORM", 4),
    "pfm": (lambda rng: _finite(pnm_file(R.PF, W, H, rng), R.PF, False), "BC6H_UF16", 12),
    "pfm_big_endian": (lambda rng: _finite(pnm_file(R.PF, W, H, rng, True), R.PF, True), "BC6H_UF16", 12),
    "phm": (lambda rng: _finite(pnm_file(R.PH, W, H, rng), R.PH, False), "BC6H_UF16", 6),
    "phm_grey": (lambda rng: _finite(pnm_file(R.Ph, W, H, rng, True), R.Ph, True), "R16G16B16A16_FLOAT", 2),
    "pfm_grey": (lambda rng: _finite(pnm_file(R.Pf, W, H, rng), R.Pf, False), "R16G16B16A16_FLOAT", 4),
}


@pytest.mark.parametrize("case", list(CASES))
def test_dxtexconv_takes_a_pixmap_like_the_equivalent_dds(tmp_path, oracle, case):
    make, target, up_bytes = CASES[case]
    data = make(np.random.default_rng(3))
    ext = {"pp": ".ppm", "pf": ".pfm", "ph": ".phm"}[case[:2]]
    src, dds = tmp_path / ("in" + ext), tmp_path / "same.dds"
    with open(src, "wb") as f:
        f.write(data)
    hr, ref = R.load(data)
    assert hr == 0 and (ref["width"], ref["height"]) == (W, H)
    oracle.ref_save_dds(ref["pixels"], W, H, ref["format"]).tofile(dds)
    a, b = tmp_path / "a.dds", tmp_path / "b.dds"
    txt = _tool(["-nologo", "-timing", "-m", "0", "-f", target, "-o", a, src])
    _tool(["-nologo", "-m", "0", "-f", target, "-o", b, dds])
    got, want = np.fromfile(a, np.uint8), np.fromfile(b, np.uint8)
    meta, _ = oracle.ref_load_dds(got)
    assert (meta["width"], meta["height"], meta["mipLevels"]) == (W, H, 7)
    assert np.array_equal(got, want)
    assert _moved(txt)[0] == W * H * up_bytes, txt          # the file's bytes a texel went up (a P3 file's decoded words)
    info = _tool(["-nologo", "-info", src])
    assert f"{W}x{H}" in info and f"format {ref['format']} " in info and "mips 1 items 1" in info, info


@pytest.mark.parametrize("fmt,ft", [(R.RGBA8, "ppm"), (R.BGRX8, "ppm"), (R.BGRA8_SRGB, "ppm"), (R.RGBA32F, "pfm"), (R.RGBA16F, "pfm"), (R.R32F, "pfm")])
def test_dxtexconv_writes_the_restatements_file(tmp_path, oracle, fmt, ft):
    """-ft ppm / -ft pfm of a DDS: the restatement's file (the halves widened by the live oracle's Convert), and the file's rows came down"""
    rng = np.random.default_rng(fmt)
    if ft == "ppm":
        px = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
        want = R.save_ppm(px, fmt)
    else:
        ch = 1 if fmt == R.R32F else 4
        v = rng.random((H, W, ch)) * 8 - 1
        px = v.astype(np.float16).view(np.uint16) if fmt == R.RGBA16F else v.astype(np.float32).view(np.uint32)
        want = R.save_pfm(px, fmt, lambda halves: oracle.ref_convert(px, W, H, R.RGBA16F, R.RGB32F).view(np.uint32).reshape(H, W, 3))
    src = tmp_path / "in.dds"
    oracle.ref_save_dds(px, W, H, fmt).tofile(src)
    txt = _tool(["-nologo", "-timing", "-m", "1", "-ft", ft, "-o", tmp_path, src])
    got = open(tmp_path / ("in." + ft), "rb").read()
    assert got == want
    # down: the file's rows, and for a format with alpha the 8-byte count of the tool's alpha-mode reduction (texconv.cpp:3738-3766)
    scan = 0 if fmt in (R.BGRX8, R.R32F) else 8
    assert _moved(txt)[1] == W * H * (3 if ft == "ppm" else 4 if fmt == R.R32F else 12) + scan, txt


def test_dxtexconv_refuses_what_the_writers_refuse(tmp_path, oracle):
    src = tmp_path / "in.dds"
    oracle.ref_save_dds(np.zeros((H, W, 4), np.float32), W, H, R.RGBA32F).tofile(src)
    r = subprocess.run([os.path.join(LIB, "dxtexconv"), "-nologo", "-m", "1", "-ft", "ppm", "-o", str(tmp_path), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "80070032" in (r.stdout + r.stderr).lower(), r.stdout + r.stderr
