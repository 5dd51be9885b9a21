"""The diagnostics above the C ABI: the host layer's overloads (tests/cpp/diag_host_test.cpp: compressed inputs, DeviceScratchImage forms,
Difference against Convert -> difference -> Convert, one upload per input) and dxtexdiag's analyze, compare and diff on files written by
dxtexconv, whose printed numbers are parsed and compared with the C ABI's results and whose diff file is compared byte for byte."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from directxtex_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_scanline_routes_gpu import Device  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
RGBA32F, RGBA8, BGRA8, BC7 = 2, 28, 87, 98
W, H = 64, 48


def _exe(name, args):
    path = os.path.join(LIB, name)
    if not os.path.exists(path):
        pytest.fail(f"directxtex_amd/lib/{name} is missing: run build()")
    return subprocess.run([path] + [str(a) for a in args], capture_output=True, text=True, timeout=300)


def test_host_overloads():
    r = _exe("diag_host_test", [])
    print(r.stdout)
    failed = [l for l in r.stdout.splitlines() if l.startswith("FAIL")]
    assert r.returncode == 0 and not failed and "0 failed" in r.stdout, r.stdout + r.stderr
    assert r.stdout.count("\nok ") + r.stdout.startswith("ok ") >= 30


@pytest.fixture(scope="module")
def files(tmp_path_factory, oracle):
    """src.dds (RGBA8) and bc7.dds, its BC7 encoding by dxtexconv; the BC7 payload as the reference's reader returns it."""
    d = tmp_path_factory.mktemp("diag")
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(11)
    img = np.stack([x * 255 // (W - 1), y * 255 // (H - 1), (x * 3 + y * 5 + rng.integers(0, 16, (H, W))) & 255, 128 + rng.integers(0, 128, (H, W))], -1).astype(np.uint8)
    src = d / "src.dds"
    src.write_bytes(bytes(oracle.ref_save_dds(img, W, H, RGBA8)))
    bc = d / "bc7.dds"
    r = _exe("dxtexconv", ["-f", "BC7_UNORM", "-m", "1", "-nologo", "-o", bc, src])
    assert r.returncode == 0, r.stdout + r.stderr
    meta, payload = oracle.ref_load_dds(np.fromfile(bc, np.uint8))
    assert meta["format"] == BC7 and meta["width"] == W and meta["height"] == H
    return {"dir": d, "src": src, "bc": bc, "img": img.reshape(-1), "payload": np.frombuffer(bytes(payload), np.uint8).copy()}


def _numbers(line):
    return [float(t) for t in re.findall(r"[-+]?(?:\d+\.\d+|inf|nan)", line)]


def _close(printed, value):
    """a value printed with %f (six decimals)"""
    return np.allclose(printed, value, rtol=1e-6, atol=1e-6)


def test_dxtexdiag_analyze(ctx, files):
    r = _exe("dxtexdiag", ["analyze", "-nologo", files["bc"], files["src"]])
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout
    parts = out.split(str(files["src"]) + "\n")
    assert len(parts) == 2 and parts[0].startswith(str(files["bc"]))
    dec = ctx.decompress(files["payload"], W, H, BC7, RGBA32F)
    hist, blocks = ctx.analyze_bc(files["payload"], W, H, BC7)
    for text, stats in ((parts[0], ctx.analyze([(dec, W, H, RGBA32F, None)])[0]), (parts[1], ctx.analyze([(files["img"], W, H, RGBA8, None)])[0])):
        rows = {k.strip(): _numbers(v) for k, v in (l.split(" - ", 1) for l in text.splitlines() if " - (" in l or "Luminance - " in l)}
        assert _close(rows["Minimum"], stats["min"]) and _close(rows["Maximum"], stats["max"]) and _close(rows["Average"], stats["avg"])
        assert _close(rows["Variance"], stats["variance"]) and _close(rows["Std Dev"], np.sqrt(stats["variance"]))
        assert _close(rows["Luminance"][0], stats["luminance"])
        assert "FP specials" not in text
    assert "Compression - BC7_UNORM" in parts[0] and f"Total blocks - {blocks}" in parts[0] and "Compression" not in parts[1]
    modes = {int(m): int(n) for m, n in re.findall(r"Mode (\d\d) blocks - (\d+)", parts[0])}
    assert modes == {m: int(hist[m]) for m in range(8) if hist[m]} and sum(modes.values()) == blocks == (W // 4) * (H // 4)


def test_dxtexdiag_compare(ctx, files):
    r = _exe("dxtexdiag", ["compare", "-nologo", files["src"], files["bc"]])
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("Result: ")]
    assert len(line) == 1 and line[0].endswith(" dB")
    mse, red, green, blue, alpha, psnr = _numbers(line[0])
    dec = ctx.decompress(files["payload"], W, H, BC7, RGBA32F)
    with Device(ctx) as d:
        a, b = capi.device_image(d.put(files["img"]), W, H, RGBA8), capi.device_image(d.put(dec), W, H, RGBA32F)
        want = ctx.compute_mse_flags_device(a, b, 0)
    assert _close([red, green, blue, alpha], want) and _close(mse, float(np.float32(want).sum()))
    assert 25.0 < psnr < 80.0 and abs(psnr - 10 * np.log10(3.0 / float(np.float32(want)[:3].astype(np.float64).sum()))) < 1e-3


def test_dxtexdiag_diff(ctx, oracle, files):
    out = files["dir"] / "diff.dds"
    r = _exe("dxtexdiag", ["diff", "-nologo", "-c", "ff00ff", "-t", "0.01", "-o", out, files["src"], files["bc"]])
    assert r.returncode == 0 and f"Difference {out}" in r.stdout, r.stdout + r.stderr
    meta, got = oracle.ref_load_dds(np.fromfile(out, np.uint8))
    assert (meta["format"], meta["width"], meta["height"], meta["mipLevels"]) == (BGRA8, W, H, 1)       # -f defaults to B8G8R8A8_UNORM
    dec = ctx.decompress(files["payload"], W, H, BC7, RGBA32F)
    step = ctx.difference(files["img"], dec.view(np.float32), W, H, RGBA8, 0xFF00FF, 0.01)
    want = ctx.convert(step, W, H, RGBA8, BGRA8)
    got = np.frombuffer(bytes(got), np.uint8)
    assert np.array_equal(got, want)
    px = got.reshape(-1, 4)
    marked = (px == np.array([255, 0, 255, 255], np.uint8)).all(axis=1)
    assert marked.any() and not marked.all()
    # an existing output is kept without -y; TGA out goes through the same map
    assert _exe("dxtexdiag", ["diff", "-nologo", "-o", out, files["src"], files["bc"]]).returncode == 1
    tga = files["dir"] / "diff.tga"
    r = _exe("dxtexdiag", ["diff", "-nologo", "-f", "R8G8B8A8_UNORM", "-c", "ff00ff", "-t", "0.01", "-o", tga, files["src"], files["bc"]])
    assert r.returncode == 0 and tga.stat().st_size > W * H * 3, r.stdout + r.stderr
