"""The host layer's resident portable pixmap codec (LoadFromPortablePixMapMemory / SaveToPortablePixMap[HDR]File with a Device, through
tests/cpp/pnm_host_test.cpp) against the host codec of the same build and tests/pnm_ref.py: pixels, metadata, files and HRESULTs are the
host codec's, and the samples cross PCIe as the bytes the file has for them."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnm_ref as R  # noqa: E402
import test_pnm_cpu as C  # noqa: E402

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "pnm_host_test")


def device_load_many(tmp, files):
    """[(resident hresult, host hresult, None | dict of the line's fields, released)]"""
    paths = []
    for i, data in enumerate(files):
        paths.append(os.path.join(tmp, f"d{i}.pnm"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    lst = os.path.join(tmp, "dlist.txt")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    r = subprocess.run([EXE, "device_load_many", lst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-2000:])
    rows = r.stdout.splitlines()
    assert len(rows) == len(files)
    out = []
    names = ("width", "height", "format", "nbytes", "ascii", "up", "down", "meta_equal", "pixels_equal")
    for i, row in enumerate(rows):
        p = row.split()
        assert int(p[0]) == i
        ok = p[3] == "ok"
        out.append((int(p[1], 16), int(p[2], 16), dict(zip(names, (int(x) for x in p[4:]))) if ok else None, p[3] == "released"))
    return out


def test_resident_load_is_the_host_loaders(tmp_path):
    """Every reader kind at every small size, the refusals and the fuzz corpus of test_pnm_cpu.py. Where the file loads: HRESULT, both
    metadata and the downloaded pixels equal the host loader's (which test_pnm_cpu.py holds to the restatement), exactly the payload
    went up and nothing came down. Where it does not: the same HRESULT, and the result is released (one DeviceScratchImage serves every
    file, so it held an image before most failures)."""
    files = C.reader_files() + [f for f, _ in C.REFUSALS] + C.fuzz_corpus()[::3]
    failed = loaded = 0
    for data, (hr, host_hr, d, released) in zip(files, device_load_many(str(tmp_path), files)):
        ref_hr, ref = R.load(data)
        where = data[:60]
        assert hr == host_hr == ref_hr, (hex(hr), hex(host_hr), hex(ref_hr), where)
        if ref_hr:
            assert released, ("the result was not released", where)
            failed += 1
            continue
        loaded += 1
        assert (d["meta_equal"], d["pixels_equal"]) == (1, 1), (d, where)
        assert (d["width"], d["height"], d["format"]) == (ref["width"], ref["height"], ref["format"]), where
        payload = ref["width"] * ref["height"] * 4 if ref["ascii"] else ref["nbytes"]
        assert (d["up"], d["down"]) == (payload, 0), (d, where)
    assert failed > 100 and loaded > 100


def _device_save(tmp, px, w, h, fmt, pitch, hdr, out):
    src = os.path.join(tmp, "px.bin")
    px.tofile(src)
    r = subprocess.run([EXE, "device_save", src, str(w), str(h), str(fmt), str(pitch), str(int(hdr)), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    p = r.stdout.split()
    assert p[0] == "hr", r.stdout
    return int(p[1], 16), int(p[2], 16), int(p[3]), int(p[4])


@pytest.mark.parametrize("fmt", [R.RGBA8, R.RGBA8_SRGB, R.BGRA8, R.BGRA8_SRGB, R.BGRX8, R.BGRX8_SRGB, R.RGBA32F, R.RGB32F, R.RGBA16F, R.R32F])
def test_resident_save_is_the_host_writers(tmp_path, oracle, fmt):
    """The file equals the host writer's and the restatement's, and exactly the file's rows came down"""
    hdr = fmt in C.TEXEL_BYTES
    S = C.TEXEL_BYTES.get(fmt, 4)
    for (w, h) in ((7, 5), (64, 4)):
        pitch = w * S + 16
        rng = np.random.default_rng(fmt + w)
        px = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
        out = tmp_path / f"out{w}.pnm"
        hr, host_hr, up, down = _device_save(str(tmp_path), px, w, h, fmt, pitch, hdr, out)
        assert hr == host_hr == 0
        texels = np.ascontiguousarray(px[:, :w * S])
        if hdr:
            dt = np.uint16 if fmt == R.RGBA16F else np.uint32
            want = R.save_pfm(texels.view(dt).reshape(h, w, -1), fmt, C.widen)
        else:
            want = R.save_ppm(texels.reshape(h, w, 4), fmt)
        got, host = open(out, "rb").read(), open(str(out) + ".host", "rb").read()
        assert got == host == want, (fmt, w, h)
        assert (up, down) == (0, w * h * (3 if not hdr else 4 if fmt == R.R32F else 12))


def test_resident_save_refuses_what_the_host_writer_refuses(tmp_path):
    out = tmp_path / "out.pnm"
    px = np.zeros(2 * 2 * 16, np.uint8)
    for fmt, pitch, hdr in ((R.RGBA32F, 32, False), (R.RGBA8, 8, True), (R.R16F, 4, True), (61, 2, False), (49, 4, True)):          # R8_UNORM 61, R8G8_UNORM 49
        hr, host_hr, up, down = _device_save(str(tmp_path), px, 2, 2, fmt, pitch, hdr, out)
        assert hr == host_hr == R.E_NOT_SUPPORTED and not out.exists() and (up, down) == (0, 0), (fmt, hex(hr), hex(host_hr))
