"""The JPEG reader's resident form (LoadFromJPEGMemory taking a Device) against the host form of the same build, through
tests/cpp/jpeg_host_test.cpp: pixels and metadata alike, one upload of exactly the coefficients and no download, one kernel for grey and two
for colour, and the output released on failure."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref as R  # noqa: E402
from test_jpeg_cpu import SAMPLINGS, damaged_files, golden, golden_cases, picture  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = os.path.join(ROOT, "directxtex_amd", "lib", "jpeg_host_test")


def _device_load_many(tmp, files):
    lines = []
    for i, (flags, data) in enumerate(files):
        path = os.path.join(tmp, f"f{i}.jpg")
        with open(path, "wb") as f:
            f.write(data)
        lines.append(f"{flags} {path}")
    listing = os.path.join(tmp, "list.txt")
    with open(listing, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([HOST, "device_load_many", listing], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(files)
    return [line.split() for line in out]


def test_resident_load_equals_the_host_load_and_moves_the_coefficients(tmp_path):
    """every golden file and the restatement's own files of every sampling at a width with a tail and at one of whole groups, with and
    without JPEG_FLAGS_DEFAULT_LINEAR: HRESULT, metadata and pixels of the host form; up exactly the coefficients (the quantiser tables
    travel in the kernel's arguments), nothing down; jpeg_idct alone for grey, jpeg_idct and jpeg_colour for colour"""
    files = [(n % 2, golden(name)) for n, name in enumerate(golden_cases()) if name != "cmyk"]
    for kind, sampling in SAMPLINGS.items():
        for w, h in ((9, 5), (64, 19)):
            px = picture(w, h, w)
            files.append((w % 2, R.encode(px[..., 0]) if sampling is None else R.encode(px, sampling, restart=3, jfif=w == 9, adobe=None if w == 9 else 0)))
    for p, (flags, data) in zip(_device_load_many(str(tmp_path), files), files):
        info = R.decode(data)
        assert int(p[1], 16) == 0 and int(p[2], 16) == 0 and p[3] == "ok", p
        width, height, fmt, coef_bytes, up, down, meta_equal, pixels_equal, launches = map(int, p[4:])
        assert (width, height, fmt) == (info["width"], info["height"], R.metadata(info, flags)[0]), p
        assert (meta_equal, pixels_equal) == (1, 1), p
        assert coef_bytes == R.coefficients(info).nbytes and (up, down) == (coef_bytes, 0), p
        assert launches == (1 if info["colour"] == R.GREY else 2), p


def test_resident_load_releases_its_output_on_failure(tmp_path):
    cases = damaged_files()
    files = [(0, data) for data, _ in cases.values()]
    for (name, (data, want)), p in zip(cases.items(), _device_load_many(str(tmp_path), files)):
        assert int(p[1], 16) == want and int(p[2], 16) == want and p[3] == "released", (name, p)


def test_upload_sizes_are_two_three_four_and_six_bytes_a_texel(tmp_path):
    """what the README says about PCIe: at a size of whole MCUs the coefficients are 2 bytes a texel for grey, 3 for 4:2:0, 4 for 4:2:2 and
    6 for 4:4:4 - the last more than the 4 of the decoded pixels"""
    w, h = 64, 32
    px = picture(w, h, 1)
    files = [(0, R.encode(px[..., 0])), (0, R.encode(px, (2, 2))), (0, R.encode(px, (2, 1))), (0, R.encode(px, (1, 1)))]
    ups = [int(p[8]) for p in _device_load_many(str(tmp_path), files)]
    assert ups == [w * h * 2, w * h * 3, w * h * 4, w * h * 6], ups
    assert np.array_equal(ups, [R.coefficients(R.decode(d)).nbytes for _, d in files])
