"""The JPEG writer's resident form (SaveToJPEGMemory taking a Device) against the host form of the same build and against libjpeg-turbo's files
(tests/golden/jpeg_write), through tests/cpp/jpeg_write_host_test.cpp: the same bytes, one download of exactly the coefficients and no
upload, one kernel for grey and two for colour, and the blob left empty on failure."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref as R  # noqa: E402
import jpeg_write_ref as W  # noqa: E402
from test_jpeg_write_cpu import HOST, QUALITY_100, fixture_images, golden, save_many  # noqa: E402

pytestmark = pytest.mark.gpu
E_NOT_SUPPORTED = 0x80070032


def test_resident_save_writes_the_fixtures_and_moves_the_coefficients(tmp_path):
    """every quality-100 fixture from each channel order and its _SRGB twin, and noise at sizes with dummy blocks: the host form's bytes and
    libjpeg-turbo's; down exactly the coefficients, nothing up; jpeg_fdct alone for grey, jpeg_samples and jpeg_fdct for colour"""
    images, wants = fixture_images()
    rng = np.random.default_rng(4)
    for w, h in ((9, 5), (64, 19), (72, 48)):
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        images += [(R.R8, px[..., 0], 0), (W.B8G8R8X8, px, 0)]
        wants += [(None, R.R8), (None, W.B8G8R8X8)]
    rows, files = save_many(HOST, str(tmp_path), images, command="device_save_many")
    for p, data, (fmt, px, _), (name, _) in zip(rows, files, images, wants):
        assert int(p[1], 16) == 0 and int(p[2], 16) == 0 and p[3] == "ok", p
        coef_bytes, up, down, equal, launches = map(int, p[4:])
        grey = fmt == R.R8
        assert equal == 1 and (name is None or data == golden(name)), (name, fmt, p)
        assert coef_bytes == R.coefficients(W.encode(px, None if grey else (2, 2))).nbytes and (up, down) == (0, coef_bytes), p
        assert launches == (1 if grey else 2), p
    assert {name for name, _ in wants if name} == set(QUALITY_100)


def test_resident_save_leaves_the_blob_empty_on_failure(tmp_path):
    """R16_UNORM, R8G8_UNORM, R16G16B16A16_UNORM, R32G32B32A32_FLOAT, R8G8B8A8_SNORM and A8_UNORM images on the device: NOT_SUPPORTED from
    both forms, and a blob that held something before is empty"""
    images = [(fmt, np.zeros((8, 8 * size), np.uint8)) for fmt, size in ((56, 2), (49, 2), (11, 8), (2, 16), (31, 4), (65, 1))]          # rows of the format's bytes
    lines = []
    for i, (fmt, rows) in enumerate(images):
        path = tmp_path / f"p{i}.bin"
        rows.tofile(path)
        lines.append(f"{fmt} 8 8 {rows.shape[1]} {path}")
    listing = tmp_path / "list.txt"
    listing.write_text("\n".join(lines) + "\n")
    r = subprocess.run([HOST, "device_save_many", str(listing)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = [line.split() for line in r.stdout.splitlines()]
    assert len(out) == len(images)
    for p in out:
        assert int(p[1], 16) == E_NOT_SUPPORTED and int(p[2], 16) == E_NOT_SUPPORTED and p[3] == "empty", p


def test_download_sizes_are_two_and_three_bytes_a_texel(tmp_path):
    """what the README says about PCIe: at a size of whole MCUs the coefficients are 2 bytes a texel for grey and 3 for colour, where the
    pixels are 1 and 4"""
    w, h = 64, 32
    px = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    rows, _ = save_many(HOST, str(tmp_path), [(R.R8, px[..., 0], 0), (R.RGBA8, px, 0)], command="device_save_many")
    assert [int(p[6]) for p in rows] == [w * h * 2, w * h * 3], rows
