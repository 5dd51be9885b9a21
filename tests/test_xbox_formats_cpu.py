"""The four console formats without a GPU: the 7e3 / 6e4 pack and unpack helpers the kernels call (dxtex_device.h, dxtex_store.h),
compiled for the host into tests/cpp/xbox_check and compared with the reference's own LoadScanline / StoreScanline, the diffusion
chain of the two formats with a dithered store, and dxtexconv's format table and header query."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import xbox_values as X  # noqa: E402

LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK = os.path.join(LIB, "xbox_check")
CONV = os.path.join(LIB, "dxtexconv")
REF = os.path.join(ROOT, "oracle", "_ref", "libdxtex_ref.so")

NAMES = {"R10G10B10_7E3_A2_FLOAT": 116, "R10G10B10_6E4_A2_FLOAT": 117, "R10G10B10_SNORM_A2_UNORM": 189, "R4G4_UNORM": 190}


def _check(args):
    if not os.path.exists(CHECK):
        pytest.fail(f"{CHECK} missing: run __graft_entry__.build()")
    r = subprocess.run([CHECK, REF] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == 2, (r.returncode, r.stdout, r.stderr)
    return [(int(l.split()[1]), int(l.split()[3]), int(l.split()[5])) for l in lines]      # (format, texels, mismatches)


def test_load_every_code(oracle):
    """all 1024 codes in each colour field and the four alpha codes, both formats: 0 mismatches with the reference's LoadScanline"""
    got = _check(["load"])
    assert [g[0] for g in got] == [116, 117] and all(n == 3 * 1024 * 4 and bad == 0 for _, n, bad in got), got


def test_store_edges_and_random(oracle, tmp_path):
    """every representable value, the midpoints with their neighbours, the saturation thresholds, the smallest normals, fp32 denormals,
    zeros, negatives, infinities, 200 000 random positive patterns, and the alpha list: 0 mismatches with the reference's StoreScanline"""
    texels = X.store_texels(X.small_float_values())
    assert texels.shape[0] > 200000 + 8 * 1023
    path = tmp_path / "texels.f32"
    texels.tofile(path)
    got = _check(["store", str(path)])
    assert [g[0] for g in got] == [116, 117] and all(n == texels.shape[0] and bad == 0 for _, n, bad in got), got


def _conv(args):
    return subprocess.run([CONV] + args, capture_output=True, text=True, timeout=60)


def test_dxtexconv_parses_the_format_names(oracle, tmp_path):
    """a name or number the table holds gets past the option parser: no usage text; the run then ends at the missing device or, where
    there is one, converts the file"""
    src = str(tmp_path / "in.dds")
    oracle.ref_save_dds(np.arange(8 * 4 * 4, dtype=np.uint8), 8, 4, 28).tofile(src)
    out = str(tmp_path / "out.dds")
    for name in list(NAMES) + [n.lower() for n in NAMES] + [str(v) for v in NAMES.values()]:
        r = _conv(["-f", name, "-m", "1", "-y", "-o", out, src])
        assert "usage: dxtexconv" not in r.stderr and "unknown" not in r.stderr and "invalid" not in r.stderr, (name, r.stderr)
    r = _conv(["-f", "R10G10B10_7E3_A2", "-o", out, src])
    assert r.returncode == 1 and "usage: dxtexconv" in r.stderr


def test_dxtexconv_info_names_the_formats(oracle, tmp_path):
    """a DDS in each format is no longer 'container only'"""
    files = []
    for name, fmt in NAMES.items():
        w, h = 12, 5
        px = X.random_packed(fmt, w, h, fmt)
        hr, blob = oracle.ref_save_dds_ex(px, w, h, 1, fmt, 1, 1, 0, 0, 3, 0)
        assert hr == 0
        path = str(tmp_path / f"{name}.dds")
        blob.tofile(path)
        files.append((path, name, fmt))
    r = _conv(["-info"] + [f[0] for f in files])
    out = r.stdout.splitlines()
    assert r.returncode == 0 and len(out) == 4, (r.stdout, r.stderr)
    for line, (path, name, fmt) in zip(out, files):
        assert line.startswith(f"{path}: 12x5 2D mips 1 items 1 format {fmt} ") and f" bpp {X.BITS[fmt]} " in line, line
        assert "container only" not in line, line


DITHER_CHECK = os.path.join(LIB, "dither_check")


@pytest.mark.parametrize("fmt", [189, 190])
def test_diffusion_chain_equals_the_reference(oracle, tmp_path, fmt):
    """dither_spec's rows for the two formats with a dithered store, through the host run of the diffusion chain (tests/cpp/dither_check):
    ConvertScanline from R32G32B32A32_FLOAT only clamps to [-1, 1] (189) or [0, 1] (190), before the error row is added; on values
    inside that range it is the identity, which is what dither_check assumes, so the serial chain and the segmented one must both give
    the bytes of the reference's Convert with TEX_FILTER_DITHER_DIFFUSION. (Values outside the range: tests/test_xbox_formats_gpu.py.)"""
    for w, h in [(1, 1), (4, 1), (37, 23), (130, 5)]:
        rng = np.random.default_rng(fmt * 100 + w)
        lo = np.float32(-1.0 if fmt == 189 else 0.0)
        img = (rng.random((h, w, 4)).astype(np.float32) * (np.float32(1.0) - lo) + lo).astype(np.float32)
        ties = rng.random((h, w, 4)) < 0.2
        scale = np.float32(511.0 if fmt == 189 else 15.0)
        img[ties] = np.clip(((np.floor(img[ties] * scale) + np.float32(0.5)) / scale).astype(np.float32), lo, np.float32(1.0))
        special = rng.random((h, w, 4))
        img[special < 0.02] = 1.0
        img[(special >= 0.02) & (special < 0.04)] = lo
        img[(special >= 0.04) & (special < 0.05)] = -0.0
        want = oracle.ref_convert(img, w, h, X.RGBA32F, fmt, 0x20000, 0.5)
        src = tmp_path / "in.f32"
        img.tofile(src)
        for seg in (0, 7):
            out = tmp_path / f"out_{seg}.bin"
            r = subprocess.run([DITHER_CHECK, str(src), str(w), str(h), str(fmt), str(seg), str(out)], capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stderr
            got = np.fromfile(out, np.uint8)
            assert np.array_equal(got, want), (fmt, w, h, seg, np.nonzero(got != want)[0][:8])
