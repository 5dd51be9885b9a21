"""The console formats through the tools and the C++ host layer: dxtexconv's payloads against the reference's Convert / Resize /
GenerateMipMaps (oracle/_ref), and tests/cpp/xbox_host_test for the DeviceScratchImage overloads."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xbox_values as X  # noqa: E402  (also teaches the oracle's size table the four formats)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
EXE = os.path.join(LIB, "dxtexconv")
RGBA16F = 10


def _run(args):
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _payload(path, nbytes):
    return np.fromfile(path, np.uint8)[-nbytes:]


def test_dxtexconv_to_6e4_and_back(tmp_path, oracle):
    w, h = 37, 23
    rng = np.random.default_rng(117)
    img = (rng.random((h, w, 4), dtype=np.float32) * 600.0 - 20.0).astype(np.float16)
    src, mid, out = tmp_path / "in.dds", tmp_path / "mid.dds", tmp_path / "out.dds"
    oracle.ref_save_dds(img, w, h, RGBA16F).tofile(src)
    _run(["-f", "R10G10B10_6E4_A2_FLOAT", "-m", "1", "-o", str(mid), str(src)])
    packed = oracle.ref_convert(img, w, h, RGBA16F, X.F6E4)
    assert np.array_equal(_payload(mid, packed.size), packed)
    _run(["-f", "R16G16B16A16_FLOAT", "-m", "1", "-o", str(out), str(mid)])
    back = oracle.ref_convert(packed, w, h, X.F6E4, RGBA16F)
    assert np.array_equal(_payload(out, back.size), back)


def test_dxtexconv_from_r4g4_with_mips(tmp_path, oracle):
    """a source file in one of the formats through the resize and mip steps: R4G4_UNORM 40 x 24 -> 32 x 16, full cubic chain"""
    w, h = 40, 24
    img = X.random_packed(X.R4G4, w, h, 190)
    src, out = tmp_path / "in.dds", tmp_path / "out.dds"
    oracle.ref_save_dds(img, w, h, X.R4G4).tofile(src)
    _run(["-w", "32", "-h", "16", "-if", "CUBIC", "-m", "0", "-o", str(out), str(src)])
    small = oracle.ref_resize(img, w, h, X.R4G4, 32, 16, 0x300000)
    want = np.concatenate(oracle.ref_generate_mips(small, 32, 16, X.R4G4, 0x300000, 6))
    assert np.array_equal(_payload(out, want.size), want)


def test_host_layer():
    exe = os.path.join(LIB, "xbox_host_test")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} missing: run __graft_entry__.build()")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "xbox host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
