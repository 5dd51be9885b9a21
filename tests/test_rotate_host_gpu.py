"""RotateColor through the C++ host layer (tests/cpp/rotate_host_test.cpp): the Image, array and DeviceScratchImage overloads on a 2-item,
3-mip R16G16B16A16_FLOAT texture against the C ABI's result image by image, the argument checks, and the resident form's transfer
counters: one upload and one download around it, none inside."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "rotate_host_test")


def test_host_layer():
    if not os.path.exists(EXE):
        pytest.fail("directxtex_amd/lib/rotate_host_test is missing: run build()")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "rotate host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
