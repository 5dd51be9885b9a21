"""FlipRotate and the cross with a turned -Z face through the C++ host layer (tests/cpp/fliprotate_host_test.cpp): the Image, array and
DeviceScratchImage overloads against the C ABI's bytes image by image (which tests/test_fliprotate_gpu.py holds to the restatement), the
metadata of a cube with three mips under ROTATE90, a 6 x 4 x 3 volume under ROTATE270 | FLIP_VERTICAL, the reference's HRESULT order,
release on failure, zero transfer bytes for the resident form, and AssembleCross / CubeFromCross with TEX_FR_ROTATE180."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "fliprotate_host_test")


def test_host_layer():
    if not os.path.exists(EXE):
        pytest.fail("directxtex_amd/lib/fliprotate_host_test is missing: run build()")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fliprotate host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
