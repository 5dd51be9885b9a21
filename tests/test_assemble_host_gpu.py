"""The host layer's assemble steps on the GPU (DirectXTexAMD_Assemble.cpp) through its C++ driver, tests/cpp/assemble_host_test.cpp: six
seeded 16 x 16 faces into every layout (h-cross, v-cross, h-tee, h-strip, v-strip) and back byte for byte, the background zero; AssembleStrip,
StackArray, StackVolume; CopyRectangle between resident images and on host images (rectangle bytes only over PCIe); MergeImages."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_assemble_steps_on_device():
    exe = os.path.join(ROOT, "directxtex_amd", "lib", "assemble_host_test")
    out = subprocess.run([exe, "gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "assemble_host_test gpu OK" in out.stdout, out.stdout + out.stderr
