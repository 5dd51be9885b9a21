"""What bc7_pre_kernel's election of one-colour subsets rests on: the reference's OptimizeOne, given n copies of
one RGBA8 value and a pair of quantised start endpoints, ends on the same endpoints for every subset size n of the partition
tables. tests/cpp/bc7_solid_check.cpp compiles the reference's D3DX_BC7 in place, as oracle/Makefile does for tools/bc7_debug.cpp,
so the test needs the reference's sources; the encoder's own use of the rule is checked by the host mirror
(tests/test_bc7_core_cpu.py) and on the GPU (tests/test_bc7_solid_alias_gpu.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("REF", "/root/reference")        # as oracle/Makefile
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def test_optimize_one_of_a_one_colour_subset_does_not_depend_on_its_size(tmp_path):
    if not os.path.isdir(os.path.join(REF, "DirectXTex")):
        pytest.skip(f"the reference's sources ({REF}/DirectXTex) are not on this machine")
    exe = str(tmp_path / "bc7_solid_check")
    subprocess.run([CLANG, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-ffp-contract=off", "-fno-fast-math", "-w",
                    "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(REF, "DirectXTex"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "bc7_solid_check.cpp"), "-o", exe,
                    "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath,/opt/rocm/lib"], check=True, timeout=600)
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=900)
    print(r.stdout)
    assert r.returncode == 0 and "20000 inputs" in r.stdout and ": 0 mismatches" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
