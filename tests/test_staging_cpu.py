"""The staging plans of the host-pointer C ABI calls (directxtex_amd/csrc/dxtex_staging.h) on the host: tests/cpp/staging_check.cpp lays
out every traffic shape capi.cpp builds at small sizes, checks the parts' alignment and bounds, every copy against its part, the up and
down totals against their closed forms and the refusal of sizes that overflow, and runs each plan on host memory. The program is built with
AddressSanitizer and UndefinedBehaviorSanitizer; the runner's own use of the header is checked on the GPU (tests/test_staging_gpu.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "staging_check")


def test_plans_stay_inside_their_parts_and_count_their_bytes():
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} missing: run __graft_entry__.build()")
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith("staging plans: 0 failures"), r.stdout[-3000:] + r.stderr[-3000:]
