"""search_common.h at kernel level: wave_prefix_min, selection_pass, the task sort's three kernels and queue_take against serial rules, by
tests/cpp/search_prims_gpu_test.hip - one translation unit that includes the header, so the kernels are the encoders' own text. The program runs
once, in a process of its own; it stops at the first HIP error, and the four groups report here one by one. Everything is integer and exact.
What the sort is asked: the histogram, the live count, every live task once as (t, tinfo[t]), sizes that do not rise, bin ends, nothing
written beyond the live entries - and no position inside a bin. What the queue is asked: every index below `live` handed out once, none beyond."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "search_prims_gpu_test")
# the least each group must have run: the minimum lanes and key orders of prefix_min (4 + 8), 4 096 selections, 7 list lengths x 9 families
# ungated plus the gate's closed and open states at every length, 9 list lengths x 3 wave counts of the queue
MIN_CASES = {"prefix_min": 12, "selection": 4096, "bin_sort": 7 * 9 + 7 * 2, "queue": 9 * 3}


@pytest.fixture(scope="module")
def groups():
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} missing: run __graft_entry__.build()")
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-4000:])
    out = {}
    for line in r.stdout.splitlines():
        m = re.match(r"group (\w+) cases (\d+) failed (\d+) first-bad (.*)", line)
        if m:
            out[m.group(1)] = (int(m.group(2)), int(m.group(3)), m.group(4))
    return r.returncode, r.stdout[-3000:], out


@pytest.mark.parametrize("name", list(MIN_CASES))
def test_group(groups, name):
    code, tail, out = groups
    assert name in out, f"group {name} did not report (exit status {code}):\n{tail}"
    cases, failed, first_bad = out[name]
    assert failed == 0, f"{name}: {failed} of {cases} cases failed, first {first_bad}"
    assert cases >= MIN_CASES[name], f"{name}: {cases} cases, fewer than {MIN_CASES[name]}"


def test_exit_status(groups):
    code, tail, out = groups
    assert code == 0 and set(out) == set(MIN_CASES), tail
