"""The texel-stream layer under the five file codecs (directxtex_amd/csrc/dxtex_stream.h) on the host:
tests/cpp/stream_check.cpp runs what no codec's own check reaches on its own - texel_of<B> against byte loads, the four-texel three-byte
repack against byte stores, the little-endian loads and stores at every offset between sentinel bytes, the launch grid's arithmetic over
its edge widths, heights and groups, and the alignment predicate over small pointers and pitches. The kernels' use of the same functions
is pinned on the GPU by the codecs' own tests (tests/test_{rgbe,tga,dds,pnm,png}_gpu.py)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "stream_check")


@pytest.mark.parametrize("what", ("texel_of", "pack3x4", "le", "grid", "align"))
def test_stream_layer_piece(what):
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} missing: run __graft_entry__.build()")
    r = subprocess.run([EXE, what], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().endswith(" cases, 0 failures") and not r.stdout.startswith(f"{what}: 0 cases"), r.stdout[-3000:] + r.stderr[-3000:]
