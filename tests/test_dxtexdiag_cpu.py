"""dxtexdiag's usage and argument errors: every one is reported before a device is opened, so they run without a GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "dxtexdiag")


def _run(args):
    if not os.path.exists(EXE):
        pytest.fail("directxtex_amd/lib/dxtexdiag is missing: run build()")
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("args,message", [
    ([], "usage: dxtexdiag analyze"),
    (["dumpbc", "a.dds"], "unknown command 'dumpbc'"),
    (["analyze"], "analyze wants at least one file"),
    (["compare", "a.dds"], "compare wants exactly two files"),
    (["compare", "a.dds", "b.dds", "c.dds"], "compare wants exactly two files"),
    (["diff", "a.dds", "b.dds"], "diff wants -o"),
    (["diff", "a.dds", "b.dds", "-o", "out.bmp"], "must be .dds, .tga or .hdr"),
    (["diff", "a.dds", "b.dds", "-o", "out.dds", "-f", "NOT_A_FORMAT"], "invalid value specified with -f"),
    (["diff", "a.dds", "b.dds", "-o", "out.dds", "-if", "SHARP"], "invalid value specified with -if"),
    (["diff", "a.dds", "b.dds", "-o", "out.dds", "-c", "xyz"], "invalid value specified with -c"),
    (["diff", "a.dds", "b.dds", "-o", "out.dds", "-t", "much"], "invalid value specified with -t"),
    (["diff", "a.dds", "b.dds", "-o", "out.dds", "-t"], "-t wants a value"),
    (["analyze", "a.dds", "-bogus"], "unknown option -bogus"),
])
def test_argument_errors(args, message):
    r = _run(args)
    assert r.returncode == 1, r.stdout + r.stderr
    assert message in r.stderr, r.stderr
    assert "usage: dxtexdiag analyze" in r.stderr
    assert "MI355X" not in r.stdout                      # no banner, no device: the arguments are checked first


def test_existing_output_needs_y(tmp_path):
    out = tmp_path / "Out.DDS"
    out.write_bytes(b"x")
    r = _run(["diff", "a.dds", "b.dds", "-o", str(out)])
    assert r.returncode == 1 and "already exists, use -y" in r.stderr
    lowered = tmp_path / "out.dds"
    lowered.write_bytes(b"x")
    r = _run(["diff", "a.dds", "b.dds", "-l", "-o", str(tmp_path / "OUT.dds")])
    assert r.returncode == 1 and str(lowered).lower() in r.stderr      # -l lower-cases the output name before it is checked
