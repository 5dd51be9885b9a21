"""texconv's HDR colour rotation without a GPU: the host build of dxtex_rotate.h (directxtex_amd/lib/rotate_check) against the numpy
restatement (tests/rotate_ref.py) bit for bit on the seeded fixture, the condition that makes the fixture a fair one, and dxtexconv's
parsing of --rotate-color and --paper-white-nits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rotate_ref as R  # noqa: E402
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK = os.path.join(LIB, "rotate_check")
EXE = os.path.join(LIB, "dxtexconv")

CASES = [(op, 200.0) for op in range(1, 9)] + [(op, nits) for op in R.HDR10_OPS for nits in (80.0, 10000.0)]
# 2^-20 of an fp32 ulp = 512 double ulps: a double pow within that of the exact result rounds to the same float
MARGIN = 2.0 ** -20


def _apply_host(tmp_path, rows, op, nits):
    if not os.path.exists(CHECK):
        pytest.fail("directxtex_amd/lib/rotate_check is missing: run build()")
    src, dst = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    np.ascontiguousarray(rows, np.float32).tofile(src)
    r = subprocess.run([CHECK, str(op), repr(float(nits)), src, dst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(dst, np.float32).reshape(rows.shape)


@pytest.mark.parametrize("op,nits", CASES)
def test_header_equals_restatement(tmp_path, op, nits):
    rows = R.fixture(R.domain_of(op))
    got = _apply_host(tmp_path, rows, op, nits)
    want = R.apply(rows, op, nits)
    ok = R.same(got, want)
    bad = np.argwhere(~ok)
    assert bad.size == 0, (op, nits, len(bad), bad[:4], got[~ok][:4], want[~ok][:4])
    assert np.array_equal(got[..., 3].view(np.uint32), rows[..., 3].view(np.uint32))          # alpha is moved: its bits survive
    assert np.isnan(want[0, :, :3]).any() and np.isfinite(want[1:, :, :3]).all()          # the specials' row makes NaNs, no other row does


def test_minus_zero_becomes_plus_zero(tmp_path):
    rows = np.array([[-0.0, -0.0, -0.0, -0.0], [0.0, -0.0, 0.0, 1.0]], np.float32)
    for op in (3, 4, 6, 7, 8):
        got = _apply_host(tmp_path, rows, op, 200.0)
        assert (got[:, :3].view(np.uint32) == 0).all(), op
        assert got[0, 3].view(np.uint32) == 0x80000000


def test_the_fixture_is_sound():
    """Every pow the checker evaluates on the fixture lies at least 2^-20 of an fp32 ulp from every fp32 rounding boundary: no value is
    excluded, so float64 pow stands in for the exactly rounded powf on any libm and on the device."""
    n = 0
    for op, nits in CASES:
        if R.PLAN[op][1] == 0:
            continue
        rows = R.fixture(R.domain_of(op))
        m = R.pow_margins(lambda: R.apply(rows, op, nits))
        assert m.size == 2 * rows[..., :3].size
        n += m.size
        assert m.min() >= MARGIN, (op, nits, float(m.min()), int((m < MARGIN).sum()))
    assert n >= 40000


def test_the_gpu_sources_are_sound():
    """The same condition for what the GPU tests feed the kernel: the fixture as each of their formats holds it."""
    for fmt in R.GPU_FORMATS:
        for op, nits in CASES:
            if R.PLAN[op][1] == 0:
                continue
            rows = R.quantised(oracle, R.domain_of(op), fmt)
            m = R.pow_margins(lambda: R.apply(rows, op, nits))
            assert m.min() >= MARGIN, (fmt, op, nits, float(m.min()))


def test_the_tool_sources_are_sound():
    """And for tests/test_rotate_tools_gpu.py's HDR10to709 case, whose halves come from the oracle's Convert of the R10G10B10A2 fixture."""
    import transform_ref as T
    px = T.store_rows(oracle, R.quantised(oracle, "hdr10", 24), 24, R.W * 4)
    half = oracle.ref_convert(px, R.W, R.H, 24, 10, 0, 0.5)
    rows = T.load_rows(oracle, half, R.W, R.H, 10, R.W * 8)
    m = R.pow_margins(lambda: R.apply(rows, 2, 200.0))
    assert m.min() >= MARGIN, float(m.min())


def _run(args):
    return subprocess.run([EXE] + args, capture_output=True, text=True, timeout=60)


@pytest.fixture(scope="module")
def dds(tmp_path_factory):
    d = tmp_path_factory.mktemp("rot")
    rng = np.random.default_rng(2)
    path = str(d / "x.dds")
    oracle.ref_save_dds(rng.integers(0, 256, 8 * 4 * 4, dtype=np.uint8), 8, 4, 28).tofile(path)
    return path


@pytest.mark.parametrize("opts", [["--rotate-color", "709to2020"], ["-rotate-color", "p3d65tohdr10", "--paper-white-nits", "400"],
                                  ["--rotate-color", "HDR10to709", "-paper-white-nits", "10000"], ["-rotate-color", "709TOHDR10"],
                                  ["--rotate-color", "2020to709"], ["--rotate-color", "P3D65to2020"], ["--rotate-color", "709toP3D65"],
                                  ["--rotate-color", "P3D65to709"], ["--paper-white-nits", "0.5"], ["--paper-white-nits", "1e3"],
                                  ["--rotate-color", "709toHDR10", "-tonemap", "-swizzle", "bgr1"]])
def test_rotate_options_are_accepted(dds, opts):
    r = _run(opts + ["-info", dds])
    assert r.returncode == 0, (opts, r.stderr)


@pytest.mark.parametrize("opts", [["--rotate-color", "bogus"], ["-rotate-color", "3"], ["--rotate-color", ""], ["--paper-white-nits", "0"],
                                  ["--paper-white-nits", "10001"], ["--paper-white-nits", "abc"], ["--paper-white-nits", "-5"],
                                  ["--paper-white-nits", "nan"], ["-paper-white-nits", "1e9"], ["--rotate-color"], ["--paper-white-nits"],
                                  ["-rotate-color"], ["-paper-white-nits"]])
def test_rotate_option_errors(dds, opts):
    r = _run(["-o", "x.dds", dds] + opts)
    assert r.returncode == 1 and "usage: dxtexconv" in r.stderr, (opts, r.stderr)
