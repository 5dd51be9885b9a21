"""texdiag's per-texel and per-block rules without a GPU: the host build of dxtex_diag.h (directxtex_amd/lib/diag_check) against the numpy
restatement (tests/diag_ref.py), bit for bit, on random and edge inputs; the BC6H / BC7 mode classifier on all 256 values of byte 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import diag_ref as R  # noqa: E402
CHECK = os.path.join(ROOT, "directxtex_amd", "lib", "diag_check")

EDGE_BITS = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000001, 0x80000001, 0x807FFFFF,
             0x3F800000, 0xBF800000, 0x3E800000, 0x3E7FFFFF, 0x3E800001, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F000000]


def _run(*args):
    if not os.path.exists(CHECK):
        pytest.fail("directxtex_amd/lib/diag_check is missing: run build()")
    r = subprocess.run([CHECK] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def _rows(seed, n=20000):
    """Random texels in [-2, 3), a quarter in [0, 1), some of any bit pattern, and every pair of the edge values in (r, g)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-2.0, 3.0, (n, 4)).astype(np.float32)
    a[: n // 4] = rng.random((n // 4, 4), dtype=np.float32)
    a[n // 2: n // 2 + n // 8] = rng.integers(0, 2**32, (n // 8, 4), dtype=np.uint64).astype(np.uint32).view(np.float32)
    e = np.array(EDGE_BITS, np.uint32)
    i, j = np.meshgrid(np.arange(len(e)), np.arange(len(e)), indexing="ij")
    edge = np.stack([e[i.ravel()], e[j.ravel()], e[(i.ravel() + 3) % len(e)], e[(j.ravel() + 5) % len(e)]], -1).view(np.float32)
    return np.concatenate([a, edge])


def _same_bits(got, want):
    g, w = np.ascontiguousarray(got, np.float32).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.nonzero((g != w).reshape(len(g), -1).any(axis=-1))[0]
    assert bad.size == 0, f"{bad.size} rows differ, first {bad[:4]}: got {g[bad[:4]]}, want {w[bad[:4]]}"


def test_luminance_and_keys(tmp_path):
    rows = _rows(1)
    src, dst = str(tmp_path / "in.f32"), str(tmp_path / "out.u32")
    rows.tofile(src)
    _run("texel", src, dst)
    got = np.fromfile(dst, np.uint32).reshape(-1, 5)
    assert np.array_equal(got[:, 0], R.lum_bits(rows))
    ok = ~np.isnan(rows)
    keys = R.key(rows)
    assert np.array_equal(got[:, 1:][ok], keys[ok])
    # the keys order as the floats do, with -0 below +0
    v = rows[ok]
    order = np.argsort(keys[ok], kind="stable")
    s = v[order].astype(np.float64)
    assert (s[1:] >= s[:-1]).all()
    assert R.key(np.float32(-0.0).reshape(1))[0] + 1 == R.key(np.float32(0.0).reshape(1))[0]


def test_min_max_of_cells(tmp_path):
    """The accumulator cells -> the reference's start values: nothing seen, values inside, and values beyond +-FLT_MAX."""
    vals = np.array([0.0, -0.0, 1.5, -2.5, np.inf, -np.inf, R.FLT_MAX, -R.FLT_MAX], np.float32)
    cells = np.zeros((len(vals) + 1, 2), np.uint32)
    cells[1:, 0] = R.key(vals)
    cells[1:, 1] = ~R.key(vals)
    src, dst = str(tmp_path / "in.u32"), str(tmp_path / "out.f32")
    cells.tofile(src)
    _run("minmax", src, dst)
    got = np.fromfile(dst, np.float32).reshape(-1, 2)
    want_max = np.concatenate([[-R.FLT_MAX], np.maximum(vals, -R.FLT_MAX)]).astype(np.float32)
    want_min = np.concatenate([[R.FLT_MAX], np.minimum(vals, R.FLT_MAX)]).astype(np.float32)
    want_max[2] = np.float32(-0.0); want_min[1] = np.float32(0.0)              # np.maximum does not order the zeros; the keys do
    _same_bits(got[:, 0], want_max)
    _same_bits(got[:, 1], want_min)


@pytest.mark.parametrize("color,threshold", [(0, 0.25), (0xFF00FF, 0.25), (0x0000FF, 0.0), (0x102030, 1.0)])
def test_difference_rule(tmp_path, color, threshold):
    a, b = _rows(2), _rows(3)
    b[:4000] = a[:4000] + np.random.default_rng(4).uniform(-0.5, 0.5, (4000, 4)).astype(np.float32)
    pa, pb, dst = str(tmp_path / "a.f32"), str(tmp_path / "b.f32"), str(tmp_path / "out.f32")
    a.tofile(pa); b.tofile(pb)
    _run("diff", f"{color:x}", f"{np.float32(threshold).view(np.uint32):x}", pa, pb, dst)
    want, hit = R.difference(a, b, color, threshold)
    if color:
        assert hit.any() and not hit.all()
    _same_bits(np.fromfile(dst, np.float32).reshape(-1, 4), want)


@pytest.mark.parametrize("srgb,bias", [(0, 1), (1, 0), (1, 1)])
def test_mse_prepare(tmp_path, srgb, bias):
    """v^2.2 on r, g, b then v * 2 - 1 on all four. The power is checked on the values 8-bit channels and halves load as, where numpy's
    powf and the correctly rounded one agree; the bias on any float."""
    rng = np.random.default_rng(5)
    rows = _rows(6) if not srgb else np.concatenate([
        (rng.integers(0, 256, (4096, 4)).astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float32),
        rng.random((4096, 4), dtype=np.float32).astype(np.float16).astype(np.float32)])
    src, dst = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    rows.tofile(src)
    _run("mse", srgb, bias, src, dst)
    got = np.fromfile(dst, np.float32).reshape(-1, 4)
    want = rows.copy()
    with np.errstate(all="ignore"):
        if srgb:
            want[:, :3] = np.power(want[:, :3].astype(np.float64), np.float64(np.float32(2.2))).astype(np.float32)
        if bias:
            want = (want * np.float32(2.0) + np.float32(-1.0)).astype(np.float32)
    ok = ~np.isnan(want).any(axis=1)
    _same_bits(got[ok], want[ok])


def test_gamma22_against_the_reference_powf(tmp_path):
    """dg_gamma22 on the 256 values an 8-bit channel loads as, squared in fp32, against what the reference's ComputeMSE returned for them
    (tests/golden/powf22_squared_u8.txt): evidence that does not come from the code's own formula."""
    golden = np.array([int(l, 16) for l in open(os.path.join(ROOT, "tests", "golden", "powf22_squared_u8.txt")) if not l.startswith("#")], np.uint32)
    assert golden.size == 256
    rows = np.zeros((256, 4), np.float32)
    rows[:, 0] = np.arange(256, dtype=np.float32) * np.float32(1.0 / 255.0)
    src, dst = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    rows.tofile(src)
    _run("mse", 1, 0, src, dst)
    p = np.fromfile(dst, np.float32).reshape(-1, 4)[:, 0]
    assert np.array_equal((p * p).astype(np.float32).view(np.uint32), golden)


def test_bc_mode_classifier_all_bytes():
    lines = [tuple(int(x) for x in l.split()) for l in _run("modes").splitlines()]
    assert [l[0] for l in lines] == list(range(256))
    for b, bc6h, bc7 in lines:
        assert bc6h == R.bc6h_bin(b) and bc7 == R.bc7_bin(b), b
    assert sorted({l[1] for l in lines}) == list(range(15)) and sorted({l[2] for l in lines}) == list(range(9))
    assert sum(1 for l in lines if l[1] == 0) == 4 * 8 and sum(1 for l in lines if l[2] == 8) == 1


@pytest.mark.parametrize("fmt", sorted(R.BC_BLOCK_BYTES))
def test_bc_bins(tmp_path, fmt):
    rng = np.random.default_rng(fmt)
    heads = rng.integers(0, 256, (4096, 16), dtype=np.uint8)
    heads[:64, 1] = heads[:64, 0]; heads[:64, 9] = heads[:64, 8]; heads[:64, 2:4] = heads[:64, 0:2]      # equal endpoints
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.i32")
    heads.tofile(src)
    _run("bc", fmt, src, dst)
    got = np.fromfile(dst, np.int32).reshape(-1, 2)
    hist = np.bincount(got[got >= 0], minlength=15).astype(np.uint64)
    bb = R.BC_BLOCK_BYTES[fmt]
    want, _ = R.bc_hist(np.ascontiguousarray(heads[:, :bb]), fmt, 4 * 4096, 4)
    assert np.array_equal(hist, want), (hist, want)
