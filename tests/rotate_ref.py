"""A numpy fp32 restatement of texconv's HDR colour rotation (Texconv/texconv.cpp:2696-2964), the checker of the rotation tests.

Each operation is stated on (..., 4) float32 rows: what the reference's LoadScanline hands to the lambda and what the lambda hands to
StoreScanline (TransformImage_, DirectXTexMisc.cpp:179-263; StoreScanline's default threshold 0). load_rows() / store_rows() are
tests/transform_ref.py's, the oracle's own compiled LoadScanline / StoreScanline, so only the lambdas are restated here. Every arithmetic
step is one IEEE fp32 numpy operation, in this order:

  XMVector3Transform(v, M)  the oracle's shim does not state it; DirectXMath's SSE2 path as published (no FMA), per output channel k:
                            t = z * M[2][k]; t = t + M[3][k]; t = y * M[1][k] + t; t = x * M[0][k] + t. M[3][k] = +0: the addition turns -0
                            into +0
  to HDR10                  n = transform(v); n = (n * nits) / 10000; LinearToST2084 on x, y, z
  from HDR10                ST2084ToLinear on x, y, z; l = (l * 10000) / nits; transform(l, 2020 -> 709)
  LinearToST2084(v)         p = powf(|v|, 0.1593017578); powf((0.8359375 + 18.8515625 * p) / (1 + 18.6875 * p), 78.84375)
  ST2084ToLinear(v)         p = powf(|v|, 1 / 78.84375); n = p - 0.8359375; n = 0 where n < 0 (std::max: a NaN n stays);
                            powf(n / (18.8515625 - 18.6875 * p), 1 / 0.1593017578); both reciprocals are fp32 divisions

powf is the correctly rounded one: np.power in float64, rounded once to fp32. libm's and MSVC's powf differ from it by 1 ulp on a small
share of values; nothing here is compared with a live powf. pow_margins() says how far every pow the checker evaluates lies from an fp32
rounding boundary, which is what lets a float64 pow of any sane error bound stand in for the exact result (tests/test_rotate_cpu.py).

Alpha is moved. A channel whose arithmetic gives a NaN is a NaN of any payload (the reference's own depends on its compiler's operand
order), so results are compared with same(): equal bits, or a NaN on both sides."""
import numpy as np

import transform_ref as T
from transform_ref import load_rows, store_rows  # noqa: F401  (the oracle's LoadScanline / StoreScanline)

_F = np.float32
TO_HDR10_709, FROM_HDR10_709, TO_2020_709, TO_709_2020, TO_HDR10_P3, TO_2020_P3, TO_P3_709, TO_709_P3 = 1, 2, 3, 4, 5, 6, 7, 8
OPS = {"709toHDR10": 1, "HDR10to709": 2, "709to2020": 3, "2020to709": 4, "P3D65toHDR10": 5, "P3D65to2020": 6, "709toP3D65": 7, "P3D65to709": 8}
HDR10_OPS = (1, 2, 5)

# texconv.cpp:1101-1143, rows 0-2 (row 3 is (0, 0, 0, 1))
M_709_2020 = np.array([[0.6274040, 0.0690970, 0.0163916], [0.3292820, 0.9195400, 0.0880132], [0.0433136, 0.0113612, 0.8955950]], np.float32)
M_2020_709 = np.array([[1.6604910, -0.1245505, -0.0181508], [-0.5876411, 1.1328999, -0.1005789], [-0.0728499, -0.0083494, 1.1187297]], np.float32)
M_P3_2020 = np.array([[0.753845, 0.0457456, -0.00121055], [0.198593, 0.941777, 0.0176041], [0.047562, 0.0124772, 0.983607]], np.float32)
M_709_P3 = np.array([[0.822461969, 0.033194199, 0.017082631], [0.1775380, 0.9668058, 0.0723974], [0.0, 0.0, 0.9105199]], np.float32)
M_P3_709 = np.array([[1.224940176, -0.042056955, -0.019637555], [-0.224940176, 1.042056955, -0.078636046], [0.0, 0.0, 1.098273600]], np.float32)
# op -> (matrix, curve): 0 none, 1 to ST.2084 after the matrix, 2 from ST.2084 before it
PLAN = {1: (M_709_2020, 1), 2: (M_2020_709, 2), 3: (M_709_2020, 0), 4: (M_2020_709, 0), 5: (M_P3_2020, 1), 6: (M_P3_2020, 0), 7: (M_709_P3, 0),
        8: (M_P3_709, 0)}

_margins = None          # a list while pow_margins() records


def _pow(x, y):
    """The correctly rounded powf(x, y): float64 pow rounded once. Records each result's distance from an fp32 rounding boundary."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        r = np.power(x.astype(np.float64), np.float64(_F(y)))
        out = r.astype(np.float32)
    if _margins is not None:
        _margins.append(_boundary_distance(r, out))
    return out


def _boundary_distance(r, f):
    """For float64 values r and their fp32 roundings f: the distance of r from the nearest fp32 rounding boundary (the midpoint of two
    neighbouring floats, or the overflow threshold), in ulps of f. NaN results have no rounding and count as far (inf)."""
    r = np.asarray(r, np.float64).ravel()
    f = np.asarray(f, np.float32).ravel()
    dist = np.full(r.shape, np.inf)
    fin = np.isfinite(r) & np.isfinite(f)
    rf, ff = r[fin], f[fin]
    with np.errstate(all="ignore"):
        up = np.nextafter(ff, _F(np.inf)).astype(np.float64)
        dn = np.nextafter(ff, _F(-np.inf)).astype(np.float64)
    f64 = ff.astype(np.float64)
    up = np.where(np.isfinite(up), up, f64 + 2.0 ** 104)          # above FLT_MAX the next value would be 2^128
    dn = np.where(np.isfinite(dn), dn, f64 - 2.0 ** 104)
    d = rf - f64
    ulp = np.where(d >= 0, up - f64, f64 - dn)                     # spacing on r's side of f
    dist[fin] = (ulp / 2 - np.abs(d)) / ulp
    over = np.isfinite(r) & ~np.isfinite(f)                        # a finite double that rounds to infinity
    fmax = np.float64(np.finfo(np.float32).max)
    dist[over] = (np.abs(r[over]) - (fmax + 2.0 ** 103)) / 2.0 ** 104
    return dist


def pow_margins(fn):
    """Runs fn() and returns the boundary distances (in fp32 ulps) of every pow the checker evaluated meanwhile, as one array."""
    global _margins
    _margins = []
    try:
        fn()
        return np.concatenate(_margins) if _margins else np.zeros(0)
    finally:
        _margins = None


def transform(v, m):
    """XMVector3Transform on (..., 3) fp32 with rows 0-2 of the matrix."""
    x, y, z = v[..., 0], v[..., 1], v[..., 2]
    out = np.empty_like(v)
    with np.errstate(all="ignore"):
        for k in range(3):
            t = z * m[2, k]
            t = t + _F(0.0)
            t = y * m[1, k] + t
            t = x * m[0, k] + t
            out[..., k] = t
    return out


def linear_to_st2084(v):
    with np.errstate(all="ignore"):
        p = _pow(np.abs(v), 0.1593017578)
        return _pow((_F(0.8359375) + _F(18.8515625) * p) / (_F(1.0) + _F(18.6875) * p), 78.84375)


def st2084_to_linear(v):
    with np.errstate(all="ignore"):
        p = _pow(np.abs(v), _F(1.0) / _F(78.84375))
        n = p - _F(0.8359375)
        n = np.where(n < _F(0.0), _F(0.0), n).astype(np.float32)
        return _pow(n / (_F(18.8515625) - _F(18.6875) * p), _F(1.0) / _F(0.1593017578))


def apply(rows, op, nits=200.0):
    """The lambda of op (1..8, texconv's ROTATE_*) on (..., 4) float32 rows."""
    rows = np.asarray(rows, np.float32)
    m, curve = PLAN[op]
    nits = _F(nits)
    v = rows[..., :3].copy()
    with np.errstate(all="ignore"):
        if curve == 2:
            v = (st2084_to_linear(v) * _F(10000.0)) / nits
        v = transform(v, m)
        if curve == 1:
            v = linear_to_st2084((v * nits) / _F(10000.0))
    out = rows.copy()
    out[..., :3] = v
    return out


def same(got, want):
    """Per float: equal bits, or a NaN on both sides."""
    g, w = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))


# ---- the seeded fixture ----------------------------------------------------------------------------------------------------------------
FIXTURE_SEED = 2          # chosen so that test_rotate_cpu.py's two soundness conditions hold (about one seed in two does)
W, H = 67, 45
SPECIAL_BITS = [0x00000000, 0x80000000, 0x00000001, 0x477FE000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000]      # +-0, denormal, 65504, FLT_MAX, +-inf, NaN


def _specials_row():
    s = np.array(SPECIAL_BITS, np.uint32).view(np.float32)
    idx = np.arange(W)
    return np.stack([s[idx % 8], s[(idx // 8 + idx) % 8], s[(idx // 3) % 8], s[(idx + 5) % 8]], -1)


def fixture(domain):
    """(45, 67, 4) float32. "linear" (the linear operations and the two to-HDR10 ones): uniform in [-2, 50]. "hdr10" (HDR10to709): uniform
    in [0, 1], rows 30-37 up to 1.5, rows 38-44 negatives in [-1, 0). Row 0 of both holds the specials."""
    rng = np.random.default_rng(FIXTURE_SEED + (0 if domain == "linear" else 1000))
    if domain == "linear":
        a = rng.uniform(-2.0, 50.0, (H, W, 4)).astype(np.float32)
    else:
        a = rng.uniform(0.0, 1.0, (H, W, 4)).astype(np.float32)
        a[30:38] = rng.uniform(1.0, 1.5, (8, W, 4)).astype(np.float32)
        a[38:] = -rng.uniform(0.0, 1.0, (H - 38, W, 4)).astype(np.float32)
    a[0] = _specials_row()
    return a


def domain_of(op):
    return "hdr10" if op == FROM_HDR10_709 else "linear"


# the formats tests/test_rotate_gpu.py builds its sources in: the six on the quad route of the issue's list, and B5G6R5_UNORM
GPU_FORMATS = [2, 10, 24, 28, 26, 6, 85]
_quantised = {}


def quantised(oracle, domain, fmt):
    """The fixture as an image of fmt holds it: through the oracle's StoreScanline and back through its LoadScanline, until storing it
    again changes nothing. Shared, not to be written to."""
    if (domain, fmt) not in _quantised:
        bpp = {2: 16, 10: 8, 24: 4, 28: 4, 26: 4, 6: 12, 85: 2}[fmt]
        rows = fixture(domain)
        for _ in range(8):          # to a fixed point: the reference's 10-bit store is not idempotent on every value it loads
            before = rows
            rows = T.load_rows(oracle, T.store_rows(oracle, rows, fmt, W * bpp), W, H, fmt, W * bpp)
            if np.array_equal(rows.view(np.uint32), before.view(np.uint32)):
                break
        else:
            raise AssertionError(f"format {fmt}: StoreScanline / LoadScanline did not settle")
        rows.setflags(write=False)
        _quantised[(domain, fmt)] = rows
    return _quantised[(domain, fmt)]
