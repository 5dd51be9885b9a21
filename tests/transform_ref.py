"""A numpy fp32 restatement of texconv's per-texel TransformImage lambdas, the checker of the transform tests.

Each op is stated on (N, 4) float32 rows: what the reference's LoadScanline hands to the lambda and what the lambda hands to StoreScanline
(TransformImage_, DirectXTexMisc.cpp:179-263; StoreScanline's default threshold 0). load_rows() / store_rows() are the oracle's own
compiled LoadScanline / StoreScanline (dxtex_ref_load_scanline / dxtex_ref_store_scanline in oracle/_ref/libdxtex_ref.so), so only the
lambdas are restated here. Every arithmetic step is one IEEE fp32 numpy operation in the order of the SSE2 DirectXMath code paths.

DirectXMath is not in the oracle's image, and its shim (oracle/shim) does not state XMLoadColor, XMVector3NearEqual, XMVector2Dot or
XMVectorSqrt. Their shapes below are the SSE2 code paths of DirectXMath as published; they are stated once, here:
  XMLoadColor        (c << shift) * 1 / (255 * 2^shift) per channel = channel * fl(1/255) exactly; alpha of 0x00RRGGBB is 0
  XMVector3NearEqual d = v - key; maxps(0 - d, d) <= eps in x, y and z (maxps(a, b) = a > b ? a : b: b when either is a NaN)
  XMVector2Dot       x * x + y * y
  XMVectorSqrt       sqrtps: correctly rounded, the default NaN for a negative operand
  XMVectorMultiplyAdd  multiply, then add (no FMA on the SSE2 path)
NaNs follow the x86 instructions: an operation on a NaN returns the first NaN operand made quiet; one that makes a NaN from numbers
(0 / 0, inf / inf, sqrt of a negative) returns the default NaN 0xFFC00000. Numpy's own NaN propagation is not relied on: nan_of()
states the rule."""
import ctypes

import numpy as np

_F = np.float32
SWIZZLE, TONEMAP, COLOR_KEY, INVERT_Y, RECONSTRUCT_Z = 0, 1, 2, 3, 4
DEFAULT_NAN = 0xFFC00000


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _isnan(a):
    return (_bits(a) & 0x7FFFFFFF) > 0x7F800000


def _quiet(a):
    return (_bits(a) | 0x00400000).view(np.float32)


def nan_of(r, a, b):
    """The x86 result of an expression r of a (then b): the first NaN input made quiet, else the default NaN where r is a NaN."""
    r = np.array(r, np.float32, copy=True)
    a = np.broadcast_to(np.asarray(a, np.float32), r.shape)
    b = np.broadcast_to(np.asarray(b, np.float32), r.shape)
    gen = _isnan(r) & ~_isnan(a) & ~_isnan(b)
    r[gen] = np.array(DEFAULT_NAN, np.uint32).view(np.float32)
    nb = _isnan(b) & ~_isnan(a)
    r[nb] = _quiet(b[nb])
    na = _isnan(a)
    r[na] = _quiet(a[na])
    return r


def parse_swizzle_mask(mask):
    """texconv's ParseSwizzleMask (texconv.cpp:1157-1248) with the caller's length rule (:1919-1931) -> (swizzle, zero, one) or None."""
    if not mask or len(mask) > 4:                                   # :1921
        return None
    swz, zero, one = [0, 1, 2, 3], [0] * 4, [0] * 4
    for j in range(min(4, len(mask))):                              # :1169-1245
        c = mask[j]
        for k in range(j, 4):
            if c in "RXrx":
                swz[k], zero[k], one[k] = 0, 0, 0
            elif c in "GYgy":
                swz[k], zero[k], one[k] = 1, 0, 0
            elif c in "BZbz":
                swz[k], zero[k], one[k] = 2, 0, 0
            elif c in "AWaw":
                swz[k], zero[k], one[k] = 3, 0, 0
            elif c == "0":
                swz[k], zero[k], one[k] = k, 1, 0
            elif c == "1":
                swz[k], zero[k], one[k] = k, 0, 1
            else:
                return None
    return swz, zero, one


def swizzle(rows, swz, zero, one):
    """texconv.cpp:2662-2673: XMVectorSwizzle, then XMVectorSelect with g_XMZero under zc, then with g_XMOne under oc."""
    rows = np.asarray(rows, np.float32)
    out = rows[..., list(swz)].copy()
    for k in range(4):
        if zero[k]:
            out[..., k] = _F(0.0)
        if one[k]:
            out[..., k] = _F(1.0)
    return out


def max_luminance(rows_list):
    """texconv.cpp:2978-2994: v = XMVector3Dot(p, (0.3, 0.59, 0.11, 0)) = (r * 0.3 + g * 0.59) + b * 0.11 (the shim's order), maxLum =
    XMVectorMax(v, maxLum) from XMVectorZero() over every image: maxps keeps maxLum for a NaN v, and a negative v never wins."""
    m = _F(0.0)
    for rows in rows_list:
        r = np.asarray(rows, np.float32).reshape(-1, 4)
        with np.errstate(all="ignore"):
            v = (r[:, 0] * _F(0.3) + r[:, 1] * _F(0.59)) + r[:, 2] * _F(0.11)
        v = v[~_isnan(v) & (v > 0)]
        if v.size:
            m = max(m, _F(v.max()))
    return _F(m)


def tonemap(rows, m):
    """texconv.cpp:3003-3025: M = m * m; scale = (1 + v / M) / (1 + v); rgb = v * scale (XMVectorSelect 1110), alpha kept."""
    rows = np.asarray(rows, np.float32)
    out = rows.copy()
    M = _F(_F(m) * _F(m))
    with np.errstate(all="ignore"):
        v = rows[..., :3]
        scale = (_F(1.0) + v / M) / (_F(1.0) + v)
        out[..., :3] = nan_of(v * scale, v, np.full_like(v, M))
    return out


def color_key_value(key):
    """XMLoadColor of colorKey & 0xFFFFFF (texconv.cpp:3144): (r, g, b) * fl(1/255), alpha 0."""
    key &= 0xFFFFFF
    s = _F(1.0) / _F(255.0)
    return np.array([_F((key >> 16) & 0xFF) * s, _F((key >> 8) & 0xFF) * s, _F(key & 0xFF) * s], np.float32)


def color_key(rows, key):
    """texconv.cpp:3146-3169: XMVector3NearEqual(v, key, 0.2) -> (0, 0, 0, 0); else alpha = 1."""
    rows = np.asarray(rows, np.float32)
    k = color_key_value(key)
    with np.errstate(all="ignore"):
        d = rows[..., :3] - k
        n = _F(0.0) - d
        mx = np.where(n > d, n, d)                      # maxps(0 - d, d): d when either is a NaN
        match = np.all(mx <= _F(0.2), axis=-1)
    out = rows.copy()
    out[..., 3] = _F(1.0)
    out[match] = _F(0.0)
    return out


def invert_y(rows):
    """texconv.cpp:3205-3217: g = 1 - g (XMVectorSelect 0100)."""
    rows = np.asarray(rows, np.float32)
    out = rows.copy()
    with np.errstate(all="ignore"):
        out[..., 1] = nan_of(_F(1.0) - rows[..., 1], rows[..., 1], _F(0.0))
    return out


def reconstruct_z(rows, unorm):
    """texconv.cpp:3256-3282: UNORM (FormatDataType): x2 = v * 2 + (-1), z = sqrt(1 - (x2.x^2 + x2.y^2)) * 0.5 + 0.5; otherwise
    z = sqrt(1 - (x^2 + y^2)). Only z is written (XMVectorSelect 0010)."""
    rows = np.asarray(rows, np.float32)
    out = rows.copy()
    x, y = rows[..., 0], rows[..., 1]
    with np.errstate(all="ignore"):
        if unorm:
            x2 = x * _F(2.0) + _F(-1.0)
            y2 = y * _F(2.0) + _F(-1.0)
            z = np.sqrt(_F(1.0) - (x2 * x2 + y2 * y2)) * _F(0.5) + _F(0.5)
        else:
            z = np.sqrt(_F(1.0) - (x * x + y * y))
    out[..., 2] = nan_of(z.astype(np.float32), x, y)
    return out


def apply(rows, op, swz=(0, 1, 2, 3), zero=(0, 0, 0, 0), one=(0, 0, 0, 0), key=0, unorm=False, m=0.0):
    if op == SWIZZLE:
        return swizzle(rows, swz, zero, one)
    if op == TONEMAP:
        return tonemap(rows, m)
    if op == COLOR_KEY:
        return color_key(rows, key)
    if op == INVERT_Y:
        return invert_y(rows)
    if op == RECONSTRUCT_Z:
        return reconstruct_z(rows, unorm)
    raise ValueError(op)


# ---- the oracle's LoadScanline / StoreScanline, row by row --------------------------------------------------------------------------
def _lib(oracle):
    lib = oracle.dxtex_oracle._load_ref()
    lib.dxtex_ref_load_scanline.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    lib.dxtex_ref_store_scanline.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float]
    return lib


def load_rows(oracle, data, width, height, fmt, row_pitch):
    """(H, W, 4) float32: the reference's LoadScanline of every row of a tight or padded image."""
    lib = _lib(oracle)
    data = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
    out = np.zeros((height, width, 4), np.float32)
    for y in range(height):
        row = np.ascontiguousarray(data[y * row_pitch:(y + 1) * row_pitch])
        buf = np.zeros((width + 8, 4), np.float32)             # packed formats fill whole elements
        assert lib.dxtex_ref_load_scanline(row.ctypes.data, row.size, fmt, buf.ctypes.data, width) == 0
        out[y] = buf[:width]
    return out


def store_rows(oracle, rows, fmt, row_pitch):
    """The reference's StoreScanline (threshold 0) of (H, W, 4) float32 rows into an image of row_pitch bytes per row."""
    lib = _lib(oracle)
    rows = np.ascontiguousarray(rows, np.float32)
    height, width = rows.shape[:2]
    out = np.zeros(height * row_pitch, np.uint8)
    for y in range(height):
        row = np.zeros(row_pitch, np.uint8)
        r = np.ascontiguousarray(rows[y])
        assert lib.dxtex_ref_store_scanline(row.ctypes.data, row.size, fmt, r.ctypes.data, width, 0.0) == 0
        out[y * row_pitch:(y + 1) * row_pitch] = row
    return out
