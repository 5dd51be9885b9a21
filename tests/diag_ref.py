"""texdiag's Analyze, AnalyzeBC and Difference (Texdiag/texdiag.cpp:698-787, :906-1226, :1285-1309) and ComputeMSE_ with CMSE_FLAGS
(DirectXTexMisc.cpp:27-176) restated in numpy over LoadScanline's floats (oracle.load_image). The yardstick of tests/test_diag_gpu.py
and tests/test_diag_cpu.py: the oracle has no entry for any of the four.

Where the reference's result depends on texel order the restatement takes the rule include/dxtex_amd.h states: a NaN takes no part in
minimum, maximum or luminance, and -0 orders below +0."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
SRGB_FORMATS = {29, 72, 75, 78, 91, 93, 99}
X8_FORMATS = {88, 93}
CMSE_IMAGE1_SRGB, CMSE_IMAGE2_SRGB = 0x1, 0x2
CMSE_IGNORE_RED, CMSE_IGNORE_GREEN, CMSE_IGNORE_BLUE, CMSE_IGNORE_ALPHA = 0x10, 0x20, 0x40, 0x80
CMSE_IMAGE1_X2_BIAS, CMSE_IMAGE2_X2_BIAS = 0x100, 0x200
BC_BLOCK_BYTES = {71: 8, 72: 8, 80: 8, 81: 8, 74: 16, 75: 16, 77: 16, 78: 16, 83: 16, 84: 16, 95: 16, 96: 16, 98: 16, 99: 16}


def key(v):
    """float32 (not NaN) -> uint32 of the same order, -0 below +0."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def luminance(v):
    """XMVector3Dot(v, (0.3, 0.59, 0.11)): (r * 0.3 + g * 0.59) + b * 0.11, every step rounded to fp32."""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        return ((v[..., 0] * F32(0.3) + v[..., 1] * F32(0.59)) + v[..., 2] * F32(0.11)).astype(np.float32)


def lum_bits(v):
    l = luminance(v)
    with np.errstate(invalid="ignore"):
        return np.where(l > 0, l.view(np.uint32), np.uint32(0)).astype(np.uint32)


def analyze(v):
    """v = (..., 4) float32 -> dict of min, max (float32[4]), avg, variance (float64[4]), luminance (float32), specials (uint64[4])."""
    v = np.ascontiguousarray(v, np.float32).reshape(-1, 4)
    n = v.shape[0]
    k = key(v)
    nan = np.isnan(v)
    lo = np.where(nan, np.uint32(0xFFFFFFFF), k).min(axis=0)
    hi = np.where(nan, np.uint32(0), k).max(axis=0)
    lo = np.minimum(lo, key(np.array([FLT_MAX], np.float32))[0])          # minv starts at g_XMFltMax
    hi = np.maximum(hi, key(np.array([-FLT_MAX], np.float32))[0])         # maxv at its negation
    with np.errstate(all="ignore"):
        avg = v.astype(np.float64).sum(axis=0) / n
        d = (v - avg.astype(np.float32)).astype(np.float32)               # XMVectorSubtract(v, avgv) in fp32
        var = (d.astype(np.float64) ** 2).sum(axis=0)
    return {"min": unkey(lo), "max": unkey(hi), "avg": avg, "variance": var,
            "luminance": lum_bits(v).max().astype(np.uint32).reshape(1).view(np.float32)[0],
            "specials": (~np.isfinite(v)).sum(axis=0).astype(np.uint64)}


def mse_implied_flags(fa, fb):
    """the flags ComputeMSE_ adds for the two formats (:47-91)"""
    flags = 0
    if fa in SRGB_FORMATS:
        flags |= CMSE_IMAGE1_SRGB
    if fb in SRGB_FORMATS:
        flags |= CMSE_IMAGE2_SRGB
    if {fa, fb} & X8_FORMATS:
        flags |= CMSE_IGNORE_ALPHA
    return flags


def powf22(v):
    """powf(v, 2.2f) as the reference's libm returns it: the power in float64 rounded once to float32. numpy's own float32 power is a
    vector routine that is up to an ulp off (62 of the 256 values an 8-bit channel loads as), while the reference build's powf
    matches the correctly rounded value on all 256 (seen through oracle.ref_compute_mse on 1 x 1 images); on a single texel that ulp
    is more than the 1e-6 the sums are held to."""
    return np.power(np.asarray(v, np.float32).astype(np.float64), np.float64(F32(2.2))).astype(np.float32)


def mse(va, fa, vb, fb, flags=0):
    """Per-channel MSE in float64 of two (H, W, 4) float32 images as LoadScanline gives them: the reference's fp32 steps before the
    subtraction (powf(v, 2.2f) on r, g, b, then v * 2 - 1 on all four), the subtraction, square and mean in float64."""
    flags |= mse_implied_flags(fa, fb)
    va, vb = np.array(va, np.float32), np.array(vb, np.float32)
    with np.errstate(all="ignore"):
        for v, srgb, bias in ((va, CMSE_IMAGE1_SRGB, CMSE_IMAGE1_X2_BIAS), (vb, CMSE_IMAGE2_SRGB, CMSE_IMAGE2_X2_BIAS)):
            if flags & srgb:
                v[..., :3] = powf22(v[..., :3])
            if flags & bias:
                v[:] = v * F32(2.0) + F32(-1.0)
        d = va.astype(np.float64) - vb.astype(np.float64)
    for c, bit in enumerate((CMSE_IGNORE_RED, CMSE_IGNORE_GREEN, CMSE_IGNORE_BLUE, CMSE_IGNORE_ALPHA)):
        if flags & bit:
            d[..., c] = 0
    return (d * d).reshape(-1, 4).mean(axis=0)


BC6H_BIN = {0x02: 3, 0x06: 4, 0x0A: 5, 0x0E: 6, 0x12: 7, 0x16: 8, 0x1A: 9, 0x1E: 10, 0x03: 11, 0x07: 12, 0x0B: 13, 0x0F: 14}


def bc6h_bin(byte0):
    if byte0 & 3 == 0:
        return 1
    if byte0 & 3 == 1:
        return 2
    return BC6H_BIN.get(byte0 & 0x1F, 0)


def bc7_bin(byte0):
    for m in range(8):
        if byte0 & (1 << m):
            return m
    return 8


def bc_hist(payload, fmt, width, height, row_pitch=None):
    """-> (15 bins as uint64, block count) of the ceil(w / 4) x ceil(h / 4) blocks of a BC image."""
    bb = BC_BLOCK_BYTES[fmt]
    bw, bh = (width + 3) // 4, (height + 3) // 4
    rp = row_pitch or bw * bb
    raw = np.ascontiguousarray(payload).view(np.uint8).reshape(-1)
    blocks = np.stack([raw[y * rp: y * rp + bw * bb] for y in range(bh)]).reshape(bh * bw, bb)
    hist = np.zeros(15, np.uint64)

    def two(a, b, first):          # a > b -> first, else first + 1
        gt = int((a > b).sum())
        hist[first] += gt
        hist[first + 1] += len(a) - gt

    if fmt in (71, 72):
        c = blocks[:, :4].copy().view("<u2")
        le = int((c[:, 0] <= c[:, 1]).sum())
        hist[1] += le
        hist[0] += len(c) - le
    elif fmt in (77, 78, 80):
        two(blocks[:, 0], blocks[:, 1], 0)
    elif fmt == 81:
        two(blocks[:, 0].view(np.int8), blocks[:, 1].view(np.int8), 0)
    elif fmt == 83:
        two(blocks[:, 0], blocks[:, 1], 0)
        two(blocks[:, 8], blocks[:, 9], 2)
    elif fmt == 84:
        two(blocks[:, 0].view(np.int8), blocks[:, 1].view(np.int8), 0)
        two(blocks[:, 8].view(np.int8), blocks[:, 9].view(np.int8), 2)
    elif fmt in (95, 96):
        lut = np.array([bc6h_bin(b) for b in range(256)])
        hist += np.bincount(lut[blocks[:, 0]], minlength=15).astype(np.uint64)
    elif fmt in (98, 99):
        lut = np.array([bc7_bin(b) for b in range(256)])
        hist += np.bincount(lut[blocks[:, 0]], minlength=15).astype(np.uint64)
    return hist, bw * bh


def diff_color(color):
    """XMLoadColor(0x00RRGGBB) with alpha 1: each byte * fl(1 / 255)."""
    s = F32(1.0) / F32(255.0)
    return np.array([F32((color >> 16) & 0xFF) * s, F32((color >> 8) & 0xFF) * s, F32(color & 0xFF) * s, F32(1.0)], np.float32)


def difference(va, vb, color, threshold):
    """Difference's lambda on (..., 4) float32 images -> ((..., 4) float32, mask of the texels that took the colour)."""
    va, vb = np.asarray(va, np.float32), np.asarray(vb, np.float32)
    with np.errstate(all="ignore"):
        d = (va[..., :3] - vb[..., :3]).astype(np.float32)
        n = (F32(0.0) - d).astype(np.float32)
        a = np.where(n > d, n, d)                                         # XMVectorAbs: maxps(0 - v, v)
        hit = (a >= F32(threshold)).all(axis=-1) & bool(color & 0xFFFFFF)
    out = np.ones(va.shape, np.float32)
    out[..., :3] = a
    out[hit] = diff_color(color)
    return out, hit
