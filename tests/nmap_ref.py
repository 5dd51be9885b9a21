"""A numpy fp32 restatement of the reference's ComputeNMap (DirectXTexNormalMaps.cpp:77-240), the checker of the normal-map tests.

Every operation is one IEEE fp32 numpy operation in the reference's order (numpy does not fuse or reassociate):
  height  EvaluateColor (:21-47) of LoadScanline's float4 (oracle.load_image); no sRGB decode
  edges   columns / rows wrap; CNMAP_MIRROR_U / _V repeat the edge texel. Row -1 under MIRROR_V is row 0 (the reference's memcpy there,
          :128, is defined only for 16-byte texels with a tight pitch; this is what it means)
  slopes  dzx = (((tL - tR) + (mL - mR)) + (bL - bR)) * amplitude / 6, dzy = (((tL - bL) + (tC - bC)) + (tR - bR)) * amplitude / 6
  normal  XMVector3Normalize(XMVector3Cross((-1, 0, dzx), (0, -1, dzy))), SSE2 shapes
  alpha   1, or the occlusion term (:189-212)
  encode  UNORM: n * (+-0.5) + 0.5; else n or 0 - n (XMVectorNegate) under CNMAP_INVERT_SIGN (:214-229)

nmap_rows() returns the float4 rows handed to StoreScanline: for an R32G32B32A32_FLOAT destination those are the bytes. For the
destinations in IDENTITY_DESTINATIONS, StoreScanline of those rows equals the reference's Convert from R32G32B32A32_FLOAT with
TEX_FILTER_RGB_COPY_RED and threshold 0 (ConvertScanline is the identity there for the values a normal map holds: components in
[-1, 1], UNORM encodings and alpha in [0, 1]; no sRGB, no luminance, no POS_ONLY, depth or video format), so store() goes through
oracle.ref_convert."""
import numpy as np

RGBA32F = 2
TEX_FILTER_RGB_COPY_RED = 0x1000
MIRROR_U, MIRROR_V, INVERT_SIGN, OCCLUSION = 0x1000, 0x2000, 0x4000, 0x8000
UNORM_DESTINATIONS = {28, 87, 11, 24, 35, 49, 61, 56, 65, 85, 86, 115}
SNORM_DESTINATIONS = {31, 13, 51, 37, 63, 58}
FLOAT_DESTINATIONS = {10, 6, 16, 34, 41, 54}
IDENTITY_DESTINATIONS = UNORM_DESTINATIONS | SNORM_DESTINATIONS | FLOAT_DESTINATIONS

_F = np.float32


def heights(rows, flags):
    """EvaluateColor over (H, W, 4) float32 rows."""
    ch = flags & 0xF
    if ch in (0, 1):
        return rows[..., 0]
    if ch in (2, 3, 4):
        return rows[..., ch - 1]
    if ch == 5:
        lr, lg, lb = rows[..., 0] * _F(0.2125), rows[..., 1] * _F(0.7154), rows[..., 2] * _F(0.0721)
        return (lr + lg) + lb
    raise ValueError(f"channel {ch}")


def _edge(n, clamp):
    idx = np.arange(-1, n + 1)
    return np.clip(idx, 0, n - 1) if clamp else np.mod(idx, n)


def nmap_rows(rows, flags, amplitude, unorm):
    """(H, W, 4) float32 LoadScanline rows -> (H, W, 4) float32 rows for StoreScanline."""
    rows = np.asarray(rows, np.float32)
    hgt, wid = rows.shape[:2]
    hm = heights(rows, flags)
    p = hm[np.ix_(_edge(hgt, bool(flags & MIRROR_V)), _edge(wid, bool(flags & MIRROR_U)))]
    t, m, b = p[:-2], p[1:-1], p[2:]
    tl, tc, tr = t[:, :-2], t[:, 1:-1], t[:, 2:]
    ml, mc, mr = m[:, :-2], m[:, 1:-1], m[:, 2:]
    bl, bc, br = b[:, :-2], b[:, 1:-1], b[:, 2:]
    amp = _F(amplitude)
    with np.errstate(all="ignore"):
        dzx = (((tl - tr) + (ml - mr)) + (bl - br)) * amp / _F(6.0)
        dzy = (((tl - bl) + (tc - bc)) + (tr - br)) * amp / _F(6.0)
        zero, neg1 = _F(0.0), _F(-1.0)
        cx = zero * dzy - dzx * neg1
        cy = dzx * zero - neg1 * dzy
        cz = np.full_like(cx, neg1 * neg1 - zero * zero)
        len2 = (cx * cx + cy * cy) + cz * cz
        ln = np.sqrt(len2)
        n = np.stack([cx / ln, cy / ln, cz / ln], -1)
        n[ln == 0] = 0.0
        n[len2 == np.inf] = np.array([0x7FC00000] * 3, np.uint32).view(np.float32)
        alpha = np.ones_like(cx)
        if flags & OCCLUSION:
            delta = np.zeros_like(cx)
            for q in (tl, tc, tr, ml, mr, bl, bc, br):
                d = q - mc
                delta = np.where(d > 0, delta + d, delta)
            delta = delta * (_F(0.125) * amp)
            r = np.sqrt(_F(1.0) + delta * delta)
            alpha = np.where(delta > 0, (r - delta) / r, alpha).astype(np.float32)
        if unorm:
            s = _F(-0.5) if flags & INVERT_SIGN else _F(0.5)
            n = s * n + _F(0.5)
        elif flags & INVERT_SIGN:
            n = zero - n
    return np.concatenate([n, alpha[..., None]], -1).astype(np.float32)


def store(oracle, out_rows, dst_fmt):
    """StoreScanline of the rows into dst_fmt (tight pitch), as bytes."""
    h, w = out_rows.shape[:2]
    flat = np.ascontiguousarray(out_rows, np.float32)
    if dst_fmt == RGBA32F:
        return flat.view(np.uint8).reshape(-1).copy()
    assert dst_fmt in IDENTITY_DESTINATIONS, dst_fmt
    return oracle.ref_convert(flat, w, h, RGBA32F, dst_fmt, TEX_FILTER_RGB_COPY_RED, 0.0)


def compute_normal_map(oracle, pixels, width, height, src_fmt, dst_fmt, flags, amplitude, row_pitch=None):
    """The reference's ComputeNormalMap of one image, restated, for an IDENTITY_DESTINATIONS (or RGBA32F) destination."""
    rows = oracle.load_image(pixels, width, height, src_fmt, row_pitch)
    return store(oracle, nmap_rows(rows, flags, amplitude, dst_fmt in UNORM_DESTINATIONS), dst_fmt)
