"""Shared inputs of the tests for the four console formats (116 R10G10B10_7E3_A2_FLOAT, 117 R10G10B10_6E4_A2_FLOAT,
189 R10G10B10_SNORM_A2_UNORM, 190 R4G4_UNORM): the sizes oracle.dxtex_oracle.BPP lacks, the reference's LoadScanline through ctypes,
packed test images, and the list of R32G32B32A32_FLOAT texels whose stores decide every rounding rule of the four formats. No NaN
anywhere (tests/test_nonfinite_gpu.py says why); +-Inf, -0, negative values and float denormals are in."""
import ctypes

import numpy as np

import oracle.dxtex_oracle as ox

F7E3, F6E4, SN10, R4G4 = 116, 117, 189, 190
XBOX = (F7E3, F6E4, SN10, R4G4)
BITS = {F7E3: 32, F6E4: 32, SN10: 32, R4G4: 8}
RGBA32F = 2

ox.BPP.update(BITS)      # the oracle's table does not know the four; its drivers take any format number


def ref_load(raw, fmt, count):
    """The reference's LoadScanline on `count` texels of `fmt` -> (count, 4) float32."""
    lib = ox._load_ref()
    lib.dxtex_ref_load_scanline.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t]
    lib.dxtex_ref_load_scanline.restype = ctypes.c_int
    raw = np.ascontiguousarray(raw).view(np.uint8).reshape(-1)
    out = np.zeros((count, 4), np.float32)
    assert lib.dxtex_ref_load_scanline(raw.ctypes.data, raw.size, fmt, out.ctypes.data, count) == 0
    return out


def field_image(count):
    """`count` packed 10:10:10:2 words: R runs through all 1024 codes, G is (7 i) mod 1024, B is 1023 - i mod 1024, A is i mod 4."""
    i = np.arange(count, dtype=np.uint32)
    return (i & 1023) | (((7 * i) & 1023) << 10) | (((1023 - (i & 1023)) & 1023) << 20) | ((i & 3) << 30)


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _around(v):
    """each value with its two fp32 neighbours"""
    v = np.asarray(v, np.float32)
    return np.concatenate([np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))])


def small_float_values(seed=116117):
    """The colour values of the 7e3 / 6e4 store test: both formats' representable values, the midpoints between neighbours with the
    floats next to them (the ties decide round-to-nearest-even), both saturation thresholds and clamp maxima, the smallest normals,
    the exponents around the capped denormal shift, fp32 denormals, zeros, negatives, infinities, and 200 000 random positive patterns."""
    parts = []
    for fmt in (F7E3, F6E4):
        rep = ref_load(np.arange(1024, dtype=np.uint32), fmt, 1024)[:, 0]
        assert (np.diff(rep) > 0).all()
        mids = ((rep[:-1].astype(np.float64) + rep[1:].astype(np.float64)) / 2).astype(np.float32)
        assert (mids.astype(np.float64) * 2 == rep[:-1].astype(np.float64) + rep[1:]).all()      # exact in fp32
        parts += [rep, _around(mids)]
    parts.append(_around(_f32([0x41FF73FF, 0x43FEFFFF, 0x3E800000, 0x3C800000])))      # saturation thresholds, smallest normals
    parts.append(_around(np.array([31.875, 508.0], np.float32)))                         # the clamp maxima
    e = np.arange(92, 106, dtype=np.uint32) << 23                                        # shifts of 20 .. 33 (7e3) and 16 .. 29 (6e4): the cap is 24
    parts.append(_f32(np.concatenate([e, e | 0x7FFFFF, e | 0x400000, e | 0x400001, e | 0x3FFFFF])))
    parts.append(_f32([1, 2, 0x00400000, 0x007FFFFF, 0x00800000, 0x00800001]))          # fp32 denormals and the first normals
    parts.append(np.array([0.0, -0.0, -1.0, -0.25, -1e-30, -3.0e38, -np.inf, np.inf, 3.4028234e38, 1e10, 1.0, 0.5], np.float32))
    parts.append(_f32([0x80000001, 0x807FFFFF]))                                         # negative denormals
    rng = np.random.default_rng(seed)
    parts.append(_f32(rng.integers(0, 0x7F800001, 200000).astype(np.uint32)))            # +0 .. +Inf
    v = np.concatenate(parts).astype(np.float32)
    bits = v.view(np.uint32)
    assert not np.isnan(v).any() and np.isinf(v).any() and (v < 0).any() and np.signbit(v[v == 0]).any()
    assert ((v != 0) & (np.abs(v) < np.float32(1.1754944e-38))).any()          # fp32 denormals
    assert all((bits == e).any() for e in (0x41FF73FF, 0x41FF7400, 0x43FEFFFF, 0x43FF0000, 0x3E800000, 0x3E7FFFFF, 0x3C800000, 0x3C7FFFFF))
    return v


def alpha_values():
    """0, 1/3, 2/3 and 1 with their neighbours (alpha truncates in 116 / 117 and rounds to nearest even in 189), the ties of v * 3,
    and values outside [0, 1]."""
    third = np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0], np.float32)
    ties = np.array([1.0 / 6.0, 0.5, 5.0 / 6.0], np.float32)
    out = np.array([-0.0, -0.5, -2.0, 1.5, 2.0, 100.0, -np.inf, np.inf], np.float32)
    return np.concatenate([_around(third), _around(ties), out]).astype(np.float32)


def norm_values():
    """k / 511 and k / 15 with their neighbours and the half-way points (k + 0.5) / 511 and (k + 0.5) / 15, over and beyond the range"""
    k = np.arange(-513, 514, dtype=np.float64)
    n = np.arange(-2, 18, dtype=np.float64)
    return np.concatenate([_around((k / 511).astype(np.float32)), _around(((k + 0.5) / 511).astype(np.float32)),
                           _around((n / 15).astype(np.float32)), _around(((n + 0.5) / 15).astype(np.float32))]).astype(np.float32)


def store_texels(colours):
    """(n, 4) float32 texels: the colour list in r, shifted copies of it in g and b, the alpha list cycling in a"""
    c = np.asarray(colours, np.float32)
    a = alpha_values()
    t = np.empty((c.size, 4), np.float32)
    t[:, 0] = c
    t[:, 1] = np.roll(c, 1)
    t[:, 2] = np.roll(c, 7)
    t[:, 3] = a[np.arange(c.size) % a.size]
    return t


def as_image(texels, width):
    """(n, 4) texels -> (rows, width, 4), the last row filled up with the first texels"""
    n = texels.shape[0]
    rows = (n + width - 1) // width
    return np.concatenate([texels, texels[:rows * width - n]]).reshape(rows, width, 4)


def random_packed(fmt, w, h, seed):
    """a w x h image of `fmt` with every bit random (all bit patterns of the four formats are valid texels)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, w * h * BITS[fmt] // 8, dtype=np.uint8)
