"""A numpy restatement of the JPEG writer in front of its Huffman coder (csrc/dxtex_jpeg.h's forward functions, csrc/jpeg_encode.hip, the host
SaveToJPEGMemory): libjpeg's RGB -> YCbCr (jccolor.c), edge replication (jcprepct.c), 2x1 / 2x2 chroma average without smoothing
(jcsample.c), JDCT_ISLOW forward DCT (jfdctint.c), quantiser (jcdctmgr.c) and dummy blocks (jccoefct.c). What comes out has the form of
jpeg_ref.decode's result - a frame and each component's quantised coefficients - so jpeg_ref.coefficients and jpeg_ref.pixels take it. Where
Pillow is installed tests/test_jpeg_write_cpu.py holds this file to the coefficients of Pillow's files (libjpeg-turbo, the library the
reference calls), exactly; tests/golden/jpeg_write holds such files for everywhere else.

No sample of an 8-bit image comes near 32 bits, so plain integers give what the wrapping 32-bit arithmetic of dxtex_jpeg.h gives."""
import numpy as np

import jpeg_ref as R

B8G8R8A8, B8G8R8X8, B8G8R8A8_SRGB, B8G8R8X8_SRGB = 87, 88, 91, 93
ONES = np.ones((4, 64), np.uint16)


def ycc(rgb):
    """(h, w, 3) uint8 R, G, B -> (h, w, 3) uint8 Y, Cb, Cr"""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    return np.stack([y, cb, cr], axis=-1).astype(np.uint8)


def plane(comp, hs, vs, bw, bh):
    """a component's block-padded plane, (bh * 8, bw * 8) uint8, from its full-size samples (h, w); hs, vs = the luma factors over its own.
    Full size: the last column and row repeat. Downsampled: hs x vs texels with clamped columns and rows, bias 1, 2, 1, 2 ... across for
    2x2 and 0, 1, 0, 1 ... for 2x1; rows past its own ceil(h / vs) repeat its LAST ROW."""
    h, w = comp.shape
    cy, cx = np.arange(bh * 8), np.arange(bw * 8)
    if hs == 1 and vs == 1:
        return comp[np.ix_(np.minimum(cy, h - 1), np.minimum(cx, w - 1))]
    assert hs == 2 and vs in (1, 2)
    cy = np.minimum(cy, R.ceil_div(h, vs) - 1)
    total = np.zeros((cy.size, cx.size), np.int64)
    for j in range(vs):
        for i in range(hs):
            total += comp[np.ix_(np.minimum(vs * cy + j, h - 1), np.minimum(hs * cx + i, w - 1))]
    bias = (1 if vs == 2 else 0) + (cx & 1)
    return ((total + bias[None, :]) >> vs).astype(np.uint8)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_pass(d, rows):
    """jfdctint.c along the last axis of an int64 array; `rows`: the first pass"""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    shift = 11 if rows else 15
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if rows else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if rows else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    out[2] = _descale(z1 + t13 * 6270, shift)
    out[6] = _descale(z1 - t12 * 15137, shift)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, shift), _descale(t5 + z2 + z4, shift), _descale(t6 + z2 + z3, shift), _descale(t7 + z1 + z4, shift)
    return np.stack(out, axis=-1)


def fdct(blocks):
    """(..., 8, 8) uint8 samples -> (..., 8, 8) int64, 8 times the DCT of the level-shifted block"""
    d = fdct_pass(blocks.astype(np.int64) - 128, True)
    return np.swapaxes(fdct_pass(np.swapaxes(d, -1, -2), False), -1, -2)


def quantise(c, q):
    """the value over 8 q, rounded half away from zero"""
    d = 8 * q.astype(np.int64)
    r = (np.abs(c) + (d >> 1)) // d
    return np.where(c < 0, -r, r)


def split(pixels, fmt):
    """tight rows of `fmt` -> (h, w) grey samples or (h, w, 3) R, G, B"""
    if fmt == R.R8:
        return pixels
    return pixels[..., :3] if fmt in (R.RGBA8, R.RGBA8_SRGB) else pixels[..., 2::-1]


def encode(pixels, sampling=None, quant=ONES, quant_of=(0, 1, 1)):
    """(h, w) uint8 grey samples, or (h, w, 3) R, G, B with sampling = luma (h, v) over 1 x 1 chroma -> what jpeg_ref.decode gives for the
    file libjpeg writes from them: width, height, colour, comps (h, v, tq, bw, bh, dw, dh, coef), quant"""
    pixels = np.asarray(pixels, np.uint8)
    height, width = pixels.shape[:2]
    grey = pixels.ndim == 2
    hmax, vmax = (1, 1) if grey else sampling
    full = [pixels] if grey else [ycc(pixels)[..., i] for i in range(3)]
    quant = np.asarray(quant, np.uint16)
    comps = []
    for i, samples in enumerate(full):
        h, v = (hmax, vmax) if i == 0 else (1, 1)
        bw, bh = R.ceil_div(width, 8 * hmax) * h, R.ceil_div(height, 8 * vmax) * v
        dw, dh = R.ceil_div(width * h, hmax), R.ceil_div(height * v, vmax)
        p = plane(samples, hmax // h, vmax // v, bw, bh)
        blocks = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        coef = quantise(fdct(blocks), quant[quant_of[i]].reshape(8, 8)).reshape(bh, bw, 64)
        # jccoefct.c: a block past the component's own has all AC zero and the DC of the block coded before it in its MCU
        rw, rh = R.ceil_div(dw, 8), R.ceil_div(dh, 8)
        for by in range(bh):
            for bx in range(bw):
                if by < rh and bx < rw:
                    continue
                sy, sx = (by, rw - 1) if by < rh else (rh - 1, min((bx // h) * h + h - 1, rw - 1))
                coef[by, bx, 1:] = 0
                coef[by, bx, 0] = coef[sy, sx, 0]
        comps.append(dict(h=h, v=v, tq=quant_of[i], bw=bw, bh=bh, dw=dw, dh=dh, coef=coef.astype(np.int16)))
    return dict(width=width, height=height, colour=R.GREY if grey else R.YCBCR, progressive=False, comps=comps, quant=[quant[t] for t in range(4)])


def quality_tables(quality):
    """jpeg_set_quality's two tables in natural order, for tests that want a quantiser other than ones"""
    luma = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
    chroma = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    tables = [np.clip((t * scale + 50) // 100, 1, 255) for t in (luma, chroma)]
    return np.array(tables + tables, np.uint16)
