"""Writes tests/golden/tiff/: files that Pillow (12.2, with libtiff) encodes, each with Pillow's own decode of it beside it - NAME.bin, the image
as the reader's destination format holds it, and NAME.txt, "width height format". Run from the repository root: python tests/golden/make_golden_tiff.py.
Predictor 2 is asked for through tiffinfo (317) on the 8- and 16-bit LZW and deflate files; predictor 3 is not asked for (libtiff aborts on it here), and Pillow neither writes nor correctly reads RGB 16 or RGB float: tests/tiff_ref.py
builds those."""
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tiff")
R32_FLOAT, R16_UNORM, R8_UNORM, R8G8B8A8_UNORM = 41, 56, 61, 28


def smooth(h, w, c, top, seed):
    """a gradient with a little noise, so that the coders and the predictor have something to do"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    planes = [(x * (k + 3) + y * (5 - k)) * top // (8 * (w + h)) + rng.integers(0, max(2, top // 64), (h, w)) for k in range(c)]
    return np.clip(np.stack(planes, axis=2), 0, top)


def decoded(path):
    """Pillow's decode of the file, as the destination format's bytes"""
    im = Image.open(path)
    im.load()
    if im.mode in ("1", "L"):
        return im.convert("L").tobytes(), R8_UNORM
    if im.mode in ("I;16", "I;16L"):
        return np.asarray(im).astype("<u2").tobytes(), R16_UNORM
    if im.mode == "F":
        return np.asarray(im).astype("<f4").tobytes(), R32_FLOAT
    return im.convert("RGBA").tobytes(), R8G8B8A8_UNORM


def main():
    os.makedirs(OUT, exist_ok=True)
    pal = Image.fromarray(smooth(9, 13, 3, 255, 5).astype(np.uint8), "RGB").quantize(16)
    cases = [
        ("l_raw", Image.fromarray(smooth(9, 11, 1, 255, 1)[:, :, 0].astype(np.uint8), "L"), "raw", {}),
        ("l_packbits", Image.fromarray(smooth(9, 40, 1, 255, 8)[:, :, 0].astype(np.uint8) // 32 * 32, "L"), "packbits", {}),
        ("i16_lzw", Image.fromarray(smooth(10, 21, 1, 65535, 2)[:, :, 0].astype(np.uint16)), "tiff_lzw", {317: 2}),
        ("i16_deflate_rps3", Image.fromarray(smooth(10, 21, 1, 65535, 9)[:, :, 0].astype(np.uint16)), "tiff_adobe_deflate", {278: 3, 317: 2}),
        ("f_deflate", Image.fromarray((smooth(6, 9, 1, 1000, 3)[:, :, 0] / 7.0).astype(np.float32)), "tiff_adobe_deflate", {}),
        ("rgb_lzw_rps4", Image.fromarray(smooth(9, 7, 3, 255, 4).astype(np.uint8), "RGB"), "tiff_lzw", {278: 4, 317: 2}),
        ("rgb_lzw_wide", Image.fromarray(smooth(3, 300, 3, 255, 10).astype(np.uint8), "RGB"), "tiff_lzw", {317: 2}),
        ("rgba_packbits", Image.fromarray(smooth(5, 12, 4, 255, 6).astype(np.uint8), "RGBA"), "packbits", {}),
        ("rgba_deflate", Image.fromarray(smooth(8, 17, 4, 255, 11).astype(np.uint8), "RGBA"), "tiff_adobe_deflate", {317: 2}),
        ("bilevel_raw", Image.fromarray((smooth(7, 19, 1, 255, 7)[:, :, 0] > 100).astype(np.uint8) * 255, "L").convert("1"), "raw", {}),
        ("p_lzw", pal, "tiff_lzw", {}),
    ]
    for name, im, compression, info in cases:
        path = os.path.join(OUT, name + ".tif")
        im.save(path, format="TIFF", compression=compression, tiffinfo=info)
        assert os.path.getsize(path) <= 8192, (name, os.path.getsize(path))
        px, fmt = decoded(path)
        with open(os.path.join(OUT, name + ".bin"), "wb") as f:
            f.write(px)
        with open(os.path.join(OUT, name + ".txt"), "w") as f:
            f.write("%d %d %d\n" % (im.width, im.height, fmt))


if __name__ == "__main__":
    main()
