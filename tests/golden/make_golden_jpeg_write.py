"""Writes tests/golden/jpeg_write: the files Pillow (libjpeg-turbo, the library the reference calls) writes at the reference's settings -
quality 100 and no `subsampling` argument, which is jpeg_set_defaults and jpeg_set_quality(100): grey as one 1 x 1 component, colour at
4:2:0 - each beside its source pixels as <name>.bin: tight rows of R8 samples for grey, of R, G, B bytes for colour. The writer must give
these bytes. The q75_* files have no .bin: they are for the raw writer, which must reproduce them from their own coefficients.

Run once where Pillow is installed: python tests/golden/make_golden_jpeg_write.py. The tests read the files and never this script."""
import io
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_write")


def picture(w, h, seed):
    """a gradient with noise and one hard edge: every frequency has something to code"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], axis=-1)
    base[h // 3:, w // 2:] = 255 - base[h // 3:, w // 2:]
    return np.clip(base + rng.integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)


def extremes(w, h, seed):
    """every channel of every texel 0 or 255: the largest coefficients an 8-bit image gives"""
    return (np.random.default_rng(seed).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)


GREY = ((1, 1), (8, 8), (17, 23))
# 9x9 and 23x41: dummy blocks right and below; 24x24 and 8x24: the repeated downsampled row beside a dummy block row; 40x24: an odd luma
# block count over an even chroma count
COLOUR = ((1, 1), (9, 9), (16, 16), (24, 24), (40, 24), (8, 24), (23, 41), (65, 35))


def save(name, im, **options):
    buf = io.BytesIO()
    im.save(buf, "JPEG", **options)
    data = buf.getvalue()
    assert len(data) <= 16384, (name, len(data))
    with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
        f.write(data)


def main():
    os.makedirs(OUT, exist_ok=True)
    cases = [(f"grey_{w}x{h}", picture(w, h, w * 100 + h)[..., 1]) for w, h in GREY] + [(f"colour_{w}x{h}", picture(w, h, w * 100 + h)) for w, h in COLOUR]
    cases.append(("extremes_33x17", extremes(33, 17, 5)))
    for name, px in cases:
        save(name, Image.fromarray(px), quality=100)
        px.tofile(os.path.join(OUT, name + ".bin"))
    px = picture(21, 13, 7)
    for name, subsampling in (("q75_444", 0), ("q75_422", 1), ("q75_420", 2)):
        save(name, Image.fromarray(px), quality=75, subsampling=subsampling)
    save("q75_grey", Image.fromarray(px[..., 1]), quality=75)


if __name__ == "__main__":
    main()
