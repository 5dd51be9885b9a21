"""Writes tests/golden/jpeg: small .jpg files from Pillow (libjpeg-turbo, the library the reference calls), each beside Pillow's own decode
of it as <name>.bin - R8 texels for grey, R8G8B8A8 with alpha 0xff for colour - and "<format> <miscFlags2> <width> <height>" as <name>.txt,
what the reader must give with no flags. cmyk.jpg has no .bin: the reader refuses it with E_FAIL.

Run once where Pillow is installed: python tests/golden/make_golden_jpeg.py. The tests read the files and never this script."""
import io
import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg")
R8, RGBA8_SRGB, OPAQUE = 61, 29, 3


def picture(w, h, seed):
    """a gradient with a little noise and one hard edge: every frequency has something to code, and the file stays small"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], axis=-1)
    base[h // 3:, w // 2:] = 255 - base[h // 3:, w // 2:]
    return np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


CASES = {
    # name: (mode, width, height, save options)
    "grey": ("L", 21, 13, dict(quality=85)),
    "c444": ("RGB", 21, 13, dict(quality=85, subsampling=0)),
    "c422": ("RGB", 21, 13, dict(quality=85, subsampling=1)),
    "c420": ("RGB", 21, 13, dict(quality=85, subsampling=2)),
    "c420_wide": ("RGB", 40, 24, dict(quality=75, subsampling=2)),
    "c420_progressive": ("RGB", 21, 13, dict(quality=85, subsampling=2, progressive=True)),
    "c420_optimize": ("RGB", 21, 13, dict(quality=85, subsampling=2, optimize=True)),
    "c420_restart": ("RGB", 37, 19, dict(quality=85, subsampling=2, restart_marker_blocks=2)),
    "cmyk": ("CMYK", 8, 8, dict(quality=75)),
}


def main():
    os.makedirs(OUT, exist_ok=True)
    for seed, (name, (mode, w, h, options)) in enumerate(CASES.items()):
        px = picture(w, h, seed)
        im = Image.fromarray(px[..., 0] if mode == "L" else px)
        if mode == "CMYK":
            im = im.convert("CMYK")
        buf = io.BytesIO()
        im.save(buf, "JPEG", **options)
        data = buf.getvalue()
        assert len(data) <= 4096, (name, len(data))
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        if mode == "CMYK":
            continue
        got = np.asarray(Image.open(io.BytesIO(data)))
        if mode == "L":
            texels, fmt, misc2 = got, R8, 0
        else:
            texels, fmt, misc2 = np.dstack([got, np.full((h, w, 1), 255, np.uint8)]), RGBA8_SRGB, OPAQUE
        texels.astype(np.uint8).tofile(os.path.join(OUT, name + ".bin"))
        with open(os.path.join(OUT, name + ".txt"), "w") as f:
            f.write(f"{fmt} {misc2} {w} {h}\n")


if __name__ == "__main__":
    main()
