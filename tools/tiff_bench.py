"""Times the TIFF codec on one GPU for profiles/tiff.md: writes the files the profile lists with tests/tiff_ref.py, runs
`tiff_host_test time_load` on each (the resident load beside this build's host load plus Upload, the Raw loader alone, the host's serial
undo and the device's kernels of the same stream in the same run) and prints the medians.

    python tools/tiff_bench.py [--runs 5] [--small]"""
import argparse
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tiff_ref as T  # noqa: E402
from codec_bench import parse_runs  # noqa: E402

EXE = os.path.join(ROOT, "directxtex_amd", "lib", "tiff_host_test")


def smooth(h, w, c, top, dtype):
    y, x = np.mgrid[0:h, 0:w]
    rng = np.random.default_rng(1)
    planes = [((np.sin(x / (40.0 + k)) + 1) * (np.cos(y / (60.0 + k)) + 1) / 4 * top + rng.random((h, w)) * top / 256) for k in range(c)]
    return np.stack(planes, 2).clip(0, top).astype(dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="a quarter of the side, for a quick look")
    args = ap.parse_args()
    d = 4 if args.small else 1
    cases = [("rgb8_lzw_p2", T.RGB8, smooth(4096 // d, 4096 // d, 3, 255, np.uint8), dict(compression=T.LZW, predictor=2, rows_per_strip=16)),
             ("grey16_deflate_p2", T.GREY16, smooth(4096 // d, 4096 // d, 1, 65535, np.uint16), dict(compression=T.ADOBE_DEFLATE, predictor=2, rows_per_strip=16)),
             ("rgb32f_deflate_p3", T.RGB32F, smooth(2048 // d, 4096 // d, 3, 1.0, np.float32), dict(compression=T.ADOBE_DEFLATE, predictor=3, rows_per_strip=16))]
    with tempfile.TemporaryDirectory() as tmp:
        for name, kind, samples, kw in cases:
            path = os.path.join(tmp, name + ".tif")
            with open(path, "wb") as f:
                f.write(T.build(samples, kind, **kw))
            r = subprocess.run([EXE, "time_load", path, str(args.runs)], capture_output=True, text=True, timeout=1200)
            if r.returncode:
                print(name, "failed:", r.stderr.strip())
                continue
            cols = {}
            for row in parse_runs(r.stdout):
                for key in ("resident", "up", "host", "raw", "undo", "undo_gpu", "texels_gpu"):
                    cols.setdefault(key, []).append(float(row["resident up" if key == "up" else key]))
            print(name, os.path.getsize(path), "bytes:", ", ".join(f"{k} {statistics.median(v):.3f}" for k, v in cols.items()))


if __name__ == "__main__":
    main()
