#!/usr/bin/env python3
"""DEVELOPMENT TOOL: what the dithered Convert costs. A 4096 x 4096 RGBA32F image (smooth gradients plus noise, some values out of
range) into R8G8B8A8_UNORM and B5G6R5_UNORM four ways: undithered, ordered (TEX_FILTER_DITHER) and error diffusion
(TEX_FILTER_DITHER_DIFFUSION) on the GPU through dxtex_convert_device (kernel time, median of --reps, device-resident: no PCIe), and
the reference's own Convert with diffusion on the host cores (oracle.ref_convert; one run, wall time). Also prints the share of
texels the exact merge of the diffusion kernel re-ran (dxtex_convert_dither_stats), and checks the diffusion bytes against the
reference. One JSON line per destination format.
    python tools/dither_probe.py [--size N] [--reps R] [--flat] [--dev]
--dev loads libdxtex_amd_dev.so, whose DXTEX_DITHER_SEGMENT sets the texels per speculated segment (e.g. to sweep it)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import directxtex_amd as dx  # noqa: E402

RGBA32F, ORDERED, DIFFUSION = 2, 0x10000, 0x20000


def image(n, flat):
    if flat:
        return np.full((n, n, 4), 0.4123, np.float32)
    y, x = np.mgrid[0:n, 0:n].astype(np.float32) / np.float32(n)
    rng = np.random.default_rng(1)
    img = np.stack([x, y, (x + y) * 0.5, 1.0 - x * y], axis=-1) * np.float32(1.1) - np.float32(0.05)
    return (img + rng.normal(0, 0.02, img.shape).astype(np.float32)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--flat", action="store_true", help="one value everywhere (the merge's worst case)")
    ap.add_argument("--dev", action="store_true", help="use the development library (reads DXTEX_DITHER_SEGMENT)")
    a = ap.parse_args()
    if a.dev:
        from directxtex_amd import capi
        capi.load(dev=True)
    n = a.size
    img = image(n, a.flat)
    ctx = dx.Context(0)
    d_src = torch.from_numpy(img.reshape(-1).view(np.uint8).copy()).cuda()
    for dst, name, bpt in ((28, "R8G8B8A8_UNORM", 4), (85, "B5G6R5_UNORM", 2)):
        d_dst = torch.zeros(n * n * bpt, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        res = {"image": f"{n}x{n} RGBA32F{' flat' if a.flat else ''}", "dst": name, "segment": os.environ.get("DXTEX_DITHER_SEGMENT", "default") if a.dev else "default"}
        for label, flags in (("undithered", 0), ("ordered", ORDERED), ("diffusion", DIFFUSION)):
            times = []
            r0 = ctx.convert_dither_stats()
            for _ in range(a.reps + 1):
                ctx.convert_device(d_src.data_ptr(), n, n, RGBA32F, d_dst.data_ptr(), dst, flags, 0.5)
                ctx.synchronize()
                times.append(ctx.last_kernel_ms())
            res[f"{label}_ms"] = round(float(np.median(times[1:])), 3)
            if flags == DIFFUSION:
                r1 = ctx.convert_dither_stats()
                res["merge_rerun_share"] = round((r1[0] - r0[0]) / max(1, r1[1] - r0[1]), 4)
                gpu_bytes = d_dst.cpu().numpy()
        try:
            import oracle
            if oracle.have_ref():
                t0 = time.perf_counter()
                ref = oracle.ref_convert(img, n, n, RGBA32F, dst, DIFFUSION, 0.5)
                res["reference_cpu_diffusion_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
                res["diffusion_identical"] = bool(np.array_equal(ref, gpu_bytes))
        except ImportError:
            pass
        print(json.dumps(res), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
