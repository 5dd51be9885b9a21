#!/usr/bin/env python3
"""DEVELOPMENT TOOL: what ComputeNormalMap costs on the GPU. A 4096 x 4096 height map, device-resident (no PCIe), through
dxtex_compute_normal_map_device: R8G8B8A8_UNORM -> R8G8B8A8_UNORM and R32_FLOAT -> R16G16B16A16_FLOAT, each with and without
CNMAP_COMPUTE_OCCLUSION, next to Convert R8G8B8A8_UNORM -> B8G8R8A8_UNORM on the same image (the bandwidth yardstick: one read and
one write of 4 bytes a texel). Kernel time from the context's event pair (dxtex_ctx_last_kernel_ms), median of --reps after one
warm-up, and the effective bandwidth of the algorithmic traffic (source once + destination once). One JSON line per case.
    python tools/nmap_probe.py [--size N] [--reps R]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import directxtex_amd as dx  # noqa: E402

RGBA8, BGRA8, R32F, RGBA16F = 28, 87, 41, 10
LUMINANCE, OCCLUSION = 5, 0x8000


def timed(ctx, fn, reps):
    times = []
    for _ in range(reps + 1):
        fn()
        ctx.synchronize()
        times.append(ctx.last_kernel_ms())
    return float(np.median(times[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    n = a.size
    rng = np.random.default_rng(1)
    ctx = dx.Context(0)
    rgba8 = torch.from_numpy(rng.integers(0, 256, n * n * 4, dtype=np.uint8)).cuda()
    r32f = torch.from_numpy(rng.random(n * n, dtype=np.float32).view(np.uint8)).cuda()
    out = torch.zeros(n * n * 8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = timed(ctx, lambda: ctx.convert_device(rgba8.data_ptr(), n, n, RGBA8, out.data_ptr(), BGRA8), a.reps)
    yard = ms
    print(json.dumps({"case": "convert RGBA8 -> BGRA8 (yardstick)", "size": n, "kernel_ms": round(ms, 4),
                      "GBps": round(n * n * 8 / ms / 1e6, 1)}), flush=True)
    for src, dst, sb, db, name in ((rgba8, RGBA8, 4, 4, "RGBA8 -> RGBA8"), (r32f, RGBA16F, 4, 8, "R32F -> RGBA16F")):
        sfmt = RGBA8 if src is rgba8 else R32F
        for occ in (0, OCCLUSION):
            flags = LUMINANCE | occ
            ms = timed(ctx, lambda: ctx.compute_normal_map_device(src.data_ptr(), n, n, sfmt, out.data_ptr(), dst, flags, 2.0), a.reps)
            print(json.dumps({"case": f"normal map {name}{' occlusion' if occ else ''}", "size": n, "kernel_ms": round(ms, 4),
                              "GBps": round(n * n * (sb + db) / ms / 1e6, 1), "vs_yardstick": round(ms / yard, 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
