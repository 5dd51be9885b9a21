"""Measures the four rows of profiles/copyrect.md on one MI355X (run from the repository root: python tools/copyrect_bench.py).
Median of 20 after 5 warm-up calls; '_ms' = dxtex_ctx_last_kernel_ms (the library's event pair around its kernels), '_wall' = 20 queued
calls + one synchronize, per call - the only clock that covers dxtex_copy_rows_device, which queues a runtime copy and no kernel of ours."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import directxtex_amd as dx
from directxtex_amd import capi
import codec_bench

ctx = dx.Context(0)
med_ms = lambda fn: codec_bench.med_ms(ctx, fn)
wall_ms = lambda fn: codec_bench.wall_ms(ctx, fn)
RGBA8, RGBA16F = 28, 10
N = 8192

src = ctx.device_alloc(N * N * 4); dst = ctx.device_alloc(N * N * 4); dst16 = ctx.device_alloc(N * N * 8)
host = np.random.default_rng(0).integers(0, 256, N * N * 4, dtype=np.uint8)
ctx.upload(src, host, sync=True)
a, b, b16 = capi.device_image(src, N, N, RGBA8), capi.device_image(dst, N, N, RGBA8), capi.device_image(dst16, N, N, RGBA16F)
out = {}
whole = lambda: ctx.copy_rectangles_device([a], [(0, 0, N, N)], [b], [0], [0])
rows = lambda: ctx.copy_rows_device(dst, N * 4, src, N * 4, N * 4, N)
out["whole_copy_rect_ms"] = med_ms(whole); out["whole_copy_rect_wall"] = wall_ms(whole); out["whole_copy_rows_wall"] = wall_ms(rows)
part = lambda: ctx.copy_rectangles_device([a], [(1, 1, 4095, 4095)], [b], [1], [1])
out["rect4095_ms"] = med_ms(part); out["rect4095_wall"] = wall_ms(part)
conv_rect = lambda: ctx.copy_rectangles_device([a], [(0, 0, N, N)], [b16], [0], [0])
conv = lambda: ctx.convert_device(src, N, N, RGBA8, dst16, RGBA16F)
out["convert_copy_rect_ms"] = med_ms(conv_rect); out["convert_device_ms"] = med_ms(conv)
out["convert_copy_rect_wall"] = wall_ms(conv_rect); out["convert_device_wall"] = wall_ms(conv)
F = 2048
cells = [(2, 1), (0, 1), (1, 0), (1, 2), (1, 1), (3, 1)]
faces = [capi.device_image(src + k * F * F * 4, F, F, RGBA8) for k in range(6)]
cross = capi.device_image(dst16, 4 * F, 3 * F, RGBA8)        # 8192 x 6144 x 4 bytes fits the 512 MiB buffer
xs, ys = [c[0] * F for c in cells], [c[1] * F for c in cells]
batch = lambda: ctx.copy_rectangles_device(faces, [(0, 0, F, F)] * 6, [cross] * 6, xs, ys)
def singles():
    for k in range(6): ctx.copy_rectangles_device([faces[k]], [(0, 0, F, F)], [cross], [xs[k]], [ys[k]])
out["cross_batch_ms"] = med_ms(batch); out["cross_batch_wall"] = wall_ms(batch); out["cross_singles_wall"] = wall_ms(singles)
for _ in range(5): singles()
s = []
for _ in range(20):
    t = 0.0
    for k in range(6):
        ctx.copy_rectangles_device([faces[k]], [(0, 0, F, F)], [cross], [xs[k]], [ys[k]]); ctx.synchronize(); t += ctx.last_kernel_ms()
    s.append(t)
out["cross_singles_sum_ms"] = float(np.median(s))
print(json.dumps(out, indent=1))
ctx.close()
