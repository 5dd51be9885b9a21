"""Measures the rows of profiles/single_plane.md on one MI355X (run from the repository root: python tools/single_plane_bench.py).
Median of 20 after 5 warm-up calls; '_ms' = dxtex_ctx_last_kernel_ms (the library's event pair around its kernels), '_wall' = 20 queued
calls + one synchronize, per call. The same-format mover (dxtex_copy_rectangles_device on a whole 8192 x 8192 YUY2 image, 128 MiB each
way) is timed in the same run, once before each conversion, as the yardstick: time per byte moved (read + written)."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import directxtex_amd as dx
from directxtex_amd import capi
import codec_bench

ctx = dx.Context(0)
med_ms = lambda fn: codec_bench.med_ms(ctx, fn)
wall_ms = lambda fn: codec_bench.wall_ms(ctx, fn)
NV12, P010, YUY2, Y210 = 103, 104, 107, 108
N, F = 8192, 2048
MiB = float(1 << 20)

def planar_pitches(fmt, w, h):
    """ComputePitch of NV12 / P010: rows of w samples, a half-height chroma plane after the luma plane"""
    rp = w * (2 if fmt == P010 else 1)
    return rp, rp * (h + h // 2)

def planar(fmt, w, h, ptr):
    rp, sp = planar_pitches(fmt, w, h)
    return capi.device_image(ptr, w, h, fmt, rp, sp), sp

src_bytes = planar_pitches(P010, N, N)[1]                  # 192 MiB: the largest source
dst_bytes = capi.compute_pitch(Y210, N, N)[1]                 # 256 MiB: the largest destination
src, dst = ctx.device_alloc(src_bytes), ctx.device_alloc(dst_bytes)
host = np.random.default_rng(0).integers(0, 256, src_bytes, dtype=np.uint8)
ctx.upload(src, host, sync=True)

nv12, nv12_bytes = planar(NV12, N, N, src)
p010, p010_bytes = planar(P010, N, N, src)
yuy2, y210 = capi.device_image(dst, N, N, YUY2), capi.device_image(dst, N, N, Y210)
yuy2_bytes, y210_bytes = capi.compute_pitch(YUY2, N, N)[1], capi.compute_pitch(Y210, N, N)[1]
mover_src = capi.device_image(src, N, N, YUY2)

cases = {
    # CopyRectangle counts a YUY2 "texel" as an element of 4 bytes (as the reference does): N / 2 of them are a whole row's 2 N bytes
    "mover_yuy2": (lambda: ctx.copy_rectangles_device([mover_src], [(0, 0, N // 2, N)], [yuy2], [0], [0]), 2 * yuy2_bytes),
    "nv12": (lambda: ctx.convert_to_single_plane_device([nv12], [yuy2]), nv12_bytes + yuy2_bytes),
    "p010": (lambda: ctx.convert_to_single_plane_device([p010], [y210]), p010_bytes + y210_bytes),
}
face_src = planar_pitches(NV12, F, F)[1]
face_dst = capi.compute_pitch(YUY2, F, F)[1]
faces = [planar(NV12, F, F, src + k * face_src)[0] for k in range(6)]
outs = [capi.device_image(dst + k * face_dst, F, F, YUY2) for k in range(6)]
def singles():
    for k in range(6): ctx.convert_to_single_plane_device([faces[k]], [outs[k]])
cases["batch6"] = (lambda: ctx.convert_to_single_plane_device(faces, outs), 6 * (face_src + face_dst))
cases["singles6"] = (singles, 6 * (face_src + face_dst))

out = {}
def measure(name):
    fn, nbytes = cases[name]
    r = {"wall": wall_ms(fn), "ms": med_ms(fn) if name != "singles6" else float("nan"), "MiB": nbytes / MiB}
    r["ns_per_MiB_wall"] = r["wall"] * 1e6 / r["MiB"]
    r["ns_per_MiB_ms"] = r["ms"] * 1e6 / r["MiB"]
    r["TBps"] = nbytes / (r["ms"] * 1e-3) / 1e12
    return r

# alternating: each conversion is timed right after a measurement of the mover of its own, and compared with that one
for name in ("nv12", "p010"):
    mover, conv = measure("mover_yuy2"), measure(name)
    out["mover_before_" + name], out[name] = mover, conv
    out[name + "_vs_mover_kernel"] = conv["ns_per_MiB_ms"] / mover["ns_per_MiB_ms"]
    out[name + "_vs_mover_wall"] = conv["ns_per_MiB_wall"] / mover["ns_per_MiB_wall"]
out["batch6"], out["singles6"] = measure("batch6"), measure("singles6")
out["batch_vs_singles_wall"] = out["batch6"]["wall"] / out["singles6"]["wall"]
print(json.dumps(out, indent=1))
ctx.device_free(src); ctx.device_free(dst)
ctx.close()
