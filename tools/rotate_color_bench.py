"""Measures the rotate_color rows of DESIGN.md section 4 on one MI355X (run from the repository root: python tools/rotate_color_bench.py).
One 4096 x 4096 R16G16B16A16_FLOAT image (128 MiB read, 128 MiB written per call) through transform<swizzle> - the memory-bound
yardstick, which moves the same bytes - and through rotate_color on both routes (the texel route by way of a row pitch of 32776 bytes,
no multiple of 16), without a curve (709to2020), to ST.2084 (709toHDR10) and from it (HDR10to709). The calls alternate inside one
dxtex_ctx_profile_begin / _end window, REPS times after a warm-up of each; the figures are the window's per-kernel totals over launches."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import directxtex_amd as dx

N, FMT, REPS = 4096, dx.DXGI_FORMAT_R16G16B16A16_FLOAT, 20
ctx = dx.Context(0)
tight, odd = N * 8, N * 8 + 8
src = ctx.device_alloc(odd * N)
dst = ctx.device_alloc(odd * N)
host = np.random.default_rng(0).random(odd * N // 2, dtype=np.float32).astype(np.float16)
ctx.upload(src, host, sync=True)

def images(rp):
    return [dx.device_image(src, N, N, FMT, rp)], [dx.device_image(dst, N, N, FMT, rp)]

swz = dx.make_transform(dx.TRANSFORM_SWIZZLE, "bgra")
calls = [lambda: ctx.transform_images_device(*images(tight), swz)]
for rp in (tight, odd):
    for op in (dx.ROTATE_709_TO_2020, dx.ROTATE_709_TO_HDR10, dx.ROTATE_HDR10_TO_709):
        calls.append(lambda rp=rp, op=op: ctx.rotate_color_device(*images(rp), op, 200.0))
for c in calls:
    for _ in range(3): c()
ctx.synchronize()
ctx.profile_begin()
for _ in range(REPS):
    for c in calls: c()
prof = ctx.profile_end()
base = prof["transform<swizzle>"][0] / prof["transform<swizzle>"][1]
out = {}
for name, (ms, n) in sorted(prof.items()):
    per = ms / n
    out[name] = {"ms": round(per, 4), "launches": n, "TBps": round(2 * tight * N / (per * 1e-3) / 1e12, 3), "vs_swizzle": round(per / base, 3)}
print(json.dumps(out, indent=1))
ctx.device_free(src); ctx.device_free(dst)
ctx.close()
