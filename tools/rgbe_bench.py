"""Measures the rgbe rows of DESIGN.md section 4 on one MI355X (run from the repository root: python tools/rgbe_bench.py).
One 4096 x 2048 image. Decode: RGBE (32 MiB) -> R32G32B32A32_FLOAT (128 MiB) on both routes (the narrow one by way of a float pitch of
width * 16 + 4), against dxtex_convert_device R8G8B8A8_UNORM -> R32G32B32A32_FLOAT on the same buffers, which moves the same bytes. Encode:
the three float formats -> RGBE, R32G32B32A32_FLOAT on both routes, against the reverse convert. The calls of a direction alternate inside
one dxtex_ctx_profile_begin / _end window, REPS times after a warm-up of each; the figures are the window's per-kernel totals over
launches. Everything the window recorded that is no rgbe kernel is the yardstick."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import directxtex_amd as dx

W, H, REPS = 4096, 2048, 20
RGBA32F, RGB32F, RGBA16F, RGBA8, RGBE = dx.DXGI_FORMAT_R32G32B32A32_FLOAT, dx.DXGI_FORMAT_R32G32B32_FLOAT, dx.DXGI_FORMAT_R16G16B16A16_FLOAT, dx.DXGI_FORMAT_R8G8B8A8_UNORM, dx.DXGI_FORMAT_R8G8B8A8_UINT
ctx = dx.Context(0)
odd = W * 16 + 4
small = ctx.device_alloc(W * 4 * H)
big = ctx.device_alloc(odd * H)
rng = np.random.default_rng(0)
ctx.upload(small, rng.integers(0, 256, W * 4 * H, dtype=np.uint8), sync=True)


def window(calls):
    for c in calls:
        for _ in range(3): c()
    ctx.synchronize()
    ctx.profile_begin()
    for _ in range(REPS):
        for c in calls: c()
    prof = ctx.profile_end()
    return {k: ms / n for k, (ms, n) in prof.items()}, {k: n for k, (ms, n) in prof.items()}


def report(title, per, launches, moved):
    yard = sum(v for k, v in per.items() if not k.startswith("rgbe_"))
    assert yard > 0, per
    out = {"yardstick": {"kernels": sorted(k for k in per if not k.startswith("rgbe_")), "ms": round(yard, 4), "TBps": round(moved / (yard * 1e-3) / 1e12, 3)}}
    for k in sorted(per):
        if k.startswith("rgbe_"):
            out[k] = {"ms": round(per[k], 4), "launches": launches[k], "vs_yardstick": round(per[k] / yard, 3)}
    print(title, json.dumps(out, indent=1))


# decode: the float side is `big`
img = dx.device_image
per, n = window([lambda: ctx.convert_device(small, W, H, RGBA8, big, RGBA32F),
                 lambda: ctx.rgbe_decode_device(img(small, W, H, RGBE), img(big, W, H, RGBA32F), 1.0),
                 lambda: ctx.rgbe_decode_device(img(small, W, H, RGBE), img(big, W, H, RGBA32F, odd), 1.0)])
report("decode", per, n, W * H * 20)

# encode: finite floats in `big` (RGBE of random bytes decodes to values up to 2^127; halves and the reverse convert take any bits)
ctx.rgbe_decode_device(img(small, W, H, RGBE), img(big, W, H, RGBA32F), 1.0)
per, n = window([lambda: ctx.convert_device(big, W, H, RGBA32F, small, RGBA8),
                 lambda: ctx.rgbe_encode_device(img(big, W, H, RGBA32F), img(small, W, H, RGBE))])
report("encode R32G32B32A32_FLOAT wide", per, n, W * H * 20)
per, n = window([lambda: ctx.convert_device(big, W, H, RGBA32F, small, RGBA8),
                 lambda: ctx.rgbe_encode_device(img(big, W, H, RGBA32F, odd), img(small, W, H, RGBE))])
report("encode R32G32B32A32_FLOAT narrow", per, n, W * H * 20)
per, n = window([lambda: ctx.convert_device(big, W, H, RGBA32F, small, RGBA8),
                 lambda: ctx.rgbe_encode_device(img(big, W, H, RGB32F), img(small, W, H, RGBE))])
report("encode R32G32B32_FLOAT (16 bytes a texel moved)", per, n, W * H * 20)
per, n = window([lambda: ctx.convert_device(big, W, H, RGBA32F, small, RGBA8),
                 lambda: ctx.rgbe_encode_device(img(big, W, H, RGBA16F), img(small, W, H, RGBE))])
report("encode R16G16B16A16_FLOAT wide (12 bytes a texel moved)", per, n, W * H * 20)
ctx.device_free(small); ctx.device_free(big)
ctx.close()
