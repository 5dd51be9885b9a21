"""Measures what profiles/png.md reports, on one MI355X (run from the repository root: python tools/png_bench.py).

Kernels: one 4096 x 4096 image through dxtex_png_unpack_device for RGB 8, palette 8 and grey 1 on the wide route, and beside them
pnm_unpack<wide> (P6) and tga_unpack<wide> (24-bit; 8-bit with a palette) on the same byte counts, each REPS times inside one
dxtex_ctx_profile_begin / _end window after a warm-up; per-kernel time and the bytes read and written over it.

The inflater: LoadFromPNGMemoryRaw (tests/cpp/png_host_test.cpp time_raw: chunks, CRC, inflate, unfilter) beside Python's zlib.decompress of
the same stream, five runs each.

End to end: `dxtexconv -nologo -timing -overlap 1 -y` on files this script writes to a temporary directory (numpy filters the rows -
adaptively, the filter of least absolute sum per row - and zlib deflates them at level 6) -
  a 4096^2 RGB 8 .png to -f R8G8B8A8_UNORM -m 1 and to -f BC1_UNORM with the full chain,
  a 2048^2 RGBA 16 .png to -f BC7_UNORM with the full chain,
  a 4096 x 2048 R32G32B32A32_FLOAT DDS to -f R16G16B16A16_UNORM -ft png
- one unmeasured run and five measured ones each; the medians and the bytes moved. The parent commit cannot read these files, so the load
and the save are set beside the same build's host path through the API (png_host_test time_load / time_save): the resident loader against
the host loader plus Upload, the resident saver against Download plus the host saver, alternating, five runs after one unmeasured."""
import argparse, json, os, statistics, subprocess, sys, tempfile, time, zlib
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import directxtex_amd as dx
import png_ref as R
from codec_bench import api_paths, measure_conv, parse_runs, profile_cases

N, REPS, RUNS = 4096, 20, 5
RGBA8, R8 = dx.DXGI_FORMAT_R8G8B8A8_UNORM, dx.DXGI_FORMAT_R8_UNORM


def kernels():
    ctx = dx.Context(0)
    stream = ctx.device_alloc(N * N * 3 + 16)
    image = ctx.device_alloc(N * N * 4)
    for at in range(0, N * N * 3, N * N):
        ctx.upload(stream + at, np.random.default_rng(at).integers(0, 256, N * N, dtype=np.uint8), sync=True)
    img = dx.device_image
    pal = np.random.default_rng(5).integers(0, 2 ** 32, 256, dtype=np.uint32)
    cases = [("png_unpack<wide>", "RGB 8 -> R8G8B8A8", 7, lambda: ctx.png_unpack_device(stream, N * N * 3, dx.PNG_RGB8, img(image, N, N, RGBA8))),
             ("pnm_unpack<wide>", "P6 -> R8G8B8A8, the same bytes", 7, lambda: ctx.pnm_unpack_device(stream, N * N * 3, dx.PNM_P6, img(image, N, N, RGBA8))),
             ("tga_unpack<wide>", "24-bit TGA texels -> R8G8B8A8, the same bytes", 7, lambda: ctx.tga_unpack_device(stream, N * N * 3, 3, img(image, N, N, RGBA8))),
             ("png_unpack<wide>", "palette 8 -> R8G8B8A8 (table in LDS)", 5, lambda: ctx.png_unpack_device(stream, N * N, dx.PNG_P8, img(image, N, N, RGBA8), 0, pal)),
             ("tga_unpack<wide>", "8-bit TGA indices -> R8G8B8A8, the same bytes", 5, lambda: ctx.tga_unpack_device(stream, N * N, 1, img(image, N, N, RGBA8), palette=pal)),
             ("png_unpack<wide>", "grey 1 -> R8 (a byte of the stream a lane)", 1.125, lambda: ctx.png_unpack_device(stream, N * N // 8, dx.PNG_G1, img(image, N, N, R8))),
             ("png_unpack<narrow>", "RGB 8 -> R8G8B8A8, rows one byte off", 7, lambda: ctx.png_unpack_device(stream + 1, N * N * 3, dx.PNG_RGB8, img(image, N, N, RGBA8)))]
    for case in cases:
        try:
            profile_cases(ctx, [case], N * N, REPS)
        except TypeError as e:          # a binding without this form: say so and go on
            print(json.dumps({"kernel": case[0], "case": case[1], "skipped": str(e)}), flush=True)
    ctx.device_free(stream); ctx.device_free(image)
    ctx.close()


def adaptive_png(path, px, ct, depth):
    """px (h, row bytes) uint8 -> a level-6 .png with, per row, the filter of least absolute sum (libpng's heuristic), by numpy"""
    h, rb = px.shape
    bpp = max(1, R.CHANNELS[ct] * depth // 8)
    x = px.astype(np.int16)
    a = np.zeros_like(x); a[:, bpp:] = x[:, :-bpp]
    b = np.zeros_like(x); b[1:] = x[:-1]
    c = np.zeros_like(x); c[1:, bpp:] = x[:-1, :-bpp]
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    cands = [(x - v).astype(np.uint8) for v in (0, a, b, (a + b) >> 1, paeth)]
    cost = np.stack([np.abs(v.view(np.int8).astype(np.int16)).sum(axis=1) for v in cands])
    best = cost.argmin(axis=0)
    stream = np.empty((h, rb + 1), np.uint8)
    stream[:, 0] = best
    for f, v in enumerate(cands):
        stream[best == f, 1:] = v[best == f]
    z = zlib.compress(stream.tobytes(), 6)
    with open(path, "wb") as f:
        f.write(R.SIGNATURE + R.ihdr(px.shape[1] * 8 // (R.CHANNELS[ct] * depth), h, depth, ct) + R.split_idat(z, 1 << 16) + R.chunk(b"IEND"))
    return z, stream.nbytes, np.bincount(best, minlength=5).tolist()


def picture(w, h, channels, rng):
    """smooth gradients with three bits of noise: what a texture source compresses like, roughly"""
    yy, xx = np.mgrid[0:h, 0:w]
    planes = [((xx * (k + 1) // 3 + yy * (4 - k) // 5 + rng.integers(0, 8, (h, w))) & 0xFF).astype(np.uint8) for k in range(channels)]
    return np.stack(planes, axis=2).reshape(h, w * channels)


def end_to_end():
    lib = os.path.dirname(dx.library_path())
    conv, exe = os.path.join(lib, "dxtexconv"), os.path.join(lib, "png_host_test")
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as tmp:
        rgb, rgba16 = os.path.join(tmp, "colour.png"), os.path.join(tmp, "deep.png")
        z, raw, filters = adaptive_png(rgb, picture(N, N, 3, rng), 2, 8)
        print(json.dumps({"file": "4096^2 RGB 8", "bytes": os.path.getsize(rgb), "inflated": raw, "rows by filter": filters}), flush=True)
        z16, raw16, filters16 = adaptive_png(rgba16, picture(N // 2, N // 2, 8, rng), 6, 16)
        print(json.dumps({"file": "2048^2 RGBA 16", "bytes": os.path.getsize(rgba16), "inflated": raw16, "rows by filter": filters16}), flush=True)
        # the inflater beside zlib, on the same stream
        r = subprocess.run([exe, "time_raw", rgb, str(RUNS)], capture_output=True, text=True, check=True)
        ours = [x["raw"] for x in parse_runs(r.stdout)]
        theirs = []
        for _ in range(RUNS):
            t0 = time.perf_counter(); zlib.decompress(z); theirs.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"case": "4096^2 RGB 8: chunks + CRC + inflate + unfilter here, zlib.decompress alone there", "LoadFromPNGMemoryRaw ms": ours,
                          "median": statistics.median(ours), "zlib.decompress ms": [round(v, 1) for v in theirs], "zlib median": round(statistics.median(theirs), 1),
                          "MB/s of inflated bytes": [round(raw / statistics.median(ours) / 1e3), round(raw / statistics.median(theirs) / 1e3)]}), flush=True)
        f32 = os.path.join(tmp, "f32.dds")
        subprocess.run([conv, "-nologo", "-y", "-m", "1", "-w", str(N), "-h", str(N // 2), "-f", "R32G32B32A32_FLOAT", "-o", f32, rgb], check=True, capture_output=True)
        out = os.path.join(tmp, "out.dds")
        cases = [(".png RGB 8 -> -f R8G8B8A8_UNORM -m 1", ["-m", "1", "-f", "R8G8B8A8_UNORM", "-o", out, rgb], out),
                 (".png RGB 8 -> -f BC1_UNORM, full chain", ["-f", "BC1_UNORM", "-o", out, rgb], out),
                 (".png RGBA 16 (2048^2) -> -f BC7_UNORM, full chain", ["-f", "BC7_UNORM", "-o", out, rgba16], out),
                 ("R32G32B32A32_FLOAT DDS (4096 x 2048) -> -f R16G16B16A16_UNORM -ft png", ["-m", "1", "-f", "R16G16B16A16_UNORM", "-ft", "png", "-o", tmp, f32], os.path.join(tmp, "f32.png"))]
        measure_conv(cases, [(None, conv)], RUNS)
        print(json.dumps({"case": "load the RGB 8 .png through the API", **api_paths(exe, "time_load", rgb, RUNS)}), flush=True)
        print(json.dumps({"case": "save the RGB 8 image as .png through the API (R8G8B8A8_UNORM_SRGB -> RGBA 8)", **api_paths(exe, "time_save", rgb, RUNS)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-end-to-end", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernels:
        kernels()
    if not a.skip_end_to_end:
        end_to_end()
