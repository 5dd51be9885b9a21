"""Measures what profiles/tga.md reports, on one MI355X (run from the repository root: python tools/tga_bench.py [--parent DIR]).

Kernels: one 4096 x 4096 image through dxtex_tga_unpack_device and dxtex_tga_pack_device on both routes (the narrow one by way of a stream
that starts one byte off), REPS times inside one dxtex_ctx_profile_begin / _end window after a warm-up; per-kernel time and the bytes read
and written over it.

End to end: `dxtexconv -nologo -timing -overlap 1 -y` on files this script writes to a temporary directory -
  a 4096^2 24-bit raw .tga and a 4096^2 32-bit run-length .tga, each to -f R8G8B8A8_UNORM -m 1 and to -f BC1_UNORM with the full chain,
  a 4096^2 B8G8R8X8 DDS to -ft tga
- five runs of this build (directxtex_amd/lib/dxtexconv) and, with --parent DIR, five of the dxtexconv in DIR (a build of the parent
commit), alternating. Prints each run's -timing line figures, the medians, the parent's spread (max - min of its five) and whether the two
builds' outputs are byte-identical."""
import argparse, os, struct, subprocess, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import directxtex_amd as dx
from codec_bench import measure_conv, profile_cases

N, REPS, RUNS = 4096, 20, 5
RGBA8, BGRX8, BGRA8, R8 = dx.DXGI_FORMAT_R8G8B8A8_UNORM, dx.DXGI_FORMAT_B8G8R8X8_UNORM, dx.DXGI_FORMAT_B8G8R8A8_UNORM, dx.DXGI_FORMAT_R8_UNORM


def kernels():
    ctx = dx.Context(0)
    stream = ctx.device_alloc(N * N * 4 + 16)
    image = ctx.device_alloc(N * N * 4)
    ctx.upload(stream, np.random.default_rng(0).integers(0, 256, N * N * 4 + 16, dtype=np.uint8), sync=True)
    img = dx.device_image
    palette = np.arange(256, dtype=np.uint32) * 0x010101 | 0xFF000000
    cases = [("tga_unpack<wide>", "24 bits -> R8G8B8A8", 7, lambda: ctx.tga_unpack_device(stream, N * N * 3, 3, img(image, N, N, RGBA8))),
             ("tga_unpack<narrow>", "24 bits -> R8G8B8A8, stream one byte off", 7, lambda: ctx.tga_unpack_device(stream + 1, N * N * 3, 3, img(image, N, N, RGBA8))),
             ("tga_unpack<wide>", "32 bits -> R8G8B8A8 (+ tga_opaque)", 8, lambda: ctx.tga_unpack_device(stream, N * N * 4, 4, img(image, N, N, RGBA8))),
             ("tga_unpack<wide>", "8 bits -> R8", 2, lambda: ctx.tga_unpack_device(stream, N * N, 1, img(image, N, N, R8))),
             ("tga_unpack<wide>", "palette -> R8G8B8A8", 5, lambda: ctx.tga_unpack_device(stream, N * N, 1, img(image, N, N, RGBA8), 0, palette)),
             ("tga_pack<wide>", "B8G8R8X8 -> 24 bits", 7, lambda: ctx.tga_pack_device(img(image, N, N, BGRX8), 3, stream, N * N * 3)),
             ("tga_pack<narrow>", "B8G8R8X8 -> 24 bits, stream one byte off", 7, lambda: ctx.tga_pack_device(img(image, N, N, BGRX8), 3, stream + 1, N * N * 3)),
             ("tga_pack<wide>", "R8G8B8A8 -> 32 bits", 8, lambda: ctx.tga_pack_device(img(image, N, N, RGBA8), 4, stream, N * N * 4))]
    rows = profile_cases(ctx, cases, N * N, REPS)
    ctx.device_free(stream); ctx.device_free(image)
    ctx.close()
    return rows


def tga_header(image_type, bits, descriptor):
    return struct.pack("<BBBHHBHHHHBB", 0, 0, image_type, 0, 0, 0, 0, 0, N, N, bits, descriptor)


def write_inputs(tmp, conv):
    rng = np.random.default_rng(1)
    raw24 = os.path.join(tmp, "raw24.tga")
    with open(raw24, "wb") as f:
        f.write(tga_header(2, 24, 0x00))
        f.write(rng.integers(0, 256, N * N * 3, dtype=np.uint8).tobytes())
    # run-length: every row is 16 pairs of a run packet (128 times one texel) and a raw packet (128 texels)
    rle32 = os.path.join(tmp, "rle32.tga")
    pairs = np.zeros((N, N // 256, 5 + 1 + 512), np.uint8)
    pairs[:, :, 0] = 0xFF
    pairs[:, :, 1:5] = rng.integers(0, 256, (N, N // 256, 4), dtype=np.uint8)
    pairs[:, :, 5] = 0x7F
    pairs[:, :, 6:] = rng.integers(0, 256, (N, N // 256, 512), dtype=np.uint8)
    with open(rle32, "wb") as f:
        f.write(tga_header(10, 32, 0x08))
        f.write(pairs.tobytes())
    bgrx = os.path.join(tmp, "bgrx.dds")
    subprocess.run([conv, "-nologo", "-y", "-m", "1", "-f", "B8G8R8X8_UNORM", "-o", bgrx, raw24], check=True, capture_output=True)
    return raw24, rle32, bgrx


def end_to_end(parent):
    ours = os.path.join(os.path.dirname(dx.library_path()), "dxtexconv")
    builds = [("this build", ours)] + ([("parent", os.path.join(parent, "dxtexconv"))] if parent else [])
    with tempfile.TemporaryDirectory() as tmp:
        raw24, rle32, bgrx = write_inputs(tmp, ours)
        out = os.path.join(tmp, "out.dds")
        cases = [("24-bit raw .tga -> -f R8G8B8A8_UNORM -m 1", ["-m", "1", "-f", "R8G8B8A8_UNORM", "-o", out, raw24], out),
                 ("24-bit raw .tga -> -f BC1_UNORM, full chain", ["-f", "BC1_UNORM", "-o", out, raw24], out),
                 ("32-bit run-length .tga -> -f R8G8B8A8_UNORM -m 1", ["-m", "1", "-f", "R8G8B8A8_UNORM", "-o", out, rle32], out),
                 ("32-bit run-length .tga -> -f BC1_UNORM, full chain", ["-f", "BC1_UNORM", "-o", out, rle32], out),
                 ("B8G8R8X8 DDS -> -ft tga", ["-m", "1", "-ft", "tga", "-o", tmp, bgrx], os.path.join(tmp, "bgrx.tga"))]
        return measure_conv(cases, builds, RUNS)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="directory holding a dxtexconv built from the parent commit (with its libraries beside it)")
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-end-to-end", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernels:
        kernels()
    if not a.skip_end_to_end:
        end_to_end(a.parent)
