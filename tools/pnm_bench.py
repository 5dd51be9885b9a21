"""Measures what profiles/pnm.md reports, on one MI355X (run from the repository root: python tools/pnm_bench.py).

Kernels: one 4096 x 4096 image through dxtex_pnm_unpack_device and dxtex_pnm_pack_device for P6, PF and PH on both routes (the narrow one by
way of samples that start one byte off), and beside them tga_unpack<wide> on 24-bit texels and dds_unpack<888,wide> on the same image size,
each REPS times inside one dxtex_ctx_profile_begin / _end window after a warm-up; per-kernel time and the bytes read and written over it.

End to end: `dxtexconv -nologo -timing -overlap 1 -y` on files this script writes to a temporary directory -
  a 4096^2 .ppm to -f R8G8B8A8_UNORM -m 1 and to -f BC1_UNORM with the full chain,
  a 4096 x 2048 .pfm to -f BC6H_UF16 with the full chain,
  a 4096 x 2048 R32G32B32A32_FLOAT DDS to -ft pfm
- one unmeasured run and five measured ones each; the medians and the bytes moved. The parent commit cannot read these files, so each case
is set beside the same build's host path through the API (tests/cpp/pnm_host_test.cpp time_load / time_save): the resident loader against
the host loader plus Upload, the resident saver against Download plus the host saver, alternating, five runs after one unmeasured."""
import argparse, json, os, subprocess, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import directxtex_amd as dx
from codec_bench import api_paths, measure_conv, profile_cases

N, REPS, RUNS = 4096, 20, 5
RGBA8, BGRX8, RGBA32F, RGBA16F = dx.DXGI_FORMAT_R8G8B8A8_UNORM, dx.DXGI_FORMAT_B8G8R8X8_UNORM, dx.DXGI_FORMAT_R32G32B32A32_FLOAT, dx.DXGI_FORMAT_R16G16B16A16_FLOAT


def kernels():
    ctx = dx.Context(0)
    stream = ctx.device_alloc(N * N * 12 + 16)
    image = ctx.device_alloc(N * N * 16)
    for at in range(0, N * N * 12, N * N * 4):
        ctx.upload(stream + at, np.random.default_rng(at).integers(0, 256, N * N * 4, dtype=np.uint8), sync=True)
    img = dx.device_image
    cases = [("tga_unpack<wide>", "24-bit TGA texels -> R8G8B8A8", 7, lambda: ctx.tga_unpack_device(stream, N * N * 3, 3, img(image, N, N, RGBA8))),
             ("dds_unpack<888,wide>", "24-bit DDS texels -> R8G8B8A8", 7, lambda: ctx.dds_unpack_device(stream, N * N * 3, dx.DDS_ROW_888, [img(image, N, N, RGBA8)], [0], [N * 3])),
             ("pnm_unpack<wide>", "P6 -> R8G8B8A8, maxval 255", 7, lambda: ctx.pnm_unpack_device(stream, N * N * 3, dx.PNM_P6, img(image, N, N, RGBA8))),
             ("pnm_unpack<wide>", "P6 -> R8G8B8A8, maxval 100 (table in LDS)", 7, lambda: ctx.pnm_unpack_device(stream, N * N * 3, dx.PNM_P6, img(image, N, N, RGBA8), 100)),
             ("pnm_unpack<narrow>", "P6 -> R8G8B8A8, samples one byte off", 7, lambda: ctx.pnm_unpack_device(stream + 1, N * N * 3, dx.PNM_P6, img(image, N, N, RGBA8))),
             ("pnm_unpack<wide>", "PF -> R32G32B32A32_FLOAT", 28, lambda: ctx.pnm_unpack_device(stream, N * N * 12, dx.PNM_PF, img(image, N, N, RGBA32F))),
             ("pnm_unpack<wide>", "PF big-endian -> R32G32B32A32_FLOAT", 28, lambda: ctx.pnm_unpack_device(stream, N * N * 12, dx.PNM_PF, img(image, N, N, RGBA32F), 255, dx.PNM_BIG_ENDIAN)),
             ("pnm_unpack<narrow>", "PF -> R32G32B32A32_FLOAT, samples one byte off", 28, lambda: ctx.pnm_unpack_device(stream + 1, N * N * 12, dx.PNM_PF, img(image, N, N, RGBA32F))),
             ("pnm_unpack<wide>", "PH -> R16G16B16A16_FLOAT", 14, lambda: ctx.pnm_unpack_device(stream, N * N * 6, dx.PNM_PH, img(image, N, N, RGBA16F))),
             ("pnm_unpack<narrow>", "PH -> R16G16B16A16_FLOAT, samples one byte off", 14, lambda: ctx.pnm_unpack_device(stream + 1, N * N * 6, dx.PNM_PH, img(image, N, N, RGBA16F))),
             ("pnm_pack<wide>", "B8G8R8X8 -> P6", 7, lambda: ctx.pnm_pack_device(img(image, N, N, BGRX8), dx.PNM_P6, stream, N * N * 3)),
             ("pnm_pack<narrow>", "B8G8R8X8 -> P6, samples one byte off", 7, lambda: ctx.pnm_pack_device(img(image, N, N, BGRX8), dx.PNM_P6, stream + 1, N * N * 3)),
             ("pnm_pack<wide>", "R32G32B32A32_FLOAT -> PF", 28, lambda: ctx.pnm_pack_device(img(image, N, N, RGBA32F), dx.PNM_PF, stream, N * N * 12)),
             ("pnm_pack<wide>", "R16G16B16A16_FLOAT -> PF", 20, lambda: ctx.pnm_pack_device(img(image, N, N, RGBA16F), dx.PNM_PF, stream, N * N * 12)),
             ("pnm_pack<narrow>", "R16G16B16A16_FLOAT -> PF, samples one byte off", 20, lambda: ctx.pnm_pack_device(img(image, N, N, RGBA16F), dx.PNM_PF, stream + 1, N * N * 12))]
    rows = profile_cases(ctx, cases, N * N, REPS)
    ctx.device_free(stream); ctx.device_free(image)
    ctx.close()
    return rows


def write_inputs(tmp, conv):
    rng = np.random.default_rng(1)
    ppm = os.path.join(tmp, "colour.ppm")
    with open(ppm, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (N, N))
        f.write(rng.integers(0, 256, N * N * 3, dtype=np.uint8).tobytes())
    pfm = os.path.join(tmp, "sky.pfm")
    with open(pfm, "wb") as f:
        f.write(b"PF\n%d %d\n-1.000000\n" % (N, N // 2))
        f.write((rng.random(N * (N // 2) * 3, dtype=np.float32) * 8).tobytes())
    rgba32f = os.path.join(tmp, "rgba32f.dds")
    subprocess.run([conv, "-nologo", "-y", "-m", "1", "-f", "R32G32B32A32_FLOAT", "-o", rgba32f, pfm], check=True, capture_output=True)
    return ppm, pfm, rgba32f


def end_to_end():
    lib = os.path.dirname(dx.library_path())
    conv, exe = os.path.join(lib, "dxtexconv"), os.path.join(lib, "pnm_host_test")
    with tempfile.TemporaryDirectory() as tmp:
        ppm, pfm, rgba32f = write_inputs(tmp, conv)
        out = os.path.join(tmp, "out.dds")
        cases = [(".ppm -> -f R8G8B8A8_UNORM -m 1", ["-m", "1", "-f", "R8G8B8A8_UNORM", "-o", out, ppm], out),
                 (".ppm -> -f BC1_UNORM, full chain", ["-f", "BC1_UNORM", "-o", out, ppm], out),
                 (".pfm -> -f BC6H_UF16, full chain", ["-f", "BC6H_UF16", "-o", out, pfm], out),
                 ("R32G32B32A32_FLOAT DDS -> -ft pfm", ["-m", "1", "-ft", "pfm", "-o", tmp, rgba32f], os.path.join(tmp, "rgba32f.pfm"))]
        measure_conv(cases, [(None, conv)], RUNS)
        print(json.dumps({"case": "load .ppm through the API", **api_paths(exe, "time_load", ppm, RUNS)}), flush=True)
        print(json.dumps({"case": "load .pfm through the API", **api_paths(exe, "time_load", pfm, RUNS)}), flush=True)
        print(json.dumps({"case": "save .pfm through the API (from R32G32B32A32_FLOAT)", **api_paths(exe, "time_save", pfm, RUNS, ("1",))}), flush=True)
        print(json.dumps({"case": "save .ppm through the API (from R8G8B8A8_UNORM)", **api_paths(exe, "time_save", ppm, RUNS, ("0",))}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-end-to-end", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernels:
        kernels()
    if not a.skip_end_to_end:
        end_to_end()
