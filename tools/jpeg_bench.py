"""Measures what profiles/jpeg.md reports, on one MI355X (run from the repository root: python tools/jpeg_bench.py --c420 A.jpg --c444 B.jpg).

Kernels: one 4096 x 4096 frame of random coefficients through dxtex_jpeg_decode_device as 4:2:0, 4:4:4 and grey, and beside them
png_unpack<wide> on an RGB 8 image of the same size in the same run, each REPS times inside one dxtex_ctx_profile_begin / _end window after a
warm-up; per-kernel time and the bytes read and written over it. (The kernels' time does not depend on the coefficients' values.)

End to end, on the two files named (4096^2, quality 90; where Pillow is installed and no file is named the script writes them to a temporary
directory): `dxtexconv -nologo -timing -overlap 1 -y` to -f R8G8B8A8_UNORM -m 1 and to -f BC1_UNORM with the full chain, one unmeasured run
and five measured ones each; the Huffman walk alone (jpeg_host_test time_raw); and the load through the API (jpeg_host_test time_load): the
resident loader against this build's host loader plus Upload, alternating. The parent commit cannot read the files, so that host path is the
only comparison there is.

The writer (--skip-encode leaves it out): one 4096 x 4096 image of noise through dxtex_jpeg_encode_device as grey, 4:2:0 and 4:4:4, measured
as the reader's kernels are, with quantiser tables of ones (the writer's) and of 8; then SaveToJPEGMemory on a resident 4096^2 image against
Download plus this build's host saver, alternating, and SaveJPEGRaw alone on the same coefficients (jpeg_write_host_test time_save). The
parent commit cannot write a .jpg, so that host path is again the only comparison."""
import argparse, json, os, statistics, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import directxtex_amd as dx
from codec_bench import measure_conv, run_rows, summary

N, REPS, RUNS = 4096, 20, 5
RGBA8, R8 = dx.DXGI_FORMAT_R8G8B8A8_UNORM, dx.DXGI_FORMAT_R8_UNORM


def kernels():
    ctx = dx.Context(0)
    coef = ctx.device_alloc(N * N * 6)
    image = ctx.device_alloc(N * N * 4)
    rng = np.random.default_rng(1)
    chunk = (rng.integers(-20, 21, N * N // 2) * (rng.integers(0, 4, N * N // 2) == 0)).astype(np.int16)
    for at in range(0, N * N * 6, chunk.nbytes):
        ctx.upload(coef + at, chunk.view(np.uint8), sync=True)
    quant = np.full((4, 64), 8, np.uint16)
    img = dx.device_image
    # bytes a texel: (idct reads + writes, colour reads + writes)
    cases = [("4:2:0 -> R8G8B8A8", dx.jpeg_frame(N, N, dx.JPEG_YCBCR, (2, 2), quant), RGBA8, (3 + 1.5, 1.5 + 4)),
             ("4:4:4 -> R8G8B8A8", dx.jpeg_frame(N, N, dx.JPEG_YCBCR, (1, 1), quant), RGBA8, (6 + 3, 3 + 4)),
             ("grey -> R8", dx.jpeg_frame(N, N, dx.JPEG_GREY, (1, 1), quant), R8, (2 + 1, 0))]
    for what, frame, fmt, moved in cases:
        call = lambda: ctx.jpeg_decode_device(coef, dx.jpeg_coefficient_count(frame) * 2, frame, img(image, N, N, fmt))
        for _ in range(3):
            call()
        ctx.synchronize()
        ctx.profile_begin()
        for _ in range(REPS):
            call()
        prof = ctx.profile_end()
        row = {"case": what}
        for (k, (ms, n)), b in zip(sorted(prof.items(), key=lambda kv: kv[0] != "jpeg_idct"), moved):
            row[k + " ms"] = round(ms / n, 4)
            row[k + " TBps"] = round(N * N * b / (ms / n * 1e-3) / 1e12, 3)
        print(json.dumps(row), flush=True)
    for _ in range(3):
        ctx.png_unpack_device(coef, N * N * 3, dx.PNG_RGB8, img(image, N, N, RGBA8))
    ctx.synchronize()
    ctx.profile_begin()
    for _ in range(REPS):
        ctx.png_unpack_device(coef, N * N * 3, dx.PNG_RGB8, img(image, N, N, RGBA8))
    ms, n = ctx.profile_end()["png_unpack<wide>"]
    print(json.dumps({"case": "png_unpack<wide> RGB 8 -> R8G8B8A8, the same size", "png_unpack<wide> ms": round(ms / n, 4), "TBps": round(N * N * 7 / (ms / n * 1e-3) / 1e12, 3)}), flush=True)
    ctx.device_free(coef); ctx.device_free(image)
    ctx.close()


def encode_kernels():
    ctx = dx.Context(0)
    coef = ctx.device_alloc(N * N * 6)
    image = ctx.device_alloc(N * N * 4)
    rng = np.random.default_rng(2)
    chunk = rng.integers(0, 256, N * N // 2, dtype=np.uint8)
    for at in range(0, N * N * 4, chunk.nbytes):
        ctx.upload(image + at, chunk, sync=True)
    img = dx.device_image
    # bytes a texel: (samples reads + writes, fdct reads + writes)
    cases = [("R8G8B8A8 -> 4:2:0", (2, 2), RGBA8, (4 + 1.5, 1.5 + 3)), ("R8G8B8A8 -> 4:4:4", (1, 1), RGBA8, (4 + 3, 3 + 6)), ("R8 -> grey", None, R8, (0, 1 + 2))]
    for q in (1, 8):
        quant = np.full((4, 64), q, np.uint16)
        for what, sampling, fmt, moved in cases:
            frame = dx.jpeg_frame(N, N, dx.JPEG_GREY if sampling is None else dx.JPEG_YCBCR, sampling or (1, 1), quant)
            call = lambda: ctx.jpeg_encode_device(img(image, N, N, fmt), frame, coef, dx.jpeg_coefficient_count(frame) * 2)
            for _ in range(3):
                call()
            ctx.synchronize()
            ctx.profile_begin()
            for _ in range(REPS):
                call()
            prof = ctx.profile_end()
            row = {"case": what, "quantiser entries": q}
            for k, (ms, n) in sorted(prof.items(), key=lambda kv: kv[0] == "jpeg_fdct"):
                b = moved[k == "jpeg_fdct"]
                row[k + " ms"] = round(ms / n, 4)
                row[k + " TBps"] = round(N * N * b / (ms / n * 1e-3) / 1e12, 3)
            print(json.dumps(row), flush=True)
    ctx.device_free(coef); ctx.device_free(image)
    ctx.close()


def save_end_to_end():
    exe = os.path.join(os.path.dirname(dx.library_path()), "jpeg_write_host_test")
    for name, fmt in (("R8_UNORM -> grey", R8), ("R8G8B8A8_UNORM -> 4:2:0", RGBA8)):
        lines = run_rows([exe, "time_save", str(N), str(N), str(fmt), str(RUNS)])
        rows, raw = [x for x in lines if "resident" in x], [x["raw"] for x in lines if "resident" not in x]
        assert len(rows) == RUNS and len(raw) == RUNS, lines
        s = summary(rows)
        print(json.dumps({"case": name + ": SaveToJPEGMemory through the API", "file bytes": rows[0]["file"], "resident ms": s["resident ms"], "resident median": s["resident median"],
                          "resident up/down": s["resident up/down"], "Download + host saver ms": s["host path ms"], "host path median": s["host path median"],
                          "host path up/down": s["host path up/down"], "SaveJPEGRaw alone ms": raw, "SaveJPEGRaw median": statistics.median(raw),
                          "share of the resident save in the Huffman coder": round(statistics.median(raw) / s["resident median"], 3)}), flush=True)


def write_files(tmp):
    from PIL import Image
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:N, 0:N]
    px = np.stack([((xx * (k + 1) // 3 + yy * (4 - k) // 5 + rng.integers(0, 8, (N, N))) & 0xFF).astype(np.uint8) for k in range(3)], axis=2)
    paths = {}
    for name, sub in (("c420", 2), ("c444", 0)):
        paths[name] = os.path.join(tmp, name + ".jpg")
        Image.fromarray(px).save(paths[name], "JPEG", quality=90, subsampling=sub)
    return paths


def end_to_end(paths, tmp):
    lib = os.path.dirname(dx.library_path())
    conv, exe = os.path.join(lib, "dxtexconv"), os.path.join(lib, "jpeg_host_test")
    out = os.path.join(tmp, "out.dds")
    for name, path in paths.items():
        print(json.dumps({"file": name, "bytes": os.path.getsize(path)}), flush=True)
        lines = run_rows([exe, "time_raw", path, str(RUNS)])
        raw = [x["raw"] for x in lines]
        print(json.dumps({"case": name + ": LoadFromJPEGMemoryRaw (markers and the Huffman walk, no device)", "ms": raw, "median": statistics.median(raw),
                          "coefficient bytes": lines[0]["coefficients"]}), flush=True)
        measure_conv([(name + " -> -f R8G8B8A8_UNORM -m 1", ["-m", "1", "-f", "R8G8B8A8_UNORM", "-o", out, path], out),
                      (name + " -> -f BC1_UNORM, full chain", ["-f", "BC1_UNORM", "-o", out, path], out)], [(None, conv)], RUNS)
        rows = run_rows([exe, "time_load", path, str(RUNS)])
        assert len(rows) == RUNS, rows
        s = summary(rows)
        del s["host path spread"]
        print(json.dumps({"case": name + ": load through the API", **s,
                          "share of the resident load in the Huffman walk": round(statistics.median(raw) / s["resident median"], 3)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-end-to-end", action="store_true")
    ap.add_argument("--skip-encode", action="store_true")
    ap.add_argument("--c420")
    ap.add_argument("--c444")
    a = ap.parse_args()
    if not a.skip_kernels:
        kernels()
    if not a.skip_encode:
        encode_kernels()
        save_end_to_end()
    if not a.skip_end_to_end:
        with tempfile.TemporaryDirectory() as tmp:
            end_to_end({"c420": a.c420, "c444": a.c444} if a.c420 and a.c444 else write_files(tmp), tmp)
