"""Measures what profiles/exr.md reports, on one MI355X (run from the repository root: python tools/exr_bench.py).

Kernels: the stream of a 4096 x 2048 RGB-half ZIP file (128 coded chunks of 16 rows, 384 KiB each) through dxtex_exr_unpack_device -
exr_undo_sums, exr_undo<wide> and exr_texels - and beside it pnm_unpack<wide> on a PH image of the same size (the same 6 bytes a texel in,
8 out, without the undo and without the plane gather), and exr_pack<wide> from R32G32B32A32_FLOAT; each REPS times inside one
dxtex_ctx_profile_begin / _end window after a warm-up; per-kernel time and the bytes read and written over it. exr_undo works in place, so
from the second repetition on it scans bytes that are already undone: the same work on other values.

End to end: `dxtexconv -nologo -timing -overlap 1 -y` on files this script writes to a temporary directory (the .exr by tests/exr_ref.py) -
  the .exr to -f R16G16B16A16_FLOAT -m 1 and to -f BC6H_UF16 with the full chain,
  a 4096 x 2048 R32G32B32A32_FLOAT DDS to -ft exr
- one unmeasured run and five measured ones each; the medians and the bytes moved. The parent commit cannot read these files, so each case
is set beside the same build's host path through the API (tests/cpp/exr_host_test.cpp time_load / time_save): the resident loader against
the host loader plus Upload, the resident saver against Download plus the host saver, alternating, five runs after one unmeasured; time_load
also times the Raw loader alone (header, table, inflate: the byte-serial share of the resident load) and the host's serial undo of the same
stream, which is what exr_undo replaces."""
import argparse, json, os, statistics, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import directxtex_amd as dx
import exr_ref as R
from codec_bench import measure_conv, profile_cases, run_rows, summary

W, H, REPS, RUNS = 4096, 2048, 20, 5
RGBA32F, RGBA16F = dx.DXGI_FORMAT_R32G32B32A32_FLOAT, dx.DXGI_FORMAT_R16G16B16A16_FLOAT


def sky(w, h, seed=1):
    """name -> (h, w) halves: a smooth HDR gradient with a little noise, so that deflate has something to do and something to gain"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    return {c: ((np.sin(x / (300.0 + 40 * k)) + 1.2) * (np.cos(y / (500.0 + 60 * k)) + 1.5) * (4.0 + k) * (1 + rng.random((h, w), dtype=np.float32) * 0.02)).astype(np.float16).view(np.uint16)
            for k, c in enumerate("RGB")}


def stream_of(samples, w, h):
    """the expanded stream of the ZIP file of these samples: every chunk coded, on a multiple of 16 bytes"""
    ch = [(c, R.HALF, 1, 1) for c in "RGB"]
    parts, chunks, at = [], [], 0
    for y in range(0, h, 16):
        rows = min(16, h - y)
        coded = R.code(R.plain_chunk(ch, samples, y, rows))
        chunks.append((at, len(coded), y, rows, 1))
        parts.append(coded + bytes(-len(coded) % 16))
        at += len(parts[-1])
    return np.frombuffer(b"".join(parts), np.uint8), chunks


def kernels():
    ctx = dx.Context(0)
    samples = sky(W, H)
    stream_host, chunks = stream_of(samples, W, H)
    stream = ctx.device_alloc(max(stream_host.nbytes, W * H * 16) + 16)
    image = ctx.device_alloc(W * H * 16)
    ctx.upload(stream, stream_host, sync=True)
    img = dx.device_image
    table = [(4 * W, dx.EXR_HALF), (2 * W, dx.EXR_HALF), (0, dx.EXR_HALF), (0, dx.EXR_ABSENT)]          # a scanline holds B, G, R: the name order
    cases = [("exr_texels", "RGB half ZIP stream -> R16G16B16A16_FLOAT (undo in place, then the gather)", 14,
              lambda: ctx.exr_unpack_device(stream, stream_host.nbytes, chunks, table, 6 * W, [img(image, W, H, RGBA16F)])),
             ("exr_texels", "the same stream as plain chunks (no undo, no planes)", 14,
              lambda: ctx.exr_unpack_device(stream, stream_host.nbytes, [c[:4] + (0,) for c in chunks], table, 6 * W, [img(image, W, H, RGBA16F)])),
             ("pnm_unpack<wide>", "PH -> R16G16B16A16_FLOAT, the same image size", 14, lambda: ctx.pnm_unpack_device(stream, W * H * 6, dx.PNM_PH, img(image, W, H, RGBA16F))),
             ("exr_pack<wide>", "R32G32B32A32_FLOAT -> the writer's half planes", 24, lambda: ctx.exr_pack_device(img(image, W, H, RGBA32F), stream, W * H * 8)),
             ("exr_pack<wide>", "R16G16B16A16_FLOAT -> the writer's half planes", 16, lambda: ctx.exr_pack_device(img(image, W, H, RGBA16F), stream, W * H * 8))]
    rows = profile_cases(ctx, cases, W * H, REPS)          # one call launches exr_undo_sums and exr_undo: milliseconds a call, not a launch
    ctx.device_free(stream); ctx.device_free(image)
    ctx.close()
    return rows


def write_inputs(tmp, conv):
    samples = sky(W, H)
    exr = os.path.join(tmp, "sky.exr")
    with open(exr, "wb") as f:
        f.write(R.write([(c, R.HALF, 1, 1) for c in "RGB"], samples, R.ZIP, (0, 0, W - 1, H - 1)))
    rgba32f = os.path.join(tmp, "rgba32f.dds")
    subprocess.run([conv, "-nologo", "-y", "-m", "1", "-f", "R32G32B32A32_FLOAT", "-o", rgba32f, exr], check=True, capture_output=True)
    return exr, rgba32f


def api_paths(exe, command, file):
    rows = run_rows([exe, command, file, str(RUNS)])
    assert len(rows) == RUNS, rows
    out = summary(rows)
    if command == "time_load":
        out["raw loader median ms"] = statistics.median(x["raw"] for x in rows)
        out["host serial undo median ms"] = statistics.median(x["undo"] for x in rows)
    return out


def end_to_end():
    lib = os.path.dirname(dx.library_path())
    conv, exe = os.path.join(lib, "dxtexconv"), os.path.join(lib, "exr_host_test")
    with tempfile.TemporaryDirectory() as tmp:
        exr, rgba32f = write_inputs(tmp, conv)
        print(json.dumps({"file": ".exr", "bytes": os.path.getsize(exr), "texels": W * H}), flush=True)
        out = os.path.join(tmp, "out.dds")
        cases = [(".exr -> -f R16G16B16A16_FLOAT -m 1", ["-m", "1", "-f", "R16G16B16A16_FLOAT", "-o", out, exr], out),
                 (".exr -> -f BC6H_UF16, full chain", ["-f", "BC6H_UF16", "-o", out, exr], out),
                 ("R32G32B32A32_FLOAT DDS -> -ft exr", ["-m", "1", "-ft", "exr", "-o", tmp, rgba32f], os.path.join(tmp, "rgba32f.exr"))]
        measure_conv(cases, [(None, conv)], RUNS)
        print(json.dumps({"case": "load .exr through the API", **api_paths(exe, "time_load", exr)}), flush=True)
        print(json.dumps({"case": "save .exr through the API (from R16G16B16A16_FLOAT)", **api_paths(exe, "time_save", exr)}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--skip-end-to-end", action="store_true")
    a = ap.parse_args()
    if not a.skip_kernels:
        kernels()
    if not a.skip_end_to_end:
        end_to_end()
