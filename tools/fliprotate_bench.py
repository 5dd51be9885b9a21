"""Measures the rows of profiles/fliprotate.md on one MI355X (run from the repository root):

    python tools/fliprotate_bench.py            the library's own event pairs: median of 20 calls after 5 warm-up calls, with min and max
    python tools/fliprotate_bench.py trace      the same calls under `rocprofv3 --kernel-trace --stats` in a process of its own: the kernel
                                                times of the trace, median, min and max of the 20 measured dispatches of each case
    python tools/fliprotate_bench.py workload   what the trace run executes (no timing of its own)

For a 4096 x 4096 R8G8B8A8_UNORM image and a 4096 x 2048 R32G32B32A32_FLOAT image: the row route (FLIP_HORIZONTAL, FLIP_VERTICAL, ROTATE180),
the transposing route (ROTATE90, ROTATE270) and, as the floor, copy_rect_kernel moving the same whole image - the same bytes in and out with
no permutation. Rates are bytes read plus bytes written over the time; `ratio` is a route's time over the floor's."""
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM, REPS = 5, 20
RGBA8, RGBA32F = 28, 2
IMAGES = (("4096x4096 R8G8B8A8_UNORM", 4096, 4096, RGBA8, 4), ("4096x2048 R32G32B32A32_FLOAT", 4096, 2048, RGBA32F, 16))
FLAGS = (("FLIP_HORIZONTAL", 0x08), ("FLIP_VERTICAL", 0x10), ("ROTATE180", 2), ("ROTATE90", 1), ("ROTATE270", 3))
KERNELS = ("copy_rect_kernel", "flip_rows_kernel", "flip_transpose_kernel")


def cases(ctx):
    """-> [(image title, case name, bytes moved, call)] in the order every mode runs them: per image the floor first, then the five words"""
    import numpy as np
    from directxtex_amd import capi
    out = []
    for title, w, h, fmt, texel in IMAGES:
        n = w * h * texel
        src, dst = ctx.device_alloc(n), ctx.device_alloc(n)
        ctx.upload(src, np.random.default_rng(0).integers(0, 256, n, dtype=np.uint8), sync=True)
        a, same, turned = capi.device_image(src, w, h, fmt), capi.device_image(dst, w, h, fmt), capi.device_image(dst, h, w, fmt)
        out.append((title, "copy_rect (floor)", 2 * n, lambda a=a, b=same, w=w, h=h: ctx.copy_rectangles_device([a], [(0, 0, w, h)], [b], [0], [0])))
        for name, f in FLAGS:
            out.append((title, name, 2 * n, lambda a=a, b=(turned if f & 1 else same), f=f: ctx.flip_rotate_device([a], [b], f)))
    return out


def workload(ctx, timed):
    rows = []
    for title, name, moved, call in cases(ctx):
        for _ in range(WARM):
            call()
        ctx.synchronize()
        ms = []
        for _ in range(REPS):
            call()
            ctx.synchronize()
            ms.append(ctx.last_kernel_ms())
        if timed:
            rows.append({"image": title, "case": name, "bytes": moved, "ms": ms})
    return rows


def report(rows, clock):
    floor = {}
    for r in rows:
        med = statistics.median(r["ms"])
        if r["case"].startswith("copy_rect"):
            floor[r["image"]] = med
        print(json.dumps({"clock": clock, "image": r["image"], "case": r["case"], "median_ms": round(med, 4), "min_ms": round(min(r["ms"]), 4),
                          "max_ms": round(max(r["ms"]), 4), "TB_per_s": round(r["bytes"] / (med * 1e-3) / 1e12, 3), "ratio_to_floor": round(med / floor[r["image"]], 3)}))


def trace():
    """The workload in a child process under rocprofv3; the kernel trace's dispatches of our three kernels, in order, are the cases' calls."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "fliprotate", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "workload"]
        subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        assert len(files) == 1, files
        with open(files[0], newline="") as f:
            disp = [r for r in csv.DictReader(f) if any(k in r["Kernel_Name"] for k in KERNELS)]
    disp.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [(title, name, 2 * w * h * texel) for title, w, h, _, texel in IMAGES for name in ["copy_rect (floor)"] + [n for n, _ in FLAGS]]
    per = WARM + REPS
    assert len(disp) == per * len(names), (len(disp), per * len(names))
    rows = []
    for i, (title, name, moved) in enumerate(names):
        mine = disp[i * per + WARM:(i + 1) * per]
        rows.append({"image": title, "case": name, "bytes": moved, "ms": [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in mine]})
    report(rows, "rocprofv3 kernel trace")


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "events"
    if mode == "trace":
        trace()
    else:
        import directxtex_amd as dx
        ctx = dx.Context(0)
        rows = workload(ctx, mode != "workload")
        if rows:
            report(rows, "library event pair")
        ctx.close()
