"""Measures what profiles/dds.md reports, on one MI355X (run from the repository root: python tools/dds_bench.py [--parent DIR]).

Kernels: one 4096 x 4096 image through dxtex_dds_unpack_device and dxtex_dds_pack24_device on both routes (the narrow one by way of a
payload that starts one byte off), REPS times inside one dxtex_ctx_profile_begin / _end window after a warm-up; per-kernel time and the
bytes read and written over it.

End to end: `dxtexconv -nologo -timing -overlap 1 -y` on files this script writes to a temporary directory -
  a 4096^2 24-bit R8G8B8 DDS to -f R8G8B8A8_UNORM -m 1 and to -f BC1_UNORM with the full chain,
  a 4096^2 L8 DDS to -f BC4_UNORM -m 1, a native R8G8B8A8_UNORM DDS to -f BC1_UNORM with the full chain,
  a 4096^2 BC7_UNORM DDS (random blocks) handed through
- five runs of this build (directxtex_amd/lib/dxtexconv) and, with --parent DIR, five of the dxtexconv in DIR (a build of the parent
commit), alternating. Prints each run's -timing line figures, the medians, the parent's spread (max - min of its five) and whether the two
builds' outputs are byte-identical. dxtexconv has no switch for DDS_FLAGS_FORCE_24BPP_RGB, so the 24-bit writer is measured as a kernel only."""
import argparse, json, os, struct, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import directxtex_amd as dx
from codec_bench import measure_conv

N, REPS, RUNS = 4096, 20, 5
RGBA8, BGRX8, RGBA16 = dx.DXGI_FORMAT_R8G8B8A8_UNORM, dx.DXGI_FORMAT_B8G8R8X8_UNORM, 11          # 11: R16G16B16A16_UNORM


def kernels():
    ctx = dx.Context(0)
    payload = ctx.device_alloc(N * N * 4 + 16)
    image = ctx.device_alloc(N * N * 8)
    ctx.upload(payload, np.random.default_rng(0).integers(0, 256, N * N * 4 + 16, dtype=np.uint8), sync=True)
    img = dx.device_image
    palette = np.arange(256, dtype=np.uint32) * 0x010101 | 0xFF000000

    def unpack(op, B, fmt, base=0, opaque=False, pal=None):
        return lambda: ctx.dds_unpack_device(payload + base, N * N * B, op, [img(image, N, N, fmt)], [0], [N * B], opaque, pal)

    cases = [("dds_unpack<888,wide>", "24 bits -> R8G8B8A8", 7, unpack(dx.DDS_ROW_888, 3, RGBA8)),
             ("dds_unpack<888,narrow>", "24 bits -> R8G8B8A8, payload one byte off", 7, unpack(dx.DDS_ROW_888, 3, RGBA8, 1)),
             ("dds_unpack<l8,wide>", "L8 -> R8G8B8A8", 5, unpack(dx.DDS_ROW_L8, 1, RGBA8)),
             ("dds_unpack<p8,wide>", "P8 -> R8G8B8A8", 5, unpack(dx.DDS_ROW_P8, 1, RGBA8, pal=palette)),
             ("dds_unpack<565,wide>", "5:6:5 -> R8G8B8A8", 6, unpack(dx.DDS_ROW_565, 2, RGBA8)),
             ("dds_unpack<l16,wide>", "L16 -> R16G16B16A16", 10, unpack(dx.DDS_ROW_L16, 2, RGBA16)),
             ("dds_unpack<swizzle,wide>", "B8G8R8A8 -> R8G8B8A8", 8, unpack(dx.DDS_ROW_SWIZZLE, 4, RGBA8)),
             ("dds_unpack<copy,wide>", "R8G8B8A8, alpha forced", 8, unpack(dx.DDS_ROW_COPY, 4, RGBA8, opaque=True)),
             ("dds_pack24<wide>", "B8G8R8X8 -> 24 bits", 7, lambda: ctx.dds_pack24_device([img(image, N, N, BGRX8)], [0], [N * 3], payload, N * N * 3)),
             ("dds_pack24<narrow>", "B8G8R8X8 -> 24 bits, output one byte off", 7, lambda: ctx.dds_pack24_device([img(image, N, N, BGRX8)], [0], [N * 3], payload + 1, N * N * 3))]
    rows = []
    for mark, what, bytes_a_texel, call in cases:
        for _ in range(3):
            call()
        ctx.synchronize()
        ctx.profile_begin()
        for _ in range(REPS):
            call()
        prof = ctx.profile_end()
        assert prof[mark][1] == REPS, prof
        row = {"kernel": mark, "case": what, "ms": round(prof[mark][0] / REPS, 4), "TBps": round(N * N * bytes_a_texel / (prof[mark][0] / REPS * 1e-3) / 1e12, 3)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    ctx.device_free(payload); ctx.device_free(image)
    ctx.close()
    return rows


def dds_header(pf, dx10=None, mips=0):
    """magic + DDS_HEADER (+ DDS_HEADER_DXT10) of an N x N texture; pf = the eight words of DDS_PIXELFORMAT"""
    b = struct.pack("<I", 0x20534444) + struct.pack("<7I", 124, 0x1007, N, N, 0, 0, mips) + bytes(44) + struct.pack("<8I", *pf) + struct.pack("<5I", 0x1000, 0, 0, 0, 0)
    return b + (struct.pack("<5I", *dx10) if dx10 else b"")


def write_inputs(tmp):
    rng = np.random.default_rng(1)
    files = {}
    for name, pf, dx10, nbytes in (("r8g8b8", (32, 0x40, 0, 24, 0xff0000, 0x00ff00, 0x0000ff, 0), None, N * N * 3),
                                   ("l8", (32, 0x20000, 0, 8, 0xff, 0, 0, 0), None, N * N),
                                   ("rgba8", (32, 0x41, 0, 32, 0x000000ff, 0x0000ff00, 0x00ff0000, 0xff000000), None, N * N * 4),
                                   ("bc7", (32, 0x4, 0x30315844, 0, 0, 0, 0, 0), (98, 3, 0, 1, 0), N * N)):
        files[name] = os.path.join(tmp, name + ".dds")
        with open(files[name], "wb") as f:
            f.write(dds_header(pf, dx10))
            f.write(rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes())
    return files


def end_to_end(parent):
    ours = os.path.join(os.path.dirname(dx.library_path()), "dxtexconv")
    builds = [("this build", ours)] + ([("parent", os.path.join(parent, "dxtexconv"))] if parent else [])
    with tempfile.TemporaryDirectory() as tmp:
        files = write_inputs(tmp)
        out = os.path.join(tmp, "out.dds")
        cases = [("24-bit R8G8B8 DDS -> -f R8G8B8A8_UNORM -m 1", ["-m", "1", "-f", "R8G8B8A8_UNORM", "-o", out, files["r8g8b8"]], out),
                 ("24-bit R8G8B8 DDS -> -f BC1_UNORM, full chain", ["-f", "BC1_UNORM", "-o", out, files["r8g8b8"]], out),
                 ("L8 DDS -> -f BC4_UNORM -m 1", ["-m", "1", "-f", "BC4_UNORM", "-o", out, files["l8"]], out),
                 ("R8G8B8A8_UNORM DDS -> -f BC1_UNORM, full chain", ["-f", "BC1_UNORM", "-o", out, files["rgba8"]], out),
                 ("BC7_UNORM DDS handed through", ["-m", "1", "-f", "BC7_UNORM", "-o", out, files["bc7"]], out)]
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
