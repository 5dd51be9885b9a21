"""The TIFF codec's resident forms (LoadFromTIFFMemory(Device&) / SaveToTIFFFile(Device&)) against the host forms of the same build, through
tests/cpp/tiff_host_test.cpp: HRESULTs, metadata and pixels, the transfer counts - up goes exactly the expanded stream, down exactly the
file's rows - the kernel launches, and release on failure."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tiff_ref as T  # noqa: E402
from test_tiff_cpu import SAVE_CASES, _colormap, _samples  # noqa: E402

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "tiff_host_test")


def _run(*args):
    r = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_resident_load_against_the_host_form(tmp_path):
    files = []
    for kind in range(14):
        bits, S, _, _ = T.KINDS[kind]
        cm = _colormap(bits) if kind in (T.PAL1, T.PAL4, T.PAL8) else None
        predictor = 2 if bits in (8, 16) else 3 if bits == 32 else 1
        extra = 2 if S == 4 else None
        for kw in (dict(compression=T.LZW, predictor=predictor, rows_per_strip=2), dict(compression=T.ADOBE_DEFLATE, predictor=predictor, tile=(16, 16), big_endian=True),
                   dict(compression=T.PACKBITS, planar=True, big_endian=True), dict()):
            files.append(T.build(_samples(kind, 18, 20, len(files)), kind, colormap=cm, extra=extra, **kw))
    golden = os.path.join(ROOT, "tests", "golden", "tiff")
    for n in sorted(os.listdir(golden)):
        if n.endswith(".tif"):
            files.append(open(os.path.join(golden, n), "rb").read())
    refused = [T.build(_samples(T.RGB8, 4, 4, 1), T.RGB8, photometric=6), files[0][:40], b""]
    paths = []
    for i, data in enumerate(files + refused):
        p = tmp_path / f"f{i}.tif"
        p.write_bytes(data)
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("".join(f"{p}\n" for p in paths))
    lines = _run("device_load_many", lst, 0).splitlines()
    assert len(lines) == len(paths)
    for i, data in enumerate(files):
        f = lines[i].split()
        hr, want = T.decode(data)
        info = want["info"]
        stream, segs = T.segments(info)
        native = T.is_native(info) and len(segs) == 1
        assert f[1:4] == ["00000000", "00000000", "ok"], lines[i]
        w, h, stream_bytes, up, down, meta, pixels, undo, texels = [int(x) for x in f[4:]]
        assert (w, h, meta, pixels) == (want["width"], want["height"], 1, 1), lines[i]
        # one upload - the stream as it left the decoder, or the image itself where the file is its image - and no download
        assert stream_bytes == len(stream) and down == 0 and up == (want["width"] * want["height"] * T.KINDS[info["kind"]][3] if native else len(stream)), (lines[i], native)
        assert (undo, texels) == ((0, 0) if native else (1 if info["predictor"] != 1 else 0, (len(segs) + 63) // 64)), (lines[i], len(segs))
    for i, want in zip(range(len(files), len(paths)), ("80070032", "80004005", "80004005")):
        assert lines[i].split()[1:] == [want, want, "released"], lines[i]


def test_resident_save_against_the_host_form(tmp_path):
    rng = np.random.default_rng(3)
    for i, (fmt, flags) in enumerate(SAVE_CASES[:13]):          # every source format once, and FORCE_SRGB; a process and a device each
        for (w, h) in (((64, 5),) if i % 2 else ((7, 3),)):
            bits, S, _, ib, fb, bgr, _ = T.SOURCES[fmt]
            px = rng.integers(0, 256, w * ib * h, dtype=np.uint8)
            src, out = tmp_path / "px.bin", tmp_path / f"out{i}_{w}.tif"
            src.write_bytes(px.tobytes())
            f = _run("device_save", src, w, h, fmt, w * ib, flags, out).split()
            assert f[:3] == ["hr", "00000000", "00000000"], f
            data = out.read_bytes()
            assert data == open(str(out) + ".host", "rb").read() == T.save(px.tobytes(), w, h, fmt, flags)[1], (fmt, flags)
            # down come exactly the file's rows, straight behind the header the host wrote; only the BGR sources run a kernel
            assert [int(x) for x in f[3:]] == [0, w * h * fb, 1 if bgr else 0], f
    src = tmp_path / "px.bin"
    src.write_bytes(bytes(4096))
    f = _run("device_save", src, 4, 4, 10, 32, 0, tmp_path / "no.tif").split()          # R16G16B16A16_FLOAT
    assert f[:3] == ["hr", "80070032", "80070032"] and [int(x) for x in f[3:]] == [0, 0, 0] and not (tmp_path / "no.tif").exists(), f
