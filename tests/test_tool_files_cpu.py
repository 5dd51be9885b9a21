"""The tools' shared file layer (directxtex_amd/tools/tool_files.h) without a GPU: tests/cpp/tool_files_test.cpp, a stand-alone program, checks
the file-type and format-name tables, and SourceFile::Parse and GetMetadata against the codecs' own calls over one file per type - the committed
.exr, .jpg and .png fixtures, and a .dds, .hdr, .tga and .ppm written here from a few bytes - and over a truncated copy of each."""
import os
import re
import shutil
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "tool_files_test")
GOLDEN = os.path.join(ROOT, "tests", "golden")
W, H = 5, 3
TYPES = {"dds": 0, "hdr": 1, "tga": 2, "ppm": 3, "png": 6, "jpg": 7, "exr": 8}          # FileType, in the enum's order


def _run(*args):
    assert os.path.exists(EXE), "directxtex_amd/lib/tool_files_test is missing: run build()"
    return subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=60)


def _dds():
    """a legacy header, 32-bit RGBA masks, one level"""
    pixel_format = struct.pack("<8I", 32, 0x41, 0, 32, 0x000000FF, 0x0000FF00, 0x00FF0000, 0xFF000000)
    header = struct.pack("<7I", 124, 0x100F, H, W, W * 4, 0, 0) + bytes(44) + pixel_format + struct.pack("<5I", 0x1000, 0, 0, 0, 0)
    assert len(header) == 124
    return b"DDS " + header + bytes(range(W * H * 4))


def _files(tmp_path):
    made = {"dds": _dds(),
            "hdr": b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (H, W) + bytes(range(1, W * H * 4 + 1)),          # flat rows: narrower than 8
            "tga": struct.pack("<BBBHHBHHHHBB", 0, 0, 2, 0, 0, 0, 0, 0, W, H, 32, 8) + bytes(range(W * H * 4)),                  # true colour, 8 alpha bits
            "ppm": b"P6\n%d %d\n255\n" % (W, H) + bytes(range(W * H * 3))}
    paths = {}
    for ext, data in made.items():
        paths[ext] = tmp_path / f"made.{ext}"
        paths[ext].write_bytes(data)
    for ext, name in (("exr", "exr/rgba_half_zip.exr"), ("jpg", "jpeg/c420.jpg"), ("png", "png/grey8.png")):
        paths[ext] = tmp_path / f"fixture.{ext}"
        shutil.copy(os.path.join(GOLDEN, name), paths[ext])
    return paths


def _lines(out):
    found = {}
    for m in re.finditer(r"^(\S+) type (\d+) parse ([0-9A-F]{8}) direct ([0-9A-F]{8}) metadata ([0-9A-F]{8})$", out, re.M):
        found[m.group(1)] = (int(m.group(2)), int(m.group(3), 16), int(m.group(4), 16), int(m.group(5), 16))
    return found


def test_tables():
    r = _run("tables")
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", r.stdout + r.stderr


def test_parse_and_metadata_agree_with_the_codecs(tmp_path):
    paths = _files(tmp_path)
    r = _run("parse", *paths.values())
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stderr == "", r.stdout + r.stderr
    lines = _lines(r.stdout)
    assert len(lines) == len(paths) == 7, r.stdout
    for ext, p in paths.items():
        assert lines[str(p)] == (TYPES[ext], 0, 0, 0), (ext, r.stdout)


def test_truncated_files_fail_like_the_codecs(tmp_path):
    paths = _files(tmp_path)
    cut = {}
    for ext, p in paths.items():
        data = p.read_bytes()
        cut[ext] = tmp_path / f"cut.{ext}"
        cut[ext].write_bytes(data[:len(data) // 2])
    missing = tmp_path / "missing.png"
    r = _run("parse", *cut.values(), missing)
    assert r.returncode == 0 and "FAILED" not in r.stdout and r.stderr == "", r.stdout + r.stderr          # Parse answers what the codec answers
    lines = _lines(r.stdout)
    assert len(lines) == 8, r.stdout
    for ext, p in cut.items():
        kind, parse, direct, _ = lines[str(p)]
        assert kind == TYPES[ext] and parse == direct and parse & 0x80000000, (ext, r.stdout)
    assert lines[str(missing)][1] == 0x80070002, r.stdout          # HRESULT_ERROR_FILE_NOT_FOUND


def test_unknown_type_is_refused(tmp_path):
    p = tmp_path / "x.bmp"
    p.write_bytes(b"BM")
    r = _run("parse", p)
    assert r.returncode == 0, r.stdout + r.stderr
    assert _lines(r.stdout)[str(p)] == (9, 0x80070032, 0x80070032, 0x80070032), r.stdout          # UNKNOWN: what to do with it is each tool's policy
