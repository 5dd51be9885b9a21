"""The host layer's CopyRectangle / texassemble steps, without a GPU: the cube-face layout tables against tests/golden/assemble_layouts.json
(numbers only: the cell of each face +X -X +Y -Y +Z -Z in a cross, tee or strip), the argument checks that need no device, and the same
driver (tests/cpp/assemble_host_test.cpp, host code with its own main) built stand-alone under AddressSanitizer and UBSan."""
import json
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden", "assemble_layouts.json")
TOOL = os.path.join(LIB, "dxtexassemble")


def _tool(*args):
    out = subprocess.run([TOOL, *[str(a) for a in args]], capture_output=True, text=True, timeout=60)
    return out.returncode, out.stdout + out.stderr


def _layouts(exe):
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120)
    assert out.stderr == "", out.stderr
    return json.loads(out.stdout)


def test_layout_tables_match_golden():
    exe = os.path.join(LIB, "assemble_host_test")
    assert os.path.exists(exe), "assemble_host_test is missing: run build()"
    want = json.load(open(GOLDEN))
    assert _layouts(exe) == want
    for name, l in want.items():            # the file itself: six distinct cells inside the grid
        cells = set(zip(l["x"], l["y"]))
        assert len(cells) == 6 and all(x < l["cols"] and y < l["rows"] for x, y in cells), name


def test_host_driver_under_sanitizers(tmp_path):
    """A stand-alone ASan + UBSan build of the driver and of DirectXTexAMD_Assemble.cpp (the code under test), linked against the
    libraries as built: it runs clean and prints the same tables."""
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the host layer: it cannot be missing where build() ran"
    exe = str(tmp_path / "assemble_host_test_san")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread",
           os.path.join(ROOT, "tests", "cpp", "assemble_host_test.cpp"), os.path.join(ROOT, "directxtex_amd", "host", "DirectXTexAMD_Assemble.cpp"),
           "-o", exe, "-L" + LIB, "-ldxtex_amd_host", "-ldxtex_amd", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    assert _layouts(exe) == json.load(open(GOLDEN))


# ---- dxtexassemble's argument handling: everything below ends before a device is created ------------------------------------------------------
def test_tool_help_and_unknown_command():
    rc, out = _tool("-help")
    assert rc == 0 and "COMMANDS" in out and "cube-from-hc" in out and "-swizzle" in out
    rc, out = _tool("h-cross", "-help")
    assert rc == 0 and "OPTIONS" in out
    rc, out = _tool("pyramid", "a.dds", "-o", "b.dds")
    assert rc == 1 and "Must use one of" in out


def test_tool_option_parsing():
    cases = [(("cube", "a.dds", "b.dds"), "Need to specify output file via -o"),
             (("h-cross", "cube.dds"), "Need to specify output file via -o"),
             (("h-cross", "a.dds", "b.dds", "-o", "x.dds"), "only accepts 1 input file"),
             (("merge", "a.dds", "b.dds", "c.dds", "-o", "x.dds"), "merge output only accepts 2 input files"),
             (("from-mips", "a.dds", "-o", "x.dds"), "requires at least 2 input files"),
             (("cube-from-mips", "a.dds", "b.dds", "-o", "x.dds"), "requires at least 12 input files"),
             (("cube", "-swizzle", "rgbA", "a.dds", "-o", "x.dds"), "-swizzle only applies to merge command"),
             (("merge", "-swizzle", "rgq", "a.dds", "b.dds", "-o", "x.dds"), "-swizzle requires a 1 to 4 character mask"),
             (("merge", "-swizzle", "rgbaa", "a.dds", "b.dds", "-o", "x.dds"), "Invalid value specified with -swizzle"),
             (("h-strip", "-stripmips", "a.dds", "-o", "x.dds"), "-stripmips only applies to"),
             (("array", "-m", "3", "a.dds", "-o", "x.dds"), "-m only applies to"),
             (("array", "-w", "wide", "a.dds", "-o", "x.dds"), "Invalid value specified with -w"),
             (("array", "-f", "NOFORMAT", "a.dds", "-o", "x.dds"), "Invalid value specified with -f"),
             (("array", "-if", "SHARP", "a.dds", "-o", "x.dds"), "Invalid value specified with -if"),
             (("array", "-fl", "13.0", "a.dds", "-o", "x.dds"), "Invalid value specified with -fl"),
             (("array", "-wrap", "-mirror", "a.dds", "-o", "x.dds"), "Can't use -wrap and -mirror"),
             (("array", "-frobnicate", "a.dds", "-o", "x.dds"), "Unknown option"),
             (("array", "a.dds", "b.dds", "-o", "x.png"), "the output file must be .dds"),
             (("gif", "a.gif"), "not supported"), (("v-cross-fnz", "a.dds"), "not supported")]
    for args, message in cases:
        rc, out = _tool(*args)
        assert rc == 1 and message in out, (args, out)


def test_tool_wrong_face_count(tmp_path):
    """The inputs are read and counted on the host before a device is created: five faces are not a cube, a 2-D texture is not a cubemap."""
    import numpy as np
    import oracle
    assert oracle.have_ref(), "oracle/_ref/libdxtex_ref.so is missing: run build()"
    paths = []
    for k in range(5):
        p = tmp_path / f"f{k}.dds"
        p.write_bytes(bytes(oracle.ref_save_dds(np.full(4 * 4 * 4, k, np.uint8), 4, 4, 28)))
        paths.append(p)
    rc, out = _tool("cube", "-o", tmp_path / "c.dds", *paths)
    assert rc == 1 and "cube requires six images" in out and "no usable" not in out
    rc, out = _tool("cubearray", "-o", tmp_path / "c.dds", *paths)
    assert rc == 1 and "multiple of 6" in out
    rc, out = _tool("array", "-o", tmp_path / "c.dds", paths[0])
    assert rc == 1 and "Need at least 2 images" in out
    rc, out = _tool("h-cross", "-o", tmp_path / "c.dds", paths[0])
    assert rc == 1 and "Input must be a cubemap" in out
    rc, out = _tool("array-strip", "-o", tmp_path / "c.dds", paths[0])
    assert rc == 1 and "Input must be a 1D/2D array" in out
    assert not (tmp_path / "c.dds").exists()
