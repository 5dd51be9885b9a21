"""dxtexassemble on files: six seeded 16 x 16 faces written with the oracle's DDS writer, assembled by the tool, and its output files compared
byte for byte with the reference's own SaveToDDSMemory of the expected texture (oracle.ref_save_dds*), or, for the crosses, cut apart again.
Resize and Convert expectations come from the oracle's drivers; merge's from tests/assemble_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import assemble_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "dxtexassemble")
RGBA8, RGBA16F, RGBA32F = 28, 10, 2
CUBE = 0x4          # TEX_MISC_TEXTURECUBE
N = 16


def _run(*args, ok=True):
    out = subprocess.run([EXE, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert (out.returncode == 0) == ok, out.stdout + out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def faces(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("assemble")
    rng = np.random.default_rng(16)
    imgs = [rng.integers(1, 256, N * N * 4, dtype=np.uint8) for _ in range(6)]       # never 0: the cross's background is
    paths = []
    for k, im in enumerate(imgs):
        p = d / f"face{k}.dds"
        p.write_bytes(bytes(oracle.ref_save_dds(im, N, N, RGBA8)))
        paths.append(p)
    return d, imgs, paths


def _same_file(path, want):
    got = np.frombuffer(path.read_bytes(), np.uint8)
    want = np.asarray(want, np.uint8)
    assert got.size == want.size and np.array_equal(got, want), (got.size, want.size, np.flatnonzero(got[:min(got.size, want.size)] != want[:min(got.size, want.size)])[:8])


def test_cube_array_volume_cubearray(oracle, faces):
    d, imgs, paths = faces
    blob = np.concatenate(imgs)
    _run("cube", "-nologo", "-y", "-o", d / "cube.dds", *paths)
    _same_file(d / "cube.dds", oracle.ref_save_dds(blob, N, N, RGBA8, array_size=6, misc_flags=CUBE))
    _run("array", "-nologo", "-y", "-o", d / "array.dds", *paths)
    _same_file(d / "array.dds", oracle.ref_save_dds(blob, N, N, RGBA8, array_size=6))
    _run("volume", "-nologo", "-y", "-o", d / "volume.dds", *paths)
    _same_file(d / "volume.dds", oracle.ref_save_dds_volume(blob, N, N, 6, RGBA8))
    _run("cubearray", "-nologo", "-y", "-o", d / "cubearray.dds", *paths, *paths[::-1])
    _same_file(d / "cubearray.dds", oracle.ref_save_dds(np.concatenate(imgs + imgs[::-1]), N, N, RGBA8, array_size=12, misc_flags=CUBE))
    _run("cube", "-nologo", "-y", "-o", d / "five.dds", *paths[:5], ok=False)


@pytest.mark.parametrize("kind", ["hc", "vc", "ht", "hs", "vs"])
def test_cross_round_trip(oracle, faces, kind):
    d, imgs, paths = faces
    command = {"hc": "h-cross", "vc": "v-cross", "ht": "h-tee", "hs": "h-strip", "vs": "v-strip"}[kind]
    cols, rows = {"hc": (4, 3), "vc": (3, 4), "ht": (4, 3), "hs": (6, 1), "vs": (1, 6)}[kind]
    cube, cross, back = d / f"cube_{kind}.dds", d / f"cross_{kind}.dds", d / f"back_{kind}.dds"
    _run("cube", "-nologo", "-y", "-o", cube, *paths)
    _run(command, "-nologo", "-y", "-o", cross, cube)
    meta, px = oracle.ref_load_dds(np.frombuffer(cross.read_bytes(), np.uint8))
    assert (meta["width"], meta["height"], meta["arraySize"], meta["format"]) == (N * cols, N * rows, 1, RGBA8)
    px = np.asarray(px, np.uint8)[:N * cols * N * rows * 4]
    assert int((px != 0).sum()) == 6 * N * N * 4             # the faces (no byte of which is 0) and a zero background
    _run(f"cube-from-{kind}", "-nologo", "-y", "-o", back, cross)
    _same_file(back, np.frombuffer(cube.read_bytes(), np.uint8))
    _same_file(back, oracle.ref_save_dds(np.concatenate(imgs), N, N, RGBA8, array_size=6, misc_flags=CUBE))


def test_from_mips(oracle, faces):
    d, _, _ = faces
    rng = np.random.default_rng(5)
    chain, paths = [], []
    for level, n in enumerate([16, 8, 4, 2, 1]):
        im = rng.integers(0, 256, n * n * 4, dtype=np.uint8)
        p = d / f"mip{level}.dds"
        p.write_bytes(bytes(oracle.ref_save_dds(im, n, n, RGBA8)))
        chain.append(im); paths.append(p)
    _run("from-mips", "-nologo", "-y", "-o", d / "chain.dds", *paths)
    _same_file(d / "chain.dds", oracle.ref_save_dds(np.concatenate(chain), N, N, RGBA8, mip_levels=5))


def test_merge(oracle, faces):
    d, imgs, paths = faces
    _run("merge", "-nologo", "-y", "-swizzle", "rgbR", "-o", d / "merged.dds", paths[0], paths[1])
    b = np.asarray(oracle.ref_convert(imgs[1], N, N, RGBA8, RGBA32F, 0, 0.5)).view(np.uint8).view(np.float32).reshape(N, N, 4)
    want = R.merge(oracle, imgs[0], b, N, N, RGBA8, N * 4, (0, 1, 2, 4))
    _same_file(d / "merged.dds", oracle.ref_save_dds(want, N, N, RGBA8))
    _run("merge", "-nologo", "-y", "-o", d / "merged_default.dds", paths[0], paths[1])       # the default mask is rgbB
    _same_file(d / "merged_default.dds", oracle.ref_save_dds(R.merge(oracle, imgs[0], b, N, N, RGBA8, N * 4, (0, 1, 2, 6)), N, N, RGBA8))


def test_format_and_size_on_mixed_inputs(oracle, faces):
    d, imgs, paths = faces
    small = (np.random.default_rng(8).random((8, 8, 4), dtype=np.float32)).astype(np.float16)
    p = d / "small16f.dds"
    p.write_bytes(bytes(oracle.ref_save_dds(small, 8, 8, RGBA16F)))
    _run("array", "-nologo", "-y", "-w", N, "-h", N, "-f", "R8G8B8A8_UNORM", "-o", d / "mixed.dds", paths[0], p)
    resized = oracle.ref_resize(small, 8, 8, RGBA16F, N, N, 0)
    second = np.asarray(oracle.ref_convert(resized, N, N, RGBA16F, RGBA8, 0, 0.5)).view(np.uint8).reshape(-1)
    _same_file(d / "mixed.dds", oracle.ref_save_dds(np.concatenate([imgs[0], second]), N, N, RGBA8, array_size=2))


@pytest.mark.parametrize("command", ["gif", "v-cross-fnz", "cube-from-vc-fnz"])
def test_commands_left_out(command):
    out = _run(command, "input.dds", "-o", "out.dds", ok=False)
    assert "not supported" in out and len(out.strip().splitlines()) == 1
