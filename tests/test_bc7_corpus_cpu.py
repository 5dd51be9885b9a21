"""What the BC7 corpus (tests/bc7_corpus.py) reaches, measured without a GPU and without the code under test: every gate reads the reference encoder's
output (oracle/_ref/libdxtex_ref.so), and the host mirror of the core (oracle/_ref/bc7_core_check, bc7_lockstep_check: tools/bc7_debug.cpp) is run
on every uint8 family.

* census: every partition wins at least 4 blocks in each of modes 1, 3 and 7 (flags 0), mode 2 (64 partitions) and mode 0 (16 partitions, both with
  BC7_USE_3SUBSETS); every rotation of modes 4 and 5 and each index selector of mode 4 at least 8; mode 6 at least 8 opaque blocks and 8 with alpha;
  every mode 0 - 7 at least 8 somewhere.
* the recorded partition masks == what the decode recipe gives on the live reference decoder.
* host mirror (straight and through the kernels' per-lane pieces) == reference on every uint8 family: 0 differing tiles.
* the golden payloads == the live reference; RGBA8 images of the tiles, BGRA8 images and sRGB -> BC7_UNORM_SRGB give the same payloads.
"""
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import bc7_corpus as C  # noqa: E402
import make_golden_bc7_corpus as G  # noqa: E402

BC7, BC7_SRGB, RGBA8, RGBA8_SRGB, BGRA8, RGBA32F = 98, 99, 28, 29, 87, 2
CORE_EXE = os.path.join(ROOT, "oracle", "_ref", "bc7_core_check")
LOCKSTEP_EXE = os.path.join(ROOT, "oracle", "_ref", "bc7_lockstep_check")
PARTITION_FLOOR, FLOOR = 4, 8
CHUNK = 256
WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))
UINT8_SETS = [(w, s) for w in ("default", "3subsets") for s in G.SETS[w] if s != "off_grid"]


@pytest.fixture(scope="module")
def tiles():
    t = C.corpus()
    for v in t.values():
        v.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def ref(oracle, tiles):
    """(file, entry) -> the reference's payloads, computed once."""
    out = {}
    for which in G.FILES:
        for name, blocks in G.reference_payloads(which, tiles).items():
            blocks.setflags(write=False)
            out[which, name] = blocks
    return out


def _counts(ref, which, sets=None):
    """Winning blocks of a file's sets: (per mode (8,), mode -> per partition, mode -> per rotation, per index selector (2,))."""
    b = np.concatenate([ref[which, s] for s in (sets or G.SETS[which])])
    m = C.mode_field(b); p = C.partition_field(b); r = C.rotation_field(b); s = C.index_selector_field(b)
    parts = {mode: np.bincount(p[m == mode], minlength=16 if mode == 0 else 64) for mode in (0, 1, 2, 3, 7)}
    rots = {mode: np.bincount(r[m == mode], minlength=4) for mode in (4, 5)}
    return np.bincount(m, minlength=9)[:8], parts, rots, np.bincount(s[m == 4], minlength=2)


def _census_line(ref, which, name):
    modes, parts, rots, sel = _counts(ref, which, (name,))
    line = f"census {which} {name} ({len(ref[which, name])} tiles): " + ", ".join(f"{m}:{int(c)}" for m, c in enumerate(modes) if c)
    line += " | partitions " + ", ".join(f"m{m} {int((c > 0).sum())}/{len(c)} (min {int(c.min())})" for m, c in parts.items() if c.sum())
    return line + f" | rotations m4 {rots[4].tolist()} m5 {rots[5].tolist()} | m4 index selector {sel.tolist()}"


def test_census_print(ref):
    for which in G.FILES:
        for name in G.SETS[which]:
            print(_census_line(ref, which, name))


@pytest.mark.parametrize("which,mode", [("default", 1), ("default", 3), ("default", 7), ("3subsets", 2), ("3subsets", 0)])
def test_census_every_partition_wins_blocks(ref, which, mode):
    c = _counts(ref, which)[1][mode]
    print(f"census {which}: mode {mode} winners per partition: {c.tolist()}")
    assert len(c) == (16 if mode == 0 else 64)
    assert int(c.min()) >= PARTITION_FLOOR, f"mode {mode}: partitions below {PARTITION_FLOOR} winning blocks: {np.nonzero(c < PARTITION_FLOOR)[0].tolist()} ({c.tolist()})"


def test_census_every_rotation_and_index_selector_wins_blocks(ref):
    _, _, rots, sel = _counts(ref, "default")
    print(f"census default: rotations mode 4 {rots[4].tolist()}, mode 5 {rots[5].tolist()}, mode 4 index selector {sel.tolist()}")
    assert int(rots[4].min()) >= FLOOR and int(rots[5].min()) >= FLOOR and int(sel.min()) >= FLOOR


def test_census_mode_6_wins_opaque_blocks_and_blocks_with_alpha(ref, tiles):
    names = [s for s in G.SETS["default"] if s != "off_grid"]
    m = C.mode_field(np.concatenate([ref["default", s] for s in names]))
    opaque = np.concatenate([(tiles[s][:, :, 3] == 255).all(axis=1) for s in names])
    got = int(((m == 6) & opaque).sum()), int(((m == 6) & ~opaque).sum())
    print(f"census default: mode 6 wins {got[0]} opaque blocks and {got[1]} blocks with alpha")
    assert min(got) >= FLOOR, got


def test_census_every_mode_wins_blocks(ref):
    modes = _counts(ref, "default")[0] + _counts(ref, "3subsets")[0]
    print(f"census, both files: winners per mode {modes.tolist()}")
    assert int(modes.min()) >= FLOOR, modes.tolist()
    assert set(np.unique(C.mode_field(ref["default", "quick"])).tolist()) == {6}


def test_partition_masks_equal_the_reference_decoder(oracle):
    two, three = G.record_masks()
    got2, got3 = C.masks()
    assert got2.shape == (64, 16) and got3.shape == (64, 16) and got2.dtype == np.uint8 and got3.dtype == np.uint8
    assert np.array_equal(got2, two) and np.array_equal(got3, three), "rerun tests/golden/make_golden_bc7_corpus.py"
    # the recipe's landmarks: left / right, top / bottom, the diagonal; every partition is distinct and uses every subset
    assert got2[0].reshape(4, 4).tolist() == [[0, 0, 1, 1]] * 4
    assert got2[13].reshape(4, 4).tolist() == [[0] * 4, [0] * 4, [1] * 4, [1] * 4]
    assert got3[63].reshape(4, 4).tolist() == [[0, 1, 1, 1], [2, 0, 1, 1], [2, 2, 0, 1], [2, 2, 2, 0]]
    assert len({r.tobytes() for r in got2}) == 64 and len({r.tobytes() for r in got3}) == 64
    assert all(set(r.tolist()) == {0, 1} for r in got2) and all(set(r.tolist()) == {0, 1, 2} for r in got3)
    assert (got2[:, 0] == 0).all() and (got3[:, 0] == 0).all()          # texel 0 is subset 0's anchor


_DIFFER = re.compile(r"^(\d+) of (\d+) tiles differ$")
_MISMATCH = re.compile(r"^tile (\d+) MISMATCH: ref mode (\d+), ours mode (\d+)")


def _mirror(exe, tiles, flags, env=None):
    """The host mirror on `tiles` through its tile-file argument, in chunks run side by side: [(tile index, reference mode, mirror mode)] of the
    tiles that differ."""
    if not os.path.exists(exe):
        pytest.fail(f"{exe} missing: run __graft_entry__.build() where /root/reference exists")
    starts = list(range(0, len(tiles), CHUNK))
    with tempfile.TemporaryDirectory() as tmp:
        def run(s):
            part = np.ascontiguousarray(tiles[s:s + CHUNK], np.uint8)
            path = os.path.join(tmp, f"{s}.bin")
            part.tofile(path)
            r = subprocess.run([exe, str(len(part)), "1", hex(flags), path], capture_output=True, text=True, timeout=900, env=dict(os.environ, **(env or {})))
            lines = r.stdout.splitlines()
            m = _DIFFER.match(lines[-1]) if lines else None
            assert m and int(m.group(2)) == len(part) and r.returncode == (1 if int(m.group(1)) else 0), r.stdout[-2000:] + r.stderr[-2000:]
            bad = [(s + int(x.group(1)), int(x.group(2)), int(x.group(3))) for x in map(_MISMATCH.match, lines) if x]
            assert len(bad) == int(m.group(1)), r.stdout[-2000:]
            return bad
        with ThreadPoolExecutor(WORKERS) as pool:
            return [b for bad in pool.map(run, starts) for b in bad]


def _report(bad, n):
    return f"{len(bad)} of {n} tiles differ; first (tile, reference mode, mirror mode): {bad[:8]}"


@pytest.mark.parametrize("which,name", UINT8_SETS)
def test_host_mirror_equals_the_reference(tiles, which, name):
    bad = _mirror(CORE_EXE, tiles[name], G.FLAGS[which])
    assert not bad, _report(bad, len(tiles[name]))


@pytest.mark.parametrize("flat", ["every", "kernel"])
@pytest.mark.parametrize("which,name", UINT8_SETS)
def test_lockstep_pieces_equal_the_reference(tiles, which, name, flat):
    """OptimizeOne through the pieces the search kernels run per lane, on all partitions (test_bc7_core_cpu.py explains `flat`)."""
    bad = _mirror(LOCKSTEP_EXE, tiles[name], G.FLAGS[which], {"DXTEX_HOST_FLAT_SKIP": flat})
    assert not bad, _report(bad, len(tiles[name]))


@pytest.mark.parametrize("which", list(G.FILES))
def test_golden_payloads_equal_the_live_reference(ref, which):
    want = [k for w, k in ref if w == which]
    with np.load(G.FILES[which]) as z:
        assert sorted(z.files) == sorted(want)
        for name in want:
            assert z[name].dtype == np.uint8 and z[name].shape == ref[which, name].shape, name
            bad = np.nonzero((z[name] != ref[which, name]).reshape(-1, 16).any(axis=1))[0]
            assert bad.size == 0, f"{name}: {bad.size} golden blocks differ from the reference, first {bad[:8].tolist()} - rerun tests/golden/make_golden_bc7_corpus.py"
    assert os.path.getsize(G.FILES[which]) <= 311212          # no larger than the largest fixture before it (bc6h_corpus_sf16.npz)


def _same(got, want, tag):
    bad = np.nonzero((np.asarray(got).reshape(-1, 16) != want).any(axis=1))[0]
    assert bad.size == 0, f"{tag}: {bad.size} blocks differ from the block encoder's payloads, first {bad[:8].tolist()}"


def test_reference_images_give_the_tiles_payloads(oracle, tiles, ref):
    """What lets the GPU test compare images with the per-tile goldens: in the reference, Compress of as_image() from RGBA8, from B8G8R8A8 (channels
    swapped on the way in) and from R8G8B8A8_UNORM_SRGB to BC7_UNORM_SRGB gives the block encoder's payloads (on every sixth tile of two_alpha, four
    per partition, and every tenth of three_opaque). off_grid does NOT: Compress saturates a float source to [0, 1] first and the encoder's seeds read
    the floats, so its image has a golden entry of its own."""
    img, w, h = C.as_image(tiles["two_alpha"][::6])
    want = C.image_payload(ref["default", "two_alpha"][::6], (w // 4) * (h // 4))
    _same(oracle.ref_compress_image(img, w, h, RGBA8, BC7, 0, 0.5), want, "RGBA8")
    _same(oracle.ref_compress_image(np.ascontiguousarray(img[:, :, [2, 1, 0, 3]]), w, h, BGRA8, BC7, 0, 0.5), want, "BGRA8")
    _same(oracle.ref_compress_image(img, w, h, RGBA8_SRGB, BC7_SRGB, 0, 0.5), want, "sRGB to BC7_UNORM_SRGB")
    img, w, h = C.as_image(tiles["three_opaque"][::10])
    _same(oracle.ref_compress_image(img, w, h, RGBA8, BC7, G.USE_3SUBSETS, 0.5), C.image_payload(ref["3subsets", "three_opaque"][::10], (w // 4) * (h // 4)), "3SUBSETS")
    n = len(tiles["off_grid"])
    assert ref["default", "off_grid_image"].shape == (n, 16) and (ref["default", "off_grid_image"] != ref["default", "off_grid"]).any()


def test_off_grid_bytes_depend_on_unfused_fp32(tiles):
    """The family does what it is for: the encoder's byte, uint8(max(0, min(255, x * 255.0f + 0.01f))) in unfused float32, differs from the same
    expression with a fused multiply-add (one rounding) on part of the values, and truncates up to k + 1 on a large share."""
    x = tiles["off_grid"].reshape(-1)
    unfused = np.clip(x * np.float32(255.0) + np.float32(0.01), np.float32(0.0), np.float32(255.0)).astype(np.uint8)
    fused = np.clip((x.astype(np.float64) * 255.0 + np.float64(np.float32(0.01))).astype(np.float32), np.float32(0.0), np.float32(255.0)).astype(np.uint8)
    share = float((unfused != fused).mean())
    print(f"off_grid: {x.size} values, a fused multiply-add changes {int((unfused != fused).sum())} bytes ({100 * share:.2f} %); "
          f"below 0: {int((x < 0).sum())}, above 1: {int((x > 1).sum())}, -0.0: {int(((x == 0) & np.signbit(x)).sum())}")
    assert share >= 0.005 and (x < 0).any() and (x > 1).any() and ((x == 0) & np.signbit(x)).any() and np.isfinite(x).all()
