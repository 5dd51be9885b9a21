"""What the BC6H corpus (tests/bc6h_corpus.py) reaches, measured without a GPU and without the code under test: every gate reads the reference
encoder's output (oracle/_ref/libdxtex_ref.so) or the host mirror of the core (oracle/_ref/bc6h_core_check, bc6h_ep16_check: tools/bc6h_debug.cpp).

* census: which modes and partition shapes WIN blocks of the `smooth` family. 13 of the 14 modes must win at least 8 tiles each, in UF16 and in both
  SF16 variants; every one of the 32 shapes at least 4 two-region blocks.
* overflow states: on the two families at the top of the half range the SF16 search of the 16-bit one-region mode must end above 32767 - B only,
  A and B, A only - in the stated shares of the tiles (bc6h_encode.hip: Ep16 / ep16_mark carry those states through 16-bit records).
* host mirror == reference on every family and format, and the golden payloads == the live reference.

Mode 0x0F (16:4), outcome of the hunt: it wins NO tile of the smooth, near-top and bright families (0 of 24 096 per format), nor of flat tiles at
bit patterns of 512 and more; it DOES win on the smallest half bit patterns (denormals: patterns below 32, spreads of at most four patterns). A
hunt over 87 000 such tiles (one minute of CPU) gave, per 3 000 tiles: SF16 2 151 winners on base randint(0, 4) + randint(0, 4), 2 042 on
randint(0, 8) per texel, 2 417 on two-value tiles below 20; UF16 160 on randint(0, 4) per texel, 25 on base + spread below 8, 0 from patterns of
16 on. (Quantize returns the value itself from 15 bits on, about half of what UF16's FinishUnquantize ((x * 31) >> 6) needs, so in UF16 the 16:4
candidate starts a factor two off and has to cross that inside its 4-bit delta: only values of a few patterns can.) These tiles are the fourth
family, `tiny_bits`, with a floor of 8 winning tiles per format.
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
import bc6h_corpus as C  # noqa: E402
import make_golden_bc6h_corpus as G  # noqa: E402

UF16, SF16 = 95, 96
CORE_EXE = os.path.join(ROOT, "oracle", "_ref", "bc6h_core_check")
EP16_EXE = os.path.join(ROOT, "oracle", "_ref", "bc6h_ep16_check")
MODES_REQUIRED = (0x00, 0x01, 0x02, 0x06, 0x0A, 0x0E, 0x12, 0x16, 0x1A, 0x1E, 0x03, 0x07, 0x0B)
MODE_FLOOR, SHAPE_FLOOR = 8, 4
CHUNK = 500
WORKERS = max(1, min(8, len(os.sched_getaffinity(0))))


@pytest.fixture(scope="module")
def tiles():
    t = C.corpus()
    for v in t.values():
        v.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def ref(oracle, tiles):
    """(format, set name) -> the reference's payloads, computed once."""
    out = {}
    for fmt in (UF16, SF16):
        for name, blocks in G.reference_payloads(fmt, tiles).items():
            blocks.setflags(write=False)
            out[fmt, name] = blocks
    return out


def _mirror(exe, tiles, signed):
    """The host mirror's `file` mode on `tiles`, in chunks run side by side: (payloads (n, 16) uint8, stdout lines that are not payload lines with the
    chunk's first tile index)."""
    if not os.path.exists(exe):
        pytest.fail(f"{exe} missing: run __graft_entry__.build() where /root/reference exists")
    n = len(tiles)
    starts = list(range(0, n, CHUNK))
    with tempfile.TemporaryDirectory() as tmp:
        def run(s):
            path = os.path.join(tmp, f"{s}.bin")
            np.ascontiguousarray(tiles[s:s + CHUNK], np.float32).tofile(path)
            r = subprocess.run([exe, "file", path, "1" if signed else "0"], capture_output=True, text=True, timeout=900)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
            return r.stdout.splitlines()
        with ThreadPoolExecutor(WORKERS) as pool:
            outs = list(pool.map(run, starts))
    blocks = np.zeros((n, 2), np.uint64)
    notes = []
    for s, lines in zip(starts, outs):
        for ln in lines:
            f = ln.split()
            if len(f) == 3 and f[0].isdigit():
                blocks[s + int(f[0])] = (int(f[1], 16), int(f[2], 16))
            else:
                notes.append((s, ln))
    return blocks.view(np.uint8).reshape(n, 16), notes


def _census_line(blocks):
    m = C.mode_field(blocks); s = C.shape_field(blocks)
    modes = {int(k): int(v) for k, v in zip(*np.unique(m, return_counts=True))}
    shapes = np.bincount(s[s >= 0], minlength=32)
    return modes, shapes, ", ".join(f"0x{k:02X}: {v}" for k, v in sorted(modes.items())) + f" | shapes reached {int((shapes > 0).sum())}, min per shape {int(shapes.min())}"


@pytest.mark.parametrize("fmt,name", [(UF16, "smooth"), (SF16, "smooth"), (SF16, "smooth_signs")])
def test_census_every_mode_but_0x0f_and_every_shape_wins_blocks(ref, fmt, name):
    modes, shapes, line = _census_line(ref[fmt, name])
    print(f"census {'UF16' if fmt == UF16 else 'SF16'} {name} (N = {C.SMOOTH_N}, seed {C.SMOOTH_SEED}): {line}")
    short = {f"0x{m:02X}": modes.get(m, 0) for m in MODES_REQUIRED if modes.get(m, 0) < MODE_FLOOR}
    assert not short, f"modes below {MODE_FLOOR} winning tiles: {short} ({line})"
    assert int(shapes.min()) >= SHAPE_FLOOR, f"shapes below {SHAPE_FLOOR} two-region winners: {np.nonzero(shapes < SHAPE_FLOOR)[0].tolist()} ({line})"


@pytest.mark.parametrize("fmt", [UF16, SF16])
def test_census_mode_0x0f_wins_blocks_of_the_tiny_family(ref, fmt):
    modes, _, line = _census_line(ref[fmt, "tiny"])
    per_kind = (C.mode_field(ref[fmt, "tiny"]).reshape(len(C.TINY_KINDS), -1) == 0x0F).sum(axis=1)
    print(f"census {'UF16' if fmt == UF16 else 'SF16'} tiny (n = {C.TINY_N} per sub-kind, seed {C.TINY_SEED}): {line} | 0x0F per sub-kind {dict(zip(C.TINY_KINDS, per_kind.tolist()))}")
    assert modes.get(0x0F, 0) >= MODE_FLOOR, line


def test_census_of_the_overflow_families(ref):
    """Reported, not gated: which modes win at the top of the half range, and that 0x0F wins none there (the GPU test asserts the same of the kernels)."""
    for fmt in (UF16, SF16):
        for name in ("near_top", "bright"):
            print(f"census {'UF16' if fmt == UF16 else 'SF16'} {name}: {_census_line(ref[fmt, name])[2]}")


_EP16 = re.compile(r"ep16: (\d+) tiles, (\d+) searched in 16:4 \| above 32767 before the swap: A only (\d+), B only (\d+), both (\d+) \| "
                   r"A <= 32767 after the swap: (\d+), (\d+), (\d+) \| fit after the swap: (\d+), (\d+), (\d+) \((\d+) with a lower error")


@pytest.fixture(scope="module")
def ep16_runs(tiles):
    """set name -> (payloads, counters summed over the chunks, tiles that fit after the swap) of the counting host mirror on SF16."""
    out = {}
    for name in ("near_top", "bright"):
        blocks, notes = _mirror(EP16_EXE, tiles[name], True)
        tot = np.zeros(12, np.int64); fits = []
        for start, ln in notes:
            m = _EP16.match(ln)
            if m:
                tot += np.array([int(x) for x in m.groups()], np.int64)
            elif ln.startswith("ep16 fit after swap: tile "):
                fits.append((start + int(ln.split()[5]), ln))
        assert tot[0] == len(tiles[name]), f"{name}: counter lines cover {tot[0]} of {len(tiles[name])} tiles"
        out[name] = (blocks, tot, fits)
    return out


# shares of the TILES of a family whose SF16 16:4 search ends in the state, before SwapIndices
@pytest.mark.parametrize("name,floors", [("near_top", {"B only": 0.30, "both": 0.05}), ("bright", {"A only": 0.02, "B only": 0.20})])
def test_sf16_16bit_search_ends_above_32767(ep16_runs, ref, name, floors):
    blocks, tot, fits = ep16_runs[name]
    n = int(tot[0])
    got = {"A only": int(tot[2]), "B only": int(tot[3]), "both": int(tot[4])}
    print(f"ep16 SF16 {name}: {n} tiles, {int(tot[1])} searched in 16:4 | before the swap: " + ", ".join(f"{k} {v} ({100.0 * v / n:.1f} %)" for k, v in got.items())
          + f" | A <= 32767 after the swap: {tot[5]}, {tot[6]}, {tot[7]} | fit after the swap: {tot[8]}, {tot[9]}, {tot[10]} ({tot[11]} with a lower error)")
    if fits:
        print(f"ep16 SF16 {name}: tiles whose endpoints FIT after the swap (class 0 / 2: A was above 32767 before it - the kernels' 'never fits' mark would change bytes):")
        for idx, ln in fits:
            print(f"  tile {idx}: {ln}")
    for k, floor in floors.items():
        assert got[k] >= floor * n, f"{name}: '{k}' reached by {got[k]} of {n} tiles, floor {floor * 100:.0f} %"
    # the counting build is the same encoder: its payloads equal the reference's too
    bad = np.nonzero((blocks != ref[SF16, name]).any(axis=1))[0]
    assert bad.size == 0, f"bc6h_ep16_check differs from the reference on {bad.size} of {n} tiles, first {bad[:8].tolist()}"


@pytest.mark.parametrize("fmt,name", [(f, s) for f in (UF16, SF16) for s in G.SETS[f]])
def test_host_mirror_equals_the_reference(tiles, ref, fmt, name):
    blocks, _ = _mirror(CORE_EXE, tiles[name], fmt == SF16)
    want = ref[fmt, name]
    bad = np.nonzero((blocks != want).any(axis=1))[0]
    assert bad.size == 0, (f"{bad.size} of {len(want)} tiles differ, first {bad[:8].tolist()}, mode fields mirror "
                           f"{[int(x) & 31 for x in blocks[bad[:8], 0]]} reference {[int(x) & 31 for x in want[bad[:8], 0]]}")


@pytest.mark.parametrize("fmt", [UF16, SF16])
def test_golden_payloads_equal_the_live_reference(ref, fmt):
    with np.load(G.FILES[fmt]) as z:
        assert sorted(z.files) == sorted(G.SETS[fmt] + ("crops",))
        for name in G.SETS[fmt] + ("crops",):
            assert z[name].dtype == np.uint8 and z[name].shape == ref[fmt, name].shape, name
            bad = np.nonzero((z[name] != ref[fmt, name]).reshape(-1, 16).any(axis=1))[0]
            assert bad.size == 0, f"{name}: {bad.size} golden blocks differ from the reference, first {bad[:8].tolist()} - rerun tests/golden/make_golden_bc6h_corpus.py"
