"""ComputeNormalMap without a GPU. Three layers of parity:
  * tests/nmap_ref.py (a numpy restatement of the reference's ComputeNMap) equals the digests of the reference's own output
    (tests/golden/normalmap.json, made by tests/golden/make_golden_normalmap.py);
  * directxtex_amd/lib/nmap_check - directxtex_amd/csrc/dxtex_nmap.h, the arithmetic the GPU kernel runs, compiled for the host -
    equals those digests, and the restatement bit for bit over a wider seeded sweep;
  * dxtexconv parses -nmap / -nmapamp as texconv does."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import nmap_ref  # noqa: E402
import make_golden_normalmap as G  # noqa: E402

EXE = os.path.join(ROOT, "directxtex_amd", "lib", "nmap_check")
CONV = os.path.join(ROOT, "directxtex_amd", "lib", "dxtexconv")
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "normalmap.json")))["cases"]
OK_CASES = [c for c in GOLDEN if c["hr"] == 0]


def _sha(b):
    return hashlib.sha256(np.ascontiguousarray(b).view(np.uint8).tobytes()).hexdigest()


def _nmap_check(rows, flags, amplitude, unorm, tmp_path):
    if not os.path.exists(EXE):
        pytest.fail(f"{EXE} missing: run __graft_entry__.build()")
    h, w = rows.shape[:2]
    fin, fout = str(tmp_path / "in.f32"), str(tmp_path / "out.f32")
    np.ascontiguousarray(rows, np.float32).tofile(fin)
    bits = struct.unpack("<I", struct.pack("<f", amplitude))[0]
    subprocess.run([EXE, fin, str(w), str(h), hex(flags), f"{bits:08x}", "1" if unorm else "0", fout], check=True, timeout=120)
    return np.fromfile(fout, np.float32).reshape(h, w, 4)


def test_golden_covers_the_issue_matrix():
    assert len(OK_CASES) >= 40
    assert {c["flags"] & 0xF for c in OK_CASES} == {0, 1, 2, 3, 4, 5}
    assert {c["src"] for c in OK_CASES} == {2, 10, 28, 87, 61, 54, 41, 65}
    assert {c["amplitude"] for c in OK_CASES} >= {0.0, 1.0, 3.7, -2.0, 100.0}
    assert {(c["width"], c["height"]) for c in OK_CASES} >= {(1, 1), (1, 9), (9, 1), (2, 2), (67, 45)}
    for bit in (0x1000, 0x2000, 0x4000, 0x8000):
        assert any(c["flags"] & bit for c in OK_CASES) and any(not c["flags"] & bit for c in OK_CASES)


@pytest.mark.parametrize("case", OK_CASES, ids=[c["name"] for c in OK_CASES])
def test_restatement_equals_the_reference(oracle, case):
    c = case
    pix = G.source_bytes(c["src"], c["width"], c["height"], c["seed"])
    got = nmap_ref.compute_normal_map(oracle, pix, c["width"], c["height"], c["src"], c["dst"], c["flags"], c["amplitude"])
    assert _sha(got) == c["sha256"], c["name"]


@pytest.mark.parametrize("case", OK_CASES, ids=[c["name"] for c in OK_CASES])
def test_kernel_arithmetic_on_the_host_equals_the_reference(oracle, case, tmp_path):
    c = case
    pix = G.source_bytes(c["src"], c["width"], c["height"], c["seed"])
    rows = oracle.load_image(pix, c["width"], c["height"], c["src"])
    out = _nmap_check(rows, c["flags"], c["amplitude"], c["dst"] in nmap_ref.UNORM_DESTINATIONS, tmp_path)
    assert _sha(nmap_ref.store(oracle, out, c["dst"])) == c["sha256"], c["name"]


def test_kernel_arithmetic_on_the_host_equals_the_restatement(tmp_path):
    """A wider seeded sweep of float heights (signed, large and tiny values, every flag combination), compared as float rows."""
    rng = np.random.default_rng(77)
    for k in range(48):
        w, h = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        rows = (rng.normal(0, 1, (h, w, 4)) * rng.choice([1e-3, 1.0, 50.0, 1e18])).astype(np.float32)
        flags = int(rng.integers(0, 6)) | int(rng.choice([0, 0x1000])) | int(rng.choice([0, 0x2000])) | int(rng.choice([0, 0x4000])) | int(rng.choice([0, 0x8000]))
        amp = float(rng.choice([0.0, 1.0, 3.7, -2.0, 100.0, float(rng.normal(0, 10))]))
        unorm = bool(k & 1)
        got = _nmap_check(rows, flags, amp, unorm, tmp_path)
        want = nmap_ref.nmap_rows(rows, flags, amp, unorm)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (k, w, h, hex(flags), amp)


def _conv(args):
    return subprocess.run([CONV] + args, capture_output=True, text=True, timeout=60)


def test_dxtexconv_nmap_options(tmp_path, oracle):
    d = str(tmp_path)
    rng = np.random.default_rng(3)
    oracle.ref_save_dds(rng.integers(0, 256, 8 * 8 * 4, dtype=np.uint8), 8, 8, 28).tofile(d + "/h.dds")
    for args in (["-nmapamp", "2", "-nmap", "l"], ["-nmap", "xyz"], ["-nmap", "l", "-nmapamp", "-1"], ["-nmap", "muio"], ["-nmap", "l", "-nmapamp", "abc"]):
        r = _conv(args + ["-o", d + "/x.dds", d + "/h.dds"])
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert "nmap" in r.stderr or "amplitude" in r.stderr, (args, r.stderr)
    for args in (["-nmap", "l", "-nmapamp", "4"], ["-nmap", "rmio", "-nmapamp", "2"], ["--normal-map", "gu", "--normal-map-amplitude", "0.5"]):
        r = _conv(args + ["-info", d + "/h.dds"])
        assert r.returncode == 0, (args, r.stderr)
    assert "-nmap" in _conv([]).stderr
    r = _conv(["-hflip", "-o", d + "/x.dds", d + "/h.dds"])          # flips stay refused
    assert r.returncode == 1 and "usage: dxtexconv" in r.stderr
