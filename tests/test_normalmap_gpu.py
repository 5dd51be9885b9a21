"""ComputeNormalMap on the MI355X (nmap_kernel, directxtex_amd/csrc/scanline.hip) against the reference: byte for byte with the
digests of the reference's own output (tests/golden/normalmap.json) and with the numpy restatement (tests/nmap_ref.py) over a
flag x source x destination x size matrix; the device variant, the host layer, the HRESULTs, non-finite input and dxtexconv -nmap.

Non-finite rule. Where a result lane is NaN, the reference's sign and payload come from x86 SSE rules (the first NaN operand is
propagated, quieted; XMVector3Normalize writes 0x7FC00000 for an infinite length) and the GPU's from its own (operands may be
canonicalised, and a product by -1 may be compiled as a negation). So a NaN lane of a 32-bit FLOAT destination must be a NaN in both,
with any sign and payload. A 16-bit float store first clamps to +-65504 (XMVectorClamp, which lets a NaN through, as store_half does): a
lane that is NaN before the store must be a NaN half in both, with any sign and payload. Every other lane, and every
UNORM / SNORM destination (whose stores saturate NaN to a defined value), must be equal bit for bit."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import directxtex_amd as dx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import nmap_ref  # noqa: E402
import make_golden_normalmap as G  # noqa: E402

GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "normalmap.json")))["cases"]
RGBA32F, RGBA8 = 2, 28
E_FAIL, E_INVALIDARG, E_NOT_SUPPORTED = 0x80004005 - (1 << 32), 0x80070057 - (1 << 32), 0x80070032 - (1 << 32)


def _hr(e):
    return e.hresult


@pytest.mark.parametrize("case", GOLDEN, ids=[c["name"] for c in GOLDEN])
def test_golden(ctx, case):
    c = case
    pix = G.source_bytes(c["src"], c["width"], c["height"], c["seed"])
    if c["hr"]:
        with pytest.raises(dx.DxtexError) as e:
            ctx.compute_normal_map(pix, c["width"], c["height"], c["src"], c["dst"], c["flags"], c["amplitude"])
        assert _hr(e.value) & 0xFFFFFFFF == c["hr"]
        return
    got = ctx.compute_normal_map(pix, c["width"], c["height"], c["src"], c["dst"], c["flags"], c["amplitude"])
    assert hashlib.sha256(got.tobytes()).hexdigest() == c["sha256"], c["name"]


SOURCES = (28, 87, 10, 2, 61, 54, 41, 65)
DESTS = sorted(nmap_ref.IDENTITY_DESTINATIONS | {RGBA32F})
SIZES = ((1, 1), (1, 17), (17, 1), (255, 3), (256, 33), (257, 31), (300, 70), (600, 5))
FLAGS = (0, 1, 2, 3, 4, 5, 0x1000 | 5, 0x2000 | 1, 0x3000 | 0x8000 | 5, 0x4000 | 0x8000 | 2, 0x7000 | 0x8000 | 3)


def _matrix():
    out, k = [], 0
    for src in SOURCES:
        for (w, h) in SIZES:
            for fl in FLAGS:
                out.append((src, DESTS[k % len(DESTS)], w, h, fl, (1.0, 3.7, -2.0, 0.0, 100.0)[k % 5], k))
                k += 1
    return out


@pytest.mark.parametrize("src", SOURCES)
def test_matrix_equals_restatement(ctx, oracle, src):
    for s, dst, w, h, fl, amp, k in _matrix():
        if s != src:
            continue
        pad = (k % 3) * 4                        # padded row pitches on a third of the cases
        pitch = w * G.BPP_BYTES[src] + pad
        pix = G.source_bytes(src, w, h, 5000 + k, pitch)
        got = ctx.compute_normal_map(pix, w, h, src, dst, fl, amp, src_row_pitch=pitch)
        want = nmap_ref.compute_normal_map(oracle, pix, w, h, src, dst, fl, amp, row_pitch=pitch)
        assert np.array_equal(got, want), (src, dst, w, h, hex(fl), amp, np.nonzero(got != want)[0][:8])


def test_every_destination(ctx, oracle):
    w, h = 67, 45
    pix = G.source_bytes(RGBA8, w, h, 77)
    for dst in DESTS:
        for fl in (5 | 0x8000, 0x4000 | 2):
            got = ctx.compute_normal_map(pix, w, h, RGBA8, dst, fl, 3.7)
            assert np.array_equal(got, nmap_ref.compute_normal_map(oracle, pix, w, h, RGBA8, dst, fl, 3.7)), (dst, hex(fl))


def test_taller_than_the_grid(ctx, oracle):
    """more than 65535 rows: the strips stride over grid.y"""
    w, h = 3, 70001
    pix = G.source_bytes(RGBA32F, w, h, 99)
    for fl in (0x8000 | 1, 0x2000 | 5):
        got = ctx.compute_normal_map(pix, w, h, RGBA32F, RGBA8, fl, 2.0)
        assert np.array_equal(got, nmap_ref.compute_normal_map(oracle, pix, w, h, RGBA32F, RGBA8, fl, 2.0)), hex(fl)


def test_packed_destinations_go_through_float_rows(ctx, oracle):
    """R8G8_B8G8 / YUY2 / R1 and kin: the kernel's float rows stored by pack_group_kernel, as Convert from RGBA32F stores them."""
    w, h = 37, 9
    pix = G.source_bytes(RGBA8, w, h, 31)
    rows = nmap_ref.nmap_rows(oracle.load_image(pix, w, h, RGBA8), 5, 1.5, True)
    for dst in (68, 69, 107, 108, 109, 66):
        got = ctx.compute_normal_map(pix, w, h, RGBA8, dst, 5, 1.5)
        assert np.array_equal(got, oracle.ref_convert(rows, w, h, RGBA32F, dst, 0x1000, 0.0)), dst


def test_device_variant_equals_host_variant(ctx):
    import torch
    w, h, src, dst = 300, 70, RGBA8, 13
    pitch = w * 4 + 12
    pix = G.source_bytes(src, w, h, 123, pitch)
    want = ctx.compute_normal_map(pix, w, h, src, dst, 0x8000 | 5, 2.0, src_row_pitch=pitch)
    d_src = torch.from_numpy(pix.copy()).cuda()
    d_dst = torch.zeros(want.size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.transfer_bytes(reset=True)
    ctx.compute_normal_map_device(d_src.data_ptr(), w, h, src, d_dst.data_ptr(), dst, 0x8000 | 5, 2.0, src_row_pitch=pitch)
    ctx.synchronize()
    assert ctx.transfer_bytes() == (0, 0)
    assert np.array_equal(d_dst.cpu().numpy(), want)
    # the stencil cannot run in place: overlapping source and destination are refused
    with pytest.raises(dx.DxtexError) as e:
        ctx.compute_normal_map_device(d_src.data_ptr(), w, h, src, d_src.data_ptr() + 64, RGBA8, 0, 1.0)
    assert _hr(e.value) == E_INVALIDARG


def test_hresults(ctx):
    w, h = 8, 8
    pix = G.source_bytes(RGBA8, w, h, 1)
    cases = [((RGBA8, RGBA8, 6), E_INVALIDARG), ((RGBA8, RGBA8, 0xF), E_INVALIDARG), ((RGBA8, 0, 0), E_INVALIDARG), ((RGBA8, 192, 0), E_INVALIDARG),
             ((RGBA8, 83, 0), E_NOT_SUPPORTED), ((71, RGBA8, 0), E_NOT_SUPPORTED), ((RGBA8, 27, 0), E_NOT_SUPPORTED),      # BC5, BC1 source, TYPELESS
             ((RGBA8, 30, 0), E_NOT_SUPPORTED), ((RGBA8, 14, 0), E_NOT_SUPPORTED), ((RGBA8, 103, 0), E_NOT_SUPPORTED)]     # UINT, SINT, NV12
    out = np.zeros(w * h * 16, np.uint8)
    for (src, dst, fl), want in cases:
        # straight through the C ABI: ComputePitch knows none of the formats the call must refuse
        s = dx.Image(w, h, src, w * 4, w * h * 4, pix.ctypes.data)
        d = dx.Image(w, h, dst, w * 16, w * h * 16, out.ctypes.data)
        hr = ctx._lib.dxtex_compute_normal_map(ctx._h, s, d, fl, 1.0)
        assert hr == want, (src, dst, fl, hex(hr & 0xFFFFFFFF))
    # a size mismatch (only the C ABI can ask for one)
    import torch
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    s = dx.device_image(d.data_ptr(), 8, 8, RGBA8)
    t = dx.device_image(d.data_ptr() + 1024, 8, 7, RGBA8)
    assert ctx._lib.dxtex_compute_normal_map_device(ctx._h, s, t, 0, 1.0) == E_FAIL
    # the same format on both sides is allowed (Convert refuses it)
    assert ctx.compute_normal_map(pix, w, h, RGBA8, RGBA8, 0, 1.0).size == w * h * 4


def _nan_equal(got, want, dst, rows):
    if dst in (RGBA32F, 41):                      # a NaN lane matches any NaN, every other lane bit for bit
        g, r = got.view(np.float32), want.view(np.float32)
        return bool(np.all((np.isnan(g) & np.isnan(r)) | (g.view(np.uint32) == r.view(np.uint32))))
    if dst == 10:                                 # a lane that is NaN before the half store is a NaN half in both, every other lane bit for bit
        g, r = got.view(np.float16), want.view(np.float16)
        return bool(np.all((np.isnan(g) & np.isnan(r)) | (got.view(np.uint16) == want.view(np.uint16))))
    return np.array_equal(got, want)


def test_nonfinite_heights_and_amplitudes(ctx, oracle):
    w, h = 19, 11
    rng = np.random.default_rng(8)
    img = rng.normal(0, 1, (h, w, 4)).astype(np.float32)
    specials = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-45, -0.0], np.float32)
    idx = rng.integers(0, img.size, 60)
    img.reshape(-1)[idx] = specials[rng.integers(0, specials.size, idx.size)]
    for amp in (1.0, np.inf, -np.inf, np.nan, 1e30):
        for fl in (5 | 0x8000, 1 | 0x4000, 3 | 0x3000 | 0x8000):
            for dst in (RGBA32F, 41, 28, 13, 10):
                got = ctx.compute_normal_map(img, w, h, RGBA32F, dst, fl, float(amp))
                want = nmap_ref.compute_normal_map(oracle, img, w, h, RGBA32F, dst, fl, float(amp))
                rows = nmap_ref.nmap_rows(img, fl, float(amp), dst in nmap_ref.UNORM_DESTINATIONS)
                assert _nan_equal(got, want, dst, rows), (amp, hex(fl), dst)


def test_host_layer():
    exe = os.path.join(ROOT, "directxtex_amd", "lib", "nmap_host_test")
    if not os.path.exists(exe):
        pytest.fail(f"{exe} missing: run __graft_entry__.build()")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "nmap host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


EXE = os.path.join(ROOT, "directxtex_amd", "lib", "dxtexconv")


def _conv(args):
    r = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def test_dxtexconv_nmap_bc5(tmp_path, oracle):
    """-nmap l -f BC5_UNORM: ComputeNormalMap into R8G8B8A8_UNORM (texconv's intermediate for an 8-bit source), then BC5, in one
    upload and one download."""
    w, h = 96, 64
    pix = G.source_bytes(RGBA8, w, h, 404)
    src, out = tmp_path / "height.dds", tmp_path / "n.dds"
    oracle.ref_save_dds(pix, w, h, RGBA8).tofile(src)
    txt = _conv(["-nmap", "l", "-f", "BC5_UNORM", "-m", "1", "-timing", "-overlap", "1", "-o", str(out), str(src)])
    nm = nmap_ref.compute_normal_map(oracle, pix, w, h, RGBA8, RGBA8, 5, 1.0)
    payload = oracle.ref_compress_image(nm, w, h, RGBA8, 83, 0, 0.5)
    assert np.array_equal(np.fromfile(out, np.uint8), oracle.ref_save_dds(payload, w, h, 83))
    m = re.search(r"host -> device (\d+) bytes, device -> host (\d+) bytes", txt)
    assert m, txt
    assert int(m.group(1)) == w * h * 4 and int(m.group(2)) == payload.size, (m.group(0), payload.size)


def test_dxtexconv_nmap_snorm(tmp_path, oracle):
    w, h = 40, 24
    pix = G.source_bytes(RGBA8, w, h, 405)
    src, out = tmp_path / "height.dds", tmp_path / "n.dds"
    oracle.ref_save_dds(pix, w, h, RGBA8).tofile(src)
    _conv(["-nmap", "rmio", "-nmapamp", "2", "-f", "R16G16B16A16_SNORM", "-m", "1", "-o", str(out), str(src)])
    nm = nmap_ref.compute_normal_map(oracle, pix, w, h, RGBA8, 13, 1 | 0x3000 | 0x4000 | 0x8000, 2.0)
    assert np.array_equal(np.fromfile(out, np.uint8), oracle.ref_save_dds(nm, w, h, 13))
