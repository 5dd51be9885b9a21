"""The portable pixmap codec of the host layer (host/DirectXTexAMD_PNM.cpp) and the texel rules it shares with the GPU kernels
(csrc/dxtex_pnm.h), against tests/pnm_ref.py, the Python restatement of Texconv/PortablePixMap.cpp: HRESULT, metadata, the raw loader's
description of the samples and the pixels, byte for byte, for every reader kind, every refusal, truncations at every byte and seeded
mutations of the header. Parity for the text parser rests on the restatement, not on the reference executed: its codec is Win32 code the
oracle cannot compile. The writer's one arithmetic step (half to float, BGRA to RGBA) is checked against the live oracle's Convert. The host
program also runs under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program. CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pnm_ref as R  # noqa: E402

LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK, HOST, HOST_ASAN = (os.path.join(LIB, n) for n in ("pnm_check", "pnm_host_test", "pnm_host_test_asan"))
WIDTHS, HEIGHTS = (1, 3, 4, 5), (1, 2, 5)
MAGIC = {R.P6: b"P6", R.PF: b"PF", R.Pf: b"Pf", R.PH: b"PH", R.Ph: b"Ph"}
# csrc/dxtex_pnm.h PnmSource, by image format
SOURCE = {R.RGBA8: 0, R.RGBA8_SRGB: 0, R.BGRA8: 1, R.BGRA8_SRGB: 1, R.BGRX8: 1, R.BGRX8_SRGB: 1, R.RGBA32F: 2, R.RGB32F: 3, R.RGBA16F: 4, R.R32F: 5}
TEXEL_BYTES = {R.RGBA32F: 16, R.RGB32F: 12, R.RGBA16F: 8, R.R32F: 4}

# bit patterns that must pass a float kind untouched: +-0, denormals, +-Inf, quiet and signalling NaNs with payloads
SPECIAL32 = np.array([0, 0x80000000, 1, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFA00000, 0x3F800000, 0x12345678], np.uint32)
SPECIAL16 = np.array([0, 0x8000, 1, 0x83FF, 0x7C00, 0xFC00, 0x7E01, 0xFE55, 0x7C01, 0xFD00, 0x3C00, 0x1234], np.uint16)


def samples(kind, w, h, rng, big_endian=False):
    """random samples of a kind as file bytes, the special bit patterns among them for the float kinds"""
    n = w * h * R.FILE_BYTES[kind]
    if kind == R.P6:
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    if kind in (R.PF, R.Pf):
        e = rng.integers(0, 2 ** 32, n // 4, dtype=np.uint32)
        e[::3] = SPECIAL32[rng.integers(0, len(SPECIAL32), len(e[::3]))]
        return e.astype(">u4" if big_endian else "<u4").tobytes()
    e = rng.integers(0, 2 ** 16, n // 2, dtype=np.uint16)
    e[::3] = SPECIAL16[rng.integers(0, len(SPECIAL16), len(e[::3]))]
    return e.astype(">u2" if big_endian else "<u2").tobytes()


def pnm_file(kind, w, h, rng, big_endian=False, maxval=255, comment=b""):
    if kind == R.P6:
        return b"P6\n" + comment + b"%d %d\n%d\n" % (w, h, maxval) + samples(kind, w, h, rng)
    return MAGIC[kind] + b"\n" + comment + b"%d %d\n" % (w, h) + (b"1.0\n" if big_endian else b"-1.000000\n") + samples(kind, w, h, rng, big_endian)


def p3_file(w, h, rng, maxval=255, sep=b" "):
    values = rng.integers(0, maxval + 40, w * h * 3)          # some above maxval: no clamp
    return b"P3\n# ascii\n%d %d\n%d\n" % (w, h, maxval) + sep.join(b"%d" % v for v in values) + b"\n"


def load_many(exe, tmp, files):
    """[(raw hresult, host hresult, None | dict of the line's fields with the pixels)] of `exe load_many` over the files"""
    paths = []
    for i, data in enumerate(files):
        paths.append(os.path.join(tmp, f"f{i}.pnm"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    listing = os.path.join(tmp, "list.txt")
    with open(listing, "w") as f:
        f.write("\n".join(paths) + "\n")
    r = subprocess.run([exe, "load_many", listing], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(files), r.stdout[-2000:]
    out = []
    names = ("width", "height", "format", "depth", "arraySize", "mipLevels", "miscFlags", "miscFlags2", "dimension", "kind", "maxval", "big_endian", "ascii", "offset", "nbytes")
    for i, line in enumerate(lines):
        t = line.split()
        assert int(t[0]) == i
        d = None
        if len(t) > 3:
            assert t[3] == "ok"
            d = dict(zip(names, (int(v) for v in t[4:])))
            d["pixels"] = np.fromfile(paths[i] + ".out", np.uint8)
        out.append((int(t[1], 16), int(t[2], 16), d))
    return out


def compare(files, got):
    for i, (data, (raw_hr, hr, d)) in enumerate(zip(files, got)):
        ref_hr, ref = R.load(data)
        where = (i, data[:80])
        assert raw_hr == ref_hr and hr == ref_hr, (where, hex(raw_hr), hex(hr), hex(ref_hr))
        if ref_hr:
            assert d is None
            continue
        for k in ("width", "height", "format", "kind", "maxval", "ascii"):
            assert d[k] == ref[k], (where, k, d[k], ref[k])
        assert (d["depth"], d["arraySize"], d["mipLevels"], d["miscFlags"], d["miscFlags2"], d["dimension"]) == (1, 1, 1, 0, 0, 3), where          # :297-302, :581-586
        assert bool(d["big_endian"]) == ref["big_endian"], where
        if not ref["ascii"]:
            assert (d["offset"], d["nbytes"]) == (ref["offset"], ref["nbytes"]), where
        assert np.array_equal(d["pixels"], ref["pixels"]), where


def reader_files():
    rng = np.random.default_rng(61)
    files = []
    for w in WIDTHS:
        for h in HEIGHTS:
            files.append(pnm_file(R.P6, w, h, rng))
            files.append(pnm_file(R.P6, w, h, rng, maxval=int(rng.integers(1, 255)), comment=b"# made by a test\n"))
            files.append(p3_file(w, h, rng))
            files.append(p3_file(w, h, rng, maxval=int(rng.integers(1, 70000)), sep=b"\n"))
            for kind in (R.PF, R.Pf, R.PH, R.Ph):
                for big in (False, True):
                    files.append(pnm_file(kind, w, h, rng, big, comment=b"# c\n" if big else b""))
    return files


def test_every_reader_kind(tmp_path):
    files = reader_files()
    got = load_many(HOST, str(tmp_path), files)
    assert all(hr == 0 for _, hr, _ in got)
    compare(files, got)


# one file per rule of the readers: (file, the HRESULT the rule names)
PX6 = bytes(range(18))
REFUSALS = [
    (b"", R.E_FAIL), (b"P6", R.E_FAIL), (b"Q6\n1 1\n255\nabc", R.E_FAIL), (b"P5\n1 1\n255\nabc", R.E_FAIL), (b"P6x1 1\n255\nabc", R.E_FAIL),
    # .ppm, :152-358
    (b"P6\n0 2\n255\n" + PX6, R.E_FAIL), (b"P6\n3 0\n255\n" + PX6, R.E_FAIL),
    (b"P6\n2147483648 1\n255\n" + PX6, R.E_NOT_SUPPORTED), (b"P6\n1 2147483648\n255\n" + PX6, R.E_NOT_SUPPORTED),
    (b"P6\n4294967299 2\n255\n" + PX6, R.S_OK),          # decimal numbers wrap in uint32_t: a width of 3
    (b"P6\n32768 32768\n255\n" + PX6, R.E_ARITHMETIC_OVERFLOW), (b"P6\n3 2\n0\n" + PX6, R.E_FAIL),
    (b"P6\n3 2\n256\n" + PX6, R.E_UNEXPECTED), (b"P6\n3 2\n255 " + PX6, R.E_FAIL), (b"P6\n3 2\n255\r\n" + PX6, R.S_OK),
    (b"P6\n3 2\n255\r" + PX6, R.E_FAIL), (b"P6\n3 2\n255\n\n" + PX6[:17], R.S_OK),          # the second '\n' is the first sample
    (b"P6\n3 2\n255\n" + PX6[:17], R.E_HANDLE_EOF), (b"P6\n3 2\n255\n" + PX6[:16], R.E_HANDLE_EOF), (b"P6\n3 2\n255\n" + PX6[:15], R.E_FAIL),
    (b"P6\n3 2\n255\n", R.E_HANDLE_EOF), (b"P6\n3 2\n255", R.E_FAIL), (b"P6\n3 2\n255\n" + PX6 + b"surplus", R.S_OK),
    (b"P6\n3 x\n255\n" + PX6, R.E_FAIL), (b"P6\n-3 2\n255\n" + PX6, R.E_FAIL), (b"P6\n3 2 # no newline", R.E_FAIL),
    (b"P3\n1 1\n255\n1 2", R.E_FAIL), (b"P3\n1 1\n255\n1 2 3", R.S_OK), (b"P3\n1 1\n0\n1 2 3", R.E_FAIL), (b"P3\n1 1\n255\n1 2 x", R.E_FAIL),
    (b"P3\n1 1\n300\n300 600 4294967295\n", R.S_OK), (b"P3\n1 1\n7\n9 8 16843010 5", R.S_OK),          # (u * 255) / max in uint32_t, no clamp
    # .pfm / .phm, :452-684
    (b"PF1 1\n-1\n" + bytes(12), R.E_FAIL), (b"PF\n", R.E_FAIL), (b"PG\n1 1\n-1\n" + bytes(12), R.E_FAIL),
    (b"PF\n\n1 1\n-1\n" + bytes(12), R.E_FAIL), (b"PF\n1 1", R.E_FAIL), (b"PF\n" + b"1" * 300 + b" 1\n-1\n" + bytes(12), R.E_FAIL),
    (b"PF\n" + b" " * 252 + b"1 1\n-1\n" + bytes(12), R.E_FAIL),          # a 255-character line
    (b"PF\n" + b" " * 251 + b"1 1\n-1\n" + bytes(12), R.S_OK), (b"PF\n#" + b"c" * 254 + b"\n1 1\n-1\n" + bytes(12), R.S_OK),
    (b"PF\n1 1 1\n-1\n" + bytes(12), R.E_FAIL), (b"PF\n1\n-1\n" + bytes(12), R.E_FAIL), (b"PF\nx 1\n-1\n" + bytes(12), R.E_FAIL),
    (b"PF\n1 1\n-1 2\n" + bytes(12), R.E_FAIL), (b"PF\n1 1\nx\n" + bytes(12), R.E_FAIL), (b"PF\n1 1\nnan\n" + bytes(12), R.S_OK),
    (b"PF\n1 1\n0x1p3\n" + bytes(12), R.S_OK), (b"PF\n1 1\n-0\n" + bytes(12), R.S_OK), (b"PF\n1 1\n-1e-50\n" + bytes(12), R.S_OK),
    (b"PF\n# a\n# b\n1 1\n# c\n-1\n" + bytes(12), R.S_OK), (b"PF\n# a\n", R.E_FAIL), (b"PF\n1 1\n", R.E_FAIL), (b"PF\n1 1\n-1\n", R.E_FAIL),
    (b"PF\n2147483648 1\n-1\n" + bytes(12), R.E_NOT_SUPPORTED), (b"PF\n1 -1\n-1\n" + bytes(12), R.E_NOT_SUPPORTED),
    (b"PF\n16384 16385\n-1\n" + bytes(12), R.E_ARITHMETIC_OVERFLOW), (b"Pf\n32768 32768\n-1\n" + bytes(12), R.E_ARITHMETIC_OVERFLOW),
    (b"Ph\n32768 65536\n-1\n" + bytes(12), R.E_ARITHMETIC_OVERFLOW), (b"PH\n16384 32768\n-1\n" + bytes(12), R.E_ARITHMETIC_OVERFLOW),
    (b"PF\n1 1\n-1\n" + bytes(11), R.E_HANDLE_EOF), (b"PH\n2 1\n-1\n" + bytes(11), R.E_HANDLE_EOF), (b"Pf\n2 2\n-1\n" + bytes(15), R.E_HANDLE_EOF),
    (b"Ph\n3 1\n-1\n" + bytes(5), R.E_HANDLE_EOF), (b"PF\n0 1\n-1\n" + bytes(12), R.E_INVALIDARG), (b"PF\n1 0\n-1\n" + bytes(12), R.E_INVALIDARG),
    (b"PF\n1\0 1\n-1\n" + bytes(12), R.E_FAIL),          # the line is cut at a NUL: one number
]


def test_every_refusal(tmp_path):
    files = [f for f, _ in REFUSALS]
    got = load_many(HOST, str(tmp_path), files)
    for (data, want), (raw_hr, hr, _) in zip(REFUSALS, got):
        assert raw_hr == want and hr == want, (data[:60], hex(raw_hr), hex(hr), hex(want))
    compare(files, got)


def fuzz_corpus():
    """truncations at every byte of a small file of each family, and seeded mutations of the header bytes"""
    rng = np.random.default_rng(67)
    bases = [pnm_file(R.P6, 3, 2, rng, comment=b"# c\n"), pnm_file(R.P6, 2, 2, rng, maxval=100), p3_file(2, 2, rng), pnm_file(R.PF, 2, 2, rng, comment=b"#x\n"),
             pnm_file(R.Ph, 3, 2, rng, True), pnm_file(R.PH, 1, 3, rng), pnm_file(R.Pf, 2, 1, rng, True)]
    files = [b[:cut] for b in bases for cut in range(len(b) + 1)]
    alphabet = b"0123456789  \n\n\r\t#-+.eP36FfHh\0\xff"
    for _ in range(600):
        b = bytearray(bases[int(rng.integers(len(bases)))])
        head = bytes(b).rfind(b"\n", 0, 24) + 2
        for _ in range(int(rng.integers(1, 4))):
            op, at = rng.random(), int(rng.integers(0, head))
            if op < 0.5:
                b[at] = alphabet[int(rng.integers(len(alphabet)))]
            elif op < 0.8:
                b.insert(at, alphabet[int(rng.integers(len(alphabet)))])
            else:
                del b[at]
        if rng.random() < 0.15:
            del b[int(rng.integers(0, len(b))):]
        files.append(bytes(b))
    return files


def test_fuzz_against_the_restatement(tmp_path):
    files = fuzz_corpus()
    got = load_many(HOST, str(tmp_path), files)
    compare(files, got)
    hrs = {hr for _, hr, _ in got}
    assert {R.S_OK, R.E_FAIL, R.E_HANDLE_EOF} <= hrs, [hex(h) for h in hrs]


def test_fuzz_under_sanitizers(tmp_path):
    """the same corpus and the refusals through the sanitized stand-alone build: same answers, no report"""
    files = fuzz_corpus() + [f for f, _ in REFUSALS] + reader_files()
    compare(files, load_many(HOST_ASAN, str(tmp_path), files))


def save(tmp, pixels, w, h, fmt, hdr, row_pitch=None, name="img"):
    src = os.path.join(tmp, name + ".bin")
    out = os.path.join(tmp, name + ".out")
    pixels = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    pixels.tofile(src)
    r = subprocess.run([HOST, "save", src, str(w), str(h), str(fmt), str(row_pitch or pixels.size // h), str(int(hdr)), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hr = int(r.stdout.split()[1], 16)
    return hr, (open(out, "rb").read() if hr == 0 else None)


def widen(halves):
    """the reference's Convert(R16G16B16A16_FLOAT -> R32G32B32_FLOAT) of (h, w, 3) halves, from the live oracle"""
    h, w = halves.shape[:2]
    rgba = np.zeros((h, w, 4), np.uint16)
    rgba[..., :3] = halves
    return oracle.ref_convert(rgba, w, h, R.RGBA16F, R.RGB32F).view(np.uint32).reshape(h, w, 3)


@pytest.mark.parametrize("fmt", [R.RGBA8, R.RGBA8_SRGB, R.BGRA8, R.BGRA8_SRGB, R.BGRX8, R.BGRX8_SRGB])
def test_ppm_writer(tmp_path, oracle, fmt):
    rng = np.random.default_rng(fmt)
    for w in WIDTHS:
        for h in HEIGHTS:
            px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
            hr, data = save(str(tmp_path), px, w, h, fmt, False)
            assert hr == 0 and data == R.save_ppm(px, fmt), (w, h)
            # the one arithmetic step, from the live oracle: Convert to R8G8B8A8 (:399-401)
            rgba = px if fmt in (R.RGBA8, R.RGBA8_SRGB) else oracle.ref_convert(px, w, h, fmt, R.RGBA8_SRGB if fmt in (R.BGRA8_SRGB, R.BGRX8_SRGB) else R.RGBA8).reshape(h, w, 4)
            assert data.endswith(np.ascontiguousarray(rgba[..., :3]).tobytes())
            # save then load returns the pixels, alpha forced to one
            back_hr, back = R.load(data)
            got = load_many(HOST, str(tmp_path), [data])[0]
            assert back_hr == 0 and got[1] == 0 and np.array_equal(got[2]["pixels"], back["pixels"])
            want = rgba.copy(); want[..., 3] = 255
            assert np.array_equal(got[2]["pixels"].reshape(h, w, 4), want)


@pytest.mark.parametrize("fmt", [R.RGBA32F, R.RGB32F, R.RGBA16F, R.R32F])
def test_pfm_writer(tmp_path, oracle, fmt):
    rng = np.random.default_rng(fmt)
    ch = {R.RGBA32F: 4, R.RGB32F: 3, R.RGBA16F: 4, R.R32F: 1}[fmt]
    for w in WIDTHS:
        for h in HEIGHTS:
            if fmt == R.RGBA16F:
                px = rng.integers(0, 2 ** 16, (h, w, ch), dtype=np.uint16)
                px[0, 0, :3] = SPECIAL16[rng.integers(0, len(SPECIAL16), 3)]
            else:
                px = rng.integers(0, 2 ** 32, (h, w, ch), dtype=np.uint32)
                px.reshape(-1)[::5] = SPECIAL32[rng.integers(0, len(SPECIAL32), len(px.reshape(-1)[::5]))]
            hr, data = save(str(tmp_path), px, w, h, fmt, True)
            assert hr == 0 and data == R.save_pfm(px, fmt, widen), (w, h)
            # the float payload is the oracle's Convert to R32G32B32_FLOAT (:727), flipped by numpy
            if fmt != R.R32F:
                conv = oracle.ref_convert(px, w, h, fmt, R.RGB32F).view(np.uint32).reshape(h, w, 3) if fmt != R.RGB32F else px
                assert data.endswith(np.ascontiguousarray(conv[::-1]).astype("<u4").tobytes())
            got = load_many(HOST, str(tmp_path), [data])[0]
            assert got[1] == 0
            if fmt == R.R32F:
                assert np.array_equal(got[2]["pixels"].view(np.uint32).reshape(h, w, 1), px)
            else:
                back = got[2]["pixels"].view(np.uint32).reshape(h, w, 4)
                assert np.array_equal(back[..., :3], widen(px[..., :3]) if fmt == R.RGBA16F else px[..., :3]) and (back[..., 3] == 0x3F800000).all()


def test_writer_refusals(tmp_path):
    px = np.zeros((2, 2, 4), np.uint32)
    for fmt, hdr in ((R.RGBA32F, False), (R.RGBA8, True), (R.R16F, True), (61, False), (R.RGB32F, False), (24, False)):          # R8_UNORM 61, R10G10B10A2_UNORM 24
        assert save(str(tmp_path), px, 2, 2, fmt, hdr, row_pitch=32)[0] == R.E_NOT_SUPPORTED, fmt


def run_check(*args):
    r = subprocess.run([CHECK, *[str(a) for a in args]], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)


def test_p6_texel_whole_domain(tmp_path):
    """every maxval 1..255 against every byte 0..255 in every channel (65 280 samples a channel), bytes above maxval and their spill included"""
    out = str(tmp_path / "p6.bin")
    run_check("p6", out)
    got = np.fromfile(out, np.uint32).reshape(256, 256)
    b = np.arange(256, dtype=np.uint32)
    texels = np.stack([b, 255 - b, b ^ 0x5A], axis=1).astype(np.uint8)
    for maxval in range(1, 256):
        want = R.unpack(texels.tobytes(), R.P6, 256, 1, maxval).view(np.uint32)
        assert np.array_equal(got[maxval - 1], want), maxval
    assert np.array_equal(got[255], got[254])          # maxval 255: the identity route and the table agree
    assert np.array_equal(got[254], texels.astype(np.uint32) @ np.array([1, 256, 65536], np.uint32) | 0xFF000000)
    # the no-clamp spill, explicitly: maxval 1, samples (255, 0, 2) -> c = (65025, 0, 510): 65025 | 510 << 16 | 0xff000000
    assert got[0][255] == (65025 | (0 << 8) | (((255 ^ 0x5A) * 255) << 16) | 0xFF000000) & 0xFFFFFFFF
    assert R.unpack(bytes([255, 0, 2]), R.P6, 1, 1, 1).view(np.uint32)[0] == 65025 | (510 << 16) | 0xFF000000
    # maxval 100, sample 200 in green: c_1 = 510 reaches into blue
    assert R.unpack(bytes([0, 200, 0]), R.P6, 1, 1, 100).view(np.uint32)[0] == (510 << 8) | 0xFF000000


def test_texel_rules_against_the_restatement(tmp_path, oracle):
    rng = np.random.default_rng(71)
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for kind in (R.P6, R.PF, R.Pf, R.PH, R.Ph):
        for big in ((False,) if kind == R.P6 else (False, True)):
            for w, h in ((1, 1), (3, 2), (5, 5)):
                maxval = int(rng.integers(1, 256)) if kind == R.P6 else 255
                data = samples(kind, w, h, rng, big)
                open(src, "wb").write(data)
                run_check("unpack", kind, int(big), maxval, w, h, src, out)
                assert np.array_equal(np.fromfile(out, np.uint8), R.unpack(data, kind, w, h, maxval, big)), (kind, big, w, h)
    for fmt in SOURCE:
        for w, h in ((1, 1), (3, 2), (5, 5)):
            if fmt in TEXEL_BYTES:
                dt = np.uint16 if fmt == R.RGBA16F else np.uint32
                px = rng.integers(0, np.iinfo(dt).max + 1, (h, w, TEXEL_BYTES[fmt] // dt().itemsize), dtype=dt)
                want = R.save_pfm(px, fmt, widen)
            else:
                px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
                want = R.save_ppm(px, fmt)
            px.tofile(src)
            run_check("pack", SOURCE[fmt], w, h, src, out)
            assert want.endswith(open(out, "rb").read()) and os.path.getsize(out) == w * h * (3 if fmt not in TEXEL_BYTES else 4 if fmt == R.R32F else 12), (fmt, w, h)


def test_every_half_widens_like_the_oracle(tmp_path, oracle):
    out = str(tmp_path / "half.bin")
    run_check("half", out)
    got = np.fromfile(out, np.uint32)
    halves = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    rgb = np.stack([halves, halves[::-1], halves.T], axis=2)
    assert np.array_equal(got[rgb], widen(rgb))


def test_format_tables_over_the_whole_domain():
    """The tables the C ABI and the host codec share (csrc/dxtex_pnm.h): the writer's source and the kind it is written as for every format
    0..191 - everything outside SOURCE refused - and the reader's one format per kind."""
    pack, unpack = {}, {}
    for line in subprocess.run([CHECK, "formats"], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines():
        p = line.split()
        if p[0] == "pack":
            pack[int(p[1])] = (int(p[2]), int(p[3]))
        else:
            unpack[int(p[1])] = int(p[2])
    kind_of_source = {0: R.P6, 1: R.P6, 2: R.PF, 3: R.PF, 4: R.PF, 5: R.Pf}
    assert pack == {f: (SOURCE[f], kind_of_source[SOURCE[f]]) if f in SOURCE else (-1, -1) for f in range(192)}
    assert unpack == R.KIND_FORMAT
