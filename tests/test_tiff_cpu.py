"""The TIFF codec without a GPU: csrc/dxtex_tiff.h as plain C++ (tiff_check), and the host codec (tiff_host_test, and tiff_host_test_asan - the
same program with AddressSanitizer and UndefinedBehaviorSanitizer on the codec, run directly) against tests/tiff_ref.py, against Pillow's decodes
of the files Pillow wrote (tests/golden/tiff) and of files built here, over a table of damaged files, every truncation of two files and a fuzz."""
import io
import os
import struct
import subprocess

import numpy as np
import pytest

import tiff_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden", "tiff")
PROGRAMS = ("tiff_host_test", "tiff_host_test_asan")
E_FAIL, NOT_SUPPORTED, E_INVALIDARG, NOT_FOUND = 0x80004005, 0x80070032, 0x80070057, 0x80070002


def _run(exe, *args):
    path = os.path.join(LIB, exe)
    assert os.path.exists(path), f"directxtex_amd/lib/{exe} is missing: run build()"
    return subprocess.run([path, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)


def _samples(kind, h, w, seed):
    rng = np.random.default_rng(seed)
    bits, S, _, _ = T.KINDS[kind]
    if bits == 32:
        a = rng.standard_normal((h, w, S)).astype(np.float32)
        a.reshape(-1).view(np.uint32)[::7] ^= 0x7F000001          # bit patterns no arithmetic would keep
        return a
    return rng.integers(0, 1 << bits, (h, w, S), dtype=np.uint16 if bits == 16 else np.uint8)


def _colormap(bits, seed=3):
    return [int(v) for v in np.random.default_rng(seed).integers(0, 65536, 3 << bits)]


def _load_many(exe, tmp_path, files, flags=0):
    """files: [bytes] -> [(raw hr, host hr, metadata hr, fields or None, pixels or None)]"""
    paths = []
    for i, data in enumerate(files):
        p = tmp_path / f"f{i}.tif"
        p.write_bytes(data)
        paths.append(p)
    lst = tmp_path / "list.txt"
    lst.write_text("".join(f"{p}\n" for p in paths))
    r = _run(exe, "load_many", lst, flags)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(files), r.stdout
    out = []
    for i, line in enumerate(lines):
        f = line.split()
        assert int(f[0]) == i
        hrs = tuple(int(x, 16) for x in f[1:4])
        if len(f) > 4:
            assert f[4] == "ok"
            out.append(hrs + ([int(x) for x in f[5:]], open(str(paths[i]) + ".out", "rb").read()))
        else:
            out.append(hrs + (None, None))
    return out


def _check_against_ref(exe, tmp_path, files, flags=0):
    got = _load_many(exe, tmp_path, files, flags)
    for i, (data, g) in enumerate(zip(files, got)):
        hr, want = T.decode(data, flags)
        assert g[0] == g[1] == hr, (i, [hex(x) for x in g[:3]], hex(hr))
        assert g[2] == hr or (hr != 0 and g[2] == 0), (i, hex(g[2]), hex(hr))          # the header alone may still be sound
        if hr:
            continue
        info = want["info"]
        width, height, fmt, misc2, compression, kind, predictor, be, planar, wiz, opaque, nseg, stream_bytes = g[3]
        assert (width, height, fmt, misc2) == (want["width"], want["height"], want["format"], want["alpha"]), (i, g[3])
        assert (compression,) + (width, height, info["bits"], info["samples"], kind, predictor, be, planar, wiz, opaque) == (info["compression"],) + T.layout_of(info), (i, g[3])
        stream, segs = T.segments(info)
        assert (nseg, stream_bytes) == (len(segs), len(stream)), (i, g[3], len(segs), len(stream))
        assert g[4] == want["pixels"], i
    return got


def test_rules_header():
    r = subprocess.run([os.path.join(LIB, "tiff_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "" and r.stderr == "", r.stdout + r.stderr


# ---- files spelled out byte by byte ---------------------------------------------------------------------------------------------------------------
def _ifd_le(entries, at):
    return struct.pack("<H", len(entries)) + b"".join(struct.pack("<HHII", *e) for e in entries) + struct.pack("<I", 0)


def _predictor3_file():
    """II, 2 x 1 grey float, uncompressed bytes under Compression 8 would need a coder, so: LZW of six literal codes is avoided too - the
    strip is stored as a deflate "stored" block, every byte of it written here. Texels 1.0 and -2.5: big-endian bytes 3F 80 00 00 and C0 20 00 00;
    the four byte planes of the row are 3F C0 | 80 20 | 00 00 | 00 00, and the byte-wise differences with stride 1 are
    3F 81 C0 A0 E0 00 00 00."""
    coded = bytes([0x3F, 0x81, 0xC0, 0xA0, 0xE0, 0x00, 0x00, 0x00])
    adler_a = (1 + sum(coded)) % 65521
    adler_b = sum((1 + sum(coded[:k + 1])) for k in range(8)) % 65521
    strip = bytes([0x78, 0x01, 0x01, 0x08, 0x00, 0xF7, 0xFF]) + coded + struct.pack(">HH", adler_b, adler_a)
    entries = [(256, 3, 1, 2), (257, 3, 1, 1), (258, 3, 1, 32), (259, 3, 1, 8), (262, 3, 1, 1), (273, 4, 1, 8), (277, 3, 1, 1), (279, 4, 1, len(strip)), (317, 3, 1, 3), (339, 3, 1, 3)]
    data = b"II" + struct.pack("<HI", 42, 8 + len(strip) + (len(strip) & 1)) + strip + bytes(len(strip) & 1) + _ifd_le(entries, 0)
    return data, struct.pack("<ff", 1.0, -2.5)


def _mm16_predictor2_file():
    """MM, 3 x 2 grey 16, predictor 2 under LZW: each row's big-endian differences. Row 0: 0x0102, 0x0304, 0x0001 -> 0102, +0202, +FCFD;
    row 1: 0xFFFF, 0x0000, 0x8000 -> FFFF, +0001, +8000. The LZW stream is written out: Clear, the twelve bytes as literals, EOI - fourteen
    9-bit codes, MSB first (no width change before code 510)."""
    coded = bytes([0x01, 0x02, 0x02, 0x02, 0xFC, 0xFD, 0xFF, 0xFF, 0x00, 0x01, 0x80, 0x00])
    bits = "".join(format(c, "09b") for c in [256] + list(coded) + [257])
    bits += "0" * (-len(bits) % 8)
    strip = bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))
    assert len(strip) == 16
    e = [(256, 3, 1, 3), (257, 3, 1, 2), (258, 3, 1, 16), (259, 3, 1, 5), (262, 3, 1, 1), (273, 4, 1, 8), (277, 3, 1, 1), (278, 3, 1, 2), (279, 4, 1, 16), (317, 3, 1, 2)]
    ifd = struct.pack(">H", len(e)) + b"".join(struct.pack(">HHI", t, ty, c) + (struct.pack(">HH", v, 0) if ty == 3 else struct.pack(">I", v)) for t, ty, c, v in e) + struct.pack(">I", 0)
    return b"MM" + struct.pack(">HI", 42, 24) + strip + ifd, struct.pack("<6H", 0x0102, 0x0304, 0x0001, 0xFFFF, 0x0000, 0x8000)


@pytest.mark.parametrize("exe", PROGRAMS)
def test_files_spelled_out(exe, tmp_path):
    (f3, want3), (f16, want16) = _predictor3_file(), _mm16_predictor2_file()
    got = _load_many(exe, tmp_path, [f3, f16])
    assert got[0][:3] == (0, 0, 0) and got[0][3][:3] == [2, 1, T.R32_FLOAT] and got[0][4] == want3, got[0]
    assert got[1][:3] == (0, 0, 0) and got[1][3][:3] == [3, 2, T.R16_UNORM] and got[1][4] == want16, got[1]
    assert got[0][3][5:8] == [T.GREY32F, 3, 0] and got[1][3][5:8] == [T.GREY16, 2, 1]
    for data, want in ((f3, want3), (f16, want16)):          # and the restatement reads them the same
        hr, d = T.decode(data)
        assert hr == 0 and d["pixels"] == want


# ---- every kind x compression x predictor x layout --------------------------------------------------------------------------------------------------
def _matrix():
    files, seed = [], 0
    for kind in range(14):
        bits, S, _, _ = T.KINDS[kind]
        predictors = [1] + ([2] if bits in (8, 16) else []) + ([3] if bits == 32 else [])
        cm = _colormap(bits) if kind in (T.PAL1, T.PAL4, T.PAL8) else None
        for compression in (T.NONE, T.LZW, T.DEFLATE, T.ADOBE_DEFLATE, T.PACKBITS):
            for predictor in predictors:
                layouts = [dict(), dict(rows_per_strip=2, big_endian=True), dict(tile=(16, 16))]
                if S > 1:
                    layouts += [dict(planar=True), dict(planar=True, tile=(16, 16), big_endian=True)]
                for lay in layouts:
                    seed += 1
                    extra = {T.RGBA8: 2, T.RGBA16: 1, T.RGBA32F: None}.get(kind) if S == 4 else None
                    files.append(T.build(_samples(kind, 5, 21, seed), kind, compression=compression, predictor=predictor, colormap=cm, extra=extra,
                                         white_is_zero=(seed % 3 == 0 and S == 1 and cm is None and bits != 32), **lay))
    return files


@pytest.mark.parametrize("exe", PROGRAMS)
def test_every_kind_compression_predictor_and_layout(exe, tmp_path):
    files = _matrix()
    assert len(files) > 250
    got = _check_against_ref(exe, tmp_path, files)
    assert all(g[0] == 0 for g in got)


@pytest.mark.parametrize("exe", PROGRAMS)
def test_golden_files_against_pillows_decode(exe, tmp_path):
    names = sorted(n[:-4] for n in os.listdir(GOLDEN) if n.endswith(".tif"))
    assert len(names) >= 10
    files = [open(os.path.join(GOLDEN, n + ".tif"), "rb").read() for n in names]
    assert all(len(f) <= 8192 for f in files)
    got = _check_against_ref(exe, tmp_path, files)
    predictors = set()
    for n, g in zip(names, got):
        w, h, fmt = [int(x) for x in open(os.path.join(GOLDEN, n + ".txt")).read().split()]
        assert g[0] == 0 and g[3][:3] == [w, h, fmt], (n, g[3])
        assert g[4] == open(os.path.join(GOLDEN, n + ".bin"), "rb").read(), n
        predictors.add((g[3][4], g[3][6]))
    assert {(5, 2), (8, 2), (32773, 1), (1, 1), (5, 1)} <= predictors          # libtiff's LZW, deflate and PackBits, with and without predictor 2


def test_restatement_against_pillow_on_files_built_here():
    """where Pillow opens what tiff_ref.build makes, both decodes agree: planar MM RGB 8, 16 x 16 tiles, strips, every coder, grey 16 of either
    byte order, bilevel WhiteIsZero and a palette"""
    Image = pytest.importorskip("PIL.Image")
    a = _samples(T.RGB8, 20, 18, 1)
    for kw in (dict(planar=True, big_endian=True), dict(tile=(16, 16)), dict(rows_per_strip=3), dict(tile=(16, 16), planar=True)):
        for compression in (T.NONE, T.LZW, T.ADOBE_DEFLATE, T.PACKBITS):
            for predictor in (1, 2):
                data = T.build(a, T.RGB8, compression=compression, predictor=predictor, **kw)
                im = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))
                hr, d = T.decode(data)
                assert hr == 0 and d["pixels"] == im.tobytes(), (kw, compression, predictor)
    g = _samples(T.GREY16, 7, 9, 2)
    for be in (False, True):
        data = T.build(g, T.GREY16, compression=T.LZW, predictor=2, big_endian=be)
        assert T.decode(data)[1]["pixels"] == np.asarray(Image.open(io.BytesIO(data))).astype("<u2").tobytes()
    b = _samples(T.GREY1, 5, 11, 3)
    data = T.build(b, T.GREY1, white_is_zero=True)
    assert T.decode(data)[1]["pixels"] == Image.open(io.BytesIO(data)).convert("L").tobytes()
    p = _samples(T.PAL4, 5, 7, 4)
    data = T.build(p, T.PAL4, colormap=_colormap(4), compression=T.PACKBITS)
    assert T.decode(data)[1]["pixels"] == Image.open(io.BytesIO(data)).convert("RGBA").tobytes()
    # the LZW coder here against libtiff's decoder beyond the first width changes and the table's end
    big = _samples(T.GREY8, 40, 300, 5)
    data = T.build(big, T.GREY8, compression=T.LZW)
    assert np.asarray(Image.open(io.BytesIO(data))).tobytes() == big.tobytes() == T.decode(data)[1]["pixels"]


# ---- damaged files, with the HRESULT each is refused with --------------------------------------------------------------------------------------------
def _damaged():
    rgb, grey, rgba = _samples(T.RGB8, 4, 6, 1), _samples(T.GREY8, 4, 6, 2), _samples(T.RGBA8, 4, 6, 3)
    g16, f32, g1 = _samples(T.GREY16, 4, 6, 4), _samples(T.GREY32F, 4, 6, 5), _samples(T.GREY1, 4, 6, 6)
    good = T.build(rgb, T.RGB8, compression=T.LZW, predictor=2, rows_per_strip=2)
    tiled = T.build(rgb, T.RGB8, tile=(16, 16))
    big = 0x7FFFFFF0
    cases = [
        # NOT_SUPPORTED, every reason DirectXTexAMD.h states
        ("BigTIFF", T.build(rgb, T.RGB8, magic=43), NOT_SUPPORTED),
        ("JPEG compression", T.build(rgb, T.RGB8, override={259: (3, [7])}), NOT_SUPPORTED),
        ("old JPEG compression", T.build(rgb, T.RGB8, override={259: (3, [6])}), NOT_SUPPORTED),
        ("CCITT RLE", T.build(g1, T.GREY1, override={259: (3, [2])}), NOT_SUPPORTED),
        ("CCITT group 4", T.build(g1, T.GREY1, override={259: (3, [4])}), NOT_SUPPORTED),
        ("an unknown compression", T.build(rgb, T.RGB8, override={259: (3, [34712])}), NOT_SUPPORTED),
        ("YCbCr", T.build(rgb, T.RGB8, photometric=6), NOT_SUPPORTED),
        ("CMYK", T.build(rgba, T.RGBA8, photometric=5), NOT_SUPPORTED),
        ("CIELab", T.build(rgb, T.RGB8, photometric=8), NOT_SUPPORTED),
        ("a transparency mask", T.build(g1, T.GREY1, photometric=4), NOT_SUPPORTED),
        ("signed integers", T.build(g16, T.GREY16, sample_format=2), NOT_SUPPORTED),
        ("16-bit floats", T.build(g16, T.GREY16, sample_format=3), NOT_SUPPORTED),
        ("64-bit floats", T.build(f32, T.GREY32F, bits_list=[64]), NOT_SUPPORTED),
        ("32-bit integers", T.build(f32, T.GREY32F, sample_format=1), NOT_SUPPORTED),
        ("complex samples", T.build(f32, T.GREY32F, sample_format=6), NOT_SUPPORTED),
        ("2 bits", T.build(grey, T.GREY8, bits_list=[2]), NOT_SUPPORTED),
        ("12 bits", T.build(g16, T.GREY16, bits_list=[12]), NOT_SUPPORTED),
        ("unequal bits", T.build(rgb, T.RGB8, bits_list=[8, 8, 16]), NOT_SUPPORTED),
        ("5-6-5 bits", T.build(rgb, T.RGB8, bits_list=[5, 6, 5]), NOT_SUPPORTED),
        ("grey plus alpha", T.build(grey, T.GREY8, override={277: (3, [2]), 258: (3, [8, 8]), 338: (3, [2])}), NOT_SUPPORTED),
        ("palette plus alpha", T.build(grey, T.PAL8, colormap=_colormap(8), override={277: (3, [2]), 258: (3, [8, 8]), 338: (3, [2])}), NOT_SUPPORTED),
        ("two extra samples", T.build(rgba, T.RGBA8, override={277: (3, [5]), 258: (3, [8] * 5), 338: (3, [0, 2])}), NOT_SUPPORTED),
        ("FillOrder 2", T.build(g1, T.GREY1, fill_order=2), NOT_SUPPORTED),
        ("old-style LZW", (lambda f: f[:8] + b"\x00\x01" + f[10:])(T.build(grey, T.GREY8, compression=T.LZW)), NOT_SUPPORTED),
        ("predictor 2 on 1 bit", T.build(g1, T.GREY1, compression=T.LZW, override={317: (3, [2])}), NOT_SUPPORTED),
        ("predictor 2 on 4 bits", T.build(_samples(T.GREY4, 4, 6, 7), T.GREY4, compression=T.LZW, override={317: (3, [2])}), NOT_SUPPORTED),
        ("predictor 2 on floats", T.build(f32, T.GREY32F, compression=T.LZW, override={317: (3, [2])}), NOT_SUPPORTED),
        ("predictor 3 on 16 bits", T.build(g16, T.GREY16, compression=T.DEFLATE, override={317: (3, [3])}), NOT_SUPPORTED),
        ("an unknown predictor", T.build(grey, T.GREY8, compression=T.DEFLATE, override={317: (3, [4])}), NOT_SUPPORTED),
        ("WhiteIsZero floats", T.build(f32, T.GREY32F, photometric=0), NOT_SUPPORTED),
        ("RGB of 4 bits", T.build(rgb, T.RGB8, bits_list=[4, 4, 4]), NOT_SUPPORTED),
        ("a 16-bit palette", T.build(g16, T.GREY16, photometric=3, colormap=_colormap(8)), NOT_SUPPORTED),
        # E_FAIL: the header
        ("no byte order", b"XX" + good[2:], E_FAIL),
        ("mixed byte order", b"IM" + good[2:], E_FAIL),
        ("magic 41", T.build(rgb, T.RGB8, magic=41), E_FAIL),
        ("seven bytes", good[:7], E_FAIL),
        ("an empty file", b"", E_FAIL),
        # E_FAIL: every offset and count against the file
        ("the IFD behind the file", good[:4] + struct.pack("<I", len(good) + 1) + good[8:], E_FAIL),
        ("the IFD in the header", good[:4] + struct.pack("<I", 4) + good[8:], E_FAIL),
        ("the IFD at the last byte", good[:4] + struct.pack("<I", len(good) - 1) + good[8:], E_FAIL),
        ("more entries than the file holds", good[:struct.unpack_from("<I", good, 4)[0]] + struct.pack("<H", 60000) + good[struct.unpack_from("<I", good, 4)[0] + 2:], E_FAIL),
        ("a strip offset behind the file", T.build(rgb, T.RGB8, override={273: (4, [big])}), E_FAIL),
        ("a strip that leaves the file", T.build(rgb, T.RGB8, override={279: (4, [big])}), E_FAIL),
        ("a strip offset of the file's size with one byte", T.build(rgb, T.RGB8, override={273: (4, [len(T.build(rgb, T.RGB8))]), 279: (4, [1])}), E_FAIL),
        ("a tile offset behind the file", T.build(rgb, T.RGB8, tile=(16, 16), override={324: (4, [big])}), E_FAIL),
        ("a tile that leaves the file", T.build(rgb, T.RGB8, tile=(16, 16), override={325: (4, [big])}), E_FAIL),
        ("BitsPerSample's values behind the file", T.build(rgba, T.RGBA8, extra=2, override={258: (4, [8, 8, 8, 8, 8, 8, 8])})[:-30], E_FAIL),
        ("a ColorMap behind the file", T.build(grey, T.PAL8, colormap=_colormap(8))[:-900], E_FAIL),
        ("the Exif IFD behind the file", T.build(rgb, T.RGB8, override={34665: (4, [big])}), E_FAIL),
        ("the Exif IFD in the header", T.build(rgb, T.RGB8, override={34665: (4, [2])}), E_FAIL),
        ("fewer strip offsets than strips", T.build(rgb, T.RGB8, rows_per_strip=1, override={273: (4, [8, 8])}), E_FAIL),
        ("fewer strip counts than strips", T.build(rgb, T.RGB8, rows_per_strip=1, override={279: (4, [18])}), E_FAIL),
        ("fewer tile offsets than tiles", T.build(_samples(T.RGB8, 20, 18, 8), T.RGB8, tile=(16, 16), override={324: (4, [8, 8])}), E_FAIL),
        # E_FAIL: what is missing or makes no image
        ("no width", T.build(rgb, T.RGB8, drop=(256,)), E_FAIL),
        ("no length", T.build(rgb, T.RGB8, drop=(257,)), E_FAIL),
        ("no photometric", T.build(rgb, T.RGB8, drop=(262,)), E_FAIL),
        ("no strip offsets", T.build(rgb, T.RGB8, drop=(273,)), E_FAIL),
        ("no strip counts", T.build(rgb, T.RGB8, drop=(279,)), E_FAIL),
        ("no tile counts", T.build(rgb, T.RGB8, tile=(16, 16), drop=(325,)), E_FAIL),
        ("no tile width", T.build(rgb, T.RGB8, tile=(16, 16), drop=(322,)), E_FAIL),
        ("a tile width of zero", T.build(rgb, T.RGB8, tile=(16, 16), override={322: (3, [0])}), E_FAIL),
        ("no ColorMap", T.build(grey, T.PAL8, colormap=_colormap(8), drop=(320,)), E_FAIL),
        ("a short ColorMap", T.build(grey, T.PAL8, colormap=_colormap(4)), E_FAIL),
        ("a width of zero", T.build(rgb, T.RGB8, override={256: (4, [0])}), E_FAIL),
        ("a width beyond the limit", T.build(rgb, T.RGB8, override={256: (4, [0x10000000])}), E_FAIL),
        ("a width as a RATIONAL", T.build(rgb, T.RGB8, override={256: (5, [(6, 1)])}), E_FAIL),
        ("RowsPerStrip of zero", T.build(rgb, T.RGB8, override={278: (3, [0])}), E_FAIL),
        ("no samples", T.build(rgb, T.RGB8, override={277: (3, [0])}), E_FAIL),
        ("RGB of two samples", T.build(rgb, T.RGB8, override={277: (3, [2])}), E_FAIL),
        ("PlanarConfiguration 3", T.build(rgb, T.RGB8, override={284: (3, [3])}), E_FAIL),
        ("FillOrder 3", T.build(rgb, T.RGB8, fill_order=3), E_FAIL),
        ("ExtraSamples of another count", T.build(rgba, T.RGBA8, override={338: (3, [2, 2])}), E_FAIL),
        ("fewer bits than samples", T.build(rgb, T.RGB8, bits_list=[8, 8]), E_FAIL),
        # E_FAIL: a segment that expands to fewer bytes than its rows need
        ("a short uncompressed strip", T.build(rgb, T.RGB8, override={279: (4, [4 * 6 * 3 - 1])}), E_FAIL),
        ("a short LZW strip", T.build(_samples(T.RGB8, 3, 6, 9), T.RGB8, compression=T.LZW, override={257: (4, [4])}), E_FAIL),
        ("a short deflate strip", T.build(_samples(T.RGB8, 3, 6, 9), T.RGB8, compression=T.DEFLATE, override={257: (4, [4])}), E_FAIL),
        ("a short PackBits strip", T.build(_samples(T.RGB8, 3, 6, 9), T.RGB8, compression=T.PACKBITS, override={257: (4, [4])}), E_FAIL),
        ("an LZW strip of no bytes", T.build(rgb, T.RGB8, compression=T.LZW, override={279: (4, [0])}), E_FAIL),
        ("an image far larger than its file could hold", T.build(grey, T.GREY8, compression=T.LZW, override={256: (4, [60000]), 257: (4, [60000])}), E_FAIL),
    ]
    # an LZW stream that names a code it has not made yet, and a deflate stream with a damaged check value
    lzw = bytearray(T.build(grey, T.GREY8, compression=T.LZW))
    lzw[8 + 1] |= 0x7F; lzw[8 + 2] |= 0xC0          # the first code behind Clear becomes 511
    cases.append(("an LZW code that is not in the table", bytes(lzw), E_FAIL))
    z = bytearray(T.build(grey, T.GREY8, compression=T.DEFLATE))
    n = struct.unpack_from("<I", z, 4)[0]
    cases.append(("a deflate strip that is not a zlib stream", bytes(z[:8]) + b"\x00\x00" + bytes(z[10:]), E_FAIL))
    return cases


@pytest.mark.parametrize("exe", PROGRAMS)
def test_damaged_files_are_refused_with_their_hresults(exe, tmp_path):
    cases = _damaged()
    assert len(cases) >= 40
    files = [c[1] for c in cases]
    got = _load_many(exe, tmp_path, files)
    for (what, data, want), g in zip(cases, got):
        assert g[0] == g[1] == want, (what, hex(g[0]), hex(g[1]), hex(want))
        assert T.decode(data)[0] == want, (what, hex(T.decode(data)[0]))          # and the restatement refuses it likewise


@pytest.mark.parametrize("exe", PROGRAMS)
def test_flags_alpha_modes_and_colour_space(exe, tmp_path):
    rgb, rgba, grey = _samples(T.RGB8, 3, 5, 1), _samples(T.RGBA8, 3, 5, 2), _samples(T.GREY8, 3, 5, 3)
    files = [T.build(rgb, T.RGB8, colour_space=1), T.build(rgb, T.RGB8, colour_space=65535), T.build(rgb, T.RGB8), T.build(grey, T.GREY8, colour_space=1),
             T.build(rgba, T.RGBA8, extra=1), T.build(rgba, T.RGBA8, extra=2), T.build(rgba, T.RGBA8, extra=0), T.build(rgba, T.RGBA8),
             T.build(grey, T.PAL8, colormap=_colormap(8), colour_space=1), T.build(_samples(T.RGBA16, 3, 5, 4), T.RGBA16, extra=1)]
    for flags, formats in ((0, [29, 28, 28, 61, 28, 28, 28, 28, 29, 11]), (T.FLAGS_IGNORE_SRGB, [28, 28, 28, 61, 28, 28, 28, 28, 28, 11]),
                           (T.FLAGS_DEFAULT_SRGB, [29, 28, 29, 61, 29, 29, 29, 29, 29, 11]), (T.FLAGS_DEFAULT_SRGB | T.FLAGS_IGNORE_SRGB, [28] * 3 + [61] + [28] * 5 + [11])):
        sub = tmp_path / f"flags{flags}"
        sub.mkdir()
        got = _check_against_ref(exe, sub, files, flags)
        assert [g[3][2] for g in got] == formats, (flags, [g[3][2] for g in got])
        assert [g[3][3] for g in got] == [3, 3, 3, 0, 2, 0, 3, 3, 3, 2], flags          # opaque, premultiplied, unknown
    # an unspecified fourth sample reads as opaque whatever it holds; associated alpha keeps the file's samples
    got = _load_many(exe, tmp_path, [files[6], files[4]])
    assert np.frombuffer(got[0][4], np.uint8)[3::4].tolist() == [255] * 15 and got[0][3][10] == 1
    assert got[1][4] == rgba.tobytes()


@pytest.mark.parametrize("exe", PROGRAMS)
def test_every_truncation_of_two_files(exe, tmp_path):
    for name, data in (("strips", T.build(_samples(T.RGB8, 5, 9, 1), T.RGB8, compression=T.LZW, predictor=2, rows_per_strip=2, colour_space=1)),
                       ("tiles", T.build(_samples(T.RGBA16, 18, 20, 2), T.RGBA16, compression=T.ADOBE_DEFLATE, predictor=2, tile=(16, 16), planar=True, big_endian=True, extra=2))):
        p = tmp_path / f"{name}.tif"
        p.write_bytes(data)
        r = _run(exe, "truncations", p)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.split() == ["truncations", "0", str(len(data))], r.stdout + r.stderr[-3000:]


@pytest.mark.parametrize("exe", PROGRAMS)
def test_fuzz_lands_on_both_sides(exe, tmp_path):
    total = [0, 0]
    for seed, data in enumerate((T.build(_samples(T.RGB8, 6, 10, 3), T.RGB8, compression=T.LZW, predictor=2, rows_per_strip=2),
                                 T.build(_samples(T.GREY32F, 17, 18, 4), T.GREY32F, compression=T.DEFLATE, predictor=3, tile=(16, 16)),
                                 T.build(_samples(T.PAL4, 9, 13, 5), T.PAL4, compression=T.PACKBITS, colormap=_colormap(4)),
                                 T.build(_samples(T.RGBA16, 4, 5, 6), T.RGBA16, planar=True, big_endian=True, extra=1))):
        p = tmp_path / f"fuzz{seed}.tif"
        p.write_bytes(data)
        r = _run(exe, "fuzz", p, 100 + seed, 500)
        assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr[-3000:]
        f = r.stdout.split()
        assert f[0] == "fuzz" and int(f[1]) + int(f[2]) == 500
        total[0] += int(f[1]); total[1] += int(f[2])
    assert sum(total) == 2000 and total[0] > 0 and total[1] > 0, total


# ---- the writer -------------------------------------------------------------------------------------------------------------------------------------------
SAVE_CASES = [(T.R8_UNORM, 0), (T.R16_UNORM, 0), (T.R32_FLOAT, 0), (T.R8G8B8A8_UNORM, 0), (T.R8G8B8A8_UNORM_SRGB, 0), (T.R16G16B16A16_UNORM, 0), (T.R32G32B32_FLOAT, 0),
              (T.R32G32B32A32_FLOAT, 0), (T.B8G8R8A8_UNORM, 0), (T.B8G8R8A8_UNORM_SRGB, 0), (T.B8G8R8X8_UNORM, 0), (T.B8G8R8X8_UNORM_SRGB, T.FLAGS_FORCE_LINEAR),
              (T.R8G8B8A8_UNORM, T.FLAGS_FORCE_SRGB), (T.R8G8B8A8_UNORM_SRGB, T.FLAGS_FORCE_LINEAR), (T.R8_UNORM, T.FLAGS_FORCE_SRGB), (T.R8G8B8A8_UNORM_SRGB, T.FLAGS_FORCE_SRGB | T.FLAGS_FORCE_LINEAR)]


@pytest.mark.parametrize("exe", PROGRAMS)
def test_writer_against_the_restatement_and_pillow(exe, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for i, (fmt, flags) in enumerate(SAVE_CASES):
        for (w, h, pad) in ((7, 5, 0), (1, 1, 0), (16, 3, 5)):
            ib = T.SOURCES[fmt][3]
            pitch = w * ib + pad
            px = rng.integers(0, 256, pitch * h, dtype=np.uint8)
            src, out = tmp_path / "px.bin", tmp_path / f"out{i}.tif"
            src.write_bytes(px.tobytes())
            r = _run(exe, "save", src, w, h, fmt, pitch, flags, out)
            assert r.returncode == 0 and r.stdout.split() == ["hr", "00000000"] and r.stderr == "", r.stdout + r.stderr[-3000:]
            hr, want = T.save(px.tobytes(), w, h, fmt, flags, pitch)
            data = out.read_bytes()
            assert hr == 0 and data == want, (fmt, flags, w, h)
            rows = T.pack_rows(px.tobytes(), w, h, fmt, pitch)
            hr, d = T.decode(data)          # and it reads back as what was written, sRGB where the file says so
            srgb = (T.SOURCES[fmt][6] or flags & T.FLAGS_FORCE_SRGB) and not flags & T.FLAGS_FORCE_LINEAR
            S = T.SOURCES[fmt][1]
            assert hr == 0 and (d["format"] == T.R8G8B8A8_UNORM_SRGB) == bool(srgb and S > 1 and T.SOURCES[fmt][0] == 8), (fmt, flags, d["format"])
            if T.SOURCES[fmt][4] != 3:
                assert d["pixels"] == rows.tobytes()
            if T.SOURCES[fmt][0] == 8 or S == 1:          # Pillow opens these
                im = Image.open(io.BytesIO(data))
                assert np.asarray(im).tobytes() == rows.tobytes() and im.info.get("dpi") == (72, 72), (fmt, im.mode)
    for fmt in (10, 24, 49, 85, 98, 65, 54, 0):          # R16G16B16A16_FLOAT, R10G10B10A2_UNORM, R8G8_UNORM, B5G6R5_UNORM, BC7_UNORM, A8_UNORM, R16_FLOAT, UNKNOWN
        src = tmp_path / "px.bin"
        src.write_bytes(bytes(4096))
        r = _run(exe, "save", src, 4, 4, fmt, 64, 0, tmp_path / "no.tif")
        assert r.returncode == 0 and r.stdout.split() == ["hr", "80070032"], (fmt, r.stdout)
        assert T.save(bytes(4096), 4, 4, fmt)[0] == NOT_SUPPORTED


@pytest.mark.parametrize("exe", PROGRAMS)
def test_file_forms_and_null_arguments(exe, tmp_path):
    p = tmp_path / "x.tif"
    p.write_bytes(T.build(_samples(T.RGB8, 3, 4, 1), T.RGB8, compression=T.LZW))
    r = _run(exe, "files", p)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    got = dict(line.split() for line in r.stdout.splitlines())
    assert got == {"load_file": "00000000", "metadata_file": "00000000", "raw_file": "00000000", "load_null": "80070057", "metadata_null": "80070057", "raw_null": "80070057",
                   "load_file_null": "80070057", "save_file_null": "80070057", "save_null": "80004003"}, got
    r = _run(exe, "files", tmp_path / "missing.tif")
    got = dict(line.split() for line in r.stdout.splitlines())
    assert got["load_file"] == got["metadata_file"] == got["raw_file"] == "80070002", got


# ---- the tools, where no GPU is needed ----------------------------------------------------------------------------------------------------------------
def test_tools_know_the_extensions_and_info_needs_no_gpu(tmp_path):
    conv = os.path.join(LIB, "dxtexconv")
    for ext in (".tif", ".tiff", ".TIF"):
        p = tmp_path / ("height16" + ext)
        p.write_bytes(T.build(_samples(T.GREY16, 6, 9, 1), T.GREY16, compression=T.DEFLATE, predictor=2))
        r = subprocess.run([conv, "-nologo", "-info", str(p)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "9x6" in r.stdout and "R16_UNORM" in r.stdout, r.stdout + r.stderr
    bad = tmp_path / "bad.tif"
    bad.write_bytes(T.build(_samples(T.RGB8, 3, 4, 1), T.RGB8, photometric=6))
    r = subprocess.run([conv, "-nologo", "-info", str(bad)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "80070032" in (r.stdout + r.stderr).upper(), r.stdout + r.stderr
    # -ft tif: -o names a directory or a .tif / .tiff file, under -ft png's mismatch rule
    r = subprocess.run([conv, "-nologo", "-ft", "tif", "-o", str(tmp_path / "out.png"), str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "-ft tif writes a .tif" in r.stderr and "usage: dxtexconv" in r.stderr, r.stderr
    r = subprocess.run([conv, "-nologo", "-ft", "bmp", "-o", str(tmp_path), str(p)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "output file types: dds, hdr, tga, ppm, pfm, png" in r.stderr, r.stderr
    r = subprocess.run([conv], capture_output=True, text=True, timeout=60)
    assert "|exr|tif]" in r.stderr and "in.tif" in r.stderr, r.stderr
