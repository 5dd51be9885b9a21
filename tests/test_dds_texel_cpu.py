"""The DDS texel rules (csrc/dxtex_dds.h, which the GPU kernels and the host codec share), built for the host as dds_check, against the
reference's LoadFromDDSMemory (oracle/_ref) on one-row files: every 8-bit value of every one-byte op, every 16-bit value of every two-byte
op, seeded texels plus the all-zero and all-ones words for the three- and four-byte ops and the forced-alpha copies, each with and without
the opaque flag where the legacy table has both. CASES also names, for each file, the op, the opaque flag and the result format the
reader must choose: tests/test_dds_gpu.py drives the kernels from the same table. CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dds_legacy_cpu import ALPHA, BUMPDUDVA, BUMPLUM, LUM, LUMA, PAL8, PAL8A, RGB, RGBA, four, header, masks  # noqa: E402,F401

CHECK = os.path.join(ROOT, "directxtex_amd", "lib", "dds_check")

# csrc/dxtex_dds.h
(ROW_COPY, ROW_SWIZZLE, ROW_565, ROW_5551, ROW_4444, ROW_ABGR4, ROW_888, ROW_332, ROW_8332, ROW_P8, ROW_A8P8, ROW_44, ROW_L8, ROW_L16, ROW_A8L8,
 ROW_L6V5U5, ROW_L8U8V8, ROW_WUV10, ROW_FAIL) = range(19)
FILE_BYTES = {ROW_SWIZZLE: 4, ROW_565: 2, ROW_5551: 2, ROW_4444: 2, ROW_ABGR4: 2, ROW_888: 3, ROW_332: 1, ROW_8332: 2, ROW_P8: 1, ROW_A8P8: 2, ROW_44: 1,
              ROW_L8: 1, ROW_L16: 2, ROW_A8L8: 2, ROW_L6V5U5: 2, ROW_L8U8V8: 4, ROW_WUV10: 4}
RGBA16, R10A2, RGBA8, RGBA8_SNORM, RG8, A8, B565, B5551, BGRA8, BGRX8, YUY2, B4444, ABGR4 = 11, 24, 28, 31, 49, 65, 85, 86, 87, 88, 107, 115, 191
RGBA32F = 2
IMAGE_BYTES = {RGBA32F: 16, RGBA16: 8, R10A2: 4, RGBA8: 4, YUY2: 4, B565: 2, B5551: 2, B4444: 2, BGRA8: 4, A8: 1}
# DDS_FLAGS of the reader
LEGACY_DWORD, FORCE_RGB, NO_16BPP, EXPAND_LUMINANCE, BAD_DXTN_TAILS, ALLOW_LARGE_FILES = 0x1, 0x8, 0x10, 0x20, 0x40, 0x1000000

DX10 = four("DX10")
# name -> (pixel format, 'DX10' extension or None, reader flags, op, opaque, result format): what DecodeDDSHeader makes of the file
CASES = {
    "332_565": (masks(RGB, 8, 0xe0, 0x1c, 0x03, 0), None, 0, ROW_332, False, B565),
    "332_8888": (masks(RGB, 8, 0xe0, 0x1c, 0x03, 0), None, NO_16BPP, ROW_332, True, RGBA8),
    "p8": (masks(PAL8, 8, 0, 0, 0, 0), None, 0, ROW_P8, False, RGBA8),
    "44_4444": (masks(LUMA, 8, 0x0f, 0, 0, 0xf0), None, 0, ROW_44, False, B4444),
    "44_8888": (masks(LUMA, 8, 0x0f, 0, 0, 0xf0), None, NO_16BPP, ROW_44, False, RGBA8),
    "l8": (masks(LUM, 8, 0xff, 0, 0, 0), None, EXPAND_LUMINANCE, ROW_L8, False, RGBA8),
    "565": (masks(RGB, 16, 0xf800, 0x07e0, 0x001f, 0), None, NO_16BPP, ROW_565, True, RGBA8),
    "5551": (masks(RGBA, 16, 0x7c00, 0x03e0, 0x001f, 0x8000), None, NO_16BPP, ROW_5551, False, RGBA8),
    "5551_opaque": (masks(RGB, 16, 0x7c00, 0x03e0, 0x001f, 0), None, NO_16BPP, ROW_5551, True, RGBA8),
    "4444": (masks(RGBA, 16, 0x0f00, 0x00f0, 0x000f, 0xf000), None, NO_16BPP, ROW_4444, False, RGBA8),
    "4444_opaque": (masks(RGB, 16, 0x0f00, 0x00f0, 0x000f, 0), None, NO_16BPP, ROW_4444, True, RGBA8),
    "abgr4": (DX10, (ABGR4, 3, 0, 1, 0), NO_16BPP, ROW_ABGR4, False, RGBA8),
    "8332": (masks(RGBA, 16, 0x00e0, 0x001c, 0x0003, 0xff00), None, 0, ROW_8332, False, RGBA8),
    "a8p8": (masks(PAL8A, 16, 0, 0, 0, 0xff00), None, 0, ROW_A8P8, False, RGBA8),
    "l16": (masks(LUM, 16, 0xffff, 0, 0, 0), None, EXPAND_LUMINANCE, ROW_L16, False, RGBA16),
    "a8l8": (masks(LUMA, 16, 0x00ff, 0, 0, 0xff00), None, EXPAND_LUMINANCE, ROW_A8L8, False, RGBA8),
    "l6v5u5": (masks(BUMPLUM, 16, 0x001f, 0x03e0, 0xfc00, 0), None, 0, ROW_L6V5U5, False, RGBA8),
    "888": (masks(RGB, 24, 0xff0000, 0x00ff00, 0x0000ff, 0), None, 0, ROW_888, True, RGBA8),
    "swizzle_8888": (masks(RGBA, 32, 0x00ff0000, 0x0000ff00, 0x000000ff, 0xff000000), None, FORCE_RGB, ROW_SWIZZLE, False, RGBA8),
    "swizzle_8888_opaque": (masks(RGB, 32, 0x00ff0000, 0x0000ff00, 0x000000ff, 0), None, FORCE_RGB, ROW_SWIZZLE, True, RGBA8),
    "swizzle_1010102": (masks(RGBA, 32, 0x000003ff, 0x000ffc00, 0x3ff00000, 0xc0000000), None, 0, ROW_SWIZZLE, False, R10A2),
    "swizzle_yuy2": (four("UYVY"), None, 0, ROW_SWIZZLE, False, YUY2),
    "l8u8v8": (masks(BUMPLUM, 32, 0x000000ff, 0x0000ff00, 0x00ff0000, 0), None, 0, ROW_L8U8V8, False, RGBA8),
    "wuv10": (masks(BUMPDUDVA, 32, 0x3ff00000, 0x000ffc00, 0x000003ff, 0xc0000000), None, 0, ROW_WUV10, False, R10A2),
    "copy": (masks(RGBA, 32, 0x000000ff, 0x0000ff00, 0x00ff0000, 0xff000000), None, 0, ROW_COPY, False, RGBA8),
    # the alpha classes of CopyScanline a .dds file can reach
    "copy_8888_opaque": (masks(RGB, 32, 0x000000ff, 0x0000ff00, 0x00ff0000, 0), None, 0, ROW_COPY, True, RGBA8),
    "copy_5551_opaque": (masks(RGB, 16, 0x7c00, 0x03e0, 0x001f, 0), None, 0, ROW_COPY, True, B5551),
    "copy_4444_opaque": (masks(RGB, 16, 0x0f00, 0x00f0, 0x000f, 0), None, 0, ROW_COPY, True, B4444),
}


def file_bytes(name):
    """bytes of a file texel of the case (for the copies: of an image texel)"""
    op, fmt = CASES[name][3], CASES[name][5]
    return FILE_BYTES.get(op, IMAGE_BYTES.get(fmt))


def palette_words(seed=77):
    return np.random.default_rng(seed).integers(0, 1 << 32, 256, dtype=np.uint64).astype(np.uint32)


def dds_file(name, width, height, payload, mips=0, flags=0x1007, depth=0, caps2=0, dx10=None, pf=None):
    """header (+ palette) + payload for a case of CASES; dx10 / pf override the case's"""
    cpf, cdx10 = CASES[name][0], CASES[name][1]
    head = header(width, height, pf or cpf, flags=flags, mips=mips, depth=depth, caps2=caps2, dx10=dx10 if dx10 is not None else cdx10)
    if CASES[name][3] in (ROW_P8, ROW_A8P8):
        head += palette_words().tobytes()
    return head + bytes(payload)


def row_of(name):
    """The texels of the case's one-row file, as bytes."""
    B = file_bytes(name)
    if B == 1:
        return np.arange(256, dtype=np.uint8)
    if B == 2:
        return np.arange(65536, dtype="<u2").view(np.uint8)
    t = np.random.default_rng(B * 1000 + len(name)).integers(0, 256, (4096 + 2, B), dtype=np.uint8)
    t[-2], t[-1] = 0x00, 0xFF
    return t.reshape(-1)


def run_check(tmp, rows):
    """rows: [(texel bytes, op, format, opaque, palette words or None)] -> [image bytes, or None where the pair is refused]"""
    lines = []
    for i, (texels, op, fmt, opaque, pal) in enumerate(rows):
        np.ascontiguousarray(texels, np.uint8).tofile(os.path.join(tmp, f"r{i}.in"))
        palette = "-"
        if pal is not None:
            palette = os.path.join(tmp, f"r{i}.pal")
            pal.tofile(palette)
        lines.append(f"{os.path.join(tmp, f'r{i}.in')} {op} {fmt} {int(opaque)} {palette} {os.path.join(tmp, f'r{i}.out')}")
    lst = os.path.join(tmp, "rows.txt")
    with open(lst, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([CHECK, "rows", lst], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-1000:])
    answers = r.stdout.split()
    assert len(answers) == len(rows)
    return [np.fromfile(os.path.join(tmp, f"r{i}.out"), np.uint8) if a == "ok" else None for i, a in enumerate(answers)]


def test_every_case_gives_the_reference_readers_row(tmp_path):
    names = list(CASES)
    rows, want = [], []
    for name in names:
        pf, dx10, flags, op, opaque, fmt = CASES[name]
        texels = row_of(name)
        width = texels.size // file_bytes(name) * (2 if fmt == YUY2 else 1)          # a YUY2 word holds two texels
        hr, meta, px = oracle.ref_load_dds_ex(np.frombuffer(dds_file(name, width, 1, texels.tobytes()), np.uint8), flags | ALLOW_LARGE_FILES, capacity=1 << 20)
        assert hr == 0 and (meta["width"], meta["height"], meta["format"]) == (width, 1, fmt), (name, hex(hr), meta)
        assert ((meta["miscFlags2"] & 7) == 3) == opaque, (name, meta)          # CASES' opaque flag is the reader's: it shows as the alpha mode
        want.append(px)
        rows.append((texels, op, fmt, opaque, palette_words() if op in (ROW_P8, ROW_A8P8) else None))
    for name, got, ref in zip(names, run_check(str(tmp_path), rows), want):
        assert got is not None and got.size == ref.size and np.array_equal(got, ref), (name, None if got is None else np.flatnonzero(got != ref[:got.size])[:8])


# CopyScanline's alpha classes (DirectXTexConvert.cpp:207-430), as the reference's code states them per format:
# format -> (bytes of a texel, bytes of its alpha at the texel's end, AND mask, OR value)
ALPHA_CLASSES = {RGBA32F: (16, 4, 0, 0x3f800000), 3: (16, 4, 0, 0xffffffff), 4: (16, 4, 0, 0x7fffffff), 1: (16, 4, 0, 0xffffffff),
                 10: (8, 2, 0, 0x3c00), RGBA16: (8, 2, 0, 0xffff), 13: (8, 2, 0, 0x7fff), 14: (8, 2, 0, 0x7fff), 12: (8, 2, 0, 0xffff),
                 R10A2: (4, 4, 0xffffffff, 0xC0000000), 89: (4, 4, 0xffffffff, 0xC0000000), 101: (4, 4, 0xffffffff, 0xC0000000),
                 RGBA8_SNORM: (4, 4, 0x00ffffff, 0x7f000000), 32: (4, 4, 0x00ffffff, 0x7f000000), BGRA8: (4, 4, 0x00ffffff, 0xff000000), 100: (4, 4, 0x00ffffff, 0xff000000),
                 ABGR4: (2, 2, 0xffff, 0x000F), A8: (1, 1, 0, 0xff)}


def forced_alpha(texels, fmt):
    """The bytes of whole texels of an ALPHA_CLASSES format with their alpha forced, in numpy; a trailing part of a texel is dropped."""
    T, A, keep, value = ALPHA_CLASSES[fmt]
    want = texels[:texels.size // T * T].reshape(-1, T).copy()
    word = np.zeros(len(want), np.uint32)
    for k in range(A):
        word |= want[:, T - A + k].astype(np.uint32) << (8 * k)
    word = (word & np.uint32(keep)) | np.uint32(value)
    for k in range(A):
        want[:, T - A + k] = (word >> (8 * k)) & 0xFF
    return want.reshape(-1)


def test_forced_alpha_of_the_classes_no_file_reaches(tmp_path):
    """CopyScanline's other alpha classes, which no .dds pixel format reaches with the opaque flag: the alpha word the reference's code
    states per format, applied to whole texels; a format outside every class passes unchanged."""
    texels = np.random.default_rng(9).integers(0, 256, 4098 * 16 + 5, dtype=np.uint8)
    texels[-16 * 2 - 5:-16 - 5], texels[-16 - 5:-5] = 0x00, 0xFF
    formats = list(ALPHA_CLASSES) + [RG8, BGRX8, B565]
    got = run_check(str(tmp_path), [(texels, ROW_COPY, f, True, None) for f in formats] + [(texels, ROW_COPY, R10A2, False, None)])
    for f, g in zip(formats, got):
        assert np.array_equal(g, forced_alpha(texels, f) if f in ALPHA_CLASSES else texels), f
    assert np.array_equal(got[-1], texels)          # without the flag a copy is a copy


def test_refusal_table(tmp_path):
    """dds_target: every expansion into anything but R8G8B8A8_UNORM is refused, except 332 into B5G6R5, 44 into B4G4R4A4, L16 into
    R16G16B16A16_UNORM and WUV10 into R10G10B10A2_UNORM; ROW_FAIL and numbers that name no op always are; a swizzle and a copy never."""
    formats = (RGBA8, 29, BGRA8, BGRX8, B565, B4444, B5551, RGBA16, R10A2, YUY2, 61, 2)
    allowed = {(op, RGBA8) for op in FILE_BYTES if op not in (ROW_L16, ROW_WUV10)} | {(ROW_332, B565), (ROW_44, B4444), (ROW_L16, RGBA16), (ROW_WUV10, R10A2)}
    allowed |= {(op, f) for op in (ROW_COPY, ROW_SWIZZLE) for f in formats}
    pairs = [(op, f) for op in list(range(ROW_FAIL + 1)) + [19, 255, -1] for f in formats]
    texels = np.arange(64, dtype=np.uint8)
    got = run_check(str(tmp_path), [(texels, op, f, False, palette_words() if op in (ROW_P8, ROW_A8P8) else None) for op, f in pairs])
    for (op, f), g in zip(pairs, got):
        assert (g is not None) == ((op, f) in allowed), (op, f)
