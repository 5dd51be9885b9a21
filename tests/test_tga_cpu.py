"""The TGA texel rules (csrc/dxtex_tga.h, which the GPU kernels and the host codec share) and the host layer's LoadFromTGAMemoryRaw, against
the reference's .tga reader and writer (oracle/_ref): HRESULT and metadata for every file of the corpus - hand-built files, truncations,
seeded mutations - and, where a file loads, the raw texels through the per-texel function, the flips and the alpha rule give the reference's
pixels byte for byte. The writer's rows through the pack function are the reference's file. The Raw loader also runs under
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program. CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_hdr_tga_cpu import tga_files  # noqa: E402

LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK, HOST, HOST_ASAN = (os.path.join(LIB, n) for n in ("tga_check", "tga_host_test", "tga_host_test_asan"))
FLAGS = (0, 0x1, 0x2, 0x10, 0x80, 0x83)          # TGA_FLAGS: BGR 0x1, ALLOW_ALL_ZERO_ALPHA 0x2, IGNORE_SRGB 0x10, DEFAULT_SRGB 0x80

# csrc/dxtex_tga.h
GREY, K5551, RGB_RGBA, RGB_BGRX, BGRA_RGBA, BGRA_BGRA, PALETTE = range(7)
RIGHT_TO_LEFT, TOP_DOWN, ALLOW_ALL_ZERO_ALPHA = 1, 2, 4
ROW_COPY, ROW_SWAP_RB, ROW_DROP_X = range(3)
IMAGE_BYTES = {GREY: 1, K5551: 2}
R8, A8, B5G5R5A1, RGBA8, RGBA8_SRGB, BGRA8, BGRA8_SRGB, BGRX8, BGRX8_SRGB = 61, 65, 86, 28, 29, 87, 91, 88, 93
OPAQUE = 3          # TEX_ALPHA_MODE_OPAQUE in the low three bits of miscFlags2


def kind_of(image_format, bytes_per_texel, paletted):
    if paletted:
        return PALETTE
    return {R8: GREY, B5G5R5A1: K5551, BGRA8: BGRA_BGRA, BGRX8: RGB_BGRX}.get(image_format, RGB_RGBA if bytes_per_texel == 3 else BGRA_RGBA)


def corpus():
    """[(file bytes, TGA_FLAGS)]: test_hdr_tga_cpu's hand-built files and its truncations under each of FLAGS, and its seeded mutations
    (same seeds, same recipe) under the two flag sets it uses."""
    entries = []
    files = tga_files(np.random.default_rng(21))
    for base in (files[4], files[0], files[6]):
        for cut in sorted(set(list(range(0, 30)) + list(range(30, len(base), 5)) + [len(base) - 1])):
            files.append(base[:cut])
    for flags in FLAGS:
        entries += [(f, flags) for f in files]
    rng = np.random.default_rng(23)
    bases = [f for f in tga_files(np.random.default_rng(5)) if len(f) > 40][:160]
    for flags in (0, 0x1 | 0x80):
        for i in range(1500):
            b = bytearray(bases[int(rng.integers(len(bases)))])
            for _ in range(int(rng.integers(1, 4))):
                r = rng.random()
                at = int(rng.integers(0, 18)) if r < 0.5 else (len(b) - 1 - int(rng.integers(0, min(len(b), 540))) if r < 0.7 else int(rng.integers(0, len(b))))
                b[at] = int(rng.choice([0, 1, 2, 3, 8, 9, 10, 11, 15, 16, 24, 32, 127, 128, 255, int(rng.integers(0, 256))]))
            if rng.random() < 0.15:
                del b[int(rng.integers(0, len(b))):]
            entries.append((bytes(b), flags))
    return entries


_shared = {}


def shared_corpus():
    """The corpus and the oracle's answer to every entry of it, computed once."""
    if not _shared:
        _shared["entries"] = corpus()
        _shared["ref"] = [oracle.ref_load_tga(data, flags) for data, flags in _shared["entries"]]
    return _shared["entries"], _shared["ref"]


def raw_load_many(exe, tmp, entries):
    """[(hresult, dict or None)] of `exe raw_load_many` over the entries; the dict holds the line's fields and the paths of the texels and
    the palette."""
    paths = []
    for i, (data, _) in enumerate(entries):
        paths.append(os.path.join(tmp, f"t{i}.tga"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    lst = os.path.join(tmp, "list.txt")
    with open(lst, "w") as f:
        f.write("".join(f"{p} {flags}\n" for p, (_, flags) in zip(paths, entries)))
    r = subprocess.run([exe, "raw_load_many", lst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    rows = r.stdout.splitlines()
    assert len(rows) == len(entries), r.stderr[-2000:]
    out = []
    keys = ("width", "height", "format", "miscFlags2Before", "miscFlags2", "plainFormat", "bytesPerTexel", "rightToLeft", "topDown", "paletted", "inside")
    for i, row in enumerate(rows):
        p = row.split()
        assert int(p[0]) == i
        if len(p) > 2:
            d = dict(zip(keys, (int(x) for x in p[3:])))
            d["texels"], d["palette"] = paths[i] + ".texels", paths[i] + ".palette"
            out.append((int(p[1], 16), d))
        else:
            out.append((int(p[1], 16), None))
    return out


def unpack_many(tmp, jobs):
    """jobs = [(texels path, kind, flags, width, height, row pitch, palette path)] -> [(pixels, answer)] of tga_check unpack_many."""
    lst = os.path.join(tmp, "unpack.txt")
    with open(lst, "w") as f:
        for i, j in enumerate(jobs):
            f.write(" ".join(str(v) for v in j) + f" {os.path.join(tmp, f'u{i}.px')}\n")
    r = subprocess.run([CHECK, "unpack_many", lst], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    answers = [int(x) for x in r.stdout.split()]
    assert len(answers) == len(jobs)
    return [(np.fromfile(os.path.join(tmp, f"u{i}.px"), np.uint8), a) for i, a in enumerate(answers)]


def compare_with_oracle(tmp, exe, texels):
    entries, ref = shared_corpus()
    ours = raw_load_many(exe, tmp, entries)
    jobs, at = [], []
    for i, ((hr, d), (rhr, rmeta, rpx), (data, flags)) in enumerate(zip(ours, ref, entries)):
        where = (i, hex(flags), data[:18].hex())
        assert hr == rhr, (hex(hr), hex(rhr), where)
        if rmeta is None:
            assert d is None, where
            continue
        # the image carries the format the metadata states (gamma relabels both); its texels were made as the plain format's
        got = {k: d[k] for k in ("width", "height", "format", "miscFlags2")}
        assert got == {k: rmeta[k] for k in got} and rmeta["imageFormat"] == d["format"], (got, rmeta, where)
        assert d["plainFormat"] in (d["format"], {RGBA8_SRGB: RGBA8, BGRA8_SRGB: BGRA8, BGRX8_SRGB: BGRX8}.get(d["format"])), where
        # a raw file's texels are handed back where they lie; a run-length file's in the blob
        assert d["inside"] == (0 if data[2] >= 9 else 1), where
        if texels:
            kind = kind_of(d["plainFormat"], d["bytesPerTexel"], d["paletted"])
            how = (RIGHT_TO_LEFT if d["rightToLeft"] else 0) | (TOP_DOWN if d["topDown"] else 0) | (ALLOW_ALL_ZERO_ALPHA if flags & 0x2 else 0)
            jobs.append((d["texels"], kind, how, d["width"], d["height"], d["width"] * IMAGE_BYTES.get(kind, 4), d["palette"]))
            at.append(i)
    for i, (px, answer) in zip(at, unpack_many(tmp, jobs)):
        d, (_, rmeta, rpx) = ours[i][1], ref[i]
        assert np.array_equal(px, rpx), (i, hex(entries[i][1]), entries[i][0][:18].hex())
        # the alpha rule is what turns the Raw loader's metadata into the loader's
        want = (d["miscFlags2Before"] & ~7) | OPAQUE if answer else d["miscFlags2Before"]
        assert d["miscFlags2"] == want == rmeta["miscFlags2"], (i, answer, d, rmeta)
    loaded = sum(1 for _, d in ours if d is not None)
    assert 1500 < loaded < len(entries)
    return loaded


def test_raw_loader_and_texel_rules_match_the_reference(tmp_path):
    """HRESULT and metadata equal the reference's for every file under every flag set; where a file loads, its raw texels through
    tga_check (dxtex_tga.h: the texel, the flips, the alpha ORs, the opaque pass) are the reference's pixels."""
    compare_with_oracle(str(tmp_path), HOST, texels=True)


def test_raw_loader_under_sanitizers(tmp_path):
    """The same corpus once through the build whose codec and main carry AddressSanitizer and UndefinedBehaviorSanitizer: any report ends
    the program with a non-zero status. Every file is parsed from a heap copy of its exact size."""
    assert os.path.exists(HOST_ASAN)
    compare_with_oracle(str(tmp_path), HOST_ASAN, texels=False)


WRITER = ((RGBA8, 4, 4, ROW_SWAP_RB), (RGBA8_SRGB, 4, 4, ROW_SWAP_RB), (BGRA8, 4, 4, ROW_COPY), (BGRA8_SRGB, 4, 4, ROW_COPY), (BGRX8, 3, 4, ROW_DROP_X),
          (BGRX8_SRGB, 3, 4, ROW_DROP_X), (R8, 1, 1, ROW_COPY), (A8, 1, 1, ROW_COPY), (B5G5R5A1, 2, 2, ROW_COPY))


@pytest.mark.parametrize("fmt,B,D,row", WRITER)
def test_pack_rows_are_the_reference_writers(tmp_path, fmt, B, D, row):
    rng = np.random.default_rng(41 + fmt)
    for (w, h) in ((7, 5), (1, 1), (130, 3)):
        pitch = w * D + 13          # a padded source pitch
        px = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
        rhr, ref = oracle.ref_save_tga(px, w, h, fmt, pitch)
        assert rhr == 0 and ref.size == 18 + w * h * B + 26
        src, out = os.path.join(str(tmp_path), "px.bin"), os.path.join(str(tmp_path), "rows.bin")
        px.tofile(src)
        subprocess.run([CHECK, "pack", str(row), str(B), str(w), str(h), str(pitch), src, out], check=True, timeout=60)
        assert np.array_equal(np.fromfile(out, np.uint8), ref[18:18 + w * h * B]), (fmt, w, h)
        assert ref[16] == 8 * B


# csrc/dxtex_tga.h's two format tables, written out; every other point of the domain is refused
PACK_TABLE = {fmt: (B, row) for fmt, B, _, row in WRITER}
UNPACK_TABLE = {(R8, 1, 0): GREY, (B5G5R5A1, 2, 0): K5551, (RGBA8, 3, 0): RGB_RGBA, (RGBA8, 4, 0): BGRA_RGBA, (BGRX8, 3, 0): RGB_BGRX, (BGRA8, 4, 0): BGRA_BGRA,
                (RGBA8, 1, 1): PALETTE, (BGRX8, 1, 1): PALETTE}


def format_tables():
    """(pack, unpack) of `tga_check formats`: {format: (bytes per texel, row)} and {(format, bytes per texel, paletted): kind}"""
    pack, unpack = {}, {}
    for line in subprocess.run([CHECK, "formats"], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines():
        p = line.split()
        v = [int(x) for x in p[1:]]
        if p[0] == "pack":
            pack[v[0]] = (v[1], v[2])
        else:
            unpack[tuple(v[:3])] = v[3]
    return pack, unpack


def test_format_tables_over_the_whole_domain():
    """The tables the C ABI and the host codec share answer the written-out table for every format 0..191 (reader: every bytes per texel
    0..5 and both palette states), and refuse everything else."""
    pack, unpack = format_tables()
    assert pack == {f: PACK_TABLE.get(f, (0, -1)) for f in range(192)}
    assert unpack == {(f, B, p): UNPACK_TABLE.get((f, B, p), -1) for f in range(192) for B in range(6) for p in (0, 1)}


def test_every_header_the_reader_accepts_is_in_the_reader_table(tmp_path):
    """Every image type x bits x colour map or not x TGA_FLAGS: where LoadFromTGAMemoryRaw accepts the file, the (format before gamma, bytes
    per texel, colour-mapped) it reports is a triple the strict table knows, with the kind the loader's own restatement gives."""
    _, unpack = format_tables()
    entries, headers = [], []
    w, h = 3, 2
    for image_type in (1, 2, 3, 9, 10, 11):
        for bits in (8, 15, 16, 24, 32):
            for mapped in (0, 1):
                B = (bits + 7) // 8
                head = bytes([0, mapped, image_type, 0, 0, 2 * mapped, 0, 24 * mapped, 0, 0, 0, 0, w, 0, h, 0, bits, 0])
                rows = [bytes((7 * (y * w + x) + c) & 0xFF for x in range(w) for c in range(B)) for y in range(h)]
                body = b"".join((bytes([w - 1]) + r) if image_type >= 9 else r for r in rows)          # one raw packet a row
                for flags in FLAGS:
                    entries.append((head + bytes(6 * mapped) + body + bytes(8), flags))
                    headers.append((image_type, bits, mapped))
    accepted = set()
    for (hr, d), header, (_, flags) in zip(raw_load_many(HOST, str(tmp_path), entries), headers, entries):
        if hr != 0:
            continue
        accepted.add(header)
        triple = (d["plainFormat"], d["bytesPerTexel"], d["paletted"])
        assert unpack[triple] >= 0 and unpack[triple] == kind_of(*triple), (header, flags, triple)
    # what DecodeTGAHeader takes: 8-bit colour-mapped, 16 / 24 / 32-bit true colour, 8-bit grey; the latter two raw or run-length encoded
    assert accepted == {(1, 8, 1)} | {(t, b, 0) for t in (2, 10) for b in (16, 24, 32)} | {(3, 8, 0), (11, 8, 0)}
