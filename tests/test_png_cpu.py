"""The PNG codec of the host layer (host/DirectXTexAMD_PNG.cpp: chunks, CRC-32, its own inflater, Adler-32, the row filters) and the texel
rules it shares with the GPU kernels (csrc/dxtex_png.h), against tests/png_ref.py, the restatement over Python's zlib: HRESULT, metadata, the
raw loader's description of the rows and the pixels, byte for byte, for every kind under every filter, zlib level, strategy, window and IDAT
split, every refusal, truncations and a seeded fuzz. libpng is not there to run the reference against; parity rests on the restatement. The
host program also runs under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program. CPU only."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import png_ref as R  # noqa: E402

LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK, HOST, HOST_ASAN = (os.path.join(LIB, n) for n in ("png_check", "png_host_test", "png_host_test_asan"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "png")
WIDTHS, HEIGHTS = (1, 3, 4, 5, 7, 8, 9, 65), (1, 2, 5)
KINDS = sorted(R.TYPE_OF)
# csrc/dxtex_png.h PngSource, by image format
SOURCE = {R.R8: 0, R.R16: 1, R.RGBA8: 2, R.RGBA8_SRGB: 2, R.BGRA8: 3, R.BGRA8_SRGB: 3, R.RGBA16: 4, R.BGRX8: 5, R.BGRX8_SRGB: 5}
HR = {n: getattr(R, n) for n in ("S_OK", "E_FAIL", "E_INVALIDARG", "E_NOT_SUPPORTED", "E_FILE_NOT_FOUND")}


def case_rows(kind, w, h, rng):
    """random unfiltered rows of a kind: [bytes] * h (the pad bits of a sub-byte row's last byte are random too: nothing may read them)"""
    rb = R.row_bytes(kind, w)
    return [rng.integers(0, 256, rb, dtype=np.uint8).tobytes() for _ in range(h)]


def case_palette(kind, rng, entries=None, trns=None):
    """(plte bytes, trns bytes or None) for a palette kind; (None, None) otherwise"""
    ct, depth = R.TYPE_OF[kind]
    if ct != 3:
        return None, None
    n = entries if entries is not None else int(rng.integers(1, (1 << depth) + 1))
    plte = rng.integers(0, 256, 3 * n, dtype=np.uint8).tobytes()
    t = rng.integers(0, 256, int(rng.integers(1, n + 1)), dtype=np.uint8).tobytes() if (trns if trns is not None else rng.integers(0, 2)) else None
    return plte, t


def expected(info, flags=0):
    """(format, miscFlags2, tight pixels) the reader gives for a decoded file"""
    fmt, misc2 = R.metadata(info["ct"], info["depth"], flags, info["srgb"], info["gama"])
    pal = R.palette_words(info["plte"], info["trns"]) if info["ct"] == 3 else None
    return fmt, misc2, R.expand(info["rows"], info["width"], info["height"], info["kind"], bool(flags & R.FLAGS_BGR), pal)


def load_many(exe, tmp, files, name="list"):
    """[(raw hresult, host hresult, metadata hresult, None | dict of the line's fields with the pixels)] of `exe load_many` over (flags, data)"""
    os.makedirs(os.path.join(tmp, name), exist_ok=True)
    lines = []
    for i, (flags, data) in enumerate(files):
        path = os.path.join(tmp, name, f"f{i}.png")
        with open(path, "wb") as f:
            f.write(data)
        lines.append(f"{flags} {path}")
    listing = os.path.join(tmp, name + ".txt")
    with open(listing, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, "load_many", listing], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    with open(listing + ".out", "rb") as f:
        blob = f.read()
    out = []
    keys = ("width", "height", "format", "depth", "arraySize", "mipLevels", "miscFlags", "miscFlags2", "dimension", "kind", "flags", "paletteCount", "rowBytes", "rowsBytes", "offset", "bytes")
    rows = r.stdout.splitlines()
    assert len(rows) == len(files)
    for i, line in enumerate(rows):
        p = line.split()
        assert int(p[0]) == i
        hrs = tuple(int(x, 16) for x in p[1:4])
        if len(p) > 4:
            assert p[4] == "ok"
            d = dict(zip(keys, map(int, p[5:])))
            d["pixels"] = np.frombuffer(blob[d["offset"]:d["offset"] + d["bytes"]], np.uint8)
            out.append(hrs + (d,))
        else:
            out.append(hrs + (None,))
    return out


def check_loaded(result, data, flags, where):
    raw_hr, hr, meta_hr, d = result
    info = R.decode(data)
    fmt, misc2, px = expected(info, flags)
    assert (raw_hr, hr, meta_hr) == (0, 0, 0) and d is not None, (where, hex(raw_hr), hex(hr), hex(meta_hr))
    assert (d["width"], d["height"], d["format"], d["miscFlags2"]) == (info["width"], info["height"], fmt, misc2), (where, d)
    assert (d["depth"], d["arraySize"], d["mipLevels"], d["miscFlags"], d["dimension"]) == (1, 1, 1, 0, 3), (where, d)
    assert d["kind"] == info["kind"] and d["rowBytes"] == R.row_bytes(info["kind"], info["width"]) and d["rowsBytes"] == d["rowBytes"] * info["height"], (where, d)
    assert np.array_equal(d["pixels"], px.reshape(-1)), where


FILTERS = [(0,), (1,), (2,), (3,), (4,), (0, 1, 2, 3, 4), None]          # None: a seeded random filter per row
# one axis at a time around level 6, the default strategy, a 32 KiB window and one IDAT
ENCODINGS = ([dict(filters=f) for f in FILTERS] + [dict(level=v) for v in (0, 1, 6, 9)] +
             [dict(strategy=s) for s in (zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE)] + [dict(wbits=9), dict(wbits=15)] +
             [dict(every=None), dict(every=1), dict(every=7), dict(every=4099)])


@pytest.mark.parametrize("kind", KINDS)
def test_reader_matches_the_restatement_under_every_encoding(tmp_path, kind):
    """Every size of a kind, each encoded every way of ENCODINGS (the other axes drawn by the seed, so that they mix): pixels, metadata and
    the raw loader's description, against the restatement's decode of the same bytes."""
    rng = np.random.default_rng(1000 + kind)
    ct, depth = R.TYPE_OF[kind]
    files, wheres = [], []
    for w in WIDTHS:
        for h in HEIGHTS:
            rows = case_rows(kind, w, h, rng)
            plte, trns = case_palette(kind, rng)
            for e in ENCODINGS:
                opts = dict(filters=FILTERS[int(rng.integers(0, 6))], level=int(rng.choice((1, 6, 9))), every=(None, 7, 4099)[int(rng.integers(0, 3))])
                opts.update(e)
                if opts["filters"] is None:
                    opts["filters"] = tuple(int(v) for v in rng.integers(0, 5, h))
                files.append((0, R.encode(w, h, ct, depth, rows, plte=plte, trns=trns, **opts)))
                wheres.append((kind, w, h, opts))
    for result, (flags, data), where in zip(load_many(HOST, str(tmp_path), files), files, wheres):
        check_loaded(result, data, flags, where)


def test_flags_and_colour_chunks_choose_the_format(tmp_path):
    """each PNG_FLAGS combination of the reader's three x each of sRGB, gAMA 1.0, gAMA 0.45455 and neither x every kind, tRNS on the palette
    kinds and on RGB (a colour key, which is ignored): format, miscFlags2 and pixels"""
    rng = np.random.default_rng(7)
    files, wheres = [], []
    for kind in KINDS:
        ct, depth = R.TYPE_OF[kind]
        w, h = 5, 2
        rows = case_rows(kind, w, h, rng)
        plte, trns = case_palette(kind, rng, trns=True)
        if ct == 2:
            trns = bytes(6 if depth == 16 else 6)          # a colour key: three 16-bit values
        for colour in (dict(srgb=0), dict(gama=100000), dict(gama=45455), dict()):
            data = R.encode(w, h, ct, depth, rows, filters=(4,), plte=plte, trns=trns, **colour)
            for flags in range(8):
                files.append((flags, data))
                wheres.append((kind, colour, flags))
    for result, (flags, data), where in zip(load_many(HOST, str(tmp_path), files), files, wheres):
        check_loaded(result, data, flags, where)
    # what the table above must have covered
    assert R.metadata(2, 8, R.FLAGS_BGR, None, None) == (R.BGRX8_SRGB, 0) and R.metadata(6, 8, R.FLAGS_BGR | R.FLAGS_DEFAULT_LINEAR) == (R.BGRA8, 0)
    assert R.metadata(4, 8, 0, 0, None) == (R.RGBA8, 0) and R.metadata(3, 8, 0, None, 100000) == (R.RGBA8, R.ALPHA_MODE_OPAQUE) and R.metadata(2, 16, 0) == (R.RGBA16, R.ALPHA_MODE_OPAQUE)


class Bits:
    """deflate's bit order: values least significant bit first, Huffman codes most significant bit first"""
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, n):
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):
        self.bits(int(format(v, f"0{n}b")[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def literal(self, v):          # the fixed code
        if v < 144:
            self.code(0x30 + v, 8)
        elif v < 256:
            self.code(0x190 + v - 144, 9)
        elif v < 280:
            self.code(v - 256, 7)
        else:
            self.code(0xC0 + v - 280, 8)

    def stored(self, data, final=0):
        self.bits(final, 1)
        self.bits(0, 2)
        self.align()
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data

    def done(self):
        self.align()
        return bytes(self.out)


def zwrap(deflate, raw):
    return b"\x78\x01" + deflate + struct.pack(">I", zlib.adler32(raw) & 0xFFFFFFFF)


def png_of(z, w=1, h=1, ct=0, depth=8, every=None):
    return R.SIGNATURE + R.ihdr(w, h, depth, ct) + R.split_idat(z, every) + R.chunk(b"IEND")


def far_match_stream():
    """71 680 bytes, 280 rows of grey 8 x 255: two stored blocks of random rows (32 768 bytes), then a fixed block of matches of length 258
    at distance 32 768 - the whole window, further than zlib's own deflate ever reaches, and across both stored blocks"""
    rng = np.random.default_rng(99)
    head = bytearray(rng.integers(0, 256, 32768, dtype=np.uint8).tobytes())
    head[::256] = rng.integers(0, 5, 128, dtype=np.uint8).tobytes()
    head = bytes(head)
    b = Bits()
    b.stored(head[:20000])
    b.stored(head[20000:])
    b.bits(1, 1)
    b.bits(1, 2)
    raw = bytearray(head)
    while len(raw) < 71680:
        n = min(258, 71680 - len(raw))
        assert n >= 3
        sym, extra, ebits = (285, 0, 0) if n == 258 else next((257 + i, n - base, eb) for i, (base, eb) in enumerate(LENGTHS) if base <= n < base + (1 << eb))
        b.literal(sym)
        b.bits(extra, ebits)
        b.code(29, 5)
        b.bits(32768 - 24577, 13)
        raw += raw[len(raw) - 32768:len(raw) - 32768 + n]
    b.literal(256)
    return zwrap(b.done(), bytes(raw)), bytes(raw)


LENGTHS = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0), (10, 0), (11, 1), (13, 1), (15, 1), (17, 1), (19, 2), (23, 2), (27, 2), (31, 2), (35, 3), (43, 3),
           (51, 3), (59, 3), (67, 4), (83, 4), (99, 4), (115, 4), (131, 5), (163, 5), (195, 5), (227, 5)]


def test_window_far_matches_and_overlapping_runs(tmp_path):
    z, raw = far_match_stream()
    assert zlib.decompress(z) == raw and len(raw) >= 70000
    far = png_of(z, 255, 280, every=4099)
    # single-byte runs: every row one value, which deflate codes as a literal and an overlapping copy at distance 1
    runs_rows = [bytes([v]) * 600 for v in (0, 255, 7, 7, 200)]
    runs = [R.encode(200, 5, 2, 8, runs_rows, filters=(0,), level=9), R.encode(600, 5, 0, 8, runs_rows, filters=(0, 2), strategy=zlib.Z_RLE, every=7)]
    # a stream with surplus rows behind the image's: ignored
    rows = case_rows(R.RGB8, 9, 5, np.random.default_rng(3))
    surplus = png_of(R.deflate(R.filter_rows(rows + rows, 3, (1, 4))), 9, 5, 2, 8)
    files = [(0, far)] + [(0, d) for d in runs] + [(0, surplus)]
    for i, (result, (flags, data)) in enumerate(zip(load_many(HOST, str(tmp_path), files), files)):
        check_loaded(result, data, flags, i)


def crafted_damage():
    """name -> the zlib stream of a 1 x 1 grey 8 file with one defect of deflate, each refused by zlib too"""
    out = {}
    good = R.deflate(b"\x00\x55", 0)
    out["stored LEN/NLEN mismatch"] = good[:5] + bytes([good[5] ^ 1]) + good[6:]
    out["block type 3"] = b"\x78\x01\x07\x00" + struct.pack(">I", 1)
    b = Bits()
    b.bits(1, 1); b.bits(1, 2); b.literal(257); b.code(0, 5); b.literal(256)          # a match of 3 at distance 1 with nothing before it
    out["distance before the start"] = zwrap(b.done(), b"")
    b = Bits()
    b.bits(1, 1); b.bits(2, 2); b.bits(0, 5); b.bits(0, 5); b.bits(2, 4)          # 6 code length codes: 16, 17, 18, 0, 8, 7
    for n in (0, 0, 0, 1, 1, 1):
        b.bits(n, 3)          # three codes of one bit
    b.bits(0, 16)
    out["over-subscribed code lengths"] = zwrap(b.done(), b"")
    b = Bits()
    b.bits(1, 1); b.bits(2, 2); b.bits(0, 5); b.bits(0, 5); b.bits(14, 4)          # 18 code length codes, so that 0 and 1 get one bit each
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1)
    for s in order:
        b.bits(1 if s in (0, 1) else 0, 3)
    for i in range(258):          # 257 literal / length codes, one distance code: literals 0 and 1 of one bit, no end-of-block code
        b.bits(1 if i in (0, 1) else 0, 1)
    b.bits(0, 16)
    out["missing end-of-block code"] = zwrap(b.done(), b"")
    out["bad Adler-32"] = good[:-1] + bytes([good[-1] ^ 1])
    out["bad zlib header"] = b"\x78\x02" + good[2:]
    out["preset dictionary"] = b"\x78\x20" + good[2:]
    out["not deflate"] = b"\x79\x18" + good[2:]
    out["stream ends before its last block"] = R.deflate(b"\x00\x55", 6)[:-5]
    for name, z in out.items():
        with pytest.raises(zlib.error):
            zlib.decompress(z)
    out["fewer bytes than the image"] = R.deflate(b"\x00", 6)
    return out


def damaged_files():
    """name -> (file, expected HRESULT): every refusal, one at a time"""
    rng = np.random.default_rng(5)
    rows = case_rows(R.RGB8, 9, 5, rng)
    good = R.encode(9, 5, 2, 8, rows, filters=(0, 1, 2, 3, 4), every=64)
    cs = R.chunks(good)
    out = {}
    out["bad signature"] = (b"\x89PNG\r\n\x1a\r" + good[8:], R.E_FAIL)
    out["empty"] = (b"", R.E_FAIL)
    out["signature only"] = (good[:8], R.E_FAIL)
    out["bad CRC of IHDR"] = (good[:29] + bytes([good[29] ^ 1]) + good[30:], R.E_FAIL)
    out["bad CRC of IDAT"] = (good[:50] + bytes([good[50] ^ 0x10]) + good[51:], R.E_FAIL)
    bad_anc = R.chunk(b"tEXt", b"k\x00v")
    out["bad CRC of a skipped chunk"] = (good[:33] + bad_anc[:-1] + bytes([bad_anc[-1] ^ 1]) + good[33:], R.E_FAIL)
    for ct, depth in ((0, 3), (2, 4), (3, 16), (4, 4), (6, 2), (1, 8), (5, 8), (7, 8), (2, 0)):
        out[f"colour type {ct} with depth {depth}"] = (R.SIGNATURE + R.ihdr(1, 1, depth, ct) + R.split_idat(R.deflate(bytes(9))) + R.chunk(b"IEND"), R.E_FAIL)
    for w, h in ((0, 1), (1, 0), (1000001, 1), (1, 1000001), (0x80000000, 1)):
        out[f"{w} x {h}"] = (R.SIGNATURE + R.ihdr(w, h, 8, 0) + R.split_idat(R.deflate(bytes(2))) + R.chunk(b"IEND"), R.E_FAIL)
    out["interlaced"] = (R.encode(9, 5, 2, 8, rows, interlace=1), R.E_NOT_SUPPORTED)
    out["interlace method 2"] = (R.encode(9, 5, 2, 8, rows, interlace=2), R.E_FAIL)
    out["palette without PLTE"] = (R.encode(3, 1, 3, 8, [b"\x00\x01\x02"]), R.E_FAIL)
    out["PLTE of 4 bytes"] = (R.encode(3, 1, 3, 8, [b"\x00\x01\x02"], plte=bytes(4)), R.E_FAIL)
    out["PLTE of 771 bytes"] = (R.encode(3, 1, 3, 8, [b"\x00\x01\x02"], plte=bytes(771)), R.E_FAIL)
    out["grey with tRNS"] = (R.encode(3, 1, 0, 8, [b"\x00\x01\x02"], trns=b"\x00\x01"), R.E_NOT_SUPPORTED)
    out["an unknown critical chunk"] = (good[:33] + R.chunk(b"ABCD", b"x") + good[33:], R.E_FAIL)
    out["IHDR of 12 bytes"] = (R.SIGNATURE + R.chunk(b"IHDR", bytes(12)) + good[33:], R.E_FAIL)
    out["no IHDR"] = (good[:8] + good[33:], R.E_FAIL)
    out["two IHDR"] = (good[:33] + good[8:], R.E_FAIL)
    out["no IDAT"] = (good[:33] + R.chunk(b"IEND"), R.E_FAIL)
    out["a chunk length past the file"] = (good[:33] + struct.pack(">I", 1 << 20) + good[37:], R.E_FAIL)
    out["a chunk length of 2^31"] = (good[:33] + struct.pack(">I", 1 << 31) + good[37:], R.E_FAIL)
    for f in (5, 255):
        stream = bytearray(R.filter_rows(rows, 3, (0,)))
        stream[28 * 2] = f
        out[f"filter byte {f}"] = (png_of(R.deflate(bytes(stream)), 9, 5, 2, 8), R.E_FAIL)
    out["one row short"] = (png_of(R.deflate(R.filter_rows(rows[:4], 3, (1,))), 9, 5, 2, 8), R.E_FAIL)
    out["one byte short"] = (png_of(R.deflate(R.filter_rows(rows, 3, (1,))[:-1]), 9, 5, 2, 8), R.E_FAIL)
    for name, z in crafted_damage().items():
        out[name] = (png_of(z), R.E_FAIL)
    # truncation at every chunk boundary and inside every chunk, and of the stream inside the IDAT chunks (lengths and CRCs in order)
    at = 8
    for i, (tag, body) in enumerate(cs):
        out[f"cut in front of chunk {i}"] = (good[:at], R.E_FAIL)
        for k in (1, 4, 8, 8 + len(body) // 2, 11 + len(body)):
            out[f"cut {k} bytes into chunk {i}"] = (good[:at + k], R.E_FAIL)
        at += 12 + len(body)
    z = b"".join(body for tag, body in cs if tag == b"IDAT")
    for k in (0, 1, 2, 3, len(z) // 2, len(z) - 5, len(z) - 4, len(z) - 1):
        out[f"stream cut at {k}"] = (png_of(z[:k], 9, 5, 2, 8, every=16), R.E_FAIL)
    return out


@pytest.mark.parametrize("exe", (HOST, HOST_ASAN), ids=("plain", "sanitizers"))
def test_damaged_files_are_refused_with_the_stated_hresult(tmp_path, exe):
    cases = damaged_files()
    files = [(0, data) for data, _ in cases.values()]
    for (name, (data, want)), (raw_hr, hr, meta_hr, d) in zip(cases.items(), load_many(exe, str(tmp_path), files)):
        assert (raw_hr, hr) == (want, want) and d is None, (name, hex(raw_hr), hex(hr), hex(want))


def test_null_arguments_and_missing_files(tmp_path):
    path = os.path.join(str(tmp_path), "one.png")
    with open(path, "wb") as f:
        f.write(R.encode(1, 1, 0, 8, [b"\x7f"]))
    r = subprocess.run([HOST_ASAN, "errors", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {k: int(v, 16) for k, v in (line.split() for line in r.stdout.splitlines())}
    assert {k: v for k, v in got.items() if k.endswith("_null")} == {k: R.E_INVALIDARG for k in ("metadata_null", "load_null", "raw_null", "memory_null", "save_null")}
    assert {k: v for k, v in got.items() if k.endswith("_missing")} == {k: R.E_FILE_NOT_FOUND for k in ("metadata_missing", "load_missing", "raw_missing")}
    assert got["load_file"] == 0 and got["metadata_file"] == 0


def test_fuzz_never_trips_a_sanitizer_or_gives_wrong_pixels(tmp_path):
    """2 000 seeded damages of valid files, half of them to the file's bytes and half to the zlib stream inside intact chunks, through the
    sanitizer build in one process of its own: any HRESULT will do; a sanitizer report (a non-zero exit) fails, and so does a success whose
    pixels differ from what zlib gives for the same bytes."""
    rng = np.random.default_rng(2024)
    bases = []
    for kind in KINDS:
        ct, depth = R.TYPE_OF[kind]
        w, h = int(rng.choice(WIDTHS[:-1])), int(rng.choice(HEIGHTS))
        plte, trns = case_palette(kind, rng)
        for strategy, level in ((zlib.Z_DEFAULT_STRATEGY, 9), (zlib.Z_FIXED, 6), (zlib.Z_DEFAULT_STRATEGY, 0)):
            data = R.encode(w, h, ct, depth, case_rows(kind, w, h, rng), filters=tuple(int(v) for v in rng.integers(0, 5, h)), level=level, strategy=strategy, plte=plte, trns=trns)
            bases.append(data)
    files = []
    for n in range(2000):
        data = bases[n % len(bases)]
        cs = R.chunks(data)
        inside = n % 2 == 1
        target = bytearray(b"".join(b for t, b in cs if t == b"IDAT") if inside else data)
        for _ in range(int(rng.choice((1, 1, 2, 5)))):
            i = int(rng.integers(0, len(target)))
            target[i] = int(rng.integers(0, 256)) if rng.integers(0, 2) else target[i] ^ (1 << int(rng.integers(0, 8)))
        if inside:
            head = b"".join(R.chunk(t, b) for t, b in cs if t not in (b"IDAT", b"IEND"))
            data = R.SIGNATURE + head + R.split_idat(bytes(target), (None, 3)[n % 4 == 3]) + R.chunk(b"IEND")
        else:
            data = bytes(target)
        files.append((0, data))
    results = load_many(HOST_ASAN, str(tmp_path), files)
    loaded = 0
    for n, ((raw_hr, hr, meta_hr, d), (flags, data)) in enumerate(zip(results, files)):
        assert raw_hr == hr, (n, hex(raw_hr), hex(hr))
        if d is not None:
            loaded += 1
            check_loaded((raw_hr, hr, meta_hr, d), data, flags, n)
    assert 0 < loaded < 2000          # some damages are harmless (a pad bit, a palette entry), most are not


# ---- the per-texel rules alone (png_check) -----------------------------------------------------------------------------------------------
def run_check(*args):
    r = subprocess.run([CHECK] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)


@pytest.mark.parametrize("kind", KINDS)
def test_texel_rules_match_the_restatement(tmp_path, kind):
    rng = np.random.default_rng(300 + kind)
    ct, depth = R.TYPE_OF[kind]
    tmp = str(tmp_path)
    for w, h in ((1, 1), (7, 2), (9, 5), (65, 3)):
        rows = b"".join(case_rows(kind, w, h, rng))
        with open(os.path.join(tmp, "rows"), "wb") as f:
            f.write(rows)
        pal_arg, words = "-", None
        if ct == 3:
            plte, trns = case_palette(kind, rng, entries=1 if w == 1 else None)
            with open(os.path.join(tmp, "plte"), "wb") as f:
                f.write(plte)
            with open(os.path.join(tmp, "trns"), "wb") as f:
                f.write(trns or b"")
            run_check("table", os.path.join(tmp, "plte"), os.path.join(tmp, "trns") if trns else "-", os.path.join(tmp, "table"))
            table = np.fromfile(os.path.join(tmp, "table"), "<u4")
            words = R.palette_words(plte, trns)
            assert np.array_equal(table[:len(words)], words) and (table[len(words):] == 0xFF000000).all()
            pal_arg = os.path.join(tmp, "table")
        for bgr in (0, 1):
            run_check("unpack", kind, bgr, w, h, os.path.join(tmp, "rows"), pal_arg, os.path.join(tmp, "out"))
            got = np.fromfile(os.path.join(tmp, "out"), np.uint8)
            assert np.array_equal(got, R.expand(rows, w, h, kind, bool(bgr), words).reshape(-1)), (kind, w, h, bgr)


def test_sub_byte_grey_is_multiplied_out():
    """what the restatement itself must say about the smallest kinds: 255, 85 and 17 times the sample, first texel in the high bits"""
    assert R.expand(b"\xA0", 3, 1, R.G1).tolist() == [[255, 0, 255]]
    assert R.expand(b"\x1B", 4, 1, R.G2).tolist() == [[0, 85, 170, 255]]
    assert R.expand(b"\xF1\x80", 3, 1, R.G4).tolist() == [[255, 17, 136]]
    assert R.expand(b"\x12\x34", 1, 1, R.G16).tolist() == [[0x34, 0x12]]
    assert R.expand(b"\x05", 1, 1, R.P8, False, np.array([1, 2], np.uint32)).tolist() == [[0, 0, 0, 255]]


# ---- the writer -----------------------------------------------------------------------------------------------------------------------------
def save(exe, tmp, px, w, h, fmt, pitch, flags=0):
    src, out = os.path.join(tmp, "src.bin"), os.path.join(tmp, "out.png")
    with open(src, "wb") as f:
        f.write(px.tobytes())
    if os.path.exists(out):
        os.remove(out)
    r = subprocess.run([exe, "save", src, str(w), str(h), str(fmt), str(pitch), str(flags), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    hr = int(r.stdout.split()[1], 16)
    return hr, (open(out, "rb").read() if hr == 0 else None)


@pytest.mark.parametrize("fmt", list(R.WRITER))
def test_writer_files_decode_to_the_images_texels(tmp_path, fmt):
    """every format the writer takes, on a padded pitch: the file decodes through zlib.decompress to the rows the restatement packs, holds
    stored blocks and filter 0 only, the colour chunks of departure 3 in front of IDAT, and comes back through the reader as the image"""
    rng = np.random.default_rng(fmt)
    ct, depth, S, F = R.WRITER[fmt]
    tmp = str(tmp_path)
    back = []
    for w, h in ((1, 1), (5, 2), (9, 5), (65, 3), (300, 120)):          # the last one takes more than one stored block
        pitch = w * S + 5
        px = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
        for flags in (0, R.FLAGS_FORCE_SRGB, R.FLAGS_FORCE_LINEAR, R.FLAGS_FORCE_SRGB | R.FLAGS_FORCE_LINEAR):
            hr, data = save(HOST_ASAN if w < 300 else HOST, tmp, px, w, h, fmt, pitch, flags)
            assert hr == 0
            info = R.decode(data)
            assert (info["width"], info["height"], info["ct"], info["depth"]) == (w, h, ct, depth)
            assert info["rows"] == R.pack_rows(px[:, :w * S], w, h, fmt).tobytes(), (fmt, w, h)
            cs = R.chunks(data)
            z = b"".join(b for t, b in cs if t == b"IDAT")
            assert zlib.decompress(z)[::w * F + 1] == bytes(h)          # filter 0 on every row
            assert len(z) == 2 + 5 * -(-(h * (w * F + 1)) // 65535) + h * (w * F + 1) + 4          # stored blocks only
            first_idat = [t for t, _ in cs].index(b"IDAT")
            assert cs[1:first_idat] == R.writer_chunks(fmt, flags) and cs[-1] == (b"IEND", b""), (fmt, flags, cs[1:first_idat])
            if flags == 0:
                back.append((px[:, :w * S], data))
    # and through this project's reader: the texels exactly (a B8G8R8X8 image comes back with X = 0xff, asked for as BGR)
    bgr = fmt in (R.BGRA8, R.BGRA8_SRGB, R.BGRX8, R.BGRX8_SRGB)
    files = [(R.FLAGS_BGR if bgr else 0, data) for _, data in back]
    for (px, data), (raw_hr, hr, meta_hr, d) in zip(back, load_many(HOST, tmp, files)):
        assert hr == 0
        want = px.copy()
        if fmt in (R.BGRX8, R.BGRX8_SRGB):
            want[:, 3::4] = 255
        want_fmt = {R.RGBA8: R.RGBA8_SRGB, R.BGRA8: R.BGRA8_SRGB, R.BGRX8: R.BGRX8_SRGB}.get(fmt, fmt)          # a file that names no colour space reads as sRGB
        assert d["format"] == want_fmt and np.array_equal(d["pixels"], want.reshape(-1)), (fmt, d["format"])


def test_writer_refuses_every_other_format(tmp_path):
    px = np.zeros((2, 64), np.uint8)
    for fmt in (R.RGBA32F, R.R32F, R.BC1, 10, 24, 49, 65, 85, 86, 0):          # float, BC, R16G16B16A16_FLOAT, R10G10B10A2, R8G8, A8, B5G6R5, B5G5R5A1, UNKNOWN
        hr, data = save(HOST_ASAN, str(tmp_path), px, 2, 2, fmt, 64)
        assert hr == R.E_NOT_SUPPORTED and data is None, (fmt, hex(hr))
    assert save(HOST_ASAN, str(tmp_path), px, 0, 2, R.RGBA8, 64)[0] == R.E_INVALIDARG
    assert save(HOST_ASAN, str(tmp_path), px, 2, 2, R.RGBA8, 7)[0] == R.E_INVALIDARG          # a pitch below the row


@pytest.mark.parametrize("fmt", list(R.WRITER))
def test_pack_rules_match_the_restatement(tmp_path, fmt):
    rng = np.random.default_rng(50 + fmt)
    tmp = str(tmp_path)
    S = R.WRITER[fmt][2]
    for w, h in ((1, 1), (7, 2), (65, 3)):
        px = rng.integers(0, 256, (h, w * S), dtype=np.uint8)
        px.tofile(os.path.join(tmp, "px"))
        run_check("pack", SOURCE[fmt], w, h, os.path.join(tmp, "px"), os.path.join(tmp, "out"))
        assert np.array_equal(np.fromfile(os.path.join(tmp, "out"), np.uint8), R.pack_rows(px, w, h, fmt).reshape(-1)), (fmt, w, h)


# ---- files another encoder wrote -------------------------------------------------------------------------------------------------------
def golden_cases():
    return sorted(n[:-4] for n in os.listdir(GOLDEN) if n.endswith(".png")) if os.path.isdir(GOLDEN) else []


def test_golden_files_written_by_pillow_load_to_their_texels(tmp_path):
    """tests/golden/png: files Pillow wrote with adaptive filters, each beside the texels (<name>.bin) and "<format> <miscFlags2> <width>
    <height>" (<name>.txt) the reader must give with no flags - an encoder the reader's author did not write"""
    names = golden_cases()
    assert len(names) >= 6
    files = [(0, open(os.path.join(GOLDEN, n + ".png"), "rb").read()) for n in names]
    assert all(len(d) <= 4096 for _, d in files)
    for n, (flags, data), result in zip(names, files, load_many(HOST_ASAN, str(tmp_path), files)):
        check_loaded(result, data, flags, n)
        fmt, misc2, w, h = map(int, open(os.path.join(GOLDEN, n + ".txt")).read().split())
        d = result[3]
        assert (d["format"], d["miscFlags2"], d["width"], d["height"]) == (fmt, misc2, w, h), n
        assert np.array_equal(d["pixels"], np.fromfile(os.path.join(GOLDEN, n + ".bin"), np.uint8)), n


def test_restatement_decodes_like_pillow():
    """png_ref's decoder against Pillow's, where Pillow is installed: grey 1 / 2 / 4 / 8 / 16, RGB 8, RGBA 8 and palette with tRNS"""
    Image = pytest.importorskip("PIL.Image")
    import io
    rng = np.random.default_rng(11)
    for kind in (R.G1, R.G2, R.G4, R.G8, R.G16, R.RGB8, R.RGBA8K, R.P8, R.P4):
        ct, depth = R.TYPE_OF[kind]
        w, h = 9, 5
        rows = case_rows(kind, w, h, rng)
        plte, trns = case_palette(kind, rng, entries=1 << depth, trns=True)
        data = R.encode(w, h, ct, depth, rows, filters=(0, 1, 2, 3, 4), plte=plte, trns=trns)
        info = R.decode(data)
        im = Image.open(io.BytesIO(data))
        if ct == 3:
            want = np.asarray(im.convert("RGBA")).reshape(h, w * 4)
            assert np.array_equal(R.expand(info["rows"], w, h, kind, False, R.palette_words(plte, trns)), want), kind
        elif kind == R.G16:
            assert np.array_equal(R.expand(info["rows"], w, h, kind).view("<u2"), np.asarray(im).astype(np.uint16)), kind
        elif ct == 0 and depth < 8:
            assert np.array_equal(R.expand(info["rows"], w, h, kind), np.asarray(im.convert("L"))), kind
        else:
            got = R.expand(info["rows"], w, h, kind).reshape(h, w, -1)
            want = np.asarray(im).reshape(h, w, -1)
            assert np.array_equal(got[..., :want.shape[2]], want), kind


# ---- dxtexconv's options ------------------------------------------------------------------------------------------------------------------
def test_dxtexconv_ft_png_wants_a_directory_or_a_png_name():
    """-ft png with an -o that names another type's file is a usage error, as a PNG under that name would be opened by nothing that goes by
    the extension; a directory or a .png name passes the options (and then wants a device, which this test does not have to have)"""
    conv = os.path.join(LIB, "dxtexconv")
    for out in ("x.dds", "x.tga", "x.HDR", "dir/x.ppm", "x.pfm"):
        r = subprocess.run([conv, "-nologo", "-ft", "png", "-o", out, "in.dds"], capture_output=True, text=True)
        assert r.returncode == 1 and "usage: dxtexconv" in r.stderr and "-ft png writes a .png" in r.stderr, (out, r.stderr)
    for out in ("x.png", "outdir", "x.dds.d"):
        r = subprocess.run([conv, "-nologo", "-ft", "png", "-o", out, "does-not-exist.dds"], capture_output=True, text=True)
        assert "usage: dxtexconv" not in r.stderr, (out, r.stderr)
    r = subprocess.run([conv], capture_output=True, text=True)
    assert "-ft dds|hdr|tga|ppm|pfm|png" in r.stderr and "-ignoresrgb" in r.stderr and "in.png" in r.stderr, r.stderr


# csrc/dxtex_png.h's reader table, written out: {(kind, PNG_BGR or not): the formats the kind unpacks into}
_RGBA = {0: (R.RGBA8, R.RGBA8_SRGB), 1: (R.BGRA8, R.BGRA8_SRGB)}
_RGBX = {0: (R.RGBA8, R.RGBA8_SRGB), 1: (R.BGRX8, R.BGRX8_SRGB)}
UNPACK_PAIRS = {(k, b): (R.R8,) for k in (R.G1, R.G2, R.G4, R.G8) for b in (0, 1)}
UNPACK_PAIRS.update({(R.G16, b): (R.R16,) for b in (0, 1)})
UNPACK_PAIRS.update({(R.GA8, 0): (R.RGBA8,), (R.GA8, 1): (R.BGRA8,)})
UNPACK_PAIRS.update({(k, b): (R.RGBA16,) for k in (R.GA16, R.RGB16, R.RGBA16K) for b in (0, 1)})
UNPACK_PAIRS.update({(R.RGBA8K, b): _RGBA[b] for b in (0, 1)})
UNPACK_PAIRS.update({(k, b): _RGBX[b] for k in (R.RGB8, R.P1, R.P2, R.P4, R.P8) for b in (0, 1)})


def format_tables():
    """(pack, unpack) of `png_check formats`: {format: source} and the set of (kind, flags, format) png_unpack_pairs accepts"""
    pack, unpack = {}, set()
    for line in subprocess.run([CHECK, "formats"], capture_output=True, text=True, check=True, timeout=60).stdout.splitlines():
        p = line.split()
        if p[0] == "pack":
            pack[int(p[1])] = int(p[2])
        else:
            unpack.add(tuple(int(x) for x in p[1:]))
    return pack, unpack


def test_format_tables_over_the_whole_domain():
    """The tables the C ABI and the host codec share answer the written-out tables for every format 0..191: the writer's source - everything
    outside SOURCE refused - and, for every kind with and without PNG_BGR, the formats it unpacks into."""
    pack, unpack = format_tables()
    assert pack == {f: SOURCE.get(f, -1) for f in range(192)}
    assert unpack == {(k, b, f) for (k, b), fmts in UNPACK_PAIRS.items() for f in fmts}


def test_every_format_the_reader_chooses_is_in_the_reader_table(tmp_path):
    """Every colour type and depth x PNG_FLAGS_BGR or not, under the flags and the chunk that move the choice between linear and sRGB: the
    (kind, raw flags, format) the loader hands on is one png_unpack_pairs accepts."""
    _, unpack = format_tables()
    rng = np.random.default_rng(11)
    files = []
    for kind in KINDS:
        ct, depth = R.TYPE_OF[kind]
        rows = case_rows(kind, 3, 2, rng)
        plte, trns = case_palette(kind, rng, trns=0)
        for flags in (0, R.FLAGS_IGNORE_SRGB, R.FLAGS_DEFAULT_LINEAR):
            for srgb in (None, 0):
                files += [(flags | bgr, R.encode(3, 2, ct, depth, rows, plte=plte, trns=trns, srgb=srgb)) for bgr in (0, R.FLAGS_BGR)]
    chosen = set()
    for (raw_hr, hr, meta_hr, d), (flags, _) in zip(load_many(HOST, str(tmp_path), files), files):
        assert (raw_hr, hr, meta_hr) == (0, 0, 0), (flags, hex(raw_hr), hex(hr), hex(meta_hr))
        assert (d["kind"], d["flags"], d["format"]) in unpack, (flags, d)
        chosen.add(d["format"])
    assert chosen == set(SOURCE)          # every format of the table is chosen by some file
