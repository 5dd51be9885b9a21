"""A numpy restatement of the TIFF reader and writer of directxtex_amd/host/DirectXTexAMD_TIFF.cpp and csrc/dxtex_tiff.h, over Python's zlib and
its own LZW and PackBits. The reference reads TIFF through WIC, which is not there to run against, so these are this project's rules; where
Pillow opens a file, tests/test_tiff_cpu.py holds this module to Pillow's decode.

Departures from WIC (DirectXTexAMD.h states them too):
  1. The Memory forms exist.
  2. NOT_SUPPORTED: BigTIFF; JPEG, CCITT and any other compression; YCbCr, CMYK, CIELab; signed integers and 16- or 64-bit floats; bits other
     than 1 / 4 / 8 / 16 / 32, or unequal across samples; grey plus alpha; more than one extra sample; FillOrder 2; old-style LSB-first LZW;
     predictor 2 on 1-, 4- or 32-bit samples; WhiteIsZero floats.
  3. Associated alpha (ExtraSamples 1) keeps the file's samples and sets TEX_ALPHA_MODE_PREMULTIPLIED; an unspecified fourth sample
     (ExtraSamples 0 or absent) reads as opaque, alpha forced to its maximum.
  4. Orientation and further IFDs are ignored.
  5. The writer stores uncompressed.

build() makes files (every layout the reader takes, and the damaged ones), decode() reads them, save() is the writer, and coded_rows() /
texels() are the two halves the GPU tests feed the kernels with."""
import struct
import zlib

import numpy as np

S_OK, E_FAIL, E_NOT_SUPPORTED = 0, 0x80004005, 0x80070032
FLAGS_NONE, FLAGS_IGNORE_SRGB, FLAGS_DEFAULT_SRGB, FLAGS_FORCE_SRGB, FLAGS_FORCE_LINEAR = 0, 1, 2, 0x20, 0x40
ALPHA_UNKNOWN, ALPHA_PREMULTIPLIED, ALPHA_OPAQUE = 0, 2, 3
(GREY1, GREY4, GREY8, GREY16, GREY32F, PAL1, PAL4, PAL8, RGB8, RGBA8, RGB16, RGBA16, RGB32F, RGBA32F) = range(14)
R32G32B32A32_FLOAT, R32G32B32_FLOAT, R16G16B16A16_UNORM, R8G8B8A8_UNORM, R8G8B8A8_UNORM_SRGB, R32_FLOAT, R16_UNORM, R8_UNORM = 2, 6, 11, 28, 29, 41, 56, 61
B8G8R8A8_UNORM, B8G8R8X8_UNORM, B8G8R8A8_UNORM_SRGB, B8G8R8X8_UNORM_SRGB = 87, 88, 91, 93
# kind -> (bits, samples, format, bytes of an image texel)
KINDS = {GREY1: (1, 1, R8_UNORM, 1), GREY4: (4, 1, R8_UNORM, 1), GREY8: (8, 1, R8_UNORM, 1), GREY16: (16, 1, R16_UNORM, 2), GREY32F: (32, 1, R32_FLOAT, 4),
         PAL1: (1, 1, R8G8B8A8_UNORM, 4), PAL4: (4, 1, R8G8B8A8_UNORM, 4), PAL8: (8, 1, R8G8B8A8_UNORM, 4), RGB8: (8, 3, R8G8B8A8_UNORM, 4),
         RGBA8: (8, 4, R8G8B8A8_UNORM, 4), RGB16: (16, 3, R16G16B16A16_UNORM, 8), RGBA16: (16, 4, R16G16B16A16_UNORM, 8),
         RGB32F: (32, 3, R32G32B32_FLOAT, 12), RGBA32F: (32, 4, R32G32B32A32_FLOAT, 16)}
NONE, LZW, DEFLATE, ADOBE_DEFLATE, PACKBITS = 1, 5, 8, 32946, 32773


# ---- the coders ---------------------------------------------------------------------------------------------------------------------------
def lzw_encode(data):
    """TIFF's LZW: MSB-first codes of 9 to 12 bits, the width changing one code early, a Clear code first and at 4094 entries"""
    out, acc, nbits = bytearray(), 0, 0

    def put(code, width):
        nonlocal acc, nbits
        acc = (acc << width) | code
        nbits += width
        while nbits >= 8:
            out.append((acc >> (nbits - 8)) & 0xFF)
            nbits -= 8
        acc &= (1 << nbits) - 1

    table, nxt, width = {}, 258, 9
    put(256, width)
    w = b""
    for byte in bytes(data):
        c = bytes([byte])
        if len(w) == 0 or (w + c) in table:
            w = w + c
            continue
        put(table[w] if len(w) > 1 else w[0], width)
        table[w + c] = nxt
        nxt += 1
        if nxt == (1 << width) and width < 12:
            width += 1
        if nxt == 4094:
            put(256, width)
            table, nxt, width = {}, 258, 9
        w = c
    if w:
        put(table[w] if len(w) > 1 else w[0], width)
        nxt += 1
        if nxt == (1 << width) and width < 12:
            width += 1
    put(257, width)
    if nbits:
        out.append((acc << (8 - nbits)) & 0xFF)
    return bytes(out)


def lzw_decode(data, cap):
    """-> cap bytes, or None for a defect or a stream that ends short; "old" for the LSB-first form"""
    if len(data) >= 2 and data[0] == 0 and (data[1] & 1):
        return "old"
    out, table, width, old, acc, nbits, at = bytearray(), None, 9, None, 0, 0, 0
    strings = [bytes([i]) for i in range(256)] + [b"", b""]
    table = list(strings)
    while len(out) < cap:
        while nbits < width:
            if at == len(data):
                return None
            acc = (acc << 8) | data[at]
            at += 1
            nbits += 8
        code = (acc >> (nbits - width)) & ((1 << width) - 1)
        nbits -= width
        acc &= (1 << nbits) - 1
        if code == 257:
            return None
        if code == 256:
            table, width, old = list(strings), 9, None
            continue
        if old is None:
            if code > 255:
                return None
            out += table[code]
            old = code
            continue
        nxt = len(table)
        if code > nxt or (code == nxt and nxt > 4095):
            return None
        if nxt < 4096:
            table.append(table[old] + (table[code][:1] if code < nxt else table[old][:1]))
        out += table[code]
        old = code
        if len(table) + 1 == (1 << width) and width < 12:
            width += 1
    return bytes(out[:cap])


def packbits_encode(data, row_bytes):
    """row by row, as the format asks: runs of three or more as a repeat, the rest as literals"""
    out = bytearray()
    data = bytes(data)
    for r in range(0, len(data), row_bytes):
        row, i = data[r:r + row_bytes], 0
        while i < len(row):
            run = 1
            while i + run < len(row) and row[i + run] == row[i] and run < 128:
                run += 1
            if run >= 3:
                out += bytes([257 - run, row[i]])
                i += run
                continue
            j = i
            while j < len(row) and j - i < 128 and not (j + 2 < len(row) and row[j] == row[j + 1] == row[j + 2]):
                j += 1
            out += bytes([j - i - 1]) + row[i:j]
            i = j
    return bytes(out)


def packbits_decode(data, cap):
    out, at = bytearray(), 0
    while len(out) < cap:
        if at == len(data):
            return None
        c = data[at] - 256 if data[at] > 127 else data[at]
        at += 1
        if c == -128:
            continue
        if c < 0:
            if at == len(data):
                return None
            out += bytes([data[at]]) * (1 - c)
            at += 1
        else:
            if len(data) - at < c + 1:
                return None
            out += data[at:at + c + 1]
            at += c + 1
    return bytes(out[:cap])


def inflate(data, cap):
    try:
        d = zlib.decompressobj()
        out = d.decompress(bytes(data), cap)
        return out if len(out) == cap else None
    except zlib.error:
        return None


# ---- rows: samples <-> the bytes of a segment's rows ------------------------------------------------------------------------------------------
def coded_rows(samples, bits, predictor=1, big_endian=False, stride=1):
    """samples: (rows, n) values of one row each - uint8 for 1 / 4 / 8 bits, uint16, float32 - n = columns * samples a pixel. -> (rows, rowBytes)
    uint8: packed at `bits`, predictor-coded with `stride` elements between neighbours, in the byte order asked for"""
    a = np.asarray(samples)
    rows, n = a.shape
    if bits in (1, 4):
        per = 8 // bits
        pad = np.zeros((rows, (n + per - 1) // per * per), np.uint8)
        pad[:, :n] = a
        pad = pad.reshape(rows, -1, per).astype(np.uint32)
        shifts = np.arange(per - 1, -1, -1, dtype=np.uint32) * bits
        return (pad << shifts).sum(axis=2).astype(np.uint8)
    if bits == 32:
        be = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(">u4").view(np.uint8).reshape(rows, n, 4)
        if predictor != 3:
            return (be if big_endian else be[:, :, ::-1]).reshape(rows, n * 4).copy()
        planes = be.transpose(0, 2, 1).reshape(rows, n * 4).astype(np.int32)          # the most significant bytes first, whatever the byte order
        planes[:, stride:] = planes[:, stride:] - planes[:, :-stride]
        return (planes & 0xFF).astype(np.uint8)
    v = a.astype(np.int64)
    if predictor == 2:
        v[:, stride:] = v[:, stride:] - v[:, :-stride]
    v &= (1 << bits) - 1
    if bits == 8:
        return v.astype(np.uint8)
    return v.astype(">u2" if big_endian else "<u2").view(np.uint8).reshape(rows, n * 2).copy()


def plain_samples(rows_bytes, bits, n, predictor=1, big_endian=False, stride=1):
    """the reverse: (rows, rowBytes) uint8 -> (rows, n) samples, through the undo"""
    b = np.asarray(rows_bytes, np.uint8)
    rows = b.shape[0]
    if bits in (1, 4):
        per = 8 // bits
        shifts = np.arange(per - 1, -1, -1, dtype=np.uint32) * bits
        v = (b[:, :, None].astype(np.uint32) >> shifts) & ((1 << bits) - 1)
        return v.reshape(rows, -1)[:, :n].astype(np.uint8)
    if bits == 32:
        if predictor == 3:
            total = b.shape[1]          # a tile's row runs over the tile's width: its planes are rowBytes / 4 long
            u = b.astype(np.int64)
            for k in range(stride):
                u[:, k::stride] = np.cumsum(u[:, k::stride], axis=1)
            u = (u & 0xFF).astype(np.uint32).reshape(rows, 4, total // 4)
            w = (u[:, 0] << 24) | (u[:, 1] << 16) | (u[:, 2] << 8) | u[:, 3]
            return w[:, :n].astype(np.uint32).view(np.float32)
        return b[:, :n * 4].copy().view(">u4" if big_endian else "<u4").astype(np.uint32).view(np.float32).reshape(rows, n)
    if bits == 8:
        v = b.astype(np.int64)
    else:
        v = b[:, :b.shape[1] // 2 * 2].copy().view(">u2" if big_endian else "<u2").astype(np.int64)
    if predictor == 2:
        for k in range(stride):
            v[:, k::stride] = np.cumsum(v[:, k::stride], axis=1)
        v &= (1 << bits) - 1
    return v[:, :n].astype(np.uint8 if bits == 8 else np.uint16)


def texels(samples, kind, white_is_zero=False, opaque=False, palette=None):
    """samples: (h, w, S) of the kind's sample type -> the image's tight rows as (h, w * imageBytes) uint8"""
    bits, S, _, _ = KINDS[kind]
    a = np.asarray(samples)
    h, w = a.shape[:2]
    if S == 1:
        v = a.reshape(h, w)
        if kind in (PAL1, PAL4, PAL8):
            return np.asarray(palette, np.uint32)[v.astype(np.int64)].astype("<u4").view(np.uint8).reshape(h, w * 4)
        if kind == GREY32F:
            return np.ascontiguousarray(v, np.float32).view(np.uint8).reshape(h, w * 4)
        v = v.astype(np.uint32)
        top = 0xFFFF if bits == 16 else (1 << bits) - 1
        if white_is_zero:
            v = top - v
        v = v * (255 if bits == 1 else 17 if bits == 4 else 1)
        return v.astype("<u2").view(np.uint8).reshape(h, w * 2) if bits == 16 else v.astype(np.uint8)
    dtype = {8: np.uint8, 16: np.uint16, 32: np.float32}[bits]
    top = {8: 0xFF, 16: 0xFFFF, 32: 1.0}[bits]
    out = np.full((h, w, 3 if kind == RGB32F else 4), top, dtype)
    out[:, :, :3] = a[:, :, :3]
    if S == 4 and not opaque:
        out[:, :, 3] = a[:, :, 3]
    return np.ascontiguousarray(out).view(np.uint8).reshape(h, -1)


def palette_words(colormap, bits):
    """the ColorMap's 3 << bits SHORTs -> the 256 words tiff_texels stores"""
    n = 1 << bits
    m = np.asarray(colormap, np.uint32)
    words = np.zeros(256, np.uint32)
    words[:n] = (m[:n] >> 8) | ((m[n:2 * n] >> 8) << 8) | ((m[2 * n:3 * n] >> 8) << 16) | 0xFF000000
    return words


# ---- build: a file around samples -----------------------------------------------------------------------------------------------------------------
def compress(data, compression, row_bytes, old_lzw=False):
    if compression == NONE:
        return bytes(data)
    if compression == LZW:
        return lzw_encode(data)
    if compression == PACKBITS:
        return packbits_encode(data, row_bytes)
    return zlib.compress(bytes(data), 6)


def build(samples, kind, compression=NONE, predictor=1, big_endian=False, planar=False, rows_per_strip=None, tile=None, white_is_zero=False,
          extra=None, colormap=None, colour_space=None, sample_format=None, override=None, drop=(), photometric=None, bits_list=None, magic=42, fill_order=None):
    """samples: (h, w, S) of the kind's sample type -> the file's bytes. tile = (width, length); extra = the ExtraSamples value of a fourth
    sample (None: no tag); colour_space = the Exif ColorSpace (None: no Exif IFD). For the damaged files: override = {tag: (type, [values])}
    replaces or adds an entry, drop = tags left out, and photometric, bits_list, sample_format, magic and fill_order state what the file
    claims whatever it holds."""
    bits, S, _, _ = KINDS[kind]
    a = np.asarray(samples)
    h, w = a.shape[:2]
    a = a.reshape(h, w, S)
    E = ">" if big_endian else "<"
    planes = S if planar and S > 1 else 1
    per_row = 1 if planes > 1 else S
    segments = []          # compressed bytes, in the file's order: plane by plane, rows of tiles
    seg_h = tile[1] if tile else min(rows_per_strip or h, h)
    seg_w = tile[0] if tile else w
    for p in range(planes):
        for y in range(0, h, seg_h):
            for x in range(0, w, seg_w):
                block = a[y:y + seg_h, x:x + seg_w, :] if planes == 1 else a[y:y + seg_h, x:x + seg_w, p:p + 1]
                if tile:          # partial edge tiles are padded in the file
                    full = np.zeros((seg_h, seg_w, block.shape[2]), a.dtype)
                    full[:block.shape[0], :block.shape[1]] = block
                    block = full
                coded = predictor if compression in (LZW, DEFLATE, ADOBE_DEFLATE) else 1          # the tag is written, and ignored by every reader
                rows = coded_rows(block.reshape(block.shape[0], -1), bits, coded, big_endian, per_row)
                segments.append(compress(rows.tobytes(), compression, rows.shape[1]))
    tags = {}

    def put(tag, typ, values):
        tags[tag] = (typ, list(values))

    put(256, 4, [w]); put(257, 4, [h])
    put(258, 3, bits_list if bits_list is not None else [bits] * S)
    put(259, 3, [compression])
    put(262, 3, [photometric if photometric is not None else (3 if kind in (PAL1, PAL4, PAL8) else 2 if S >= 3 else 0 if white_is_zero else 1)])
    if fill_order is not None:
        put(266, 3, [fill_order])
    put(277, 3, [S])
    put(284, 3, [2 if planar else 1])
    if predictor != 1:
        put(317, 3, [predictor])
    if colormap is not None:
        put(320, 3, colormap)
    if extra is not None:
        put(338, 3, [extra])
    fmt = sample_format if sample_format is not None else (3 if bits == 32 else None)
    if fmt is not None:
        put(339, 3, [fmt] * S)
    if tile:
        put(322, 3, [tile[0]]); put(323, 3, [tile[1]])
        put(324, 4, [0] * len(segments)); put(325, 4, [len(s) for s in segments])
    else:
        if rows_per_strip is not None:
            put(278, 3 if rows_per_strip < 65536 else 4, [rows_per_strip])
        put(273, 4, [0] * len(segments)); put(279, 4, [len(s) for s in segments])
    if colour_space is not None:
        put(34665, 4, [0])
    for t in drop:
        tags.pop(t, None)
    # layout: header, segments, IFD, values, Exif IFD
    at = 8
    offsets = []
    for s in segments:
        offsets.append(at)
        at += len(s) + (len(s) & 1)
    where = 324 if tile else 273
    if where in tags:
        tags[where] = (4, offsets)
    for t, v in (override or {}).items():
        tags[t] = v
    ifd_at = at
    size = {1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 16: 8}
    code = {1: "B", 2: "B", 3: "H", 4: "I", 16: "Q"}
    values_at = ifd_at + 2 + 12 * len(tags) + 4
    body, entries = bytearray(), bytearray()
    exif_fix = None
    for t in sorted(tags):
        typ, vals = tags[t]
        raw = struct.pack(E + code.get(typ, "B") * len(vals), *vals) if typ != 5 else b"".join(struct.pack(E + "II", *v) for v in vals)
        count = len(vals)
        if len(raw) <= 4:
            field = raw + bytes(4 - len(raw))
        else:
            field = struct.pack(E + "I", values_at + len(body))
            body += raw + bytes(len(raw) & 1)
        if t == 34665 and (override is None or 34665 not in override):
            exif_fix = len(entries) + 8
        entries += struct.pack(E + "HHI", t, typ, count) + field
    exif = b""
    if exif_fix is not None:
        entries[exif_fix:exif_fix + 4] = struct.pack(E + "I", values_at + len(body))
        exif = struct.pack(E + "H", 1) + struct.pack(E + "HHIHH", 40961, 3, 1, colour_space, 0) + struct.pack(E + "I", 0)
    out = bytearray((b"MM" if big_endian else b"II") + struct.pack(E + "HI", magic, ifd_at))
    for s in segments:
        out += s + bytes(len(s) & 1)
    out += struct.pack(E + "H", len(tags)) + entries + struct.pack(E + "I", 0) + body + exif
    return bytes(out)


# ---- decode: the reader -------------------------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, hr):
        self.hr = hr


def _ifd(data, E, at, wanted):
    if at < 8 or at > len(data) or len(data) - at < 6:
        raise Refused(E_FAIL)
    n = struct.unpack_from(E + "H", data, at)[0]
    if (len(data) - at - 6) // 12 < n:          # the entries and the offset of the next IFD behind them
        raise Refused(E_FAIL)
    sizes = [0, 1, 1, 2, 4, 8, 1, 1, 2, 4, 8, 4, 8]
    found = {}
    for i in range(n):
        e = at + 2 + 12 * i
        tag, typ, count = struct.unpack_from(E + "HHI", data, e)
        if tag not in wanted or tag in found:
            continue
        nbytes = (sizes[typ] if typ < 13 else 0) * count
        if not nbytes:
            raise Refused(E_FAIL)
        pos = e + 8
        if nbytes > 4:
            pos = struct.unpack_from(E + "I", data, e + 8)[0]
            if pos > len(data) or nbytes > len(data) - pos:
                raise Refused(E_FAIL)
        found[tag] = (typ, count, pos)
    return found


def _value(data, E, entry, k=0):
    typ, count, pos = entry
    if k >= count or typ not in (1, 3, 4):
        raise Refused(E_FAIL)
    return struct.unpack_from(E + {1: "B", 3: "H", 4: "I"}[typ], data, pos + k * {1: 1, 3: 2, 4: 4}[typ])[0]


def parse(data, flags=FLAGS_NONE):
    """-> a dict of what the IFD says (the layout, the metadata, the segments' places in the file); raises Refused"""
    data = bytes(data)
    if len(data) < 8 or data[:2] not in (b"II", b"MM"):
        raise Refused(E_FAIL)
    be = data[:2] == b"MM"
    E = ">" if be else "<"
    magic, first = struct.unpack_from(E + "HI", data, 2)
    if magic == 43:
        raise Refused(E_NOT_SUPPORTED)
    if magic != 42:
        raise Refused(E_FAIL)
    wanted = (256, 257, 258, 259, 262, 266, 273, 277, 278, 279, 284, 317, 320, 322, 323, 324, 325, 338, 339, 34665)
    t = _ifd(data, E, first, wanted)

    def one(tag, default):
        return _value(data, E, t[tag]) if tag in t else default

    if 256 not in t or 257 not in t or 262 not in t:
        raise Refused(E_FAIL)
    w, h, photometric = one(256, 0), one(257, 0), one(262, 0)
    if not w or not h or w > 0x0FFFFFFF or h > 0x0FFFFFFF:
        raise Refused(E_FAIL)
    S, compression, fill, planar, predictor = one(277, 1), one(259, 1), one(266, 1), one(284, 1), one(317, 1)
    if not S or planar not in (1, 2) or fill not in (1, 2) or not predictor:
        raise Refused(E_FAIL)
    if compression in (NONE, PACKBITS):
        predictor = 1          # the predictor belongs to the LZW and deflate coders: libtiff ignores the tag elsewhere, and so does this reader
    equal = True

    def per_sample(tag, default):
        nonlocal equal
        if tag not in t:
            return default
        v = _value(data, E, t[tag])
        for k in range(1, min(t[tag][1], S)):
            if _value(data, E, t[tag], k) != v:
                equal = False
        return v

    bits, fmt = per_sample(258, 1), per_sample(339, 1)
    if (258 in t and t[258][1] < S) or (339 in t and t[339][1] < S and t[339][1] != 1):
        raise Refused(E_FAIL)
    if compression not in (NONE, LZW, DEFLATE, ADOBE_DEFLATE, PACKBITS) or photometric > 3 or fill == 2 or not equal or bits not in (1, 4, 8, 16, 32):
        raise Refused(E_NOT_SUPPORTED)
    fmt = 1 if fmt == 4 else fmt
    if fmt not in (1, 3) or (fmt == 3) != (bits == 32):
        raise Refused(E_NOT_SUPPORTED)
    colours = 3 if photometric == 2 else 1
    if S < colours:
        raise Refused(E_FAIL)
    extras = S - colours
    if 338 in t and t[338][1] != extras:
        raise Refused(E_FAIL)
    if extras > 1 or (extras and colours == 1) or (colours == 3 and bits < 8) or (photometric == 3 and bits > 8) or (photometric == 0 and bits == 32):
        raise Refused(E_NOT_SUPPORTED)
    if not (predictor == 1 or (predictor == 2 and bits in (8, 16)) or (predictor == 3 and bits == 32)):
        raise Refused(E_NOT_SUPPORTED)
    if photometric == 3 and (320 not in t or t[320][0] != 3 or t[320][1] < (3 << bits)):
        raise Refused(E_FAIL)
    if photometric == 3:
        kind = {1: PAL1, 4: PAL4, 8: PAL8}[bits]
    elif colours == 1:
        kind = {1: GREY1, 4: GREY4, 8: GREY8, 16: GREY16, 32: GREY32F}[bits]
    else:
        kind = {8: RGB8, 16: RGB16, 32: RGB32F}[bits] + extras
    extra = _value(data, E, t[338]) if extras and 338 in t else 0
    opaque = bool(extras) and extra not in (1, 2)
    is_planar = planar == 2 and S > 1
    planes = S if is_planar else 1
    tiled = 324 in t
    if tiled:
        if 322 not in t or 323 not in t or 325 not in t:
            raise Refused(E_FAIL)
        seg_w, seg_h = one(322, 0), one(323, 0)
        if not seg_w or not seg_h or seg_w > 0x0FFFFFFF or seg_h > 0x0FFFFFFF:
            raise Refused(E_FAIL)
    else:
        if 273 not in t or 279 not in t:
            raise Refused(E_FAIL)
        rps = one(278, 0xFFFFFFFF)
        if not rps:
            raise Refused(E_FAIL)
        seg_w, seg_h = w, min(rps, h)
    across, down = (w + seg_w - 1) // seg_w, (h + seg_h - 1) // seg_h
    count = across * down * planes
    offs, cnts = t[324 if tiled else 273], t[325 if tiled else 279]
    if offs[1] < count or cnts[1] < count or offs[0] not in (3, 4) or cnts[0] not in (3, 4):
        raise Refused(E_FAIL)
    if (seg_w * (1 if is_planar else S) * 32 + 7) // 8 > 0x3FFFFFFF:
        raise Refused(E_FAIL)
    srgb = False
    if kind in (PAL1, PAL4, PAL8, RGB8, RGBA8):
        named = False
        if 34665 in t:
            if t[34665][0] != 4:
                raise Refused(E_FAIL)
            sub = _ifd(data, E, _value(data, E, t[34665]), (40961,))
            if 40961 in sub:
                named, srgb = True, _value(data, E, sub[40961]) == 1
        if not named and flags & FLAGS_DEFAULT_SRGB:
            srgb = True
        if flags & FLAGS_IGNORE_SRGB:
            srgb = False
    alpha = ALPHA_UNKNOWN
    if kind in (PAL1, PAL4, PAL8) or (colours == 3 and kind != RGB32F):
        if not extras or opaque:
            alpha = ALPHA_OPAQUE
        elif extra == 1:
            alpha = ALPHA_PREMULTIPLIED
    return dict(data=data, E=E, tags=t, width=w, height=h, bits=bits, samples=S, kind=kind, predictor=predictor, big_endian=be, planar=is_planar,
                white_is_zero=photometric == 0, opaque=opaque, compression=compression, tiled=tiled, seg_w=seg_w, seg_h=seg_h, across=across, down=down,
                planes=planes, offsets=offs, counts=cnts, format=R8G8B8A8_UNORM_SRGB if srgb else KINDS[kind][2], alpha=alpha)


def segments(info):
    """the host Raw loader's half: -> (stream bytes, [(offset, first row, rows, first column, columns, row bytes, plane)]) with strips that
    follow one another merged and every other segment on a multiple of 16 bytes; raises Refused"""
    data, E = info["data"], info["E"]
    per_plane = info["across"] * info["down"]
    count = per_plane * info["planes"]
    row_bytes = (info["seg_w"] * (1 if info["planar"] else info["samples"]) * info["bits"] + 7) // 8
    if count > len(data):
        raise Refused(E_FAIL)
    placed, at = [], 0
    for i in range(count):
        off, n = _value(data, E, info["offsets"], i), _value(data, E, info["counts"], i)
        if off > len(data) or n > len(data) - off:
            raise Refused(E_FAIL)
        plane, j = divmod(i, per_plane)
        ty, tx = divmod(j, info["across"])
        first_row, first_col = ty * info["seg_h"], tx * info["seg_w"]
        rows, cols = min(info["seg_h"], info["height"] - first_row), min(info["seg_w"], info["width"] - first_col)
        if info["tiled"] or j == 0:
            at = (at + 15) & ~15
        placed.append((at, first_row, rows, first_col, cols, row_bytes, plane, off, n))
        at += rows * row_bytes
    if at // 4096 > len(data):
        raise Refused(E_FAIL)
    stream = bytearray(at)
    out = []
    for (o, first_row, rows, first_col, cols, rb, plane, off, n) in placed:
        body, cap = data[off:off + n], rows * rb
        c = info["compression"]
        if c == NONE:
            got = body[:cap] if n >= cap else None
        elif c == PACKBITS:
            got = packbits_decode(body, cap)
        elif c == LZW:
            got = lzw_decode(body, cap)
            if got == "old":
                raise Refused(E_NOT_SUPPORTED)
        else:
            got = inflate(body, cap)
        if got is None:
            raise Refused(E_FAIL)
        stream[o:o + cap] = got
        last = out[-1] if out else None
        if last and not info["tiled"] and last[6] == plane and last[0] + last[2] * last[5] == o and last[1] + last[2] == first_row:
            out[-1] = (last[0], last[1], last[2] + rows, last[3], last[4], last[5], last[6])
        else:
            out.append((o, first_row, rows, first_col, cols, rb, plane))
    return bytes(stream), out


def layout_of(info):
    """the ten fields of dxtex_tiff_layout"""
    return (info["width"], info["height"], info["bits"], info["samples"], info["kind"], info["predictor"], int(info["big_endian"]), int(info["planar"]),
            int(info["white_is_zero"]), int(info["opaque"]))


def is_native(info):
    """a file that is its image already (csrc/dxtex_tiff.h's tiff_is_native): its rows are copied and no kernel runs"""
    return (info["predictor"] == 1 and not info["planar"] and (not info["big_endian"] or info["bits"] == 8) and not info["white_is_zero"] and not info["opaque"] and
            not info["tiled"] and info["kind"] in (GREY8, GREY16, GREY32F, RGBA8, RGBA16, RGBA32F, RGB32F))


def palette_of(info):
    if info["kind"] not in (PAL1, PAL4, PAL8):
        return None
    typ, count, pos = info["tags"][320]
    n = 3 << info["bits"]
    return palette_words(struct.unpack_from(info["E"] + "H" * n, info["data"], pos), info["bits"])


def decode(data, flags=FLAGS_NONE):
    """-> (S_OK, dict(width, height, format, alpha, pixels = the tight rows as bytes, info)) or (hresult, None)"""
    try:
        info = parse(data, flags)
        stream, segs = segments(info)
    except Refused as r:
        return r.hr, None
    kind, bits, S = info["kind"], info["bits"], info["samples"]
    w, h = info["width"], info["height"]
    per_row = 1 if info["planar"] else S
    dtype = np.float32 if bits == 32 else np.uint16 if bits == 16 else np.uint8
    full = np.zeros((h, w, S), dtype)
    buf = np.frombuffer(stream, np.uint8)
    for (o, first_row, rows, first_col, cols, rb, plane) in segs:
        block = plain_samples(buf[o:o + rows * rb].reshape(rows, rb), bits, cols * per_row, info["predictor"], info["big_endian"], per_row)
        if info["planar"]:
            full[first_row:first_row + rows, first_col:first_col + cols, plane] = block
        else:
            full[first_row:first_row + rows, first_col:first_col + cols, :] = block.reshape(rows, cols, S)
    px = texels(full, kind, info["white_is_zero"], info["opaque"], palette_of(info))
    return S_OK, dict(width=w, height=h, format=info["format"], alpha=info["alpha"], pixels=px.tobytes(), info=info)


# ---- save: the writer -----------------------------------------------------------------------------------------------------------------------------------
# format -> (bits, samples, SampleFormat, bytes of an image texel, bytes of a file texel, BGR, sRGB)
SOURCES = {R8_UNORM: (8, 1, 1, 1, 1, False, False), R16_UNORM: (16, 1, 1, 2, 2, False, False), R32_FLOAT: (32, 1, 3, 4, 4, False, False),
           R8G8B8A8_UNORM: (8, 4, 1, 4, 4, False, False), R8G8B8A8_UNORM_SRGB: (8, 4, 1, 4, 4, False, True), R16G16B16A16_UNORM: (16, 4, 1, 8, 8, False, False),
           R32G32B32_FLOAT: (32, 3, 3, 12, 12, False, False), R32G32B32A32_FLOAT: (32, 4, 3, 16, 16, False, False),
           B8G8R8A8_UNORM: (8, 4, 1, 4, 4, True, False), B8G8R8A8_UNORM_SRGB: (8, 4, 1, 4, 4, True, True),
           B8G8R8X8_UNORM: (8, 3, 1, 4, 3, True, False), B8G8R8X8_UNORM_SRGB: (8, 3, 1, 4, 3, True, True)}


def pack_rows(pixels, width, height, fmt, row_pitch=None):
    """the writer's tight rows (what dxtex_tiff_pack leaves) from an image's bytes"""
    bits, S, _, ib, fb, bgr, _ = SOURCES[fmt]
    pitch = width * ib if row_pitch is None else row_pitch
    px = np.frombuffer(bytes(pixels), np.uint8)[:pitch * height].reshape(height, pitch)[:, :width * ib]
    if not bgr:
        return px.copy()
    t = px.reshape(height, width, 4)
    return np.ascontiguousarray(t[:, :, [2, 1, 0, 3][:fb]]).reshape(height, width * fb)


def save(pixels, width, height, fmt, flags=FLAGS_NONE, row_pitch=None):
    """-> (S_OK, the file's bytes) or (hresult, None): II, one IFD behind the header, one uncompressed chunky strip on a multiple of 16"""
    if fmt not in SOURCES:
        return E_NOT_SUPPORTED, None
    bits, S, sf, ib, fb, bgr, srgb = SOURCES[fmt]
    srgb = (srgb or bool(flags & FLAGS_FORCE_SRGB)) and not (flags & FLAGS_FORCE_LINEAR)
    rows = pack_rows(pixels, width, height, fmt, row_pitch).tobytes()
    n = 15 + (1 if S == 4 else 0) + (1 if srgb else 0)
    extra_at = 8 + 2 + 12 * n + 4
    head = extra_at + (4 * S if S > 2 else 0) + 16 + 12 + (18 if srgb else 0)
    head = (head + 15) & ~15
    entries, extra = bytearray(), bytearray()

    def entry(tag, typ, count, value):
        entries.extend(struct.pack("<HHII", tag, typ, count, value))

    def shorts(tag, count, value):
        if count <= 2:
            entry(tag, 3, count, value | (value << 16) if count == 2 else value)
        else:
            entry(tag, 3, count, extra_at + len(extra))
            extra.extend(struct.pack("<" + "H" * count, *([value] * count)))

    def rational(tag, num, den):
        entry(tag, 5, 1, extra_at + len(extra))
        extra.extend(struct.pack("<II", num, den))

    entry(256, 4, 1, width); entry(257, 4, 1, height)
    shorts(258, S, bits)
    entry(259, 3, 1, 1); entry(262, 3, 1, 1 if S == 1 else 2); entry(273, 4, 1, head); entry(277, 3, 1, S); entry(278, 4, 1, height); entry(279, 4, 1, len(rows))
    rational(282, 72, 1); rational(283, 72, 1)
    entry(284, 3, 1, 1); entry(296, 3, 1, 2)
    entry(305, 2, 11, extra_at + len(extra)); extra.extend(b"DirectXTex\0\0")
    if S == 4:
        entry(338, 3, 1, 2)
    shorts(339, S, sf)
    if srgb:
        entry(34665, 4, 1, extra_at + len(extra))
        extra.extend(struct.pack("<HHHIII", 1, 40961, 3, 1, 1, 0))
    out = b"II" + struct.pack("<HI", 42, 8) + struct.pack("<H", n) + bytes(entries) + struct.pack("<I", 0) + bytes(extra)
    assert len(out) <= head
    return S_OK, out + bytes(head - len(out)) + rows
