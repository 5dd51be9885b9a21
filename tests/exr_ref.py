"""A numpy restatement of the OpenEXR scanline rules that directxtex_amd/host/DirectXTexAMD_EXR.cpp and csrc/dxtex_exr.h implement, over
Python's zlib: a writer for compression NONE / RLE / ZIPS / ZIP with any channel list, window and line order, and a reader. The OpenEXR
library is not available to run the reference's codec (Auxiliary/DirectXTexEXR.cpp) against, so this is the yardstick, as tests/pnm_ref.py
and tests/png_ref.py are for their codecs.

The file (all integers and floats little-endian): magic 76 2f 31 01; a version word (low byte 2; 0x200 tiled, 0x400 long names, 0x800 deep,
0x1000 multipart); attributes `name\\0 type\\0 int32 size, value` up to one 0 byte; one uint64 offset per chunk, entry i the chunk that starts
at yMin + i * lines; chunks `int32 y, int32 dataSize, data`. The plain layout of a chunk: for each scanline, for each channel in the byte
order of the names, `width` samples of 2 (HALF) or 4 (UINT, FLOAT) bytes. A chunk of RLE / ZIPS / ZIP whose dataSize is the plain size is
plain; otherwise it expands (zlib, or RLE packets) to exactly the plain size n in coded form: t[i] = t[i-1] + t[i] - 128 (mod 256) for
i >= 1, then plain[2k] = t[k], plain[2k+1] = t[(n+1)/2 + k].

Departures of this project from the library, which this file shares (DirectXTexAMD.h lists them): HRESULT_E_NOT_SUPPORTED for tiled, deep
and multipart files, for PIZ, PXR24, B44, B44A, DWAA and DWAB, for RY / BY channels and for any channel whose sampling is not 1; chunks are
read through the offset table alone; an `envmap` file whose height / 6 is its width but whose height is not six widths is E_FAIL; the
writer stores compression NONE."""
import struct
import zlib

import numpy as np

S_OK = 0
E_FAIL = 0x80004005
E_INVALIDARG = 0x80070057
E_POINTER = 0x80004003
E_NOT_SUPPORTED = 0x80070032
E_FILE_NOT_FOUND = 0x80070002

MAGIC = bytes([0x76, 0x2F, 0x31, 0x01])
TILED, LONG_NAMES, DEEP, MULTIPART = 0x200, 0x400, 0x800, 0x1000
UINT, HALF, FLOAT, ABSENT = 0, 1, 2, 3
TYPE_BYTES = {UINT: 4, HALF: 2, FLOAT: 4}
NONE, RLE, ZIPS, ZIP, PIZ, PXR24, B44, B44A, DWAA, DWAB = range(10)
LINES = {NONE: 1, RLE: 1, ZIPS: 1, ZIP: 16}
INCREASING, DECREASING, RANDOM = 0, 1, 2
RGBA16F, RGBA32F, RGB32F = 10, 2, 6          # DXGI_FORMAT_*: what the writer takes


# ---- the sample conversions --------------------------------------------------------------------------------------------------------------
def _round_half(mag_bits):
    """bits of float magnitudes below 2^16 -> half bits, rounded to nearest even by numpy's own conversion"""
    with np.errstate(over="ignore"):
        return np.asarray(mag_bits, np.uint32).view(np.float32).astype(np.float16).view(np.uint16).astype(np.uint32)


def float_to_half(bits):
    """the reader's FLOAT: beyond +-65504 the infinity, a NaN keeps its top ten mantissa bits (bit 0 set where they are zero), else RNE"""
    bits = np.asarray(bits, np.uint32)
    sign, x = (bits >> 16) & 0x8000, bits & 0x7FFFFFFF
    nan_m = (x >> 13) & 0x3FF
    nan = 0x7C00 | nan_m | (nan_m == 0)
    finite = _round_half(np.where(x > 0x477FE000, 0, x))
    return (sign | np.where(x > 0x7F800000, nan, np.where(x > 0x477FE000, 0x7C00, finite))).astype(np.uint16)


def uint_to_half(u):
    u = np.asarray(u, np.uint32)
    small = np.where(u > 65504, 0, u).astype(np.float32).view(np.uint32)
    return np.where(u > 65504, 0x7C00, _round_half(small)).astype(np.uint16)


def sample_to_half(typ, raw):
    return np.asarray(raw).astype(np.uint16) if typ == HALF else float_to_half(raw) if typ == FLOAT else uint_to_half(raw)


def xm_float_to_half(bits):
    """the writer's conversion, XMConvertFloatToHalf: RNE, overflow becomes infinity, a NaN is sign | 0x7e00 | mantissa >> 13"""
    bits = np.asarray(bits, np.uint32)
    sign, x = (bits >> 16) & 0x8000, bits & 0x7FFFFFFF
    finite = _round_half(np.where(x >= 0x7F800000, 0, x))
    return (sign | np.where(x > 0x7F800000, 0x7E00 | ((x >> 13) & 0x3FF), np.where(x == 0x7F800000, 0x7C00, finite))).astype(np.uint16)


# ---- the coded form ----------------------------------------------------------------------------------------------------------------------
def code(plain):
    """the plain bytes of a chunk -> what the compressor sees: the two byte planes, delta-coded"""
    p = np.frombuffer(plain, np.uint8)
    t = np.concatenate([p[0::2], p[1::2]]).astype(np.int32)
    d = t.copy()
    d[1:] = t[1:] - t[:-1] + 128
    return (d & 0xFF).astype(np.uint8).tobytes()


def uncode(coded):
    t = (np.cumsum(np.frombuffer(coded, np.uint8).astype(np.int64)) - 128 * np.arange(len(coded))) & 0xFF
    n = len(coded)
    out = np.zeros(n, np.uint8)
    out[0::2] = t[:(n + 1) // 2]
    out[1::2] = t[(n + 1) // 2:]
    return out.tobytes()


def rle(data):
    """the library's packets: a run of 3 to 128 equal bytes as (count - 1, byte); up to 127 others as (-count, bytes)"""
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        j = i + 1
        while j < n and data[j] == data[i] and j - i < 128:
            j += 1
        if j - i >= 3:
            out += bytes([j - i - 1, data[i]])
            i = j
            continue
        j = i
        while j < n and j - i < 127 and not (j + 2 < n and data[j] == data[j + 1] == data[j + 2]):
            j += 1
        out += bytes([256 - (j - i)]) + data[i:j]
        i = j
    return bytes(out)


def unrle(data, cap):
    """None unless the packets are used up as the last of cap bytes comes out"""
    out, i, n = bytearray(), 0, len(data)
    while i < n:
        c = data[i] - 256 if data[i] > 127 else data[i]
        i += 1
        if c < 0:
            if n - i < -c or cap - len(out) < -c:
                return None
            out += data[i:i - c]
            i -= c
        else:
            if i == n or cap - len(out) < c + 1:
                return None
            out += bytes([data[i]]) * (c + 1)
            i += 1
    return bytes(out) if len(out) == cap else None


# ---- the writer --------------------------------------------------------------------------------------------------------------------------
def attribute(name, typ, value):
    return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(value)) + value


def chlist(channels):
    """channels = [(name, type, xSampling, ySampling)], written in the order given"""
    return b"".join(n.encode() + b"\0" + struct.pack("<iB3xii", t, 0, xs, ys) for n, t, xs, ys in channels) + b"\0"


def header(channels, compression, window, display=None, line_order=INCREASING, extra=(), version=2, omit=()):
    """the eight needed attributes in name order, `extra` = [(name, type, value)] behind them, minus the names in `omit`"""
    display = window if display is None else display
    attrs = [("channels", "chlist", chlist(channels)), ("compression", "compression", bytes([compression])),
             ("dataWindow", "box2i", struct.pack("<4i", *window)), ("displayWindow", "box2i", struct.pack("<4i", *display)),
             ("lineOrder", "lineOrder", bytes([line_order])), ("pixelAspectRatio", "float", struct.pack("<f", 1.0)),
             ("screenWindowCenter", "v2f", struct.pack("<2f", 0.0, 0.0)), ("screenWindowWidth", "float", struct.pack("<f", 1.0))]
    attrs = [a for a in attrs if a[0] not in omit] + list(extra)
    return MAGIC + struct.pack("<I", version) + b"".join(attribute(*a) for a in attrs) + b"\0"


def plain_chunk(channels, samples, y0, rows):
    """rows y0 .. y0 + rows - 1 (from the window's top) in the plain layout. samples: name -> (height, width) array, uint16 for HALF and
    uint32 (a FLOAT's bits) otherwise"""
    out = bytearray()
    for y in range(y0, y0 + rows):
        for name, typ, _, _ in sorted(channels, key=lambda c: c[0].encode()):
            out += np.ascontiguousarray(samples[name][y], "<u2" if typ == HALF else "<u4").tobytes()
    return bytes(out)


def write(channels, samples, compression, window, line_order=INCREASING, extra=(), raw_chunks=(), seed=0, level=6, display=None):
    """an .exr file. window = (xMin, yMin, xMax, yMax); raw_chunks: indices of chunks stored plain whatever coding would give (the raw-chunk
    rule stores every chunk plain that coding does not shrink); line_order decides where the chunks lie in the file, the table is always
    indexed from the top"""
    height = window[3] - window[1] + 1
    lines = LINES[compression]
    count = (height + lines - 1) // lines
    bodies = []
    for i in range(count):
        plain = plain_chunk(channels, samples, i * lines, min(lines, height - i * lines))
        data = plain
        if compression != NONE and i not in raw_chunks:
            coded = rle(code(plain)) if compression == RLE else zlib.compress(code(plain), level)
            if len(coded) < len(plain):
                data = coded
        bodies.append(struct.pack("<ii", window[1] + i * lines, len(data)) + data)
    order = list(range(count))
    if line_order == DECREASING:
        order.reverse()
    elif line_order == RANDOM:
        order = [int(k) for k in np.random.default_rng(seed).permutation(count)]
    head = header(channels, compression, window, display, line_order, extra)
    at, offsets = len(head) + 8 * count, [0] * count
    for i in order:
        offsets[i] = at
        at += len(bodies[i])
    return head + struct.pack(f"<{count}Q", *offsets) + b"".join(bodies[i] for i in order)


def save(pixels, width, height, fmt):
    """the project's writer, byte for byte: version 2, the needed attributes in name order, channels A, B, G, R as HALF, increasing Y,
    compression NONE. pixels: tight rows of RGBA16F (halves), RGBA32F or RGB32F (floats, alpha 1.0) as a uint8 buffer"""
    px = np.frombuffer(np.ascontiguousarray(pixels, np.uint8).tobytes(), np.uint8)
    if fmt == RGBA16F:
        h = px.view("<u2").reshape(height, width, 4)
    else:
        n = 4 if fmt == RGBA32F else 3
        h = xm_float_to_half(px.view("<u4").reshape(height, width, n))
        if n == 3:
            h = np.concatenate([h, np.full((height, width, 1), 0x3C00, np.uint16)], axis=2)
    channels = [(c, HALF, 1, 1) for c in "ABGR"]
    samples = {"R": h[..., 0], "G": h[..., 1], "B": h[..., 2], "A": h[..., 3]}
    return write(channels, samples, NONE, (0, 0, width - 1, height - 1))


def pack_rows(pixels, width, height, fmt):
    """what dxtex_exr_pack leaves: for each row the A, B, G, R half planes, 8 * width bytes"""
    data = save(pixels, width, height, fmt)
    first = len(data) - height * (8 + 8 * width)
    return b"".join(data[first + y * (8 + 8 * width) + 8:first + (y + 1) * (8 + 8 * width)] for y in range(height))


# ---- the reader --------------------------------------------------------------------------------------------------------------------------
class Refused(Exception):
    def __init__(self, hr):
        super().__init__(hex(hr))
        self.hr = hr


def _name(data, at):
    end = data.find(b"\0", at, at + 256)
    if end <= at:
        raise Refused(E_FAIL)
    return data[at:end], end + 1


NEEDED = {b"channels": (b"chlist", 0), b"compression": (b"compression", 1), b"dataWindow": (b"box2i", 16), b"displayWindow": (b"box2i", 16),
          b"lineOrder": (b"lineOrder", 1), b"pixelAspectRatio": (b"float", 4), b"screenWindowCenter": (b"v2f", 8), b"screenWindowWidth": (b"float", 4)}


def parse_header(data):
    """-> (attributes of the needed names and envmap, the first byte behind the header)"""
    if len(data) < 8 or data[:4] != MAGIC:
        raise Refused(E_FAIL)
    version = struct.unpack_from("<I", data, 4)[0]
    if version & 0xFF != 2:
        raise Refused(E_FAIL)
    if version & (TILED | DEEP | MULTIPART):
        raise Refused(E_NOT_SUPPORTED)
    if version & ~(0xFF | LONG_NAMES):
        raise Refused(E_FAIL)
    got, at = {}, 8
    while True:
        if at >= len(data):
            raise Refused(E_FAIL)
        if data[at] == 0:
            at += 1
            break
        name, at = _name(data, at)
        if at >= len(data):
            raise Refused(E_FAIL)
        typ, at = _name(data, at)
        if len(data) - at < 4:
            raise Refused(E_FAIL)
        size = struct.unpack_from("<I", data, at)[0]
        at += 4
        if size > 0x7FFFFFFF or size > len(data) - at:
            raise Refused(E_FAIL)
        value = data[at:at + size]
        at += size
        if name == b"envmap":
            got[name] = value
        elif name in NEEDED:
            want_type, want_size = NEEDED[name]
            if typ != want_type or (want_size and size != want_size) or name in got:
                raise Refused(E_FAIL)
            got[name] = value
            if name == b"channels":
                got[b"list"] = parse_chlist(value)
            elif name == b"compression" and value[0] >= 10:
                raise Refused(E_FAIL)
            elif name == b"lineOrder" and value[0] > 2:
                raise Refused(E_FAIL)
    if any(n not in got for n in NEEDED):
        raise Refused(E_FAIL)
    return got, at


def parse_chlist(value):
    out, at = [], 0
    while True:
        if at >= len(value):
            raise Refused(E_FAIL)
        if value[at] == 0:
            break
        name, at = _name(value, at)
        if len(value) - at < 16 or len(out) == 1024:
            raise Refused(E_FAIL)
        typ, _, xs, ys = struct.unpack_from("<iB3xii", value, at)
        at += 16
        if not 0 <= typ <= 2 or xs < 1 or ys < 1:
            raise Refused(E_FAIL)
        out.append((name, typ, xs, ys))
    out.sort(key=lambda c: c[0])
    if not out or any(a[0] == b[0] for a, b in zip(out, out[1:])):
        raise Refused(E_FAIL)
    return out


def shape(got):
    """-> dict(width, height (of the window), items, item_height, compression, scanline, table = [(offset, type) or None for R, G, B, A])"""
    x0, y0, x1, y1 = struct.unpack("<4i", got[b"dataWindow"])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    if w < 1 or h < 1 or w > 0x7FFFFFFF or h > 0x7FFFFFFF:
        raise Refused(E_FAIL)
    compression = got[b"compression"][0]
    if compression > ZIP:
        raise Refused(E_NOT_SUPPORTED)
    line, where = 0, {}
    for name, typ, xs, ys in got[b"list"]:
        if name in (b"RY", b"BY") or xs != 1 or ys != 1:
            raise Refused(E_NOT_SUPPORTED)
        where[name] = (line, typ)
        line += w * TYPE_BYTES[typ]
        if line > 0x7FFFFFFF // 16:
            raise Refused(E_FAIL)
    table = [where.get(n) for n in (b"R", b"G", b"B", b"A")]
    if b"Y" in where and table[:3] == [None] * 3:
        table[:3] = [where[b"Y"]] * 3
    items, item_height = 1, h
    if b"envmap" in got and w == h // 6:
        if h != 6 * w:
            raise Refused(E_FAIL)
        items, item_height = 6, w
    return dict(width=w, height=h, y_min=y0, items=items, item_height=item_height, compression=compression, scanline=line, table=table)


def metadata(data):
    """(hresult, (width, height, arraySize) or None): GetMetadataFromEXRMemory"""
    try:
        s = shape(parse_header(data)[0])
    except Refused as r:
        return r.hr, None
    return S_OK, (s["width"], s["item_height"], s["items"])


def texels(plain, s, rows):
    """the plain bytes of `rows` scanlines -> (rows, width, 4) halves"""
    w = s["width"]
    p = np.frombuffer(plain, np.uint8).reshape(rows, s["scanline"])
    out = np.zeros((rows, w, 4), np.uint16)
    out[..., 3] = 0x3C00
    for c, entry in enumerate(s["table"]):
        if entry is not None:
            off, typ = entry
            raw = np.ascontiguousarray(p[:, off:off + w * TYPE_BYTES[typ]]).view("<u2" if typ == HALF else "<u4")
            out[..., c] = sample_to_half(typ, raw)
    return out


def read(data):
    """LoadFromEXRMemory: (hresult, None) or (S_OK, dict(width, height, items, pixels = (items * height, width, 4) uint16, stream_bytes,
    chunks = [(first row, rows, coded)]))"""
    try:
        got, at = parse_header(data)
        s = shape(got)
        lines = LINES[s["compression"]]
        count = (s["height"] + lines - 1) // lines
        if (len(data) - at) // 8 < count:
            raise Refused(E_FAIL)
        pixels = np.zeros((s["height"], s["width"], 4), np.uint16)
        chunks, stream = [], 0
        for i in range(count):
            off = struct.unpack_from("<Q", data, at + 8 * i)[0]
            if off == 0 or off > len(data) or len(data) - off < 8:
                raise Refused(E_FAIL)
            y, size = struct.unpack_from("<iI", data, off)
            rows = min(lines, s["height"] - i * lines)
            plain_size = rows * s["scanline"]
            if y != s["y_min"] + i * lines or size > 0x7FFFFFFF or size > len(data) - off - 8:
                raise Refused(E_FAIL)
            if size > plain_size or (s["compression"] == NONE and size != plain_size):
                raise Refused(E_FAIL)
            body = data[off + 8:off + 8 + size]
            coded = size != plain_size
            if coded:
                if s["compression"] == RLE:
                    t = unrle(body, plain_size)
                else:
                    z = zlib.decompressobj()
                    try:
                        t = z.decompress(body)
                    except zlib.error:
                        t = None
                    if t is not None and (not z.eof or z.unused_data or len(t) != plain_size):
                        t = None
                if t is None:
                    raise Refused(E_FAIL)
                body = uncode(t)
                stream = (stream + 15) & ~15
            stream += plain_size
            pixels[i * lines:i * lines + rows] = texels(body, s, rows)
            chunks.append((i * lines, rows, coded))
    except Refused as r:
        return r.hr, None
    return S_OK, dict(width=s["width"], height=s["item_height"], items=s["items"], pixels=pixels, stream_bytes=stream, chunks=chunks, shape=s)
