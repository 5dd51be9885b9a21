"""A restatement of the PNG codec's rules (directxtex_amd/host/DirectXTexAMD_PNG.cpp, csrc/dxtex_png.h) over Python's zlib, the yardstick of
tests/test_png_*.py. libpng is not there to run Auxiliary/DirectXTexPNG.cpp against; what is restated are its Update, GuessFormat, GetHeader and
WriteImage, with the project's four departures: no alpha association and no gamma correction (every sample is the file's), grey with tRNS is
NOT_SUPPORTED, the writer emits gAMA / sRGB in front of IDAT, and the memory forms exist.

  chunk / filter_rows / encode    a PNG file from unfiltered rows, with a chosen filter per row, any zlib level, strategy and window, IDAT split
                                  at any size
  decode                          a file's chunks -> unfiltered rows, through zlib.decompress and an unfilter of its own
  metadata / expand               format, miscFlags2 and texels the reader gives
  pack_rows / writer_chunks       the rows and the chunks the writer emits
"""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
R8, R16, RGBA8, RGBA8_SRGB, BGRA8, BGRX8, BGRA8_SRGB, BGRX8_SRGB, RGBA16 = 61, 56, 28, 29, 87, 88, 91, 93, 11
RGBA32F, R32F, BC1 = 2, 41, 71
FLAGS_BGR, FLAGS_IGNORE_SRGB, FLAGS_DEFAULT_LINEAR, FLAGS_FORCE_SRGB, FLAGS_FORCE_LINEAR = 0x1, 0x2, 0x4, 0x20, 0x40
ALPHA_MODE_OPAQUE = 3
S_OK, E_FAIL, E_INVALIDARG, E_POINTER, E_NOT_SUPPORTED, E_FILE_NOT_FOUND = 0, 0x80004005, 0x80070057, 0x80004003, 0x80070032, 0x80070002

# kind (DXTEX_PNG_*, directxtex_amd.formats) by (colour type, depth)
G1, G2, G4, G8, G16, GA8, GA16, RGB8, RGB16, RGBA8K, RGBA16K, P1, P2, P4, P8 = range(15)
KIND = {(0, 1): G1, (0, 2): G2, (0, 4): G4, (0, 8): G8, (0, 16): G16, (4, 8): GA8, (4, 16): GA16, (2, 8): RGB8, (2, 16): RGB16, (6, 8): RGBA8K,
        (6, 16): RGBA16K, (3, 1): P1, (3, 2): P2, (3, 4): P4, (3, 8): P8}
TYPE_OF = {k: v for v, k in KIND.items()}
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
IMAGE_BYTES = {G1: 1, G2: 1, G4: 1, G8: 1, G16: 2, GA8: 4, GA16: 8, RGB8: 4, RGB16: 8, RGBA8K: 4, RGBA16K: 8, P1: 4, P2: 4, P4: 4, P8: 4}


def file_bits(kind):
    ct, depth = TYPE_OF[kind]
    return CHANNELS[ct] * depth


def row_bytes(kind, width):
    return (width * file_bits(kind) + 7) // 8


def chunk(tag, body=b""):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_rows(rows, bpp, filters):
    """unfiltered rows -> the filtered stream: filter byte filters[y % len] in front of each row; the row above the first is zeros"""
    out = bytearray()
    prev = bytes(len(rows[0]))
    for y, row in enumerate(rows):
        f = filters[y % len(filters)]
        out.append(f)
        for i, x in enumerate(row):
            a = row[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            out.append((x - (0, a, b, (a + b) >> 1, _paeth(a, b, c))[f]) & 0xFF)
        prev = row
    return bytes(out)


def unfilter(stream, height, rowb, bpp):
    """the filtered stream -> tight unfiltered rows; ValueError for a filter byte above 4"""
    out = bytearray()
    prev = bytes(rowb)
    for y in range(height):
        f = stream[y * (rowb + 1)]
        if f > 4:
            raise ValueError("filter")
        src = stream[y * (rowb + 1) + 1:(y + 1) * (rowb + 1)]
        row = bytearray(rowb)
        for i, x in enumerate(src):
            a = row[i - bpp] if i >= bpp else 0
            b = prev[i]
            c = prev[i - bpp] if i >= bpp else 0
            row[i] = (x + (0, a, b, (a + b) >> 1, _paeth(a, b, c))[f]) & 0xFF
        out += row
        prev = row
    return bytes(out)


def ihdr(width, height, depth, ct, interlace=0):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, depth, ct, 0, 0, interlace))


def deflate(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 9, strategy)
    return c.compress(raw) + c.flush()


def split_idat(z, every=None):
    if not every:
        return chunk(b"IDAT", z)
    return b"".join(chunk(b"IDAT", z[i:i + every]) for i in range(0, len(z), every))


def encode(width, height, ct, depth, rows, filters=(0,), level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, every=None, plte=None, trns=None,
           gama=None, srgb=None, extra=b"", interlace=0):
    """rows: `height` unfiltered rows of row_bytes each. plte: 3 * n bytes; trns: bytes; gama: the integer; srgb: the intent; extra: whole
    chunks to put in front of IDAT."""
    bpp = max(1, CHANNELS[ct] * depth // 8)
    out = SIGNATURE + ihdr(width, height, depth, ct, interlace)
    if gama is not None:
        out += chunk(b"gAMA", struct.pack(">I", gama))
    if srgb is not None:
        out += chunk(b"sRGB", bytes([srgb]))
    if plte is not None:
        out += chunk(b"PLTE", plte)
    if trns is not None:
        out += chunk(b"tRNS", trns)
    out += extra
    return out + split_idat(deflate(filter_rows(rows, bpp, filters), level, strategy, wbits), every) + chunk(b"IEND")


def chunks(data):
    """[(tag, body)] of a file; ValueError for a bad signature, CRC or a chunk that runs past the end"""
    if data[:8] != SIGNATURE:
        raise ValueError("signature")
    at, out = 8, []
    while at < len(data):
        if len(data) - at < 12:
            raise ValueError("truncated")
        n, = struct.unpack(">I", data[at:at + 4])
        tag, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        if len(data) - at - 12 < n or struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] != zlib.crc32(tag + body) & 0xFFFFFFFF:
            raise ValueError("crc")
        out.append((tag, body))
        at += 12 + n
        if tag == b"IEND":
            break
    return out


def decode(data):
    """a file -> dict(width, height, ct, depth, kind, rows (tight unfiltered bytes), plte, trns, gama, srgb, tags). The stream's first
    height * (1 + row bytes) bytes count, as in the reader; zlib.error / ValueError for a defect."""
    cs = chunks(data)
    if not cs or cs[0][0] != b"IHDR" or cs[-1][0] != b"IEND":
        raise ValueError("chunks")
    w, h, depth, ct, comp, flt, lace = struct.unpack(">IIBBBBB", cs[0][1])
    kind = KIND[(ct, depth)]
    info = dict(width=w, height=h, ct=ct, depth=depth, kind=kind, plte=None, trns=None, gama=None, srgb=None, tags=[t for t, _ in cs])
    idat = b""
    for tag, body in cs[1:]:
        if tag == b"IDAT":
            idat += body
        elif not idat and tag == b"PLTE":
            info["plte"] = body
        elif not idat and tag == b"tRNS":
            info["trns"] = body
        elif not idat and tag == b"gAMA":
            info["gama"], = struct.unpack(">I", body)
        elif not idat and tag == b"sRGB":
            info["srgb"] = body[0]
    rowb = row_bytes(kind, w)
    need = h * (rowb + 1)
    d = zlib.decompressobj()
    raw = d.decompress(idat, need)
    # zlib goes on until it needs room: a stream that ends here has had its check value tested, one that goes on is left alone (surplus)
    if len(raw) < need:
        raise ValueError("short")
    info["rows"] = unfilter(raw, h, rowb, max(1, file_bits(kind) // 8))
    return info


def metadata(ct, depth, flags=0, srgb=None, gama=None):
    """(format, miscFlags2): Update's flag change, GuessFormat and GetHeader (DirectXTexPNG.cpp:126-251)"""
    if ct == 4:
        flags |= FLAGS_IGNORE_SRGB
    if ct == 0:
        return (R16 if depth == 16 else R8), 0
    if depth == 16:
        fmt = RGBA16
    else:
        linear, s = (BGRA8, BGRA8_SRGB) if flags & FLAGS_BGR else (RGBA8, RGBA8_SRGB)
        if flags & FLAGS_IGNORE_SRGB:
            fmt = linear
        elif srgb is not None:
            fmt = s
        elif gama is not None and gama != 0 and abs(gama / 100000.0 - 1.0) <= 1e-6:
            fmt = linear
        else:
            fmt = linear if flags & FLAGS_DEFAULT_LINEAR else s
    misc2 = 0
    if not ct & 4:
        if fmt == BGRA8:
            fmt = BGRX8
        elif fmt == BGRA8_SRGB:
            fmt = BGRX8_SRGB
        else:
            misc2 = ALPHA_MODE_OPAQUE
    return fmt, misc2


def palette_words(plte, trns=None):
    """the palette as the C ABI takes it: R | G << 8 | B << 16 | A << 24, A from tRNS where present, else 255"""
    n = len(plte) // 3
    p = np.frombuffer(plte, np.uint8).reshape(n, 3).astype(np.uint32)
    a = np.full(n, 255, np.uint32)
    if trns:
        a[:len(trns)] = np.frombuffer(trns, np.uint8)[:n]
    return p[:, 0] | (p[:, 1] << 8) | (p[:, 2] << 16) | (a << 24)


def expand(rows, width, height, kind, bgr=False, palette=None):
    """unfiltered rows -> the image's tight texels, (height, width * IMAGE_BYTES) uint8. palette: palette_words' result."""
    ct, depth = TYPE_OF[kind]
    rowb = row_bytes(kind, width)
    r = np.frombuffer(rows, np.uint8)[:height * rowb].reshape(height, rowb)
    if depth < 8:          # the first texel sits in the high bits; every row starts on a byte
        bits = np.unpackbits(r, axis=1)[:, :width * depth].reshape(height, width, depth)
        s = np.zeros((height, width), np.uint32)
        for b in range(depth):
            s = (s << 1) | bits[..., b]
    if ct == 0 and depth < 8:
        return (s * {1: 255, 2: 85, 4: 17}[depth]).astype(np.uint8)
    if ct == 3:
        idx = s if depth < 8 else r.astype(np.uint32)
        table = np.full(256, 0xFF000000, np.uint32)          # opaque black at and past the palette's end
        table[:len(palette)] = palette
        px = table[idx].astype("<u4").view(np.uint8).reshape(height, width, 4).copy()
        if bgr:
            px = px[..., [2, 1, 0, 3]]
        return np.ascontiguousarray(px).reshape(height, width * 4)
    c = CHANNELS[ct]
    if depth == 8:
        v = r.reshape(height, width, c)
        full = np.uint8(255)
    else:
        v = r.view(">u2").astype("<u2").reshape(height, width, c)
        full = np.uint16(65535)
    if ct == 0:
        out = v
    elif ct == 4:
        out = np.stack([v[..., 0], v[..., 0], v[..., 0], v[..., 1]], axis=2)
    elif ct == 2:
        out = np.concatenate([v, np.full((height, width, 1), full, v.dtype)], axis=2)
    else:
        out = v
    if bgr and depth == 8 and ct in (2, 6):
        out = out[..., [2, 1, 0, 3]]
    return np.ascontiguousarray(out).view(np.uint8).reshape(height, -1)


# ---- the writer ---------------------------------------------------------------------------------------------------------------------------
# format -> (colour type, depth, bytes of an image texel, bytes of a file texel)
WRITER = {R8: (0, 8, 1, 1), R16: (0, 16, 2, 2), RGBA8: (6, 8, 4, 4), RGBA8_SRGB: (6, 8, 4, 4), BGRA8: (6, 8, 4, 4), BGRA8_SRGB: (6, 8, 4, 4),
          RGBA16: (6, 16, 8, 8), BGRX8: (2, 8, 4, 3), BGRX8_SRGB: (2, 8, 4, 3)}


def pack_rows(px, width, height, fmt):
    """the image's tight texels (height, width * S) uint8 -> the file's rows (height, width * F) uint8 (WriteImage :315-404)"""
    ct, depth, S, F = WRITER[fmt]
    px = np.ascontiguousarray(px, np.uint8).reshape(height, width, S)
    if depth == 16:
        return np.ascontiguousarray(px.reshape(height, width, S // 2, 2)[..., ::-1]).reshape(height, width * F)
    if fmt in (BGRA8, BGRA8_SRGB):
        px = px[..., [2, 1, 0, 3]]
    elif fmt in (BGRX8, BGRX8_SRGB):
        px = px[..., [2, 1, 0]]
    return np.ascontiguousarray(px).reshape(height, width * F)


def writer_chunks(fmt, flags=0):
    """the tags in front of IDAT besides IHDR, with their bodies (departure 3)"""
    if WRITER[fmt][0] == 0:
        return []
    if flags & FLAGS_FORCE_LINEAR:
        return [(b"gAMA", struct.pack(">I", 100000))]
    if fmt in (RGBA8_SRGB, BGRA8_SRGB, BGRX8_SRGB) or flags & FLAGS_FORCE_SRGB:
        return [(b"sRGB", b"\x00")]
    return []
