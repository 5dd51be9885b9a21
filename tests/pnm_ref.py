"""The portable pixmap codec of the reference's texconv (Texconv/PortablePixMap.cpp) restated in Python / numpy, on bytes in memory. The
reference's file is Win32 code (CreateFile2, sscanf_s) that the test oracle cannot compile, so this restatement - written from the
reference's rules, with its line numbers - is the yardstick for the reader, the refusals and the file layout of tests/test_pnm_*.py, as
rotate_ref.py and diag_ref.py are for texconv and texdiag code. Nothing here is shared with the code under test.

    load(data)            -> (hresult, None | dict(width, height, format, kind, maxval, big_endian, ascii, offset, nbytes, pixels))
    unpack(...)           -> the image's tight rows from the samples behind the header (the reader's texel loops)
    save_ppm / save_pfm   -> the file the writers emit (or an hresult)
"""
import re

import numpy as np

S_OK = 0
E_FAIL = 0x80004005
E_UNEXPECTED = 0x8000FFFF
E_INVALIDARG = 0x80070057
E_NOT_SUPPORTED = 0x80070032          # HRESULT_FROM_WIN32(ERROR_NOT_SUPPORTED)
E_ARITHMETIC_OVERFLOW = 0x80070216    # HRESULT_FROM_WIN32(ERROR_ARITHMETIC_OVERFLOW)
E_HANDLE_EOF = 0x80070026             # HRESULT_FROM_WIN32(ERROR_HANDLE_EOF)
INT32_MAX, UINT32_MAX = 2 ** 31 - 1, 2 ** 32 - 1

RGBA32F, RGB32F, RGBA16F, R32F, R16F, RGBA8, RGBA8_SRGB, BGRA8, BGRX8, BGRA8_SRGB, BGRX8_SRGB = 2, 6, 10, 41, 54, 28, 29, 87, 88, 91, 93
P6, PF, Pf, PH, Ph = range(5)          # DXTEX_PNM_*
FILE_BYTES = {P6: 3, PF: 12, Pf: 4, PH: 6, Ph: 2}
IMAGE_BYTES = {P6: 4, PF: 16, Pf: 4, PH: 8, Ph: 2}
KIND_FORMAT = {P6: RGBA8, PF: RGBA32F, Pf: R32F, PH: RGBA16F, Ph: R16F}

SPACE = b" \t\n\v\f\r"          # C isspace


def _ppm(data):
    """LoadFromPortablePixMap, :152-358"""
    ascii_ = data[1:2] == b"3"
    pos, n = 2, len(data)          # :178
    mode = 0                       # width, height, max, r, g, b
    width = height = 0
    maxval = 255
    words = None
    filled = 0
    while pos < n:
        if not ascii_ and mode == 3:          # :188-226
            if maxval > 255:
                return E_UNEXPECTED, None
            if n - pos > 1 and data[pos] == 0x0D:
                pos += 1
            if data[pos] != 0x0A:
                return E_FAIL, None
            if n - pos > 1:
                pos += 1
            start = pos
            texels = 0
            while pos < n and texels < width * height:
                if n - pos < 3:
                    return E_HANDLE_EOF, None
                texels += 1
                pos += 3
            if texels != width * height:
                return E_FAIL, None
            return S_OK, dict(width=width, height=height, format=RGBA8, kind=P6, maxval=maxval, big_endian=False, ascii=False, offset=start, nbytes=texels * 3)
        c = data[pos]
        if c in SPACE:
            pos += 1
        elif c == 0x23:          # '#', :234-248
            while pos < n and data[pos] != 0x0A:
                pos += 1
            if pos < n:
                pos += 1
        else:
            u = 0
            while pos < n and data[pos] not in SPACE:          # :252-263
                if not 0x30 <= data[pos] <= 0x39:
                    return E_FAIL, None
                u = (u * 10 + data[pos] - 0x30) & UINT32_MAX
                pos += 1
            if mode == 0:
                if u == 0:
                    return E_FAIL, None
                if u > INT32_MAX:
                    return E_NOT_SUPPORTED, None
                width = u
            elif mode == 1:
                if u == 0:
                    return E_FAIL, None
                if u > INT32_MAX:
                    return E_NOT_SUPPORTED, None
                if width * u * 4 > UINT32_MAX:
                    return E_ARITHMETIC_OVERFLOW, None
                height = u
                if ascii_:
                    if width * height > len(data):          # no file this short fills the image: what follows can only end in :357
                        return E_FAIL, None
                    words = np.zeros(width * height, np.uint32)
            elif mode == 2:
                if u == 0:
                    return E_FAIL, None
                maxval = u
            elif mode == 3:
                words[filled] = (((u * 255) & UINT32_MAX) // maxval) | 0xFF000000          # :327
            elif mode == 4:
                words[filled] |= ((((u * 255) & UINT32_MAX) // maxval) << 8) & UINT32_MAX          # :334
            else:
                words[filled] |= ((((u * 255) & UINT32_MAX) // maxval) << 16) & UINT32_MAX          # :341
                filled += 1
                if filled == width * height:
                    return S_OK, dict(width=width, height=height, format=RGBA8, kind=P6, maxval=255, big_endian=False, ascii=True, offset=0, nbytes=0,
                                      pixels=words.view(np.uint8).copy())
                mode = 2
            mode += 1
    return E_FAIL, None


def _scan_ulong(s, i):
    """%zu of sscanf: white space, an optional sign, decimal digits; the value as strtoul gives it. (value, next) or None."""
    while i < len(s) and s[i] in SPACE:
        i += 1
    m = re.compile(rb"([+-]?)([0-9]+)").match(s, i)
    if not m:
        return None
    v = int(m.group(2))
    if v >= 2 ** 64:
        v = 2 ** 64 - 1
    elif m.group(1) == b"-":
        v = (-v) % 2 ** 64
    return v, m.end()


# The C library's scanf takes an exponent letter and its sign even where no digit follows ("1e", "1e+": the value is 1), which strtod
# would leave unread; the host layer calls sscanf, so that is the rule here. A hexadecimal float with no digit at all ("0x.", which the
# library reads as 0) is outside this pattern; the tests build no such line.
_FLOAT = re.compile(rb"[+-]?(?:(nan)|(inf(?:inity)?)|(0x(?:[0-9a-f]+\.?[0-9a-f]*|\.[0-9a-f]+)(?:p[+-]?[0-9]*)?)|((?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:e[+-]?[0-9]*)?))", re.I)


def _scan_float(s, i):
    """%f of sscanf: (True where the value is >= 0 as a float, next) or None"""
    while i < len(s) and s[i] in SPACE:
        i += 1
    m = _FLOAT.match(s, i)
    if not m:
        return None
    text = re.sub(r"[pP][+-]?$" if m.group(3) else r"[eE][+-]?$", "", m.group(0).decode("ascii"))
    if m.group(1):
        return False, m.end()          # a NaN is not >= 0
    if m.group(3):
        sign = -1.0 if text.startswith("-") else 1.0
        value = sign * float.fromhex(text.lstrip("+-"))
    else:
        value = float(text)
    with np.errstate(over="ignore"):
        return bool(np.float32(value) >= 0), m.end()


def _no_junk(s, i):
    """the trailing %s converts nothing"""
    return not s[i:].strip(SPACE)


def _find_eol(data, pos, limit):
    """FindEOL, :72-85: 0 for no '\\n' within `limit` bytes - or for one at position 0"""
    at = data.find(b"\n", pos, pos + limit)
    return 0 if at < 0 else at - pos


def _next_line(data, pos):
    """:488-507, :537-556: (hresult, pos, len) of the next line that is no comment"""
    n = len(data)
    length = 0
    while pos < n:
        length = _find_eol(data, pos, min(256, n - pos))
        if not length:
            return E_FAIL, pos, 0
        if data[pos] != 0x23:
            break
        pos += length + 1
        if pos == n:
            return E_FAIL, pos, 0
    return S_OK, pos, length


def _pfm(data):
    """LoadFromPortablePixMapHDR, :452-684"""
    kinds = {0x66: Pf, 0x46: PF, 0x68: Ph, 0x48: PH}
    if data[1] not in kinds:
        return E_FAIL, None
    kind = kinds[data[1]]
    pos, n = 3, len(data)
    if pos == n:
        return E_FAIL, None
    hr, pos, length = _next_line(data, pos)
    if hr:
        return hr, None
    if length >= 255:          # strncpy_s of 256 bytes into dataStr[256]: the reference overruns; E_FAIL here
        return E_FAIL, None
    line = data[pos:pos + length + 1].split(b"\0")[0]
    a = _scan_ulong(line, 0)          # "%zu %zu%s" == 2, :514
    b = _scan_ulong(line, a[1]) if a else None
    if not a or not b or not _no_junk(line, b[1]):
        return E_FAIL, None
    width, height = a[0], b[0]
    if width > INT32_MAX or height > INT32_MAX:
        return E_NOT_SUPPORTED, None
    if width * height * IMAGE_BYTES[kind] > UINT32_MAX:
        return E_ARITHMETIC_OVERFLOW, None
    pos += length + 1
    if pos == n:
        return E_FAIL, None
    hr, pos, length = _next_line(data, pos)
    if hr:
        return hr, None
    if length >= 255:
        return E_FAIL, None
    line = data[pos:pos + length + 1].split(b"\0")[0]
    f = _scan_float(line, 0)          # "%f%s" == 1, :561
    if not f or not _no_junk(line, f[1]):
        return E_FAIL, None
    big_endian = f[0]          # :564
    pos += length + 1
    if pos == n:
        return E_FAIL, None
    need = width * FILE_BYTES[kind] * height
    if n - pos < need:
        return E_HANDLE_EOF, None          # :575-577
    if width == 0 or height == 0:
        return E_INVALIDARG, None          # ScratchImage::Initialize2D, DirectXTexImage.cpp:300-303
    return S_OK, dict(width=width, height=height, format=KIND_FORMAT[kind], kind=kind, maxval=255, big_endian=big_endian, ascii=False, offset=pos, nbytes=need)


def unpack(samples, kind, width, height, maxval=255, big_endian=False):
    """The reader's texel loops (:209-223, :595-681): the samples -> the image's tight rows, as uint8"""
    samples = np.frombuffer(bytes(samples), np.uint8)[:width * height * FILE_BYTES[kind]]
    if kind == P6:
        c = (255 * samples.astype(np.uint32)) // np.uint32(maxval)          # no clamp
        c = c.reshape(height, width, 3)
        words = c[..., 0] | (c[..., 1] << 8) | (c[..., 2] << 16) | np.uint32(0xFF000000)
        return words.astype("<u4").view(np.uint8).reshape(-1).copy()
    dt = np.dtype(">u4" if big_endian else "<u4") if kind in (PF, Pf) else np.dtype(">u2" if big_endian else "<u2")
    native = np.dtype("<u4") if kind in (PF, Pf) else np.dtype("<u2")
    e = samples.view(dt).astype(native)
    if kind in (Pf, Ph):
        img = e.reshape(height, width)[::-1]
    else:
        img = np.empty((height, width, 4), native)
        img[..., :3] = e.reshape(height, width, 3)[::-1]
        img[..., 3] = 0x3F800000 if kind == PF else 0x3C00
    return np.ascontiguousarray(img).view(np.uint8).reshape(-1).copy()


def load(data):
    """Either reader, told apart by the second byte as texconv tells them apart by extension."""
    data = bytes(data)
    if len(data) < 3 or data[0] != 0x50 or data[2] not in SPACE:          # :163-167, :463-467
        return E_FAIL, None
    hr, r = _ppm(data) if data[1] in b"36" else _pfm(data)
    if hr:
        return hr, None
    if not r["ascii"]:
        r["pixels"] = unpack(data[r["offset"]:r["offset"] + r["nbytes"]], r["kind"], r["width"], r["height"], r["maxval"], r["big_endian"])
    return S_OK, r


def save_ppm(pixels, fmt):
    """SaveToPortablePixMap, :361-443. pixels: (height, width, 4) uint8."""
    if fmt not in (RGBA8, RGBA8_SRGB, BGRA8, BGRX8, BGRA8_SRGB, BGRX8_SRGB):
        return E_NOT_SUPPORTED
    h, w = pixels.shape[:2]
    rgb = pixels[..., :3] if fmt in (RGBA8, RGBA8_SRGB) else pixels[..., 2::-1]          # Convert to R8G8B8A8: B and R trade places (:399-401)
    return b"P6\n%d %d\n255\n" % (w, h) + np.ascontiguousarray(rgb).tobytes()


def save_pfm(pixels, fmt, widen=None):
    """SaveToPortablePixMapHDR, :688-758. pixels: (height, width, channels) of uint32 / uint16 bit patterns. widen(halves) -> float bits:
    the reference's Convert to R32G32B32_FLOAT (:727), which the caller takes from the oracle."""
    if fmt not in (RGBA32F, RGB32F, RGBA16F, R32F):
        return E_NOT_SUPPORTED
    h, w = pixels.shape[:2]
    rgb = pixels if fmt == R32F else pixels[..., :3]
    if fmt == RGBA16F:
        rgb = widen(np.ascontiguousarray(rgb))
    flipped = np.ascontiguousarray(rgb[::-1]).astype("<u4")          # FlipRotate(TEX_FR_FLIP_VERTICAL), :733
    return b"P%c\n%d %d\n-1.000000\n" % (b"f" if fmt == R32F else b"F", w, h) + flipped.tobytes()
