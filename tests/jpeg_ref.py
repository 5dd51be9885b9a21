"""A numpy restatement of the JPEG reader (host/DirectXTexAMD_JPEG.cpp, csrc/dxtex_jpeg.h, csrc/jpeg.hip): the marker walk, Huffman and
progressive decode to quantised coefficients, and the pixel stage - dequantisation, libjpeg's JDCT_ISLOW inverse DCT, fancy upsampling,
YCbCr -> RGB. The reference's codec (Auxiliary/DirectXTexJPEG.cpp) calls libjpeg-turbo with its defaults; Pillow links the same library, and
where Pillow is installed tests/test_jpeg_cpu.py holds this file to it byte for byte. Everywhere else this file is the oracle.

Departures from the reference, as host/DirectXTexAMD.h states them:
  1. the Memory forms exist;
  2. HRESULT_E_NOT_SUPPORTED for arithmetic coding (SOF9 - SOF15), lossless and hierarchical frames (SOF3, SOF5 - SOF7), 12-bit precision,
     a DNL-defined height, sampling other than luma 1x1 / 2x1 / 2x2 over 1x1 chroma (grey with any factors is 1x1), and a progressive file
     whose scans do not bring every coefficient of every component to Al = 0;
  3. a truncated or corrupt entropy segment is E_FAIL where libjpeg pads with zeros and warns;
  4. EXIF orientation, thumbnails and ICC profiles are ignored, as libjpeg ignores them.

Also a small baseline writer (encode), so that tests can make files where Pillow is absent: one Huffman table per class in which every
symbol has a code of the same length. Its files are valid and differ from libjpeg's."""
import struct

import numpy as np

S_OK, E_FAIL, E_INVALIDARG, E_NOT_SUPPORTED, E_FILE_NOT_FOUND, E_POINTER = 0, 0x80004005, 0x80070057, 0x80070032, 0x80070002, 0x80004003
R8, RGBA8, RGBA8_SRGB = 61, 28, 29
ALPHA_MODE_OPAQUE = 3
FLAGS_NONE, FLAGS_DEFAULT_LINEAR = 0, 0x1
GREY, YCBCR, RGB = 0, 1, 2

NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


class Refused(Exception):
    def __init__(self, hr, why):
        super().__init__(why)
        self.hr = hr


def fail(why):
    raise Refused(E_FAIL, why)


def unsupported(why):
    raise Refused(E_NOT_SUPPORTED, why)


def ceil_div(a, b):
    return -(-a // b)


# ---- entropy segments ---------------------------------------------------------------------------------------------------------------------
class Bits:
    """the bits of one restart interval, stuffing removed; reading past the end is a defect"""
    def __init__(self, data):
        self.s = "".join(format(b, "08b") for b in data)
        self.at = 0

    def get(self, n):
        if n == 0:
            return 0
        if self.at + n > len(self.s):
            fail("the entropy segment ends early")
        v = int(self.s[self.at:self.at + n], 2)
        self.at += n
        return v


def split_scan(data, at):
    """the entropy-coded bytes from `at` -> ([bytes of each restart interval, unstuffed], the offset of the marker (or the end) behind
    them). RSTn must count up from 0."""
    parts, cur, expect = [], bytearray(), 0
    n = len(data)
    while at < n:
        b = data[at]
        if b != 0xFF:
            cur.append(b)
            at += 1
            continue
        k = at + 1
        while k < n and data[k] == 0xFF:
            k += 1
        if k >= n:
            at = n
            break
        m = data[k]
        if m == 0:
            cur.append(0xFF)
            at = k + 1
        elif 0xD0 <= m <= 0xD7:
            if m != 0xD0 + expect:
                parts.append(bytes(cur))
                return parts, at, "a wrong RSTn"
            expect = (expect + 1) & 7
            parts.append(bytes(cur))
            cur = bytearray()
            at = k + 1
        else:
            break
    parts.append(bytes(cur))
    return parts, at, None


class Huff:
    def __init__(self, counts, symbols):
        self.codes = {}
        code, k = 0, 0
        for length in range(1, 17):
            for _ in range(counts[length - 1]):
                if code >= (1 << length):
                    fail("an over-subscribed Huffman table")
                self.codes[(length, code)] = symbols[k]
                code += 1
                k += 1
            code <<= 1

    def decode(self, bits):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | bits.get(1)
            s = self.codes.get((length, code))
            if s is not None:
                return s
        fail("a bad Huffman code")


def extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def i16(v):
    return ((v + 0x8000) & 0xFFFF) - 0x8000


# ---- the marker walk ------------------------------------------------------------------------------------------------------------------------
def decode(data):
    """the file -> a dict: width, height, colour, progressive, comps [{id, h, v, tq, bw, bh (blocks, padded to whole MCUs), dw, dh, coef
    (bh, bw, 64) int16 in natural order}], quant [4] of 64 in natural order or None. Raises Refused with the HRESULT."""
    data = bytes(data)
    n = len(data)
    if n < 2 or data[0] != 0xFF or data[1] != 0xD8:
        fail("no SOI")
    at = 2
    quant, dc_tab, ac_tab = [None] * 4, [None] * 4, [None] * 4
    frame, jfif, adobe, restart = None, False, None, 0
    scans_seen = False
    while True:
        if at >= n:
            fail("no EOI")
        if data[at] != 0xFF:
            if not scans_seen:
                fail("not a marker")
            at += 1          # bytes between a scan's data and the next marker are skipped
            continue
        while at < n and data[at] == 0xFF:
            at += 1
        if at >= n:
            fail("no EOI")
        m = data[at]
        at += 1
        if m == 0 and scans_seen:
            continue
        if m == 0xD9:
            break
        if m == 0xD8 or m == 0 or 0xD0 <= m <= 0xD7 or m == 0x01:
            if m == 0x01:
                continue
            fail("a marker out of place")
        if at + 2 > n:
            fail("a segment length past the file")
        length = struct.unpack(">H", data[at:at + 2])[0]
        if length < 2 or at + length > n:
            fail("a segment length past the file")
        body = data[at + 2:at + length]
        at += length
        if m == 0xE0:
            if len(body) >= 5 and body[:5] == b"JFIF\0":
                jfif = True
        elif m == 0xEE:
            if len(body) >= 12 and body[:5] == b"Adobe":
                adobe = body[11]
        elif m == 0xDB:
            k = 0
            while k < len(body):
                pq, tq = body[k] >> 4, body[k] & 15
                k += 1
                if pq > 1 or tq > 3:
                    fail("a bad DQT")
                size = 128 if pq else 64
                if k + size > len(body):
                    fail("a short DQT")
                vals = np.frombuffer(body[k:k + size], ">u2" if pq else np.uint8).astype(np.uint16)
                k += size
                t = np.zeros(64, np.uint16)
                t[NATURAL] = vals
                quant[tq] = t
        elif m == 0xC4:
            k = 0
            while k < len(body):
                if k + 17 > len(body):
                    fail("a short DHT")
                tc, th = body[k] >> 4, body[k] & 15
                counts = list(body[k + 1:k + 17])
                k += 17
                total = sum(counts)
                if tc > 1 or th > 3 or total > 256 or k + total > len(body):
                    fail("a bad DHT")
                table = Huff(counts, list(body[k:k + total]))
                k += total
                (ac_tab if tc else dc_tab)[th] = table
        elif m == 0xDD:
            if len(body) != 2:
                fail("a bad DRI")
            restart = struct.unpack(">H", body)[0]
        elif m in (0xC0, 0xC1, 0xC2):
            if frame is not None:
                fail("two frames")
            frame = parse_frame(body, m == 0xC2)
        elif m in (0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            unsupported("arithmetic, lossless or hierarchical")
        elif m == 0xDA:
            if frame is None:
                fail("a scan in front of the frame")
            at = decode_scan(data, at, body, frame, dc_tab, ac_tab, restart)
            scans_seen = True
        elif m == 0xC8 or m == 0xDC:
            fail("a marker this reader does not take")
        # every other segment (APPn, COM, DAC, ...) is skipped
    if frame is None or not scans_seen:
        fail("no image")
    for c in frame["comps"]:
        if quant[c["tq"]] is None:
            fail("a missing quantisation table")
        if frame["progressive"]:
            if (c["bits"] != 0).any():
                unsupported("an incomplete progressive file")
        elif not c["seen"]:
            fail("a component without a scan")
    ids = [c["id"] for c in frame["comps"]]
    if len(ids) == 1:
        colour = GREY
    elif jfif:
        colour = YCBCR          # libjpeg asks for the JFIF marker first: with it, an Adobe marker's transform is not looked at
    elif adobe is not None:
        colour = RGB if adobe == 0 else YCBCR
    else:
        colour = RGB if ids == [ord("R"), ord("G"), ord("B")] else YCBCR
    return dict(width=frame["width"], height=frame["height"], colour=colour, progressive=frame["progressive"], comps=frame["comps"], quant=quant)


def parse_frame(body, progressive):
    if len(body) < 6:
        fail("a short SOF")
    precision, height, width, ncomp = struct.unpack(">BHHB", body[:6])
    if precision == 12:
        unsupported("12-bit")
    if precision != 8:
        fail("precision")
    if ncomp == 4:
        fail("four components")
    if ncomp not in (1, 3) or len(body) != 6 + 3 * ncomp:
        fail("a bad SOF")
    if width == 0:
        fail("width 0")
    if height == 0:
        unsupported("a DNL height")
    comps = []
    for i in range(ncomp):
        cid, hv, tq = body[6 + 3 * i:9 + 3 * i]
        h, v = hv >> 4, hv & 15
        if not (1 <= h <= 4 and 1 <= v <= 4) or tq > 3 or cid in [c["id"] for c in comps]:
            fail("a bad component")
        comps.append(dict(id=cid, h=h, v=v, tq=tq))
    if ncomp == 1:
        comps[0]["h"] = comps[0]["v"] = 1
    elif (comps[0]["h"], comps[0]["v"]) not in ((1, 1), (2, 1), (2, 2)) or any((c["h"], c["v"]) != (1, 1) for c in comps[1:]):
        unsupported("sampling")
    hmax, vmax = comps[0]["h"], comps[0]["v"]
    for c in comps:
        c["bw"] = ceil_div(width, 8 * hmax) * c["h"]
        c["bh"] = ceil_div(height, 8 * vmax) * c["v"]
        c["dw"] = ceil_div(width * c["h"], hmax)
        c["dh"] = ceil_div(height * c["v"], vmax)
        c["coef"] = np.zeros((c["bh"], c["bw"], 64), np.int16)
        c["bits"] = np.full(64, -1, np.int32)          # progressive: the Al each coefficient has reached
        c["seen"] = False
    return dict(width=width, height=height, progressive=progressive, comps=comps, hmax=hmax, vmax=vmax)


def decode_scan(data, at, body, frame, dc_tab, ac_tab, restart):
    if len(body) < 1:
        fail("a short SOS")
    ns = body[0]
    if ns < 1 or ns > len(frame["comps"]) or len(body) != 4 + 2 * ns:
        fail("a bad SOS")
    comps = []
    for i in range(ns):
        cid, t = body[1 + 2 * i], body[2 + 2 * i]
        c = next((c for c in frame["comps"] if c["id"] == cid), None)
        if c is None or any(c is o for o, _, _ in comps) or (t >> 4) > 3 or (t & 15) > 3:
            fail("a bad SOS component")
        comps.append((c, t >> 4, t & 15))
    ss, se, a = body[1 + 2 * ns:4 + 2 * ns]
    ah, al = a >> 4, a & 15
    prog = frame["progressive"]
    if prog:
        if ss > se or se > 63 or (ss == 0 and se != 0) or (ss > 0 and ns != 1) or ah > 13 or al > 13 or (ah and al != ah - 1):
            fail("a bad progressive scan")
        for c, _, _ in comps:
            cur = c["bits"][ss:se + 1]
            if ah == 0 and (cur >= 0).any() or ah and (cur != ah).any():
                fail("a scan out of its order")
            if ss > 0 and c["bits"][0] < 0:
                fail("an AC scan in front of the DC scan")
    else:
        ss, se, ah, al = 0, 63, 0, 0
    for c, td, ta in comps:
        if (not prog or (ss == 0 and ah == 0)) and dc_tab[td] is None:
            fail("a missing DC table")
        if (not prog or ss > 0) and ac_tab[ta] is None:
            fail("a missing AC table")
    # the blocks in the order the scan holds them
    if ns > 1:
        mw, mh = ceil_div(frame["width"], 8 * frame["hmax"]), ceil_div(frame["height"], 8 * frame["vmax"])
        if sum(c["h"] * c["v"] for c, _, _ in comps) > 10:
            fail("an MCU of more than ten blocks")
        units = [[(i, my * c["v"] + vv, mx * c["h"] + hh) for i, (c, _, _) in enumerate(comps) for vv in range(c["v"]) for hh in range(c["h"])]
                 for my in range(mh) for mx in range(mw)]
    else:
        c = comps[0][0]
        units = [[(0, by, bx)] for by in range(ceil_div(c["dh"], 8)) for bx in range(ceil_div(c["dw"], 8))]
    parts, end, why = split_scan(data, at)
    per = restart if restart else len(units)
    u = 0
    for p, part in enumerate(parts):
        if u >= len(units):
            break
        bits = Bits(part)
        pred = [0] * ns
        eobrun = 0
        for unit in units[u:u + per]:
            for i, by, bx in unit:
                c, td, ta = comps[i]
                blk = c["coef"][by, bx]
                if not prog:
                    pred[i] = baseline_block(bits, blk, dc_tab[td], ac_tab[ta], pred[i])
                elif ss == 0:
                    if ah == 0:
                        s = dc_tab[td].decode(bits)
                        if s > 15:
                            fail("a bad DC size")
                        pred[i] = (pred[i] + extend(bits.get(s), s)) & 0xFFFFFFFF
                        blk[0] = i16(pred[i] << al)
                    elif bits.get(1):
                        blk[0] = i16(int(blk[0]) | (1 << al))
                elif ah == 0:
                    eobrun = ac_first(bits, blk, ac_tab[ta], ss, se, al, eobrun)
                else:
                    eobrun = ac_refine(bits, blk, ac_tab[ta], ss, se, al, eobrun)
        u += per
        if u < len(units) and p == len(parts) - 1:
            fail(why or "the scan ends before its last MCU")
    if u < len(units):
        fail("the scan ends before its last MCU")
    for c, _, _ in comps:
        c["bits"][ss:se + 1] = al
        c["seen"] = True
    return end


def baseline_block(bits, blk, dc, ac, pred):
    s = dc.decode(bits)
    if s > 15:
        fail("a bad DC size")
    pred = (pred + extend(bits.get(s), s)) & 0xFFFFFFFF
    blk[:] = 0
    blk[0] = i16(pred)
    k = 1
    while k < 64:
        rs = ac.decode(bits)
        r, s = rs >> 4, rs & 15
        if s:
            k += r
            if k > 63:
                fail("a run past coefficient 63")
            blk[NATURAL[k]] = i16(extend(bits.get(s), s))
            k += 1
        elif r == 15:
            if k + 16 > 64:
                fail("a run past coefficient 63")
            k += 16
        else:
            break
    return pred


def ac_first(bits, blk, ac, ss, se, al, eobrun):
    if eobrun > 0:
        return eobrun - 1
    k = ss
    while k <= se:
        rs = ac.decode(bits)
        r, s = rs >> 4, rs & 15
        if s:
            k += r
            if k > se:
                fail("a run past the band")
            blk[NATURAL[k]] = i16(extend(bits.get(s), s) * (1 << al))
            k += 1
        elif r == 15:
            if k + 16 > se + 1:
                fail("a run past the band")
            k += 16
        else:
            return (1 << r) + bits.get(r) - 1
    return 0


def ac_refine(bits, blk, ac, ss, se, al, eobrun):
    p1, m1 = 1 << al, -(1 << al)

    def correct(k):
        v = int(blk[NATURAL[k]])
        if bits.get(1) and (v & p1) == 0:
            blk[NATURAL[k]] = i16(v + (p1 if v >= 0 else m1))

    k = ss
    if eobrun == 0:
        while k <= se:
            rs = ac.decode(bits)
            r, s = rs >> 4, rs & 15
            value = 0
            if s:
                if s != 1:
                    fail("a bad refinement code")
                value = p1 if bits.get(1) else m1
            elif r != 15:
                eobrun = (1 << r) + bits.get(r)
                break
            while k <= se:
                if blk[NATURAL[k]] != 0:
                    correct(k)
                else:
                    r -= 1
                    if r < 0:
                        break
                k += 1
            if value:
                if k > se:
                    fail("a run past the band")
                blk[NATURAL[k]] = value
            k += 1
    if eobrun > 0:
        while k <= se:
            if blk[NATURAL[k]] != 0:
                correct(k)
            k += 1
        eobrun -= 1
    return eobrun


# ---- the pixel stage ------------------------------------------------------------------------------------------------------------------------
def _u(a):
    return np.asarray(a).astype(np.int64).astype(np.uint32) if np.asarray(a).dtype != np.uint32 else np.asarray(a)


def _mul(a, k):
    return a * np.uint32(k & 0xFFFFFFFF)


def _sar(a, n):
    return (a.view(np.int32) >> n).view(np.uint32)


def _descale(a, n):
    return _sar(a + np.uint32(1 << (n - 1)), n)


def idct_pass(x, shift):
    """x: (..., 8) uint32 holding int32 values; one pass of jidctint.c, wrapping at 32 bits"""
    i = [x[..., k] for k in range(8)]
    z1 = _mul(i[2] + i[6], 4433)
    t2 = z1 - _mul(i[6], 15137)
    t3 = z1 + _mul(i[2], 6270)
    t0 = (i[0] + i[4]) << np.uint32(13)
    t1 = (i[0] - i[4]) << np.uint32(13)
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
    z5 = _mul(z3 + z4, 9633)
    o0, o1, o2, o3 = _mul(o0, 2446), _mul(o1, 16819), _mul(o2, 25172), _mul(o3, 12299)
    z1, z2 = _mul(z1, -7373), _mul(z2, -20995)
    z3, z4 = _mul(z3, -16069) + z5, _mul(z4, -3196) + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = [t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3]
    return np.stack([_descale(v, shift) for v in out], axis=-1)


def idct(coef, quant):
    """coef (..., 64) int16 and quant (64,) uint16, natural order -> (..., 8, 8) uint8 samples"""
    with np.errstate(over="ignore"):
        x = _u(coef) * quant.astype(np.uint32)
        x = x.reshape(x.shape[:-1] + (8, 8))
        ws = np.swapaxes(idct_pass(np.swapaxes(x, -1, -2), 11), -1, -2)          # down each column
        o = idct_pass(ws, 18)                                                    # along each row
        w = ((o + np.uint32(512)) & np.uint32(1023)).astype(np.int64) - 512 + 128
    return np.clip(w, 0, 255).astype(np.uint8)


def plane_of(c, quant):
    """a component's block-padded samples (bh * 8, bw * 8)"""
    s = idct(c["coef"], quant)
    return s.transpose(0, 2, 1, 3).reshape(c["bh"] * 8, c["bw"] * 8)


def upsample(plane, dw, dh, hs, vs):
    """the component's dw x dh samples -> (dh * vs, dw * hs), jdsample.c with fancy upsampling"""
    p = plane[:dh, :dw].astype(np.int64)
    if hs == 1:
        return p
    if dw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), 2, axis=1)
    if vs == 1:
        out = np.zeros((dh, dw * 2), np.int64)
        prev = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
        nxt = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
        out[:, 0::2] = (3 * p + prev + 1) >> 2
        out[:, 1::2] = (3 * p + nxt + 2) >> 2
        out[:, 0] = p[:, 0]
        out[:, -1] = p[:, -1]
        return out
    out = np.zeros((dh * 2, dw * 2), np.int64)
    above = np.concatenate([p[:1], p[:-1]], axis=0)
    below = np.concatenate([p[1:], p[-1:]], axis=0)
    for v, nb in ((0, above), (1, below)):
        s = 3 * p + nb
        prev = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        nxt = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        rows = np.zeros((dh, dw * 2), np.int64)
        rows[:, 0::2] = (3 * s + prev + 8) >> 4
        rows[:, 1::2] = (3 * s + nxt + 7) >> 4
        rows[:, 0] = (4 * s[:, 0] + 8) >> 4
        rows[:, -1] = (4 * s[:, -1] + 7) >> 4
        out[v::2] = rows
    return out


def colour_texels(kind, a, b, c):
    """three (h, w) int64 sample planes -> (h, w, 4) uint8, jdcolor.c"""
    if kind == YCBCR:
        cb, cr = b - 128, c - 128
        r = a + ((91881 * cr + 32768) >> 16)
        g = a + ((-22554 * cb - 46802 * cr + 32768) >> 16)
        bl = a + ((116130 * cb + 32768) >> 16)
    else:
        r, g, bl = a, b, c
    out = np.full(a.shape + (4,), 255, np.uint8)
    for i, v in enumerate((r, g, bl)):
        out[..., i] = np.clip(v, 0, 255)
    return out


def pixels_from(width, height, colour, comps, quant):
    """comps: dicts with h, v, tq, bw, bh, dw, dh, coef -> tight pixels (height, width * texel bytes) uint8"""
    planes = [plane_of(c, quant[c["tq"]]) for c in comps]
    if colour == GREY:
        return planes[0][:height, :width].copy()
    hmax, vmax = comps[0]["h"], comps[0]["v"]
    up = [upsample(p, c["dw"], c["dh"], hmax // c["h"], vmax // c["v"])[:height, :width] for p, c in zip(planes, comps)]
    return colour_texels(colour, *up).reshape(height, width * 4)


def pixels(info):
    return pixels_from(info["width"], info["height"], info["colour"], info["comps"], info["quant"])


def metadata(info, flags=0):
    """(format, miscFlags2) as TranslateColor / GetMetadata give them"""
    if info["colour"] == GREY:
        return R8, 0
    return (RGBA8 if flags & FLAGS_DEFAULT_LINEAR else RGBA8_SRGB), ALPHA_MODE_OPAQUE


def coefficients(info):
    """the upload: every component's blocks in raster order, one component after another, int16"""
    return np.concatenate([c["coef"].reshape(-1) for c in info["comps"]])


# ---- a small baseline writer ----------------------------------------------------------------------------------------------------------------
_DCT = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])
_LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
AC_SYMBOLS = [0x00, 0xF0] + [(r << 4) | s for r in range(16) for s in range(1, 11)]          # 162 symbols, each with an 8-bit code
DC_SYMBOLS = list(range(12))                                                                  # each with a 4-bit code


def segment(marker, body=b""):
    return bytes([0xFF, marker]) + struct.pack(">H", len(body) + 2) + body


class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, v, n):
        self.acc = (self.acc << n) | (v & ((1 << n) - 1))
        self.n += n
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def size_of(v):
    return int(abs(v)).bit_length()


def put_value(w, v, s):
    w.put(v if v >= 0 else v + (1 << s) - 1, s)


def encode(img, sampling=(1, 1), quality_scale=1.0, restart=0, jfif=True, adobe=None, ids=None):
    """a baseline file of `img`: (h, w) uint8 for grey or (h, w, 3) for colour, whose three channels are stored as they are (the caller
    says what they mean through jfif / adobe / ids). sampling = luma (h, v) over 1 x 1 chroma; chroma is box-averaged."""
    img = np.asarray(img)
    grey = img.ndim == 2
    height, width = img.shape[:2]
    hmax, vmax = (1, 1) if grey else sampling
    q = np.clip(np.round(_LUMA_Q * quality_scale), 1, 255).astype(np.uint16)
    planes = [img.astype(np.float64)] if grey else [img[..., i].astype(np.float64) for i in range(3)]
    factors = [(1, 1)] if grey else [(hmax, vmax), (1, 1), (1, 1)]
    mw, mh = ceil_div(width, 8 * hmax), ceil_div(height, 8 * vmax)
    coefs = []
    for p, (h, v) in zip(planes, factors):
        full = np.pad(p, ((0, mh * 8 * vmax - height), (0, mw * 8 * hmax - width)), mode="edge")
        sx, sy = hmax // h, vmax // v
        small = full.reshape(mh * 8 * v, sy, mw * 8 * h, sx).mean(axis=(1, 3))
        blocks = small.reshape(mh * v, 8, mw * h, 8).transpose(0, 2, 1, 3) - 128.0
        c = np.einsum("ux,abxy,vy->abuv", _DCT, blocks, _DCT).reshape(mh * v, mw * h, 64)
        coefs.append(np.clip(np.round(c / q), -1023, 1023).astype(np.int64))
    ids = ids or ([1] if grey else [1, 2, 3])
    out = bytearray(b"\xFF\xD8")
    if jfif:
        out += segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if adobe is not None:
        out += segment(0xEE, b"Adobe\0\x64\0\0\0\0" + bytes([adobe]))
    zz = np.zeros(64, np.uint8)
    zz[:] = q[NATURAL]
    out += segment(0xDB, b"\x00" + zz.tobytes())
    out += segment(0xC0, struct.pack(">BHHB", 8, height, width, len(ids)) + b"".join(bytes([i, (h << 4) | v, 0]) for i, (h, v) in zip(ids, factors)))
    out += segment(0xC4, b"\x00" + bytes([0, 0, 0, 12] + [0] * 12) + bytes(DC_SYMBOLS))
    out += segment(0xC4, b"\x10" + bytes([0] * 7 + [162] + [0] * 8) + bytes(AC_SYMBOLS))
    if restart:
        out += segment(0xDD, struct.pack(">H", restart))
    out += segment(0xDA, bytes([len(ids)]) + b"".join(bytes([i, 0]) for i in ids) + b"\x00\x3F\x00")
    ac_code = {s: k for k, s in enumerate(AC_SYMBOLS)}
    w = BitWriter()
    pred = [0] * len(ids)
    count = 0
    for my in range(mh):
        for mx in range(mw):
            if restart and count and count % restart == 0:
                w.flush()
                out += w.out + bytes([0xFF, 0xD0 + ((count // restart - 1) & 7)])
                w = BitWriter()
                pred = [0] * len(ids)
            count += 1
            for i, (h, v) in enumerate(factors):
                for vv in range(v):
                    for hh in range(h):
                        blk = coefs[i][my * v + vv, mx * h + hh][NATURAL]
                        d = int(blk[0]) - pred[i]
                        pred[i] = int(blk[0])
                        s = size_of(d)
                        w.put(s, 4)
                        put_value(w, d, s)
                        run = 0
                        last = max([k for k in range(1, 64) if blk[k]], default=0)
                        for k in range(1, last + 1):
                            if blk[k] == 0:
                                run += 1
                                continue
                            while run > 15:
                                w.put(ac_code[0xF0], 8)
                                run -= 16
                            s = size_of(int(blk[k]))
                            w.put(ac_code[(run << 4) | s], 8)
                            put_value(w, int(blk[k]), s)
                            run = 0
                        if last < 63:
                            w.put(ac_code[0x00], 8)
    w.flush()
    out += w.out + b"\xFF\xD9"
    return bytes(out)
