"""Helpers of the Radiance RGBE tests (test_rgbe_cpu.py, test_rgbe_gpu.py, test_rgbe_host_gpu.py, test_rgbe_tools_gpu.py): .hdr files built
from raw shared-exponent texels, the reverse for files the reference's writer made, and the inputs both sides of the tests share. Every
expectation the tests hold comes from the oracle (oracle.ref_load_hdr / oracle.ref_save_hdr); nothing here restates the arithmetic."""
import numpy as np

RGBA32F, RGB32F, RGBA16F, RGBE = 2, 6, 10, 30
BPT = {RGBA32F: 16, RGB32F: 12, RGBA16F: 8}
EXPOSURES = (None, "0.5", "3.7", "1e-12")


def hdr_file(rgbe, exposure=None):
    """An .hdr file of raw scanlines holding the (h, w, 4) uint8 texels `rgbe`, with an EXPOSURE= line where `exposure` (a string) is given.
    The caller keeps the texels clear of the run-length markers: no row starts with (2, 2, < 128) and no texel is (1, 1, 1, .)."""
    rgbe = np.ascontiguousarray(rgbe, np.uint8)
    h, w = rgbe.shape[:2]
    assert rgbe.shape == (h, w, 4)
    assert not ((rgbe[:, 0, 0] == 2) & (rgbe[:, 0, 1] == 2) & (rgbe[:, 0, 2] < 128)).any()
    assert not ((rgbe[..., 0] == 1) & (rgbe[..., 1] == 1) & (rgbe[..., 2] == 1)).any()
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n" + (f"EXPOSURE={exposure}\n".encode() if exposure is not None else b"")
    return head + f"\n-Y {h} +X {w}\n".encode() + rgbe.tobytes()


def exhaustive_rgbe():
    """256 x 256: texel (m, e) - column m of row e - holds (m, 255 - m, (7 * m) & 255, e): every mantissa byte with every exponent byte.
    Green at 255 - m keeps every row and texel clear of the run-length markers."""
    m = np.arange(256, dtype=np.uint32)
    row = np.stack([m, 255 - m, (7 * m) & 255, np.zeros(256, np.uint32)], axis=1)
    img = np.broadcast_to(row[None], (256, 256, 4)).copy()
    img[..., 3] = np.arange(256)[:, None]
    return img.astype(np.uint8)


def random_rgbe(rng, w, h):
    """(h, w, 4) random texels under the same green rule: red and the exponent are random, green = 255 - red."""
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 1] = 255 - img[..., 0]
    return img


def unrle(data):
    """(width, height, (h, w, 4) uint8 texels) of a file oracle.ref_save_hdr wrote: its header, then rows that are run-length coded in the
    new scheme (2, 2, width hi, width lo, then each channel as runs and literals) or raw."""
    data = bytes(data)
    head = b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y "
    assert data.startswith(head)
    end = data.index(b"\n", len(head))
    hs, xs, ws = data[len(head):end].split()
    assert xs == b"+X"
    h, w = int(hs), int(ws)
    at = end + 1
    out = np.zeros((h, w, 4), np.uint8)
    for y in range(h):
        if 8 <= w <= 32767 and data[at] == 2 and data[at + 1] == 2 and data[at + 2] < 128:
            assert (data[at + 2] << 8) + data[at + 3] == w
            at += 4
            for c in range(4):
                x = 0
                while x < w:
                    n = data[at]
                    if n > 128:
                        n &= 127
                        out[y, x:x + n, c] = data[at + 1]
                        at += 2
                    else:
                        assert n > 0
                        out[y, x:x + n, c] = np.frombuffer(data, np.uint8, n, at + 1)
                        at += n + 1
                    x += n
                assert x == w
        else:
            out[y] = np.frombuffer(data, np.uint8, w * 4, at).reshape(w, 4)
            at += w * 4
    assert at == len(data)
    return w, h, out


def _f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def special_texels():
    """(n, 4) float32: the fixed list of texels at the encoder's edges. No channel is +Inf (that rule is this project's own and is checked
    apart); alpha is never read."""
    lim = np.float32(1e-32)
    up, down = np.nextafter(lim, np.float32(1)), np.nextafter(lim, np.float32(0))
    nan, fmax = np.float32(np.nan), np.finfo(np.float32).max
    t = [(0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-1.0, 0.5, -2.0), (-1.0, -1.0, -1.0), (-0.0, 1.0, 0.0),
         (nan, 1.0, 2.0), (nan, nan, nan), (1.0, nan, 0.25), (-nan, 0.5, 0.5),
         (lim, 0.0, 0.0), (up, 0.0, 0.0), (down, down, down), (up, lim, down), (0.0, up, up),
         (1e-40, 0.0, 0.0), (1.4e-45, 1.4e-45, 1.4e-45), (1e-40, 1.0, 0.0), (1e-38, 1e-40, 1e-39),
         (2.0 ** -24, 0.0, 0.0), (1023 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -14), (2.0 ** -14, 2.0 ** -24, 0.0),
         (fmax, 1.0, 0.0), (fmax, fmax, fmax), (fmax, fmax / 2, fmax / 256), (65504.0, 1.0, 65504.0 / 3),
         (0.7, 0.7, 0.1), (3.0, 1.0, 3.0), (0.2, 5.0, 5.0), (9.0, 9.0, 9.0)]
    rows = [np.array(v + (1.0,), np.float32) for v in t]
    base = _f32([0x3F7FFFFF])[0]
    for k in range(-100, 121, 20):
        v = np.ldexp(base, k).astype(np.float32)
        rows.append(np.array([v, v / np.float32(3), v / np.float32(300), 0.5], np.float32))
        rows.append(np.array([v / np.float32(2), v, v, 0.5], np.float32))
    return np.stack(rows).astype(np.float32)


def special_halves():
    """(n, 4) float16 texels only the half format can hold exactly as listed: its denormals, its largest value, NaN payloads, -0."""
    bits = [(0x0001, 0x0000, 0x0000), (0x03FF, 0x0001, 0x0200), (0x0400, 0x03FF, 0x0001), (0x7BFF, 0x3C00, 0x0001), (0x7BFF, 0x7BFF, 0x7BFF),
            (0x7E00, 0x3C00, 0x4000), (0xFE01, 0x7C01, 0x3800), (0x8000, 0x8001, 0xBC00), (0x3555, 0x3555, 0x2E66)]
    return np.array([b + (0x3C00,) for b in bits], np.uint16).view(np.float16)


def as_format(img, fmt):
    """(h, w, 4) float32 -> the array of `fmt` the codec tests feed: halves are clipped to the range that stays finite, as test_hdr_tga_cpu does."""
    if fmt == RGBA32F:
        return np.ascontiguousarray(img, np.float32)
    if fmt == RGB32F:
        return np.ascontiguousarray(img[..., :3], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.clip(img, -60000, 60000).astype(np.float16)


def tile(texels, w, h):
    """(h, w, C) image that repeats the (n, C) texels in order."""
    idx = np.arange(w * h) % texels.shape[0]
    return np.ascontiguousarray(texels[idx].reshape(h, w, texels.shape[1]))


def padded(px, w, h, fmt, row_pitch):
    """The tight image `px` of `fmt` as bytes with rows `row_pitch` apart; the padding holds 0xA5."""
    tight = w * BPT[fmt]
    out = np.full((h, row_pitch), 0xA5, np.uint8)
    out[:, :tight] = np.ascontiguousarray(px).view(np.uint8).reshape(h, tight)
    return out.reshape(-1)


def ref_rgbe_rows(oracle, px, w, h, fmt):
    """The reference writer's texels for the tight image `px`: oracle.ref_save_hdr with its run-length coding undone -> (h, w, 4) uint8."""
    hr, data = oracle.ref_save_hdr(px, w, h, fmt, w * BPT[fmt])
    assert hr == 0
    rw, rh, rows = unrle(data)
    assert (rw, rh) == (w, h)
    return rows
