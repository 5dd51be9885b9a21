"""FlipRotate restated in numpy: what every FlipRotate test of this suite compares against.

THE RULE (this project's): the source turned CLOCKWISE by the angle, then mirrored left-right if FLIP_HORIZONTAL is set, then mirrored
top-bottom if FLIP_VERTICAL is set. A flip or a quarter turn is a permutation of texels, so these lines are its whole definition.

STATED DEPARTURE: the reference hands the flag word to WIC, whose documentation does not say whether a flip combined with a rotation is
applied before or after it. Its tools never combine them (texconv passes flips only, texassemble ROTATE180 only), so nothing they produce
depends on the order, and nothing here can check it. The library keeps the order in one function (fr_resolve, dxtex_fliprotate.h).
Two more: the reference converts formats WIC lacks through float and back (not the identity for, say, R32_UINT above 2^24) - here bits
are kept - and it would convert the two-texel packed formats, which are refused here."""
import numpy as np

ROTATE0, ROTATE90, ROTATE180, ROTATE270, FLIP_HORIZONTAL, FLIP_VERTICAL = 0, 1, 2, 3, 0x08, 0x10
LEGAL = tuple(f for f in range(1, 0x20) if (f & ~0x1B) == 0)            # fifteen values
ILLEGAL = (0, 4, 0x20, 0x1F)
# the eight symmetries of the rectangle, as pairs of flag words with the same result
CLASSES = ({2, 24}, {1, 27}, {3, 25}, {8, 18}, {16, 10}, {9, 19}, {11, 17}, {26})

S_OK, E_POINTER, E_INVALIDARG, E_FAIL, E_NOT_SUPPORTED = 0, -2147467261, -2147024809, -2147467259, -2147024846


def legal(flags):
    return flags != 0 and (flags & ~0x1B) == 0


def transposes(flags):
    return bool(flags & 1)


def flip_rotate(src, flags):
    """src: [h, w, ...] -> the result, [w, h, ...] for 90 / 270."""
    assert legal(flags)
    out = np.rot90(src, k=-(flags & 3))
    if flags & FLIP_HORIZONTAL:
        out = out[:, ::-1]
    if flags & FLIP_VERTICAL:
        out = out[::-1]
    return np.ascontiguousarray(out)


def source_coords(w, h, flags):
    """[H, W, 2]: the (x, y) of the source texel of every texel of the result, by pushing a coordinate image through flip_rotate."""
    ys, xs = np.mgrid[0:h, 0:w]
    return flip_rotate(np.stack([xs, ys], axis=-1), flags)


def texels(buf, w, h, texel_bytes, pitch):
    """The [h, w, texel_bytes] texels of a byte buffer with rows `pitch` apart (the last row may end with its texels)."""
    buf = np.asarray(buf, np.uint8).reshape(-1)
    rows = np.stack([buf[y * pitch:y * pitch + w * texel_bytes] for y in range(h)]) if h else np.zeros((0, w * texel_bytes), np.uint8)
    return rows.reshape(h, w, texel_bytes)


def expected(start, dst_pitch, src, w, h, texel_bytes, src_pitch, flags, at=0):
    """What a destination buffer that starts as `start` must hold afterwards: the result's texels in rows `dst_pitch` apart from byte
    `at`, every other byte - row padding, what lies outside a cell - as it was."""
    res = flip_rotate(texels(src, w, h, texel_bytes, src_pitch), flags)
    out = np.array(start, np.uint8).reshape(-1).copy()
    for y in range(res.shape[0]):
        row = res[y].reshape(-1)
        out[at + y * dst_pitch:at + y * dst_pitch + row.size] = row
    return out
