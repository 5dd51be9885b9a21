"""BC7 test corpus: 4x4 tiles on which every mode of the encoder wins blocks, with every partition of the two- and three-subset modes, every rotation
of modes 4 and 5 and both index selectors of mode 4 - and tiles some mode represents with zero error, and float sources off the 1/255 grid.

numpy only, deterministic (fixed seeds), no GPU and no oracle; the only file read is tests/golden/bc7_partition_masks.npz, the region masks recorded
from the reference DECODER (tests/golden/make_golden_bc7_corpus.py: record_masks). Every family but `off_grid` returns (n, 16, 4) uint8 tiles, texel
i = 4 * y + x; unit() is the float32 form every consumer shares (byte * (1 / 255), what LoadScanline makes of an RGBA8 texel). What the reference
encoder does with the tiles - which modes, partitions and rotations win - is measured by tests/test_bc7_corpus_cpu.py; the expected payloads live in
tests/golden/bc7_corpus_*.npz."""
import os

import numpy as np

TILES_PER_ROW = 64
MASKS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bc7_partition_masks.npz")

_X = ((np.arange(16) % 4).astype(np.float64) - 1.5) / 1.5
_Y = ((np.arange(16) // 4).astype(np.float64) - 1.5) / 1.5

# seeds and sizes the tests and the golden files share. PER = tiles per partition (and per noise level of two_opaque)
TWO_OPAQUE_PER, TWO_OPAQUE_SEED = 24, 7001
TWO_ALPHA_PER, TWO_ALPHA_SEED = 24, 7002
THREE_OPAQUE_PER, THREE_OPAQUE_SEED = 40, 7003
THREE_FIRST16_PER, THREE_FIRST16_SEED = 88, 7004
VECTOR_SCALAR_N, VECTOR_SCALAR_SEED = 1024, 7005
RAMP_ALPHA_N, RAMP_ALPHA_SEED = 640, 7006
GREY_RAMP_N, GREY_RAMP_SEED = 384, 7007
EXACT_N, EXACT_SEED = 512, 7008
OFF_GRID_N, OFF_GRID_SEED = 256, 7009

DEFAULT_SETS = ("two_opaque", "two_alpha", "vector_scalar", "ramp_alpha", "grey_ramp_opaque", "exact", "off_grid")          # flags 0
THREE_SETS = ("three_opaque", "three_first16")                                                                             # BC7_USE_3SUBSETS
MIXED_SETS = ("vector_scalar", "ramp_alpha", "exact", "grey_ramp_opaque")                                                  # the mixed image


def masks():
    """(two (64, 16) values 0/1, three (64, 16) values 0/1/2): the subset of every texel per partition, as the reference decoder has it."""
    with np.load(MASKS_FILE) as z:
        return z["two"].copy(), z["three"].copy()


def _surface(rng, n, ch, amp, noise):
    """(n, 16, ch) float64: a base U(0, 255) per channel, plus a planar ramp along a gaussian direction per channel of amplitude U(amp) per tile, plus
    gaussian noise per texel and channel of sigma 2^U(log2 noise) per tile. amp and noise are (low, high) pairs."""
    base = rng.uniform(0.0, 255.0, (n, 1, ch))
    d = rng.standard_normal((n, 2, ch))
    a = rng.uniform(amp[0], amp[1], (n, 1, 1))
    ramp = (d[:, 0:1, :] * _X[None, :, None] + d[:, 1:2, :] * _Y[None, :, None]) * a
    sigma = np.exp2(rng.uniform(np.log2(noise[0]), np.log2(noise[1]), (n, 1, 1)))
    return base + ramp + sigma * rng.standard_normal((n, 16, ch))


def _bytes(v, opaque=False):
    """(n, 16, 3 | 4) float64 -> (n, 16, 4) uint8, rounded and clipped; three channels get alpha 255."""
    t = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    if t.shape[2] == 3:
        t = np.concatenate([t, np.full(t.shape[:2] + (1,), 255, np.uint8)], -1)
    if opaque:
        t[:, :, 3] = 255
    return t


def _regions(rng, region_of_texel, per, ch, amp, noise):
    """`per` tiles per row of region_of_texel (partitions, 16), partition-major: every region of a tile is an independent surface."""
    part = np.repeat(np.arange(region_of_texel.shape[0]), per)
    reg = region_of_texel[part]                                           # (n, 16)
    n = len(part)
    v = _surface(rng, n, ch, amp, noise)
    for r in range(1, int(region_of_texel.max()) + 1):
        v = np.where((reg == r)[:, :, None], _surface(rng, n, ch, amp, noise), v)
    return v


def two_opaque(per, seed):
    """The 64 two-subset partitions, an independent RGB surface per region, alpha 255: a noisy half (amp 25, noise up to 6) and then a quiet half
    (amp 10, noise up to 1.5), each partition-major. Modes 1 and 3 win with every partition."""
    rng = np.random.default_rng(seed)
    two, _ = masks()
    return _bytes(np.concatenate([_regions(rng, two, per, 3, (0.0, 25.0), (0.25, 6.0)), _regions(rng, two, per, 3, (0.0, 10.0), (0.25, 1.5))]))


def two_alpha(per, seed):
    """two_opaque's noisy half with four-channel surfaces: mode 7 wins with every partition."""
    rng = np.random.default_rng(seed)
    two, _ = masks()
    return _bytes(_regions(rng, two, per, 4, (0.0, 25.0), (0.25, 6.0)))


def three_opaque(per, seed):
    """The 64 three-subset partitions, an RGB surface per region (amp 25, noise up to 6): with BC7_USE_3SUBSETS mode 2 wins with every partition."""
    rng = np.random.default_rng(seed)
    _, three = masks()
    return _bytes(_regions(rng, three, per, 3, (0.0, 25.0), (0.25, 6.0)))


def three_first16(per, seed):
    """The first 16 three-subset partitions (mode 0's) with steep, noisy surfaces (amp 40 - 60, noise 10 - 24): what lets mode 0's 4-bit endpoints
    with 3-bit indices beat mode 2. Gentler surfaces leave some partitions with two or three mode 0 winners."""
    rng = np.random.default_rng(seed)
    _, three = masks()
    return _bytes(_regions(rng, three[:16], per, 3, (40.0, 60.0), (10.0, 24.0)))


def vector_scalar(n, seed):
    """Three channels affine in one shared surface, the fourth - R, G, B or A, uniformly per tile - an independent surface: the layout modes 4 and 5
    are made for (a colour vector plus a scalar, the scalar rotated into the alpha slot), next to modes 6 and 7."""
    rng = np.random.default_rng(seed)
    s = _surface(rng, n, 1, (0.0, 60.0), (0.25, 6.0))
    s = s - s.mean(axis=1, keepdims=True)
    v = rng.uniform(0.0, 255.0, (n, 1, 4)) + rng.uniform(-1.0, 1.0, (n, 1, 4)) * s
    own = _surface(rng, n, 1, (0.0, 60.0), (0.25, 6.0))
    slot = rng.integers(0, 4, n)
    v = np.where((np.arange(4)[None, :] == slot[:, None])[:, None, :], own, v)
    return _bytes(v)


def ramp_alpha(n, seed):
    """One region, four channels, steep ramps (amp 120 - 200) with little noise (1 - 3): mode 5 wins with every rotation."""
    rng = np.random.default_rng(seed)
    return _bytes(_surface(rng, n, 4, (120.0, 200.0), (1.0, 3.0)))


def grey_ramp_opaque(n, seed):
    """RGB = one steep ramp (amp 120, noise up to 2) times a gain in [0.5, 1] per channel, plus noise of 0.7 sigma, alpha 255: opaque tiles on which
    mode 6 wins."""
    rng = np.random.default_rng(seed)
    s = _surface(rng, n, 1, (0.0, 120.0), (0.25, 2.0))
    v = s * rng.uniform(0.5, 1.0, (n, 1, 3)) + 0.7 * rng.standard_normal((n, 16, 3))
    return _bytes(v)


def exact(n, seed):
    """Tiles some mode encodes with zero error: n / 2 flat tiles, then n / 2 two-value tiles (random bytes, a random side per texel), every second
    tile opaque. The search reaches error 0 in different modes and its `best error > 0` early-outs fire at different depths; the block that wins is
    the FIRST candidate in the reference's order that reaches the winning error."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (n, 1, 4)); b = rng.integers(0, 256, (n, 1, 4))
    side = rng.random((n, 16, 1)) < 0.5
    side[: n // 2] = False
    t = np.where(side, b, a).astype(np.uint8)
    t[::2, :, 3] = 255
    return t


def unit(tiles):
    """uint8 tiles -> float32 in [0, 1]: byte * (1 / 255) in float32, bit for bit what the RGBA8 scanline loader produces."""
    return np.asarray(tiles, np.uint8).astype(np.float32) * np.float32(1.0 / 255.0)


def off_grid(tiles, seed):
    """float32 tiles OFF the 1/255 grid, from uint8 tiles: byte k becomes the float32 nearest (k + 0.99) / 255 moved by -3 .. +3 ulp, so that
    x * 255.0f + 0.01f lands within rounding of k + 1 and the encoder's byte (a truncation) is k or k + 1 depending on the last bit - and on whether the
    multiply and the add are fused. One value in 16 is replaced by one below 0, above 1 or -0.0 (all finite)."""
    rng = np.random.default_rng(seed)
    k = np.asarray(tiles, np.uint8).astype(np.float64)
    v = ((k + 0.99) / 255.0).astype(np.float32)
    step = rng.integers(-3, 4, v.shape)
    for s in range(1, 4):
        v = np.where(step >= s, np.nextafter(v, np.float32(2.0)), v)
        v = np.where(step <= -s, np.nextafter(v, np.float32(-2.0)), v)
    odd = np.array([-0.0, -1e-6, -0.004, -0.5, -3.0, 1.0000001, 1.004, 1.5, 300.0], np.float32)
    pick = rng.random(v.shape) < 1.0 / 16.0
    v = np.where(pick, odd[rng.integers(0, len(odd), v.shape)], v).astype(np.float32)
    assert np.isfinite(v).all()
    return v


def as_image(tiles):
    """n tiles as an (H, W, 4) image of the tiles' dtype, TILES_PER_ROW tiles wide, block b of the image = tile b. A last row that n does not fill is
    completed with the first tiles again (tile b % n), so every block of the image has a known expected payload. Returns (image, width, height)."""
    tiles = np.asarray(tiles)
    n = tiles.shape[0]
    rows = (n + TILES_PER_ROW - 1) // TILES_PER_ROW
    t = tiles[np.arange(rows * TILES_PER_ROW) % n].reshape(rows, TILES_PER_ROW, 4, 4, 4)
    img = np.ascontiguousarray(t.transpose(0, 2, 1, 3, 4).reshape(rows * 4, TILES_PER_ROW * 4, 4))
    return img, TILES_PER_ROW * 4, rows * 4


def image_payload(blocks, n_image_blocks):
    """The expected payload of as_image()'s image from the n tiles' expected blocks."""
    blocks = np.asarray(blocks, np.uint8).reshape(-1, 16)
    return blocks[np.arange(n_image_blocks) % blocks.shape[0]]


CROP_W, CROP_H = 13, 9
CROP_ORIGINS = tuple((32 * i, 12 * i) for i in range(8))          # multiples of 4, inside the 256 x 96 image of two_alpha


def crops(tiles):
    """CROP_W x CROP_H windows of as_image(tiles) at CROP_ORIGINS: partial blocks on the right and bottom edges, whose missing texels the encoder's
    driver replicates."""
    img, w, h = as_image(tiles)
    assert all(x + CROP_W <= w and y + CROP_H <= h for x, y in CROP_ORIGINS)
    return [np.ascontiguousarray(img[y:y + CROP_H, x:x + CROP_W]) for x, y in CROP_ORIGINS]


def corpus():
    """name -> tiles: uint8 for every family but off_grid (float32)."""
    t = {
        "two_opaque": two_opaque(TWO_OPAQUE_PER, TWO_OPAQUE_SEED),
        "two_alpha": two_alpha(TWO_ALPHA_PER, TWO_ALPHA_SEED),
        "three_opaque": three_opaque(THREE_OPAQUE_PER, THREE_OPAQUE_SEED),
        "three_first16": three_first16(THREE_FIRST16_PER, THREE_FIRST16_SEED),
        "vector_scalar": vector_scalar(VECTOR_SCALAR_N, VECTOR_SCALAR_SEED),
        "ramp_alpha": ramp_alpha(RAMP_ALPHA_N, RAMP_ALPHA_SEED),
        "grey_ramp_opaque": grey_ramp_opaque(GREY_RAMP_N, GREY_RAMP_SEED),
        "exact": exact(EXACT_N, EXACT_SEED),
    }
    # off_grid: every k-th tile of the flags-0 families above, so regions, ramps, alpha and exact tiles are all in it
    pool = np.concatenate([t[name] for name in DEFAULT_SETS if name != "off_grid"])
    t["off_grid"] = off_grid(pool[np.arange(OFF_GRID_N) * len(pool) // OFF_GRID_N], OFF_GRID_SEED)
    return t


def floats(name, tiles):
    """The float32 tiles the block encoders are handed for a family."""
    return tiles if name == "off_grid" else unit(tiles)


def mode_field(blocks):
    """The mode of BC7 blocks (the position of the lowest set bit of byte 0; 8 for the reserved all-zero byte): (n, 16) uint8 -> (n,) int."""
    b0 = np.asarray(blocks, np.uint8).reshape(-1, 16)[:, 0].astype(np.int64)
    low = b0 & -b0
    return np.where(b0 == 0, 8, np.log2(np.maximum(low, 1)).astype(np.int64))


def _bits(blocks, first, count):
    b = np.asarray(blocks, np.uint8).reshape(-1, 16)
    lo = b[:, 0].astype(np.int64) | (b[:, 1].astype(np.int64) << 8)
    return (lo >> first) & ((1 << count) - 1)


def partition_field(blocks):
    """The partition of blocks of modes 0 (4 bits), 1, 2, 3 and 7 (6 bits; the field follows the mode's unary prefix), -1 for modes 4, 5 and 6."""
    m = mode_field(blocks)
    out = np.full(len(m), -1, np.int64)
    for mode, count in ((0, 4), (1, 6), (2, 6), (3, 6), (7, 6)):
        out = np.where(m == mode, _bits(blocks, mode + 1, count), out)
    return out


def rotation_field(blocks):
    """The 2-bit rotation of blocks of modes 4 and 5, -1 otherwise."""
    m = mode_field(blocks)
    return np.where(m == 4, _bits(blocks, 5, 2), np.where(m == 5, _bits(blocks, 6, 2), -1))


def index_selector_field(blocks):
    """Mode 4's index selector bit, -1 otherwise."""
    return np.where(mode_field(blocks) == 4, _bits(blocks, 7, 1), -1)
