"""BC6H test corpus: 4x4 tiles that let every mode of the encoder win blocks, and tiles at the top of the half range on which the SF16 search of
the 16-bit one-region mode ends above 32767 (bc6h_encode.hip: Ep16 / ep16_mark).

numpy only, deterministic (fixed seeds), no GPU and no oracle. Every family returns (n, 16, 4) float32 tiles, texel i = 4 * y + x, alpha 1, colour
values already rounded through float16 (so RGBA16F and RGBA32F sources hold the same numbers). What the reference encoder does with them - which modes
and partition shapes win, which end states the 16-bit search reaches - is measured by tests/test_bc6h_corpus_cpu.py; the expected payloads live in
tests/golden/bc6h_corpus_*.npz (tests/golden/make_golden_bc6h_corpus.py)."""
import numpy as np

HALF_MAX = 65504.0
TILES_PER_ROW = 64

_X = (np.arange(16) % 4).astype(np.float64)
_Y = (np.arange(16) // 4).astype(np.float64)

# seeds and sizes the tests and the golden files share
SMOOTH_N, SMOOTH_SEED = 4096, 6001
NEAR_TOP_N, NEAR_TOP_SEED = 2000, 6002            # per sub-kind: 7 sub-kinds
BRIGHT_N, BRIGHT_SEED = 6000, 6003
TINY_N, TINY_SEED = 500, 6004                     # per sub-kind: 6 sub-kinds
TINY_KINDS = ("rand4", "rand8", "flat4+4", "flat8+2", "two16", "flat32+4 signs")
NEAR_TOP_KINDS = ("k2", "k3", "k5", "k8", "k12", "base", "two")


def _finish(rgb, lo, hi):
    """(n, 16, 3) float64 -> (n, 16, 4) float32, clipped to [lo, hi], rounded through half, alpha 1."""
    v = np.clip(rgb, lo, hi).astype(np.float32).astype(np.float16).astype(np.float32)
    return np.concatenate([v, np.ones(v.shape[:2] + (1,), np.float32)], -1)


def _surface(rng, n, base, amp_log2, noise_log2):
    """base * (1 + planar ramp + noise): ramp of relative amplitude 2^U(amp_log2) per tile along a gaussian direction per channel, relative noise
    2^U(noise_log2) * N(0, 1) per texel and channel."""
    amp = np.exp2(rng.uniform(*amp_log2, (n, 1, 1)))
    d = rng.standard_normal((n, 2, 3))
    ramp = (d[:, 0:1, :] * ((_X - 1.5) / 1.5)[None, :, None] + d[:, 1:2, :] * ((_Y - 1.5) / 1.5)[None, :, None]) * amp
    noise = np.exp2(rng.uniform(*noise_log2, (n, 1, 1))) * rng.standard_normal((n, 16, 3))
    return base[:, None, :] * (1.0 + ramp + noise)


def smooth(n, seed, signs=False):
    """Smooth tiles over the whole half range, half of them with a second surface on one side of a random line: the family on which 13 of the 14
    modes and all 32 partition shapes win blocks. signs=False: all positive (UF16, and SF16's first variant); signs=True: one random sign per tile
    and channel (SF16's second variant - a sign per TEXEL would leave one mode only)."""
    rng = np.random.default_rng(seed)
    base = np.exp2(rng.uniform(-10.0, 15.9, (n, 3))) * rng.uniform(0.3, 1.0, (n, 3))
    v = _surface(rng, n, base, (-12.0, 0.0), (-14.0, -3.0))
    base2 = base * np.exp2(rng.uniform(-3.0, 3.0, (n, 3)))
    v2 = _surface(rng, n, base2, (-12.0, 0.0), (-14.0, -3.0))
    ang = rng.uniform(0.0, np.pi, (n, 1)); off = rng.uniform(0.2, 0.8, (n, 1))
    side = ((_X / 3.0)[None, :] * np.cos(ang) + (_Y / 3.0)[None, :] * np.sin(ang)) > off
    two = rng.random((n, 1)) < 0.5
    v = np.where((side & two)[:, :, None], v2, v)
    v = np.clip(v, 0.0, HALF_MAX)
    if signs:
        v = v * np.where(rng.random((n, 1, 3)) < 0.5, -1.0, 1.0)
    return _finish(v, -HALF_MAX if signs else 0.0, HALF_MAX)


def _from_bits(bits, negative=None):
    b = np.minimum(bits, 0x7BFF).astype(np.uint16)
    if negative is not None:
        b = b | (np.broadcast_to(negative, b.shape).astype(np.uint16) << 15)
    v = b.view(np.float16).astype(np.float32)
    return np.concatenate([v, np.ones(v.shape[:2] + (1,), np.float32)], -1)


def near_top_bits(n, seed):
    """Tiles of half BIT PATTERNS just below 0x7BFF (65504), n per sub-kind, in the order of NEAR_TOP_KINDS: 0x7BFF - randint(0, k) per texel and
    channel for k = 2, 3, 5, 8, 12; a base 0x7BFF - randint(0, 40) per channel plus randint(-3, 4) per texel; two-value tiles a = 0x7BFF -
    randint(0, 6), b = a - randint(0, 8). In SF16 the 16-bit one-region search ends above 32767 on most of them."""
    rng = np.random.default_rng(seed)
    out = []
    for k in (2, 3, 5, 8, 12):
        out.append(0x7BFF - rng.integers(0, k, (n, 16, 3)))
    out.append(0x7BFF - rng.integers(0, 40, (n, 1, 3)) + rng.integers(-3, 4, (n, 16, 3)))
    a = 0x7BFF - rng.integers(0, 6, (n, 1, 3)); b = a - rng.integers(0, 8, (n, 1, 3))
    out.append(np.where(rng.random((n, 16, 1)) < 0.5, a, b))
    return _from_bits(np.concatenate(out))


def tiny_bits(n, seed):
    """Tiles of the SMALLEST half bit patterns (denormals, values below 4e-6), n per sub-kind, in the order of TINY_KINDS: the family on which the
    16-bit one-region mode (0x0F, 16:4) wins blocks - nothing else found does. randint(0, k) per texel and channel for k = 4, 8; a base
    randint(0, k) per channel plus randint(0, s) per texel for (k, s) = (4, 4), (8, 2); two-value tiles a = randint(0, 16), b = a + randint(0, 4);
    base randint(0, 32) plus randint(0, 4) with one random sign per tile and channel (negative endpoints in SF16's 16-bit fields; UF16 reads the
    negative channels as 0)."""
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 4, (n, 16, 3)), rng.integers(0, 8, (n, 16, 3)),
           rng.integers(0, 4, (n, 1, 3)) + rng.integers(0, 4, (n, 16, 3)), rng.integers(0, 8, (n, 1, 3)) + rng.integers(0, 2, (n, 16, 3))]
    a = rng.integers(0, 16, (n, 1, 3)); b = a + rng.integers(0, 4, (n, 1, 3))
    out.append(np.where(rng.random((n, 16, 1)) < 0.5, a, b))
    out.append(rng.integers(0, 32, (n, 1, 3)) + rng.integers(0, 4, (n, 16, 3)))
    neg = np.zeros((6 * n, 1, 3), bool); neg[5 * n:] = rng.random((n, 1, 3)) < 0.5
    return _from_bits(np.concatenate(out), neg)


def bright_smooth(n, seed):
    """smooth() without the second surface, at the top of the range: the family on which the SF16 16-bit search ends with A alone above 32767."""
    rng = np.random.default_rng(seed)
    base = np.exp2(rng.uniform(14.5, 16.0, (n, 3))) * rng.uniform(0.7, 1.0, (n, 3))
    return _finish(_surface(rng, n, base, (-14.0, -5.0), (-16.0, -8.0)), 0.0, HALF_MAX)


def as_image(tiles):
    """n tiles as an (H, W, 4) float32 image, TILES_PER_ROW tiles wide, block b of the image = tile b. A last row that n does not fill is completed
    with the first tiles again (tile b % n), so every block of the image has a known expected payload. Returns (image, width, height)."""
    tiles = np.asarray(tiles, np.float32)
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
CROP_ORIGINS = tuple((32 * i, 32 * i) for i in range(8))


def crops(tiles):
    """CROP_W x CROP_H windows of as_image(tiles) at CROP_ORIGINS (multiples of 4), as float16 RGBA16F images: partial blocks on the right and
    bottom edges, whose missing texels the encoder's driver replicates."""
    img, _, _ = as_image(tiles)
    return [np.ascontiguousarray(img[y:y + CROP_H, x:x + CROP_W]).astype(np.float16) for x, y in CROP_ORIGINS]


def corpus():
    """name -> tiles, the sets the golden files hold (the same arrays for both formats unless the name says otherwise)."""
    return {
        "smooth": smooth(SMOOTH_N, SMOOTH_SEED),
        "smooth_signs": smooth(SMOOTH_N, SMOOTH_SEED, signs=True),          # SF16 only
        "near_top": near_top_bits(NEAR_TOP_N, NEAR_TOP_SEED),
        "bright": bright_smooth(BRIGHT_N, BRIGHT_SEED),
        "tiny": tiny_bits(TINY_N, TINY_SEED),
    }


def mode_field(blocks):
    """The 5-bit mode field of BC6H blocks, the two-bit modes (0x00, 0x01) folded: (n, 16) uint8 -> (n,) int."""
    m = np.asarray(blocks, np.uint8).reshape(-1, 16)[:, 0].astype(np.int64) & 31
    return np.where((m & 3) < 2, m & 3, m)


def shape_field(blocks):
    """The 5-bit partition shape of two-region blocks (bits 77 - 81), -1 for one-region modes."""
    b = np.asarray(blocks, np.uint8).reshape(-1, 16)
    v = (b[:, 9].astype(np.int64) | (b[:, 10].astype(np.int64) << 8)) >> 5 & 31
    one = np.isin(mode_field(b), (0x03, 0x07, 0x0B, 0x0F))
    return np.where(one, -1, v)
