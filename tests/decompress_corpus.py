"""The block payloads and format lists of the Decompress tests (test_decompress_formats_gpu.py, test_decompress_corpus_cpu.py).

payload() gives uniformly random blocks with planted blocks at fixed indices, so that every image of the matrix holds the blocks where a
decoder, the ConvertScanline plan or a store can go wrong: both BC1 colour orders, both BC3 / BC4 alpha layouts, the SNORM -128 endpoint,
every BC7 mode and the reserved one, and for BC6H_SF16 the one infinity the format can decode to next to real encoder output. Random
SF16 payloads of 275 and of 4096 blocks held no infinity, so that block has to be planted; about 12 % of random BC6H blocks are reserved
modes, so those come by themselves."""
import functools

import numpy as np

SOURCES = [71, 72, 74, 75, 77, 78, 80, 81, 83, 84, 95, 96, 98, 99]
# Every destination the reference's Decompress accepts and this library writes: the uncompressed formats whose element is one texel.
DESTS = [2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14, 16, 17, 18, 20, 24, 25, 26, 28, 29, 30, 31, 32, 34, 35, 36, 37, 38, 40, 41, 42, 43, 45, 49, 50,
         51, 52, 54, 55, 56, 57, 58, 59, 61, 62, 63, 64, 65, 67, 85, 86, 87, 88, 89, 91, 93, 100, 101, 102, 115, 191]
# R8G8_B8G8, G8R8_G8B8, YUY2, Y210, Y216: two texels per element. The reference's Decompress accepts them and then corrupts its heap
# (DecompressBC stores four-texel runs into rows of two-texel elements), so it is NEVER called with these; the library refuses them.
GROUPED = [68, 69, 107, 108, 109]
# What the reference's Decompress returned S_OK for when it was measured (13 x 7, 16 x 8, 100 x 44; a child process per grouped format)
REFERENCE_ACCEPTS = [2, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14, 16, 17, 18, 20, 24, 25, 26, 28, 29, 30, 31, 32, 34, 35, 36, 37, 38, 40, 41, 42, 43,
                     45, 49, 50, 51, 52, 54, 55, 56, 57, 58, 59, 61, 62, 63, 64, 65, 67, 68, 69, 85, 86, 87, 88, 89, 91, 93, 100, 101, 102,
                     107, 108, 109, 115, 191]
BC_DESTS = SOURCES               # refused with E_INVALIDARG by the reference and the library alike
R1 = 66                          # refused with HRESULT_E_NOT_SUPPORTED by both

BLOCK_BYTES = {71: 8, 72: 8, 74: 16, 75: 16, 77: 16, 78: 16, 80: 8, 81: 8, 83: 16, 84: 16, 95: 16, 96: 16, 98: 16, 99: 16}
SRGB_SOURCES = {72, 75, 78, 99}
SRGB_DESTS = {29, 91, 93}
SIZES = [(16, 8), (13, 7), (100, 44)]

BC6H_VALID_MODES = {0x00, 0x01, 0x02, 0x06, 0x0A, 0x0E, 0x12, 0x16, 0x1A, 0x1E, 0x03, 0x07, 0x0B, 0x0F}
BITMAP_0123 = 0xE4E4E4E4                                            # 2-bit indices 0, 1, 2, 3 in every row
INDEX3_0TO7 = sum((i % 8) << (3 * i) for i in range(16))            # 3-bit indices 0 .. 7, twice


def _colour_block(c0, c1):
    return np.frombuffer(int(c0 | (c1 << 16) | (BITMAP_0123 << 32)).to_bytes(8, "little"), np.uint8)


def _alpha_block(a0, a1):
    return np.frombuffer(int((a0 & 0xFF) | ((a1 & 0xFF) << 8) | (INDEX3_0TO7 << 16)).to_bytes(8, "little"), np.uint8)


def bc6h_mode(block):
    m = int(block[0]) & 3
    return m if m < 2 else int(block[0]) & 31


@functools.lru_cache(maxsize=None)
def _sf16_encoder_blocks(oracle):
    """Real BC6H_SF16 encoder output on four signed HDR tiles of growing range."""
    rng = np.random.default_rng(96)
    tiles = (rng.random((4, 16, 4), dtype=np.float32) * 2 - 1) * np.array([1, 8, 100, 1000], np.float32)[:, None, None]
    tiles[..., 3] = 1
    return oracle.ref_encode_blocks(96, tiles)


def planted(fmt, oracle):
    """-> [(name, block)], in the order payload() places them."""
    bb = BLOCK_BYTES[fmt]
    rng = np.random.default_rng(1000 + fmt)

    def random_block():
        return rng.integers(0, 256, bb, dtype=np.uint8)

    out = [("zero", np.zeros(bb, np.uint8)), ("ones", np.full(bb, 255, np.uint8))]
    if fmt in (71, 72, 74, 75, 77, 78):
        at = 0 if fmt in (71, 72) else 8
        for name, (c0, c1) in (("c0>c1", (0x8410, 0x0821)), ("c0<=c1", (0x0821, 0x8410))):
            b = random_block()
            b[at:at + 8] = _colour_block(c0, c1)
            out.append((name, b))
    if fmt in (77, 78, 80, 81, 83, 84):
        signed = fmt in (81, 84)
        hi, lo = (100, -100) if signed else (200, 50)
        pairs = [("a0>a1", (hi, lo)), ("a0<=a1", (lo, hi))]
        if signed:
            pairs += [("-128,127", (0x80, 0x7F)), ("127,-128", (0x7F, 0x80))]
        for name, (a0, a1) in pairs:
            b = random_block()
            b[0:8] = _alpha_block(a0, a1)
            if fmt in (83, 84):
                b[8:16] = _alpha_block(a0, a1)
            out.append((name, b))
    if fmt in (98, 99):
        for m in range(8):
            b = random_block()
            b[0] = 1 << m
            out.append((f"mode{m}", b))
        b = random_block()
        b[0] = 0
        out.append(("mode-none", b))
    if fmt in (95, 96):
        b = np.zeros(bb, np.uint8)
        b[0] = 0x07                                                 # mode bits only
        out.append(("mode-bits-only", b))
    if fmt == 96:
        b = np.zeros(bb, np.uint8)
        b[0] = 0x0F                                                 # mode 0x0f (16:4), one region
        b[4] = 0x80                                                 # header bit 39 = bit 15 of the red base endpoint: -32768 when signed
        out.append(("inf", b))
        out += [(f"encoded{i}", blk) for i, blk in enumerate(_sf16_encoder_blocks(oracle))]
    return out


def payload(fmt, nblocks, oracle, first=0):
    """-> ((nblocks, block bytes) uint8, {name: index}): random blocks, the planted ones at indices 0, 1, ... starting with planted block
    `first` and wrapping round, as many as fit. An image of eight blocks holds every planted block of a format but BC7's eleven, which
    two images with first = 0 and first = 8 hold between them."""
    bb = BLOCK_BYTES[fmt]
    blocks = np.random.default_rng(fmt * 7919 + nblocks).integers(0, 256, (nblocks, bb), dtype=np.uint8)
    plants = planted(fmt, oracle)
    first %= len(plants)
    plants = plants[first:] + plants[:first]
    where = {}
    for i, (name, b) in enumerate(plants[:nblocks]):
        blocks[i] = b
        where[name] = i
    return blocks, where


def blocks_of(w, h):
    return ((w + 3) // 4) * ((h + 3) // 4)
