"""Writes tests/golden/bc7_partition_masks.npz, bc7_corpus_default.npz and bc7_corpus_3subsets.npz: the region masks of BC7's partitions as the
reference DECODER has them, and the reference encoder's payloads (16 bytes per tile) for the tile sets of tests/bc7_corpus.py, so that
tests/test_bc7_corpus_gpu.py spends no reference CPU time. Run it where oracle/_ref/libdxtex_ref.so exists:

    python tests/golden/make_golden_bc7_corpus.py

It writes the masks first (the corpus is generated from them). tests/test_bc7_corpus_cpu.py asserts that all three files equal the live reference,
so they cannot drift from the generators."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bc7_corpus  # noqa: E402
import oracle  # noqa: E402

BC7, RGBA8, RGBA32F = 98, 28, 2
USE_3SUBSETS, QUICK = 0x80000, 0x100000
FLAGS = {"default": 0, "3subsets": USE_3SUBSETS}
SETS = {"default": bc7_corpus.DEFAULT_SETS, "3subsets": bc7_corpus.THREE_SETS}
FILES = {"default": os.path.join(HERE, "bc7_corpus_default.npz"), "3subsets": os.path.join(HERE, "bc7_corpus_3subsets.npz")}
QUICK_SETS = bc7_corpus.DEFAULT_SETS + bc7_corpus.THREE_SETS          # "quick": the whole corpus in this order, in the default file
CROP_SET = "two_alpha"


def _put(blocks, first, count, value):
    """Write `count` bits of value (an int or an (n,) array) at bit `first` of (n, 16) uint8 blocks, least significant bit first."""
    value = np.broadcast_to(np.asarray(value, np.int64), (blocks.shape[0],))
    for i in range(count):
        bit = ((value >> i) & 1).astype(np.uint8)
        blocks[:, (first + i) // 8] |= bit << ((first + i) % 8)


def record_masks():
    """The subset of every texel for the 64 two-subset and the 64 three-subset partitions, read off the reference decoder: hand-built blocks whose
    subsets decode to distinct reds (no partition table of the encoder or of the reference is consulted).
      mode 3, partition p: subset 0 endpoints 0 with p-bit 0, subset 1 endpoints 127 with p-bit 1 (red 0 / 255), indices 0;
      mode 2, partition p: endpoints 0 / 15 / 31 for the three subsets (red 0 / 123 / 255), indices 0."""
    p = np.arange(64)
    m3 = np.zeros((64, 16), np.uint8)
    _put(m3, 3, 1, 1)                         # mode 3: bit 3
    _put(m3, 4, 6, p)
    for ch in range(3):                       # 7-bit fields, per channel: subset 0 A, B, subset 1 A, B
        _put(m3, 10 + ch * 28 + 14, 7, 127)
        _put(m3, 10 + ch * 28 + 21, 7, 127)
    _put(m3, 94 + 2, 2, 3)                    # p-bits of subset 1's endpoints
    two = (oracle.ref_decode_blocks(BC7, m3)[:, :, 0] > 0.5).astype(np.uint8)
    m2 = np.zeros((64, 16), np.uint8)
    _put(m2, 2, 1, 1)                         # mode 2: bit 2
    _put(m2, 3, 6, p)
    for ch in range(3):                       # 5-bit fields, per channel: subset 0 A, B, subset 1 A, B, subset 2 A, B
        for e, v in ((2, 15), (3, 15), (4, 31), (5, 31)):
            _put(m2, 9 + ch * 30 + e * 5, 5, v)
    red = oracle.ref_decode_blocks(BC7, m2)[:, :, 0]
    three = ((red > 0.25).astype(np.uint8) + (red > 0.75).astype(np.uint8))
    return two, three


def reference_payloads(which, tiles):
    """set name -> (n, 16) payloads of the tiles under the file's flags; "crops" -> (windows, 12, 16) payloads of bc7_corpus.crops() through the
    Compress driver; in the default file "quick" -> the whole corpus under BC7_QUICK, and "off_grid_image" -> as_image() of off_grid through the
    Compress driver from R32G32B32A32_FLOAT (which saturates the values to [0, 1] before the encoder sees them; the block encoder gets them raw)."""
    flags = FLAGS[which]
    out = {name: oracle.ref_encode_blocks(BC7, bc7_corpus.floats(name, tiles[name]), flags) for name in SETS[which]}
    crop_set = CROP_SET if which == "default" else SETS[which][0]
    out["crops"] = np.stack([oracle.ref_compress_image(c, bc7_corpus.CROP_W, bc7_corpus.CROP_H, RGBA8, BC7, flags, 0.5).reshape(-1, 16)
                             for c in bc7_corpus.crops(tiles[crop_set])])
    if which == "default":
        out["quick"] = oracle.ref_encode_blocks(BC7, np.concatenate([bc7_corpus.floats(name, tiles[name]) for name in QUICK_SETS]), QUICK)
        img, w, h = bc7_corpus.as_image(tiles["off_grid"])
        out["off_grid_image"] = oracle.ref_compress_image(img, w, h, RGBA32F, BC7, 0, 0.5).reshape(-1, 16)
    return out


if __name__ == "__main__":
    two, three = record_masks()
    np.savez_compressed(bc7_corpus.MASKS_FILE, two=two, three=three)
    print(bc7_corpus.MASKS_FILE, os.path.getsize(bc7_corpus.MASKS_FILE), "bytes")
    tiles = bc7_corpus.corpus()
    for which, path in FILES.items():
        np.savez_compressed(path, **reference_payloads(which, tiles))
        print(path, os.path.getsize(path), "bytes")
