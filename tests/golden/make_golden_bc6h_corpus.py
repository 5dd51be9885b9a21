"""Writes tests/golden/bc6h_corpus_uf16.npz and bc6h_corpus_sf16.npz: the reference encoder's payloads (16 bytes per tile) for the tile sets of
tests/bc6h_corpus.py, so that tests/test_bc6h_corpus_gpu.py spends no reference CPU time. Run it where oracle/_ref/libdxtex_ref.so exists:

    python tests/golden/make_golden_bc6h_corpus.py

tests/test_bc6h_corpus_cpu.py asserts that the files equal the live reference, so they cannot drift from the generators."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bc6h_corpus  # noqa: E402
import oracle  # noqa: E402

UF16, SF16 = 95, 96
SETS = {UF16: ("smooth", "near_top", "bright", "tiny"), SF16: ("smooth", "smooth_signs", "near_top", "bright", "tiny")}
FILES = {UF16: os.path.join(HERE, "bc6h_corpus_uf16.npz"), SF16: os.path.join(HERE, "bc6h_corpus_sf16.npz")}


CROP_SET = {UF16: "smooth", SF16: "smooth_signs"}          # the set whose image the 13 x 9 crops are cut from
RGBA16F = 10


def reference_payloads(fmt, tiles):
    """set name -> (n, 16) payloads of the tiles, and "crops" -> (windows, 12, 16) payloads of bc6h_corpus.crops() through the Compress driver."""
    out = {name: oracle.ref_encode_blocks(fmt, tiles[name], 0) for name in SETS[fmt]}
    out["crops"] = np.stack([oracle.ref_compress_image(c, bc6h_corpus.CROP_W, bc6h_corpus.CROP_H, RGBA16F, fmt, 0, 0.5).reshape(-1, 16)
                             for c in bc6h_corpus.crops(tiles[CROP_SET[fmt]])])
    return out


if __name__ == "__main__":
    tiles = bc6h_corpus.corpus()
    for fmt, path in FILES.items():
        np.savez_compressed(path, **reference_payloads(fmt, tiles))
        print(path, os.path.getsize(path), "bytes")
