"""The inputs of test_decompress_formats_gpu.py, checked with the oracle alone: the planted blocks of decompress_corpus.payload() decode
to what they are planted for, the BC6H payload reaches every mode, the reference's Decompress is repeatable on every (source,
destination) pair of the matrix, and the destination list is the measured one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decompress_corpus as dc  # noqa: E402


def _decoded(oracle, fmt, nblocks=8, first=0):
    blocks, where = dc.payload(fmt, nblocks, oracle, first)
    return blocks, where, oracle.ref_decode_blocks(fmt, blocks)


@pytest.mark.parametrize("fmt", [71, 72, 74, 75, 77, 78])
def test_planted_colour_orders(oracle, fmt):
    """Index 3 of a BC1 block with c0 <= c1 is transparent black and index 2 the midpoint; BC2 / BC3 ignore the order."""
    _, where, t = _decoded(oracle, fmt)
    gt, le = t[where["c0>c1"]], t[where["c0<=c1"]]
    assert np.array_equal(gt[:4, :3], gt[4:8, :3]) and len({tuple(c) for c in gt[:4, :3]}) == 4       # indices 0 .. 3 in every row
    third = gt[0, :3] + (gt[1, :3] - gt[0, :3]) * np.float32(1 / 3)
    assert np.allclose(gt[2, :3], third, atol=1e-6) and not np.allclose(gt[3, :3], 0)
    if fmt in (71, 72):
        assert (gt[:, 3] == 1).all()
        assert not le[3].any() and le[2, 3] == 1
        assert np.allclose(le[2, :3], (le[0, :3] + le[1, :3]) / 2, atol=1e-6)
    else:
        assert np.allclose(le[2, :3], le[0, :3] + (le[1, :3] - le[0, :3]) * np.float32(1 / 3), atol=1e-6) and le[3, :3].any()
    assert not t[where["zero"]][:, :3].any()
    ones = t[where["ones"]]                                               # c0 == c1, every index 3
    assert not ones.any() if fmt in (71, 72) else (ones == 1).all()


@pytest.mark.parametrize("fmt", [77, 78, 80, 81, 83, 84])
def test_planted_alpha_layouts(oracle, fmt):
    """a0 > a1: eight ramp values; a0 <= a1: six, then the two constants (0 or -1, and 1). SNORM -128 decodes as -127."""
    _, where, t = _decoded(oracle, fmt)
    channels = [3] if fmt in (77, 78) else [0] if fmt in (80, 81) else [0, 1]
    low = -1.0 if fmt in (81, 84) else 0.0
    for c in channels:
        eight, six = t[where["a0>a1"]][:8, c], t[where["a0<=a1"]][:8, c]
        assert len(set(eight)) == 8 and eight[1] < eight[7] < eight[2] < eight[0]
        assert six[6] == low and six[7] == 1.0 and len(set(six[:6])) == 6 and six[0] < six[5] < six[1]
        if fmt in (81, 84):
            a, b = t[where["-128,127"]][:8, c], t[where["127,-128"]][:8, c]
            assert a[0] == -1.0 and a[1] == 1.0 and a[6] == -1.0 and a[7] == 1.0       # -128 <= 127: the six-value layout
            assert b[0] == 1.0 and b[1] == -1.0 and len(set(b)) == 8


@pytest.mark.parametrize("fmt", [98, 99])
def test_planted_bc7_modes(oracle, fmt):
    """The two images of the matrix (first = 0 and first = 8) hold every mode between them. Modes 0 - 3 have no alpha; the reserved
    block is transparent black."""
    seen = set()
    for first in (0, 8):
        blocks, where, t = _decoded(oracle, fmt, 8, first)
        for name, i in where.items():
            seen.add(name)
            if name.startswith("mode") and name != "mode-none":
                m = int(name[4:])
                assert blocks[i, 0] == 1 << m
                assert t[i].any()
                if m < 4:
                    assert (t[i][:, 3] == 1).all()
                else:
                    assert (t[i][:, 3] != 1).any() or (t[i][:, :3] != 1).any()
            elif name == "mode-none":
                assert blocks[i, 0] == 0 and not t[i].any()
    assert seen >= {f"mode{m}" for m in range(8)} | {"mode-none", "zero", "ones"}
    _, where, _ = _decoded(oracle, fmt, 275)
    assert len(where) == 11


@pytest.mark.parametrize("fmt", [95, 96])
def test_bc6h_modes_and_infinity(oracle, fmt):
    blocks, where, t = _decoded(oracle, fmt, 275)
    modes = [dc.bc6h_mode(b) for b in blocks]
    assert set(modes) >= dc.BC6H_VALID_MODES
    reserved = [i for i, m in enumerate(modes) if m not in dc.BC6H_VALID_MODES]
    assert reserved
    for i in reserved:
        assert np.array_equal(t[i], np.tile(np.float32([0, 0, 0, 1]), (16, 1)))
    assert np.isfinite(t[where["mode-bits-only"]]).all()
    if fmt == 96:
        for n in (8, 275):
            _, where, t = _decoded(oracle, fmt, n)
            assert np.isneginf(t[where["inf"]][:, 0]).all() and not t[where["inf"]][:, 1:3].any()
            enc = np.stack([t[where[f"encoded{i}"]] for i in range(4)])
            assert np.isfinite(enc).all() and (enc[..., :3] < 0).any() and np.abs(enc[3]).max() > 100
        assert np.isinf(t).sum() == 16                                   # 275 blocks: the random ones bring no infinity, it has to be planted


@pytest.mark.parametrize("src", dc.SOURCES)
def test_reference_is_repeatable(oracle, src):
    """DecompressBC twice on every pair and size of the matrix: the same bytes, and as many as the format's tight pitch says."""
    for w, h in dc.SIZES:
        blocks, _ = dc.payload(src, dc.blocks_of(w, h), oracle)
        for dst in dc.DESTS:
            a = oracle.ref_decompress_image(blocks, w, h, src, dst)
            b = oracle.ref_decompress_image(blocks, w, h, src, dst)
            assert a.nbytes == oracle.image_bytes(dst, w, h) and np.array_equal(a, b), (src, dst, (w, h))


def test_destination_list():
    """DESTS and the five grouped formats are exactly what the reference accepted when measured. Literal: no oracle call on the five."""
    assert len(dc.DESTS) == 61 and len(set(dc.DESTS)) == 61 and len(dc.SOURCES) == 14
    assert sorted(dc.DESTS + dc.GROUPED) == dc.REFERENCE_ACCEPTS and len(dc.REFERENCE_ACCEPTS) == 66
    assert not set(dc.DESTS) & set(dc.GROUPED) and not set(dc.REFERENCE_ACCEPTS) & (set(dc.BC_DESTS) | {dc.R1})
