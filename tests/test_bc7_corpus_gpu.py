"""The BC7 kernels on the corpus of tests/bc7_corpus.py, byte for byte against the reference encoder's payloads recorded in
tests/golden/bc7_corpus_{default,3subsets}.npz (tests/test_bc7_corpus_cpu.py keeps those equal to the live reference, and measures what the corpus
reaches: every partition of modes 0, 1, 2, 3 and 7, every rotation of modes 4 and 5, both index selectors of mode 4, mode 6 with and without alpha,
zero-error tiles, float sources off the 1/255 grid). The images of test_bc7_parity.py let half of mode 3's partitions win. Reads nothing of the
reference."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bc7_corpus as C  # noqa: E402

pytestmark = pytest.mark.gpu
BC7, BC7_SRGB, RGBA8, RGBA8_SRGB, BGRA8, RGBA32F = 98, 99, 28, 29, 87, 2
USE_3SUBSETS, QUICK = 0x80000, 0x100000
GOLDEN = {"default": os.path.join(ROOT, "tests", "golden", "bc7_corpus_default.npz"), "3subsets": os.path.join(ROOT, "tests", "golden", "bc7_corpus_3subsets.npz")}
FLAGS = {"default": 0, "3subsets": USE_3SUBSETS}
SETS = {"default": C.DEFAULT_SETS, "3subsets": C.THREE_SETS}
QUICK_SETS = C.DEFAULT_SETS + C.THREE_SETS
CROP_SET = {"default": "two_alpha", "3subsets": "three_opaque"}


@pytest.fixture(scope="module")
def tiles():
    t = C.corpus()
    for v in t.values():
        v.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def golden():
    out = {}
    for which, path in GOLDEN.items():
        with np.load(path) as z:
            for name in z.files:
                out[which, name] = z[name]
                out[which, name].setflags(write=False)
    return out


def _check(got, want, tag):
    g = np.asarray(got).reshape(-1, 16); r = np.asarray(want).reshape(-1, 16)
    assert g.shape == r.shape, f"{tag}: {g.shape} against {r.shape}"
    bad = np.nonzero((g != r).any(axis=1))[0]
    f = bad[:8]
    assert bad.size == 0, (f"{tag}: {bad.size} of {len(g)} blocks differ; first {f.tolist()}, modes gpu {C.mode_field(g[f]).tolist()} reference {C.mode_field(r[f]).tolist()}, "
                           f"partitions gpu {C.partition_field(g[f]).tolist()} reference {C.partition_field(r[f]).tolist()}, "
                           f"rotations gpu {C.rotation_field(g[f]).tolist()} reference {C.rotation_field(r[f]).tolist()}")


def _image_check(ctx, ts, want, src, dst, flags, tag, swap=False):
    img, w, h = C.as_image(ts)
    if swap:
        img = np.ascontiguousarray(img[:, :, [2, 1, 0, 3]])
    _check(ctx.compress(img, w, h, src, dst, flags, 0.5), C.image_payload(want, (w // 4) * (h // 4)), tag)


@pytest.mark.parametrize("which,name", [(w, s) for w in SETS for s in SETS[w]])
def test_corpus_through_the_block_hook(ctx, tiles, golden, which, name):
    _check(ctx.encode_blocks(BC7, C.floats(name, tiles[name]), FLAGS[which]), golden[which, name], f"{which} {name} encode_blocks")


def test_whole_corpus_quick_through_the_block_hook(ctx, tiles, golden):
    got = ctx.encode_blocks(BC7, np.concatenate([C.floats(name, tiles[name]) for name in QUICK_SETS]), QUICK)
    assert (C.mode_field(got) == 6).all()
    _check(got, golden["default", "quick"], "quick encode_blocks")


@pytest.mark.parametrize("name", ["two_opaque", "two_alpha"])
@pytest.mark.parametrize("src", [RGBA8, BGRA8])
def test_two_subset_images_through_compress(ctx, tiles, golden, name, src):
    """two_opaque is 256 x 192, the largest image of this file: the rough-error shortlists, the task lists and their sort with all 64 partitions live."""
    if name == "two_opaque":
        assert C.as_image(tiles[name])[1:] == (256, 192)
    _image_check(ctx, tiles[name], golden["default", name], src, BC7, 0, f"{name} compress from format {src}", swap=src == BGRA8)


def test_three_subset_image_through_compress(ctx, tiles, golden):
    _image_check(ctx, tiles["three_opaque"], golden["3subsets", "three_opaque"], RGBA8, BC7, USE_3SUBSETS, "three_opaque compress with 3SUBSETS")


def test_off_grid_image_from_float32(ctx, tiles, golden):
    """The bytes the encoder sees come from uint8(x * 255.0f + 0.01f) in unfused float32 on values a last bit away from the next byte. Compress
    saturates a float source first, so the image's payloads are not the block hook's: the golden file has an entry for it."""
    assert C.as_image(tiles["off_grid"])[1:] == (256, 16)
    _image_check(ctx, tiles["off_grid"], golden["default", "off_grid_image"], RGBA32F, BC7, 0, "off_grid compress from R32G32B32A32_FLOAT")


def test_srgb_image_gives_the_unorm_payload(ctx, tiles, golden):
    """R8G8B8A8_UNORM_SRGB -> BC7_UNORM_SRGB converts nothing: the payload is the UNORM one (asserted of the reference in test_bc7_corpus_cpu.py)."""
    _image_check(ctx, tiles["two_alpha"], golden["default", "two_alpha"], RGBA8_SRGB, BC7_SRGB, 0, "two_alpha compress sRGB to BC7_UNORM_SRGB")


def test_mixed_image_through_compress(ctx, tiles, golden):
    """vector_scalar + ramp_alpha + exact + grey_ramp_opaque in one submission: the early phases, the late modes 4 / 5 on the side streams and mode
    6's groups meet, next to tiles whose search ends at error 0."""
    ts = np.concatenate([tiles[s] for s in C.MIXED_SETS])
    want = np.concatenate([golden["default", s] for s in C.MIXED_SETS])
    _image_check(ctx, ts, want, RGBA8, BC7, 0, "mixed image")


@pytest.mark.parametrize("which", ["default", "3subsets"])
def test_partial_blocks(ctx, tiles, golden, which):
    """13 x 9 windows: the right and bottom blocks hold replicated texels."""
    for i, crop in enumerate(C.crops(tiles[CROP_SET[which]])):
        _check(ctx.compress(crop, C.CROP_W, C.CROP_H, RGBA8, BC7, FLAGS[which], 0.5), golden[which, "crops"][i], f"{which} crop {i} at {C.CROP_ORIGINS[i]}")


def test_image_twice_through_compress_many(ctx, tiles, golden):
    img, w, h = C.as_image(tiles["two_alpha"])
    outs = ctx.compress_many([img, img.copy()], w, h, RGBA8, BC7, 0, 0.5)
    assert len(outs) == 2
    for i, got in enumerate(outs):
        _check(got, C.image_payload(golden["default", "two_alpha"], (w // 4) * (h // 4)), f"two_alpha compress_many image {i}")
