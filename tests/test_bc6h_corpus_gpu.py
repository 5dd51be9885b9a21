"""The BC6H kernels on the corpus of tests/bc6h_corpus.py, byte for byte against the reference encoder's payloads recorded in
tests/golden/bc6h_corpus_{uf16,sf16}.npz (tests/test_bc6h_corpus_cpu.py keeps those equal to the live reference, and measures what the corpus
reaches: 13 modes and 32 shapes win blocks of `smooth`, mode 0x0F wins blocks of `tiny`, and on `near_top` / `bright` the SF16 search of the 16-bit
mode ends above 32767 in every state bc6h_encode.hip's Ep16 marks stand for). The images of test_bc6h_parity.py let two to six modes win."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bc6h_corpus as C  # noqa: E402

pytestmark = pytest.mark.gpu
UF16, SF16, RGBA16F, RGBA32F = 95, 96, 10, 2
GOLDEN = {UF16: os.path.join(ROOT, "tests", "golden", "bc6h_corpus_uf16.npz"), SF16: os.path.join(ROOT, "tests", "golden", "bc6h_corpus_sf16.npz")}
SETS = {UF16: ("smooth", "near_top", "bright", "tiny"), SF16: ("smooth", "smooth_signs", "near_top", "bright", "tiny")}
CROP_SET = {UF16: "smooth", SF16: "smooth_signs"}


@pytest.fixture(scope="module")
def tiles():
    t = C.corpus()
    for v in t.values():
        v.setflags(write=False)
    return t


@pytest.fixture(scope="module")
def golden():
    out = {}
    for fmt, path in GOLDEN.items():
        with np.load(path) as z:
            for name in z.files:
                out[fmt, name] = z[name]
                out[fmt, name].setflags(write=False)
    return out


def _check(got, want, tag):
    g = np.asarray(got).reshape(-1, 16); r = np.asarray(want).reshape(-1, 16)
    assert g.shape == r.shape, f"{tag}: {g.shape} against {r.shape}"
    bad = np.nonzero((g != r).any(axis=1))[0]
    assert bad.size == 0, (f"{tag}: {bad.size} of {len(g)} blocks differ; first {bad[:8].tolist()}, mode fields gpu {[hex(int(x)) for x in C.mode_field(g[bad[:8]])]} "
                           f"reference {[hex(int(x)) for x in C.mode_field(r[bad[:8]])]}")


def _no_new_0x0f(got, want, tag):
    """A wrapped 16-bit endpoint accepted as fitting would surface as a 16:4 block the reference does not emit."""
    g = C.mode_field(np.asarray(got).reshape(-1, 16)) == 0x0F; r = C.mode_field(np.asarray(want).reshape(-1, 16)) == 0x0F
    extra = np.nonzero(g & ~r)[0]
    assert extra.size == 0, f"{tag}: {extra.size} blocks are mode 0x0F on the GPU and not in the reference, first {extra[:8].tolist()}"


def _image(ts, dtype):
    img, w, h = C.as_image(ts)
    return img.astype(dtype), w, h


@pytest.mark.parametrize("fmt,name", [(f, s) for f in (UF16, SF16) for s in SETS[f]])
def test_corpus_through_the_block_hook(ctx, tiles, golden, fmt, name):
    got = ctx.encode_blocks(fmt, tiles[name], 0)
    _no_new_0x0f(got, golden[fmt, name], f"{fmt} {name} encode_blocks")
    _check(got, golden[fmt, name], f"{fmt} {name} encode_blocks")


@pytest.mark.parametrize("fmt,name,src", [(UF16, "smooth", RGBA16F), (SF16, "smooth", RGBA16F), (SF16, "smooth_signs", RGBA16F), (UF16, "smooth", RGBA32F), (SF16, "smooth_signs", RGBA32F)])
def test_smooth_image_through_compress(ctx, tiles, golden, fmt, name, src):
    """256 x 256: the task lists, the bin sort and the forked one-region stream with all three precision trios live in one launch."""
    img, w, h = _image(tiles[name], np.float16 if src == RGBA16F else np.float32)
    assert (w, h) == (256, 256)
    _check(ctx.compress(img, w, h, src, fmt, 0, 0.5), golden[fmt, name], f"{fmt} {name} compress from format {src}")


@pytest.mark.parametrize("fmt", [SF16, UF16])
def test_overflow_families_as_one_image(ctx, tiles, golden, fmt):
    """near_top + bright (+ tiny, whose 16:4 search ends in range and WINS) in one image: in SF16 the overflow marks travel through the task records next
    to ordinary tasks; in UF16 the marks must be inert."""
    ts = np.concatenate([tiles["near_top"], tiles["bright"], tiles["tiny"]])
    want = np.concatenate([golden[fmt, "near_top"], golden[fmt, "bright"], golden[fmt, "tiny"]])
    img, w, h = _image(ts, np.float16)
    got = ctx.compress(img, w, h, RGBA16F, fmt, 0, 0.5)
    want = C.image_payload(want, (w // 4) * (h // 4))
    _no_new_0x0f(got, want, f"{fmt} overflow image")
    _check(got, want, f"{fmt} overflow image")
    top = len(tiles["near_top"]) + len(tiles["bright"])
    assert not (C.mode_field(np.asarray(got).reshape(-1, 16)[:top]) == 0x0F).any()          # (the reference has none there: test_bc6h_corpus_cpu.py)


@pytest.mark.parametrize("fmt", [UF16, SF16])
def test_partial_blocks_of_the_smooth_image(ctx, tiles, golden, fmt):
    """13 x 9 windows: the right and bottom blocks hold replicated texels."""
    for i, crop in enumerate(C.crops(tiles[CROP_SET[fmt]])):
        _check(ctx.compress(crop, C.CROP_W, C.CROP_H, RGBA16F, fmt, 0, 0.5), golden[fmt, "crops"][i], f"{fmt} crop {i} at {C.CROP_ORIGINS[i]}")


@pytest.mark.parametrize("fmt,name", [(UF16, "smooth"), (SF16, "smooth_signs")])
def test_smooth_image_twice_through_compress_many(ctx, tiles, golden, fmt, name):
    img, w, h = _image(tiles[name], np.float16)
    outs = ctx.compress_many([img, img.copy()], w, h, RGBA16F, fmt, 0, 0.5)
    assert len(outs) == 2
    for i, got in enumerate(outs):
        _check(got, golden[fmt, name], f"{fmt} {name} compress_many image {i}")
