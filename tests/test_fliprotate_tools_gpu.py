"""dxtexconv --horizontal-flip / --vertical-flip end to end, on files oracle.ref_save_dds wrote, against the restatement
(tests/fliprotate_ref.py): the flipped file, the step's place before the mip chain (the levels are the oracle's mips OF THE FLIPPED image),
and the end of a BC hand-through (the oracle's compression of the flipped decompressed image, not the input's blocks)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fliprotate_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
EXE = os.path.join(ROOT, "directxtex_amd", "lib", "dxtexconv")
RGBA8, BC1 = 28, 71


def _conv(args, ok=True):
    r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout + r.stderr


def _flipped(px, w, h, flags):
    return R.flip_rotate(np.asarray(px, np.uint8).reshape(h, w, 4), flags).reshape(-1)


@pytest.mark.parametrize("opts,flags", [(["--horizontal-flip"], R.FLIP_HORIZONTAL), (["--vertical-flip"], R.FLIP_VERTICAL),
                                        (["--horizontal-flip", "--vertical-flip"], R.FLIP_HORIZONTAL | R.FLIP_VERTICAL)], ids=("h", "v", "hv"))
def test_flipped_file(tmp_path, oracle, opts, flags):
    w, h = 37, 21
    px = np.random.default_rng(flags).integers(0, 256, w * h * 4, dtype=np.uint8)
    src, out = tmp_path / "s.dds", tmp_path / "o.dds"
    oracle.ref_save_dds(px, w, h, RGBA8).tofile(src)
    _conv([*opts, "-f", "R8G8B8A8_UNORM", "-m", "1", "-o", out, src])
    want = _flipped(px, w, h, flags)
    meta, got = oracle.ref_load_dds(np.fromfile(out, np.uint8))
    assert (meta["width"], meta["height"], meta["format"], meta["mipLevels"]) == (w, h, RGBA8, 1)
    assert np.array_equal(np.asarray(got, np.uint8), want)
    assert np.array_equal(np.fromfile(out, np.uint8), oracle.ref_save_dds(want, w, h, RGBA8))


def test_mips_are_made_from_the_flipped_image(tmp_path, oracle):
    w, h, levels = 37, 21, 6
    px = np.random.default_rng(40).integers(0, 256, w * h * 4, dtype=np.uint8)
    src, out = tmp_path / "s.dds", tmp_path / "o.dds"
    oracle.ref_save_dds(px, w, h, RGBA8).tofile(src)
    _conv(["--horizontal-flip", "--vertical-flip", "-f", "R8G8B8A8_UNORM", "-o", out, src])
    flipped = _flipped(px, w, h, R.FLIP_HORIZONTAL | R.FLIP_VERTICAL)
    want = np.concatenate(oracle.ref_generate_mips(flipped, w, h, RGBA8, 0, levels))
    meta, got = oracle.ref_load_dds(np.fromfile(out, np.uint8))
    assert (meta["width"], meta["height"], meta["format"], meta["mipLevels"]) == (w, h, RGBA8, levels)
    assert np.array_equal(np.asarray(got, np.uint8), want)
    assert np.array_equal(np.fromfile(out, np.uint8), oracle.ref_save_dds(want, w, h, RGBA8, 1, levels))
    # the order shows: an odd side is not halved symmetrically, so the flipped levels of the unflipped image are another chain
    other = [_flipped(m, mw, mh, R.FLIP_HORIZONTAL | R.FLIP_VERTICAL) for m, (mw, mh) in zip(oracle.ref_generate_mips(px, w, h, RGBA8, 0, levels), oracle.mip_sizes(w, h, levels))]
    assert not np.array_equal(np.concatenate(other), want)


def test_flip_ends_the_bc1_hand_through(tmp_path, oracle):
    w, h = 32, 24
    rgba = np.random.default_rng(41).integers(0, 256, w * h * 4, dtype=np.uint8)
    bc = oracle.ref_compress_image(rgba, w, h, RGBA8, BC1, 0, 0.5)
    src, out = tmp_path / "b.dds", tmp_path / "o.dds"
    oracle.ref_save_dds(bc, w, h, BC1).tofile(src)
    # without a flip the blocks are handed through
    _conv(["-f", "BC1_UNORM", "-m", "1", "-o", out, src])
    assert np.array_equal(np.asarray(oracle.ref_load_dds(np.fromfile(out, np.uint8))[1], np.uint8), bc)
    _conv(["--vertical-flip", "-f", "BC1_UNORM", "-m", "1", "-y", "-o", out, src])
    dec = oracle.ref_decompress_image(bc, w, h, BC1, RGBA8)
    want = oracle.ref_compress_image(_flipped(dec, w, h, R.FLIP_VERTICAL), w, h, RGBA8, BC1, 0, 0.5)
    meta, got = oracle.ref_load_dds(np.fromfile(out, np.uint8))
    assert meta["format"] == BC1 and np.array_equal(np.asarray(got, np.uint8), want) and not np.array_equal(np.asarray(got, np.uint8), bc)


def test_short_names_stay_refused(tmp_path):
    for short in ("-hflip", "-vflip"):
        txt = _conv([short, "-o", tmp_path / "o.dds", tmp_path / "none.dds"], ok=False)
        assert "usage: dxtexconv" in txt
