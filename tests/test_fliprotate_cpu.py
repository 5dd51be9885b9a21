"""FlipRotate without a GPU: the host build of dxtex_fliprotate.h (directxtex_amd/lib/fliprotate_check) against the numpy restatement
(tests/fliprotate_ref.py). The source coordinate of every destination texel, the eight classes of the fifteen flag words, the refusal of
illegal words, and a walk over the launch geometry of both kernels that moves the bytes as they do: the destination must equal the
restatement, every byte of a destination texel must have been written exactly once and no other byte at all (the program itself fails on
an access outside a row's texels, a misaligned one, and an LDS read of something the tile did not store)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fliprotate_ref as R  # noqa: E402
LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK = os.path.join(LIB, "fliprotate_check")

# source shapes (w, h): the degenerate ones, two small ones, and one that spans two tiles with ragged edges in both directions for both
# tile sides (64 up to 4-byte texels, 32 above)
SHAPES = ((1, 1), (1, 5), (5, 1), (3, 2), (7, 5), (70, 37))
TEXELS = (1, 2, 4, 8, 12, 16)
ROUTE_WIDE, ROUTE_NARROW, ROUTE_TILE = 0, 1, 2


def check(*args):
    if not os.path.exists(CHECK):
        pytest.fail("directxtex_amd/lib/fliprotate_check is missing: run build()")
    r = subprocess.run([CHECK, *[str(a) for a in args]], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stderr)
    return r.stdout


def test_restatement_is_the_per_texel_form():
    """The numpy lines against the per-texel form the issue and include/dxtex_amd.h give, written out here once more."""
    for (w, h) in SHAPES[:5]:
        for f in R.LEGAL:
            got = R.source_coords(w, h, f)
            W, H = (h, w) if f & 1 else (w, h)
            assert got.shape == (H, W, 2)
            for yd in range(H):
                for xd in range(W):
                    x1 = W - 1 - xd if f & 8 else xd
                    y1 = H - 1 - yd if f & 16 else yd
                    want = ((x1, y1), (y1, h - 1 - x1), (w - 1 - x1, h - 1 - y1), (w - 1 - y1, x1))[f & 3]
                    assert tuple(got[yd, xd]) == want, (w, h, f, xd, yd)


@pytest.mark.parametrize("shape", SHAPES)
def test_source_coordinates(shape):
    w, h = shape
    lines = check("coords", w, h).splitlines()
    assert len(lines) == 2 * len(R.LEGAL)
    for i, f in enumerate(R.LEGAL):
        head = [int(v) for v in lines[2 * i].split()]
        want = R.source_coords(w, h, f)
        assert head == [f, want.shape[1], want.shape[0]]
        got = np.array(lines[2 * i + 1].split(), np.int64).reshape(want.shape)
        assert np.array_equal(got, want), (shape, f)


def test_fifteen_words_eight_classes():
    rows = [tuple(int(v) for v in line.split()) for line in check("classes").splitlines()]
    assert tuple(r[0] for r in rows) == R.LEGAL and len(rows) == 15
    groups = {}
    for f, t, mx, my in rows:
        assert t == (f & 1)
        groups.setdefault((t, mx, my), set()).add(f)
    assert sorted(map(sorted, groups.values())) == sorted(map(sorted, R.CLASSES))
    assert groups[(0, 0, 0)] == {26}
    # and the restatement agrees that the words of a class are one operation
    src = np.arange(7 * 5).reshape(5, 7)
    for cls in R.CLASSES:
        res = [R.flip_rotate(src, f) for f in sorted(cls)]
        assert all(np.array_equal(res[0], r) for r in res)
    assert len({R.flip_rotate(src, min(c)).tobytes() + bytes(R.flip_rotate(src, min(c)).shape) for c in R.CLASSES}) == 8


def test_illegal_flags_refused():
    out = dict(tuple(int(v) for v in line.split()) for line in check("legal", *R.ILLEGAL, *R.LEGAL).splitlines())
    assert all(out[f] == 0 for f in R.ILLEGAL) and all(out[f] == 1 for f in R.LEGAL)
    assert all(not R.legal(f) for f in R.ILLEGAL)


def source_bytes(n):
    return (((np.arange(n, dtype=np.uint64) & 0xFFFFFFFF) * 2654435761 & 0xFFFFFFFF) >> 13).astype(np.uint8)


def walk(tmp_path, w, h, texel, src_pad, dst_pad, src_shift, dst_shift, flags):
    """-> (route, access, destination bytes, write counts, expected bytes, mask of the bytes that belong to texels)"""
    W, H = (h, w) if flags & 1 else (w, h)
    sp, dp = w * texel + src_pad, W * texel + dst_pad
    out = str(tmp_path / "out.bin")
    route, access, gx, gy = (int(v) for v in check("walk", w, h, texel, sp, dp, src_shift, dst_shift, flags, out).split())
    raw = np.fromfile(out, np.uint8)
    assert raw.size == 2 * H * dp
    want = R.expected(np.zeros(H * dp, np.uint8), dp, source_bytes(h * sp), w, h, texel, sp, flags)
    mask = np.zeros((H, dp), np.uint8)
    mask[:, :W * texel] = 1
    return route, access, raw[:H * dp], raw[H * dp:], want, mask.reshape(-1)


@pytest.mark.parametrize("texel", TEXELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_walk_writes_every_texel_once(tmp_path, shape, texel):
    w, h = shape
    for f in R.LEGAL:
        # everything aligned and tight; pitches padded by 3, which leaves nothing aligned; aligned pitches from shifted addresses
        for (src_pad, dst_pad, ss, ds) in ((0, 0, 0, 0), (3, 3, 0, 0), (16, 32, 4, 8)):
            route, access, got, count, want, mask = walk(tmp_path, w, h, texel, src_pad, dst_pad, ss, ds, f)
            assert np.array_equal(count, mask), (shape, texel, f, src_pad)
            assert np.array_equal(got, want), (shape, texel, f, src_pad)
            assert (route == ROUTE_TILE) == bool(f & 1)
            assert texel % access == 0


def test_routes(tmp_path):
    """The route choice: wide needs every row start and the row's byte count on 16 bytes and a texel that is not 12 bytes."""
    tmp = tmp_path
    for texel in TEXELS:
        route, access, *_ = walk(tmp, 128, 48, texel, 0, 0, 0, 0, R.FLIP_HORIZONTAL)
        assert route == (ROUTE_NARROW if texel == 12 else ROUTE_WIDE)
        assert access == (4 if texel == 12 else texel)
        route, access, *_ = walk(tmp, 128, 48, texel, 3, 3, 0, 0, R.FLIP_HORIZONTAL)
        assert (route, access) == (ROUTE_NARROW, 1)
        route, access, *_ = walk(tmp, 128, 48, texel, 0, 0, 4, 0, R.FLIP_VERTICAL)
        assert route == ROUTE_NARROW and access == min(4, texel)
        route, access, *_ = walk(tmp, 128, 1, texel, 3, 5, 0, 0, R.ROTATE180)                 # one row: the pitches do not matter
        assert route == (ROUTE_NARROW if texel == 12 else ROUTE_WIDE)
        route, access, *_ = walk(tmp, 48, 40, texel, 0, 0, 0, 0, R.ROTATE90)
        assert (route, access) == (ROUTE_TILE, 4 if texel == 12 else texel)
        route, access, *_ = walk(tmp, 48, 40, texel, 3, 0, 0, 0, R.ROTATE270)
        assert (route, access) == (ROUTE_TILE, 1)


def test_dxtexconv_takes_the_long_names(tmp_path):
    """--horizontal-flip / --vertical-flip are options dxtexconv knows (a usage error exits before -info reads the file)."""
    import oracle
    exe = os.path.join(LIB, "dxtexconv")
    if not os.path.exists(exe):
        pytest.fail("directxtex_amd/lib/dxtexconv is missing: run build()")
    path = tmp_path / "x.dds"
    oracle.ref_save_dds(np.arange(32, dtype=np.uint8), 4, 2, 28).tofile(str(path))
    r = subprocess.run([exe, "--horizontal-flip", "--vertical-flip", "-info", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    for short in ("-hflip", "-vflip"):
        r = subprocess.run([exe, short, "-info", str(path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0
