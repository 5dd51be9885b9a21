"""BC7: blocks of a pass with the same sixteen texels are encoded once (bc7_dedupe_insert_kernel / bc7_dedupe_resolve_kernel, DESIGN.md
section 4.2) and every payload stays what it was, byte for byte. The base image is 64 x 64 (256 blocks) laid out from 40 distinct 4 x 4
tiles - one-colour tiles, two-colour tiles that share words with them, noise, tiles with alpha below 255 - so that copies sit next to
each other in a row, in the next block row and at opposite corners. The development build runs in processes of its own: with the dedupe
on, with it off (DXTEX_BC7_NO_DEDUPE), with the hash cut to two bits so that unequal blocks collide and only the texel comparison tells
them apart (DXTEX_BC7_DEDUPE_HASH_BITS), and with 64 blocks a pass. Every run must give the same bytes, and the duplicates it reports
(DXTEX_BC7_STATS) must be numpy's: blocks minus distinct tiles, per pass."""
import functools
import hashlib
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import directxtex_amd as dx
from directxtex_amd import synth

pytestmark = pytest.mark.gpu
BC7 = dx.DXGI_FORMAT_BC7_UNORM
RGBA8 = dx.DXGI_FORMAT_R8G8B8A8_UNORM
BGRA8 = dx.DXGI_FORMAT_B8G8R8A8_UNORM
FLAGS = (0, dx.TEX_COMPRESS_BC7_QUICK, 0x80000)          # default, mode 6 only, BC7_USE_3SUBSETS


def _tiles():
    """40 distinct 4 x 4 RGBA8 tiles."""
    rng = np.random.default_rng(801)
    words = rng.integers(0, 256, (10, 4), dtype=np.uint8)
    words[:, 3] = 255
    tiles = [np.broadcast_to(w, (4, 4, 4)).copy() for w in words]                         # 10 one-colour tiles
    for k in range(10):                                                                   # 10 two-colour tiles; the first colour is a one-colour tile's word
        t = np.broadcast_to(words[k % 4], (4, 4, 4)).copy()
        m = rng.integers(0, 2, (4, 4)).astype(bool)
        m[0, 0], m[3, 3] = False, True
        other = rng.integers(0, 256, 4, dtype=np.uint8); other[3] = 255
        t[m] = other
        tiles.append(t)
    for k in range(12):                                                                   # 12 noisy opaque tiles
        t = rng.integers(0, 256, (4, 4, 4), dtype=np.uint8); t[:, :, 3] = 255
        tiles.append(t)
    for k in range(8):                                                                    # 8 tiles with alpha below 255: one colour, two alphas, noise
        if k < 2:
            t = np.broadcast_to(np.append(words[k][:3], np.uint8(40 + 90 * k)), (4, 4, 4)).copy()
        elif k < 5:
            t = np.broadcast_to(words[k], (4, 4, 4)).copy()
            t[rng.integers(0, 2, (4, 4)).astype(bool) | np.eye(4, dtype=bool), 3] = 17 * k
        else:
            t = rng.integers(0, 256, (4, 4, 4), dtype=np.uint8)
        tiles.append(t)
    assert len(tiles) == 40 and len({t.tobytes() for t in tiles}) == 40
    return tiles


def _base_image():
    tiles = _tiles()
    rng = np.random.default_rng(802)
    which = rng.integers(0, 40, (16, 16))
    which[3:15].reshape(-1)[rng.permutation(192)[:40]] = np.arange(40)  # every tile somewhere
    which[0] = np.repeat(np.arange(8), 2)                               # copies next to each other in a row ...
    which[1] = which[0]                                                 # ... and in the next block row
    which[2] = np.arange(24, 40)
    which[15, 15], which[15, 0] = which[0, 0], 39                       # ... and at opposite corners
    which[0, 15] = 39
    img = np.zeros((64, 64, 4), np.uint8)
    for by in range(16):
        for bx in range(16):
            img[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] = tiles[which[by, bx]]
    return img


def _partial_image():
    """30 x 22, one flat colour and a noisy corner: the replicated texels of the edge blocks make them equal to interior ones."""
    img = np.empty((22, 30, 4), np.uint8)
    img[:] = (90, 140, 200, 255)
    img[:7, :6] = np.random.default_rng(803).integers(0, 256, (7, 6, 4), dtype=np.uint8)
    return img


@functools.lru_cache(maxsize=None)
def _images():
    imgs = {
        "base": _base_image(),
        "partial-30x22": _partial_image(),
        "no-duplicates": np.ascontiguousarray(synth.survey_rgba8(64, 64, 2, "random")).reshape(64, 64, 4),
    }
    for v in imgs.values():
        v.setflags(write=False)
    return imgs


def _block_keys(img):
    """The sixteen texels Encode reads per block, in block order, with the reference's partial-block replication (replicate_src)."""
    h, w = img.shape[:2]

    def axis(n):
        idx = []
        for b in range((n + 3) // 4):
            ext = min(4, n - b * 4)
            idx.append([b * 4 + (s if s < ext else (1 if s == 3 and ext > 1 else 0)) for s in range(4)])
        return np.array(idx)
    ys, xs = axis(h), axis(w)
    return [img[np.ix_(ys[by], xs[bx])].tobytes() for by in range(len(ys)) for bx in range(len(xs))]


def _duplicates(keys, per_pass=None):
    """numpy's count, per pass of `per_pass` consecutive blocks: blocks minus distinct keys."""
    per_pass = per_pass or len(keys)
    return [len(keys[i:i + per_pass]) - len(set(keys[i:i + per_pass])) for i in range(0, len(keys), per_pass)]


def test_the_images_are_what_the_cases_need():
    base = _block_keys(_images()["base"])
    assert len(base) == 256 and len(set(base)) == 40
    assert base[0] == base[1] == base[16] == base[255] and base[15] == base[240]      # in a row, next block row, opposite corners
    assert all(n > 0 for n in _duplicates(base, 64))
    part = _block_keys(_images()["partial-30x22"])
    flat = bytes((90, 140, 200, 255)) * 16
    assert len(part) == 48 and part[7] == part[47] == part[20] == flat                # right edge, bottom-right corner, interior
    assert _duplicates(_block_keys(_images()["no-duplicates"])) == [0]


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _dev_run(env_items):
    """Every case through the development build in one process of its own. Per payload a line `payload NAME FLAGS SHA256`, preceded by the
    `bc7 stats dedupe` lines of its passes. Returns {(name, flags): (sha, [duplicates per pass], [blocks per pass])}."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)
        import numpy as np, torch, directxtex_amd as dx
        import test_bc7_block_dedupe_gpu as t
        dx.capi.load(dev=True)          # only the -DDXTEX_DEV build reads knobs
        c = dx.Context(0)
        def say(name, flags, payload):
            sys.stderr.flush()
            print("payload", name, hex(flags), t._sha(payload), flush=True)
        for name, im in t._images().items():
            for flags in (t.FLAGS if name == "base" else (0,)):
                say(name, flags, c.compress(im, im.shape[1], im.shape[0], t.RGBA8, t.BC7, flags, 0.5))
        # one submission of three images: the base image twice, and once more as B8G8R8A8 with the channels arranged to the same values
        dev = torch.device("cuda", 0)
        base = t._images()["base"]
        bgra = np.ascontiguousarray(base[:, :, [2, 1, 0, 3]])
        say("base-as-bgra", 0, c.compress(bgra, 64, 64, t.BGRA8, t.BC7, 0, 0.5))
        pix = [base, base, bgra]; fmts = [t.RGBA8, t.RGBA8, t.BGRA8]
        src_t = [torch.from_numpy(p.reshape(-1).copy()).to(dev) for p in pix]
        dst_t = [torch.zeros(dx.compute_pitch(t.BC7, 64, 64)[1], dtype=torch.uint8, device=dev) for _ in pix]
        srcs = [dx.capi.device_image(s.data_ptr(), 64, 64, f) for s, f in zip(src_t, fmts)]
        dsts = [dx.capi.device_image(d.data_ptr(), 64, 64, t.BC7) for d in dst_t]
        c.compress_many_device(srcs, dsts, 0, 0.5)
        torch.cuda.synchronize()
        for i, d in enumerate(dst_t):
            say("many-%%d" %% i, 0, d.cpu().numpy())
        c.close()
    """ % (root, os.path.join(root, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DXTEX_BC7_STATS="1", **dict(env_items)), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    out, dups, blocks = {}, [], []
    for line in r.stdout.splitlines():
        m = re.match(r"bc7 stats dedupe: (\d+) of (\d+) blocks are duplicates", line)
        if m:
            dups.append(int(m.group(1))); blocks.append(int(m.group(2)))
        elif line.startswith("payload "):
            _, name, flags, sha = line.split()
            if not name.startswith("many-") or name == "many-0":
                out[(name, int(flags, 16))] = (sha, dups, blocks)
                dups, blocks = [], []
            else:
                out[(name, int(flags, 16))] = (sha, [], [])
    assert len(out) == 9, r.stdout[-3000:]
    return out


def _run(**env):
    return _dev_run(tuple(sorted(env.items())))


def _shas(run):
    return {k: v[0] for k, v in run.items()}


_refs = {}


def _ref_sha(oracle, flags):
    if flags not in _refs:
        _refs[flags] = _sha(oracle.ref_compress_image(_images()["base"], 64, 64, RGBA8, BC7, flags, 0.5))
    return _refs[flags]


def test_bytes_and_count(oracle):
    """Dedupe on against dedupe off and against the reference, at the three flag settings; the count is numpy's."""
    on, off = _run(), _run(DXTEX_BC7_NO_DEDUPE="1")
    print("duplicates reported:", {k: v[1] for k, v in on.items()})
    assert _shas(on) == _shas(off)
    for flags in FLAGS:
        assert on[("base", flags)][0] == _ref_sha(oracle, flags), hex(flags)
        assert on[("base", flags)][1:] == ([256 - 40], [256]), hex(flags)
        assert off[("base", flags)][1:] == ([0], [256]), hex(flags)


def test_forced_collisions():
    """Two bits of hash: four leaders at most, every other block meets a leader it is not equal to and must be encoded normally."""
    on, cut = _run(), _run(DXTEX_BC7_DEDUPE_HASH_BITS="2")
    assert _shas(cut) == _shas(on)
    for flags in FLAGS:
        n = cut[("base", flags)][1]
        assert len(n) == 1 and 0 < n[0] < 256 - 40, (hex(flags), n)        # the first block always leads, and its copies are found


def test_several_passes():
    """64 blocks a pass: copies fall into different passes and pair up only inside one."""
    on, cut = _run(), _run(DXTEX_MAX_BLOCKS_PER_PASS="64")
    assert _shas(cut) == _shas(on)
    per_pass = _duplicates(_block_keys(_images()["base"]), 64)
    for flags in FLAGS:
        assert cut[("base", flags)][1:] == (per_pass, [64] * 4), hex(flags)


def test_partial_blocks(oracle):
    on, off = _run(), _run(DXTEX_BC7_NO_DEDUPE="1")
    key = ("partial-30x22", 0)
    img = _images()["partial-30x22"]
    assert on[key][0] == off[key][0] == _sha(oracle.ref_compress_image(img, 30, 22, RGBA8, BC7, 0, 0.5))
    assert on[key][1:] == (_duplicates(_block_keys(img)), [48])
    assert on[key][1][0] >= 30           # the flat blocks, edge blocks among them


def test_compress_many():
    """The same content twice, and once more as B8G8R8A8, in one submission: blocks pair up across the images (same float texels), and every
    payload is that image's encoded alone."""
    on, off = _run(), _run(DXTEX_BC7_NO_DEDUPE="1")
    alone = on[("base", 0)][0]
    assert on[("base-as-bgra", 0)][0] == off[("base-as-bgra", 0)][0]
    for run in (on, off):
        assert run[("many-0", 0)][0] == alone and run[("many-1", 0)][0] == alone
        assert run[("many-2", 0)][0] == run[("base-as-bgra", 0)][0]
    assert on[("many-0", 0)][1:] == ([3 * 256 - 40], [3 * 256])


def test_no_duplicates():
    on, off = _run(), _run(DXTEX_BC7_NO_DEDUPE="1")
    key = ("no-duplicates", 0)
    assert on[key][0] == off[key][0]
    assert on[key][1:] == ([0], [256])
