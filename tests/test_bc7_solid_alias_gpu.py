"""BC7: one-colour subsets of a block are searched once (bc7_pre_kernel's election) and every payload stays the
reference's, byte for byte. The images are made of what the election acts on: blocks of one colour (a quarter of them values mode 6
encodes exactly, so Encode's early return runs), blocks of two colours split along partition shapes and at random, flat blocks next to
noisy ones in one wavefront of the pre kernel, and partial blocks whose replicated texels make one-colour subsets. The development
build must give the same bytes with the election off (DXTEX_BC7_NO_ALIAS) and must report that it aliased tasks with it on."""
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
FLAGS = (0, dx.TEX_COMPRESS_BC7_USE_3SUBSETS)
# kPart2Mask (directxtex_amd/csrc/bc67_tables.h) of shapes 0, 1, 13 and 33: bit y * 4 + x set = texel in subset 1
SHAPE_MASKS = (0xCCCC, 0x8888, 0xFF00, 0xF0F0)


def _mask_block(mask):
    return np.array([(mask >> i) & 1 for i in range(16)], dtype=bool).reshape(4, 4)


def _solid_value(rng, alpha, exact6):
    """A random RGBA8 value with the given alpha (None: opaque). exact6: one that mode 6 encodes exactly - its endpoints carry seven bits and
    one p-bit shared by the four channels, so Unquantize(Quantize(v)) == v for every value whose channels have the parity of its alpha."""
    a = 255 if alpha is None else alpha
    v = rng.integers(0, 256, 3)
    if exact6:
        v = (v & 0xFE) | (a & 1)
    return np.array([v[0], v[1], v[2], a], dtype=np.uint8)


def _solid_image(alpha):
    rng = np.random.default_rng(101 if alpha is None else 102)
    img = np.zeros((64, 64, 4), np.uint8)
    for by in range(16):
        for bx in range(16):
            img[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] = _solid_value(rng, alpha, (by * 16 + bx) % 4 == 0)
    return img


def _two_colour_block(rng, k):
    """k even: split along one of SHAPE_MASKS or its complement; k odd: texel by texel at random (both colours present)."""
    c0, c1 = _solid_value(rng, None, False), _solid_value(rng, None, False)
    if k % 2 == 0:
        m = _mask_block(SHAPE_MASKS[(k // 2) % 4])
        if (k // 8) % 2:
            m = ~m
    else:
        m = rng.integers(0, 2, (4, 4)).astype(bool)
        m[0, 0], m[3, 3] = False, True
    return np.where(m[:, :, None], c1, c0).astype(np.uint8)


def _two_colour_image():
    rng = np.random.default_rng(103)
    img = np.zeros((64, 64, 4), np.uint8)
    for k in range(256):
        by, bx = divmod(k, 16)
        img[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] = _two_colour_block(rng, k)
    return img


def _mixed_image():
    """64 x 32: one-colour, two-colour and noise blocks alternating in x, so that every pair of kinds shares a wavefront of the pre kernel
    (two blocks per wavefront in the two-subset modes)."""
    rng = np.random.default_rng(104)
    img = np.zeros((32, 64, 4), np.uint8)
    for by in range(8):
        for bx in range(16):
            kind = bx % 3
            if kind == 0:
                blk = np.broadcast_to(_solid_value(rng, None if by % 2 else 77, False), (4, 4, 4))
            elif kind == 1:
                blk = _two_colour_block(rng, by * 16 + bx)
            else:
                blk = rng.integers(0, 256, (4, 4, 4), dtype=np.uint8)
                blk[:, :, 3] = 255 if by % 2 else blk[:, :, 3]
            img[by * 4:by * 4 + 4, bx * 4:bx * 4 + 4] = blk
    return img


@functools.lru_cache(maxsize=None)
def _images():
    imgs = {
        "solid-opaque": _solid_image(None),
        "solid-alpha128": _solid_image(128),
        "two-colour": _two_colour_image(),
        "mixed": _mixed_image(),
        "partial-13x9": np.ascontiguousarray(synth.rgba8(13, 9, seed=31, alpha="opaque")).reshape(9, 13, 4),
        "partial-5x5": np.ascontiguousarray(synth.rgba8(5, 5, seed=32, alpha="smooth")).reshape(5, 5, 4),
    }
    for v in imgs.values():
        v.setflags(write=False)
    return imgs


CASES = ("solid-opaque", "solid-alpha128", "two-colour", "mixed", "partial-13x9", "partial-5x5")
_refs = {}


def _ref(oracle, name, flags):
    """The reference's payload, computed once per (image, flags) and shared by the tests below."""
    if (name, flags) not in _refs:
        img = _images()[name]
        h, w = img.shape[:2]
        r = oracle.ref_compress_image(img, w, h, RGBA8, BC7, flags, 0.5)
        r.setflags(write=False)
        _refs[(name, flags)] = r
    return _refs[(name, flags)]


def _differing(got, ref):
    g = np.asarray(got).reshape(-1, 16); r = np.asarray(ref).reshape(-1, 16)
    return np.nonzero((g != r).any(axis=1))[0]


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", CASES)
def test_payload_is_the_reference_s(ctx, oracle, name, flags):
    img = _images()[name]
    h, w = img.shape[:2]
    got = ctx.compress(img, w, h, RGBA8, BC7, flags, 0.5)
    bad = _differing(got, _ref(oracle, name, flags))
    assert bad.size == 0, f"{name} flags {flags:#x}: {bad.size} blocks differ, first {bad[:8]}"


@pytest.mark.parametrize("flags", FLAGS)
def test_one_submission_of_several_images(ctx, oracle, flags):
    """The 64 x 64 and 64 x 32 images as one dxtex_compress_many_device submission: one block list, the election per block of it."""
    import torch
    dev = torch.device("cuda", 0)
    names = ("solid-opaque", "solid-alpha128", "two-colour", "mixed")
    imgs = [_images()[n] for n in names]
    src_t = [torch.from_numpy(im.reshape(-1).copy()).to(dev) for im in imgs]
    dst_t = [torch.zeros(dx.compute_pitch(BC7, im.shape[1], im.shape[0])[1], dtype=torch.uint8, device=dev) for im in imgs]
    srcs = [dx.capi.device_image(t.data_ptr(), im.shape[1], im.shape[0], RGBA8) for t, im in zip(src_t, imgs)]
    dsts = [dx.capi.device_image(t.data_ptr(), im.shape[1], im.shape[0], BC7) for t, im in zip(dst_t, imgs)]
    ctx.compress_many_device(srcs, dsts, flags, 0.5)
    torch.cuda.synchronize()
    for n, t in zip(names, dst_t):
        bad = _differing(t.cpu().numpy(), _ref(oracle, n, flags))
        assert bad.size == 0, f"{n} flags {flags:#x} in one submission: {bad.size} blocks differ, first {bad[:8]}"


def _dev_run(env):
    """The one- and two-colour images through the development build in a process of its own: per image and flags a line `image NAME FLAGS
    SHA256`, preceded by the `bc7 stats` lines of its launches (DXTEX_BC7_STATS)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r)
        import numpy as np, directxtex_amd as dx
        import test_bc7_solid_alias_gpu as t
        dx.capi.load(dev=True)          # only the -DDXTEX_DEV build reads knobs
        c = dx.Context(0)
        for name in ("solid-opaque", "solid-alpha128", "two-colour"):
            im = t._images()[name]
            for flags in t.FLAGS:
                out = c.compress(im, im.shape[1], im.shape[0], t.RGBA8, t.BC7, flags, 0.5)
                sys.stderr.flush()
                print("image", name, hex(flags), hashlib.sha256(out.tobytes()).hexdigest(), flush=True)
        c.close()
    """ % (root, os.path.join(root, "tests")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DXTEX_BC7_STATS="1", **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    shas, aliased, cur = {}, {}, {}
    for line in r.stdout.splitlines():
        m = re.match(r"bc7 stats bc7_pre_mode(\d)\s.*?(\d+) aliased", line)
        if m:
            cur[int(m.group(1))] = cur.get(int(m.group(1)), 0) + int(m.group(2))
        elif line.startswith("image "):
            _, name, flags, sha = line.split()
            shas[(name, flags)] = sha
            aliased[(name, flags)] = cur
            cur = {}
    assert len(shas) == 6, r.stdout[-3000:]
    return shas, aliased


def test_election_off_gives_the_same_bytes_and_on_it_aliases(oracle):
    on_sha, on_aliased = _dev_run({})
    off_sha, off_aliased = _dev_run({"DXTEX_BC7_NO_ALIAS": "1"})
    print("aliased tasks per image and mode:", on_aliased)
    assert on_sha == off_sha
    for (name, flags), sha in on_sha.items():
        assert sha == hashlib.sha256(_ref(oracle, name, int(flags, 16)).tobytes()).hexdigest(), (name, flags)
    # A test that passed with the rule silently off would prove nothing: modes 1 and 3 must have aliased tasks on the one- and on the
    # two-colour blocks. On the opaque images that is certain - the bound of a one-colour subset is 0, nothing prunes it. With alpha 128
    # modes 1 and 3 decode alpha as 255: 127^2 a texel is an exact part of their bound, any alpha-carrying mode that finished earlier puts
    # less on the table, and whether one has finished depends on how the side streams of a small submission interleave. Their tasks are
    # then pruned, and a pruned task is no alias; the mode that image is there for, mode 7, is never pruned on it and must alias.
    for (name, flags), per_mode in on_aliased.items():
        if name == "solid-alpha128":
            assert per_mode.get(7, 0) > 0, (name, flags, per_mode)
        else:
            assert per_mode.get(1, 0) > 0 and per_mode.get(3, 0) > 0, (name, flags, per_mode)
    for key, per_mode in off_aliased.items():
        assert not any(per_mode.values()), (key, per_mode)
