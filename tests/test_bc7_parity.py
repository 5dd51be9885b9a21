"""BC7: the HIP encoder reproduces the reference CPU search (D3DX_BC7::Encode, BC6HBC7.cpp:2783-2889)
exactly, so the parity bar is byte equality per block; the north_star's one-sided MSE tolerance
(MSE_gpu <= 1.02 * MSE_cpu + 1e-7) is asserted as well, measured by decoding both
outputs with the reference decoder.

What these images reach, read from the winning blocks of the reference encoder ("BC7 corpus", has the table): on the 64x64 seed 2
images mode 3 wins with 32 of its 64 partitions, mode 1 with 56, mode 7 with 46; opaque mode 6 never wins; mode 5 wins with rotations 1 - 3 on
zero to three blocks each. On the 48x32 seed 9 image with 3SUBSETS mode 0 wins with 7 of 16 partitions and mode 2 with 27 of 64. This file checks
the drivers, flags, partial blocks, passes and knobs; the partitions, rotations and index selectors are covered by tests/test_bc7_corpus_gpu.py."""
import numpy as np
import pytest

import directxtex_amd as dx
from directxtex_amd import synth

pytestmark = pytest.mark.gpu
BC7 = dx.DXGI_FORMAT_BC7_UNORM
RGBA8 = dx.DXGI_FORMAT_R8G8B8A8_UNORM


def _compare(oracle, got, ref, img, w, h, tag):
    g = got.reshape(-1, 16); r = ref.reshape(-1, 16)
    bad = np.nonzero((g != r).any(axis=1))[0]
    src = oracle.load_image(img, w, h, RGBA8)
    mse_g = oracle.compute_mse(oracle.decode_image(got, w, h, BC7), src)
    mse_r = oracle.compute_mse(oracle.decode_image(ref, w, h, BC7), src)
    # stated tolerance (RGB and alpha): one-sided
    assert mse_g[:3].sum() <= 1.02 * mse_r[:3].sum() + 1e-7, (tag, mse_g, mse_r)
    assert mse_g[3] <= 1.02 * mse_r[3] + 1e-7, (tag, mse_g, mse_r)
    modes_g = [int(np.log2(int(b) & -int(b))) if b else 8 for b in g[bad[:8], 0]]
    modes_r = [int(np.log2(int(b) & -int(b))) if b else 8 for b in r[bad[:8], 0]]
    assert bad.size == 0, f"{tag}: {bad.size} of {len(g)} blocks differ; first {bad[:8]} gpu modes {modes_g} ref modes {modes_r}"


@pytest.mark.parametrize("alpha", ["opaque", "smooth", "random", "binary"])
def test_bc7_default_bit_exact(ctx, oracle, alpha):
    w, h = 64, 64
    img = synth.rgba8(w, h, seed=2, alpha=alpha)
    got = ctx.compress(img, w, h, RGBA8, BC7, 0, 0.5)
    ref = oracle.compress_image(img, w, h, RGBA8, BC7, 0, 0.5)
    _compare(oracle, got, ref, img, w, h, alpha)


def test_bc7_quick_bit_exact(ctx, oracle):
    w, h = 64, 48
    img = synth.rgba8(w, h, seed=4, alpha="smooth")
    got = ctx.compress(img, w, h, RGBA8, BC7, dx.TEX_COMPRESS_BC7_QUICK, 0.5)
    ref = oracle.compress_image(img, w, h, RGBA8, BC7, dx.TEX_COMPRESS_BC7_QUICK, 0.5)
    _compare(oracle, got, ref, img, w, h, "quick")


@pytest.mark.parametrize("alpha", ["opaque", "smooth"])
def test_bc7_3subsets_bit_exact(ctx, oracle, alpha):
    """TEX_COMPRESS_BC7_USE_3SUBSETS adds modes 0 and 2 (BC6HBC7.cpp:2805-2815)."""
    w, h = 48, 32
    img = synth.rgba8(w, h, seed=9, alpha=alpha)
    got = ctx.compress(img, w, h, RGBA8, BC7, dx.TEX_COMPRESS_BC7_USE_3SUBSETS, 0.5)
    ref = oracle.compress_image(img, w, h, RGBA8, BC7, dx.TEX_COMPRESS_BC7_USE_3SUBSETS, 0.5)
    _compare(oracle, got, ref, img, w, h, "3subsets-" + alpha)


@pytest.mark.parametrize("flags", [0, dx.TEX_COMPRESS_BC7_QUICK])
@pytest.mark.parametrize("const", [{3: 255}, {1: 128}, {0: 255, 3: 255}, {2: 0, 3: 37}, {0: 9, 1: 200}])
def test_bc7_constant_channels(ctx, oracle, const, flags):
    """Channels that are constant over whole blocks: mode 6 skips the PerturbOne calls that provably find nothing there (bc7_core.h flat_call /
    eval_nearest), and the pruning bound charges rounding slack only to the channels that vary - every byte must stay the reference's. The
    constants include values that the endpoint precision represents exactly and ones it does not; half of the image keeps noise in the channel."""
    w, h = 64, 64
    img = synth.rgba8(w, h, seed=9, alpha="random").copy()
    for ch, v in const.items():
        img[:, : w // 2, ch] = v            # left half: constant; right half: as generated (blocks on the seam are constant too - 4-aligned)
    got = ctx.compress(img, w, h, RGBA8, BC7, flags, 0.5)
    ref = oracle.compress_image(img, w, h, RGBA8, BC7, flags, 0.5)
    _compare(oracle, got, ref, img, w, h, f"const {const} flags {flags}")


@pytest.mark.parametrize("size", [(1, 1), (3, 5), (7, 2), (13, 9)])
def test_bc7_partial_blocks(ctx, oracle, size):
    w, h = size
    img = synth.rgba8(w, h, seed=6, alpha="smooth")
    got = ctx.compress(img, w, h, RGBA8, BC7, 0, 0.5)
    ref = oracle.compress_image(img, w, h, RGBA8, BC7, 0, 0.5)
    _compare(oracle, got, ref, img, w, h, f"{w}x{h}")


def test_bc7_special_blocks(ctx, oracle):
    """flat, two-colour, ramps, single-channel, extreme alpha: exercises the np==1/2 seeds, zero-error early
    outs and the anchor fix-ups."""
    rng = np.random.default_rng(7)
    tiles = []
    for v in (0, 255, 128, 1):
        tiles.append(np.full((16, 4), v, np.uint8))
    t = np.zeros((16, 4), np.uint8); t[:, 3] = 255; t[::2, :3] = 255; tiles.append(t)
    t = np.tile(np.arange(0, 256, 16, dtype=np.uint8)[:, None], (1, 4)); t[:, 3] = 255; tiles.append(t)
    t = t.copy(); t[:, 3] = np.arange(255, -1, -17, dtype=np.uint8)[:16]; tiles.append(t)
    for _ in range(120):
        base = rng.integers(0, 256, (1, 4))
        spread = int(rng.choice([0, 1, 3, 10, 40, 120]))
        t = np.clip(base + rng.integers(-spread, spread + 1, (16, 4)), 0, 255).astype(np.uint8)
        if rng.integers(0, 2):
            t[:, 3] = 255
        tiles.append(t)
    tiles = np.stack(tiles)
    rgba = tiles.astype(np.float32) * np.float32(1.0 / 255.0)
    got = ctx.encode_blocks(BC7, rgba, 0)
    ref = oracle.ref_encode_blocks(BC7, rgba, 0)
    bad = np.nonzero((got != ref).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {len(tiles)} blocks differ, first {bad[:8]}"


def test_multi_pass_images(oracle):
    """Images with more than 2^22 blocks are encoded in passes over block ranges; shrink the pass size to exercise that."""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys; sys.path.insert(0, %r)
        import numpy as np, directxtex_amd as dx, oracle
        from directxtex_amd import synth
        dx.capi.load(dev=True)             # only the -DDXTEX_DEV build reads knobs
        c = dx.Context(0)
        w, h = 52, 36                      # 13 x 9 = 117 blocks, 7 passes of 17 blocks
        img = synth.rgba8(w, h, seed=8, alpha="smooth")
        assert np.array_equal(c.compress(img, w, h, 28, 98, 0, 0.5), oracle.ref_compress_image(img, w, h, 28, 98, 0, 0.5))
        hdr = (img.astype(np.float32) / 255 * 6).astype(np.float16)
        assert np.array_equal(c.compress(hdr, w, h, 10, 95, 0, 0.5), oracle.ref_compress_image(hdr, w, h, 10, 95, 0, 0.5))
        print("multi-pass OK")
    """ % root)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DXTEX_MAX_BLOCKS_PER_PASS="17", DXTEX_BC7_STATS="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "multi-pass OK" in r.stdout, r.stdout + r.stderr
    # the knob really reached the code that ran (the development build's own kernels, not the product library's under the same symbol names):
    # its statistics line appears once per pass and mode, 117 blocks in passes of 17 are 7 passes
    assert r.stderr.count("bc7 stats bc7_pre_mode1 ") == 7, r.stderr[-2000:]


@pytest.mark.parametrize("pass_blocks", [None, "23"])
def test_array_goes_through_one_block_list(oracle, pass_blocks):
    """dxtex_compress_many_device hands a BC7 array (here: a mip chain plus two unrelated images, different sizes and source
    formats) to the pipeline as ONE block list cut into per-image segments; with a 23-block pass the segments also straddle
    passes. Every image must still be byte-identical to the reference's per-image Compress."""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys; sys.path.insert(0, %r)
        import numpy as np, torch, directxtex_amd as dx, oracle
        from directxtex_amd import synth
        if "--dev" in sys.argv: dx.capi.load(dev=True)          # only the -DDXTEX_DEV build reads knobs
        c = dx.Context(0); dev = torch.device("cuda", 0)
        base = synth.rgba8(40, 24, seed=3, alpha="smooth")
        imgs = [(m, w, h, 28) for m, (w, h) in zip(oracle.ref_generate_mips(base, 40, 24, 28, 0x200000, 6), oracle.mip_sizes(40, 24, 6))]
        imgs.append((synth.rgba8(17, 9, seed=4, alpha="opaque"), 17, 9, 28))
        imgs.append(((synth.rgba8(12, 12, seed=5, alpha="smooth").astype(np.float32) / 255).astype(np.float16), 12, 12, 10))
        src_t = [torch.from_numpy(np.ascontiguousarray(p).view(np.uint8).reshape(-1).copy()).to(dev) for p, _, _, _ in imgs]
        dst_t = [torch.zeros(dx.compute_pitch(98, w, h)[1], dtype=torch.uint8, device=dev) for _, w, h, _ in imgs]
        srcs = [dx.capi.device_image(t.data_ptr(), w, h, f) for t, (_, w, h, f) in zip(src_t, imgs)]
        dsts = [dx.capi.device_image(t.data_ptr(), w, h, 98) for t, (_, w, h, _) in zip(dst_t, imgs)]
        c.compress_many_device(srcs, dsts, 0, 0.5)
        torch.cuda.synchronize()
        for t, (p, w, h, f) in zip(dst_t, imgs):
            assert np.array_equal(t.cpu().numpy(), oracle.ref_compress_image(p, w, h, f, 98, 0, 0.5)), (w, h, f)
        # the same through BC6H_UF16 (shares the pass / segment machinery)
        hdr = [((synth.rgba8(w, h, seed=20 + i, alpha="opaque").astype(np.float32) / 255 * 5).astype(np.float16), w, h) for i, (w, h) in enumerate([(20, 12), (7, 5), (1, 1), (33, 4)])]
        hs = [torch.from_numpy(p.view(np.uint8).reshape(-1).copy()).to(dev) for p, _, _ in hdr]
        hd = [torch.zeros(dx.compute_pitch(95, w, h)[1], dtype=torch.uint8, device=dev) for _, w, h in hdr]
        c.compress_many_device([dx.capi.device_image(t.data_ptr(), w, h, 10) for t, (_, w, h) in zip(hs, hdr)],
                               [dx.capi.device_image(t.data_ptr(), w, h, 95) for t, (_, w, h) in zip(hd, hdr)], 0, 0.5)
        torch.cuda.synchronize()
        for t, (p, w, h) in zip(hd, hdr):
            assert np.array_equal(t.cpu().numpy(), oracle.ref_compress_image(p, w, h, 10, 95, 0, 0.5)), ("bc6h", w, h)
        print("array OK")
    """ % root)
    env = dict(os.environ)
    if pass_blocks:
        env["DXTEX_MAX_BLOCKS_PER_PASS"] = pass_blocks
    r = subprocess.run([sys.executable, "-c", code] + (["--dev"] if pass_blocks else []), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "array OK" in r.stdout, r.stdout + r.stderr


def test_pruning_changes_nothing():
    """subset_lower_bound / region_lower_bound6 only drop candidates that cannot win: the payloads with pruning (default) and
    without (DXTEX_BC7_NO_PRUNE / DXTEX_BC6H_NO_PRUNE) must be the same bytes, and so must any legal order of the modes - and
    BC6H's one-region modes searched by a lane per task (DXTEX_BC6H_WAVE_MAX=0) or by a wavefront per task (the default for lists this
    short) are the same search, as is mode 1's PerturbOne with (default) and without (DXTEX_BC7_PERTURB_PLAIN) the bound filter and the PerturbOne of
    BC6H's two-region modes with (default) and without (DXTEX_BC6H_PERTURB_PLAIN) its bound filter, and BC6H's
    modes of equal endpoint precision sharing one search (default) or searching each from scratch (DXTEX_BC6H_NO_REUSE), and BC7's
    two-region modes in the encoder's order (DXTEX_BC6H_ORDER) instead of the default running order, and BC7's
    whole-block tasks (modes 4 / 5 / 6) searched by groups of lanes (default on lists this short) or a lane each (DXTEX_BC7_NO_GROUP), and the
    late modes 4 / 5 on the context's side streams (default) or one after the other on its stream (DXTEX_BC7_SERIAL), and a small submission's
    modes side by side as the default plan has them, in the large-pass order (DXTEX_BC7_NO_SMALL_PLAN) or in another plan (DXTEX_BC7_SMALL_PLAN), and
    (round 6) BC6H's one-region search after the two-region modes (DXTEX_BC6H_FORK_BACK=0) or on a side stream next to the last one / two (default) / three
    of them, and a large pass's modes through a plan (DXTEX_BC7_LARGE_PLAN: late mode 6 beside mode 3)."""
    import subprocess, sys, os, textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent("""
        import sys, hashlib; sys.path.insert(0, %r)
        import numpy as np, directxtex_amd as dx
        from directxtex_amd import synth
        if "--dev" in sys.argv: dx.capi.load(dev=True)          # only the -DDXTEX_DEV build reads knobs; the first run is the product library
        c = dx.Context(0)
        yy, xx = np.mgrid[0:256, 0:256]
        smooth = np.stack([xx, yy, (xx + yy) // 2, 255 - xx // 2], -1).astype(np.uint8)
        imgs = [synth.rgba8(384, 256, seed=21, alpha="opaque"), synth.rgba8(256, 256, seed=22, alpha="smooth"), synth.rgba8(256, 256, seed=23, alpha="binary"),
                smooth, np.random.default_rng(5).integers(0, 256, (128, 128, 4), dtype=np.uint8)]
        for im in imgs:
            h, w = im.shape[:2]
            for flags in (0, 0x80000):
                print(hashlib.sha256(c.compress(im, w, h, 28, 98, flags, 0.5).tobytes()).hexdigest())
            hdr = (im.astype(np.float32) / 255 * 7 - (2 if flags else 0)).astype(np.float16)
            for fmt in (95, 96):
                print(hashlib.sha256(c.compress(hdr, w, h, 10, fmt, 0, 0.5).tobytes()).hexdigest())
    """ % root)
    outs = []
    for env in ({}, {"DXTEX_BC7_NO_PRUNE": "1", "DXTEX_BC6H_NO_PRUNE": "1"}, {"DXTEX_BC7_ORDER": "7,6,5,8,4,3,2,1,0", "DXTEX_BC7_PERTURB_PLAIN": "1", "DXTEX_BC7_NO_GROUP": "1", "DXTEX_BC7_SERIAL": "1", "DXTEX_BC6H_PERTURB_PLAIN": "1"},
                {"DXTEX_BC7_NO_SMALL_PLAN": "1"}, {"DXTEX_BC7_SMALL_PLAN": "16/1/3,2|7,14,15,18|24,26/28/25,0"},
                {"DXTEX_BC7_NO_SMALL_PLAN": "1", "DXTEX_BC7_EARLY6_MIN_PCT": "0", "DXTEX_BC7_EARLYA_MIN_PCT": "0"},          # every early phase that has a block
                {"DXTEX_BC7_NO_SMALL_PLAN": "1", "DXTEX_BC7_EARLY6_MIN_PCT": "101", "DXTEX_BC7_EARLYA_MIN_PCT": "101"},      # no early phase at all
                {"DXTEX_BC7_ORDER": "26,25,3,1,16,7,15,14,18,24,28,0,2", "DXTEX_BC6H_WAVE_MAX": "0", "DXTEX_BC6H_NO_REUSE": "1", "DXTEX_BC6H_ORDER": "0,1,2,3,4,5,6,7,8,9"},
                {"DXTEX_BC6H_FORK_BACK": "0", "DXTEX_BC7_NO_SMALL_PLAN": "1", "DXTEX_BC7_LARGE_PLAN": "16,7|14/18/15|0,1|3,2/26|24/28/25"},
                {"DXTEX_BC6H_FORK_BACK": "1"}, {"DXTEX_BC6H_FORK_BACK": "3", "DXTEX_BC6H_ORDER": "9,1,5,6,7,8,0,2,3,4"}):
        r = subprocess.run([sys.executable, "-c", code] + (["--dev"] if env else []), env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.split())
    assert len(outs[0]) == 20
    for o in outs[1:]:
        assert o == outs[0]
