"""The Radiance RGBE texel (csrc/dxtex_rgbe.h, which the GPU kernels and the host codec share) and the host layer's LoadFromHDRMemoryRGBE,
against the reference's .hdr reader and writer (oracle/_ref): decoded floats bit for bit, encoded texels byte for byte, HRESULTs for
damaged files. The loader also runs under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program. CPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rgbe_ref as R  # noqa: E402
from test_hdr_tga_cpu import _rows_old_rle, hdr_images  # noqa: E402

LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK, HOST, HOST_ASAN = (os.path.join(LIB, n) for n in ("rgbe_check", "hdr_rgbe_host_test", "hdr_rgbe_host_test_asan"))


def check_decode(tmp, rgbe, exposure):
    """(n, 4) float32 of rgbe_check's decode; exposure = a decimal string, or the bits of a float."""
    src, out = os.path.join(tmp, "in.rgbe"), os.path.join(tmp, "out.f32")
    np.ascontiguousarray(rgbe, np.uint8).tofile(src)
    arg = f"0x{exposure:08x}" if isinstance(exposure, int) else ("1" if exposure is None else exposure)
    subprocess.run([CHECK, "decode", arg, src, out], check=True, timeout=60)
    return np.fromfile(out, np.float32).reshape(-1, 4)


def check_encode(tmp, px, fmt):
    """(n, 4) uint8 of rgbe_check's encode of the tight texels `px` of `fmt`."""
    src, out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.rgbe")
    np.ascontiguousarray(px).view(np.uint8).reshape(-1).tofile(src)
    subprocess.run([CHECK, "encode", str(fmt), src, out], check=True, timeout=60)
    return np.fromfile(out, np.uint8).reshape(-1, 4)


@pytest.mark.parametrize("exposure", R.EXPOSURES)
def test_decode_every_mantissa_with_every_exponent(tmp_path, exposure):
    rgbe = R.exhaustive_rgbe()
    hr, meta, want = oracle.ref_load_hdr(R.hdr_file(rgbe, exposure))
    assert hr == 0 and (meta["width"], meta["height"]) == (256, 256)
    want = want.view(np.uint32).reshape(-1, 4)
    got = check_decode(str(tmp_path), rgbe, exposure).view(np.uint32)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (exposure, len(bad), bad[:4], got[got != want][:4], want[got != want][:4])
    if exposure is None:
        # the denormal rows are there: exponent bytes 0 .. 10 with small mantissas lie below 2^-126
        f = want.view(np.float32)[:, :3]
        assert ((f > 0) & (f < np.float32(2.0 ** -126))).sum() > 1000
        assert want.view(np.float32)[0, 0] == np.float32(2.0 ** -137)


def encode_cases():
    """[(name, (n, 4) float32 texels)]: the five image kinds of test_hdr_tga_cpu.hdr_images (one size of each is kept whole: 129 x 3) and
    the special texels."""
    rng = np.random.default_rng(11)
    cases = []
    for w, h, imgs in hdr_images(rng):
        for name, img in zip(("noise", "ramp", "flat", "mixed", "wild"), imgs):
            cases.append((f"{name}{w}x{h}", img.reshape(-1, 4)))
    cases.append(("special", R.special_texels()))
    return cases


@pytest.mark.parametrize("fmt", [R.RGBA32F, R.RGB32F, R.RGBA16F])
def test_encode_matches_the_reference_writer(tmp_path, fmt):
    n = 0
    for name, texels in encode_cases() + ([("halves", None)] if fmt == R.RGBA16F else []):
        px = R.special_halves() if texels is None else R.as_format(texels[None], fmt)[0]
        count = px.shape[0]
        # one row of `count` texels: the writer's row coder runs over it, unrle undoes it
        want = R.ref_rgbe_rows(oracle, px, count, 1, fmt).reshape(-1, 4)
        got = check_encode(str(tmp_path), px, fmt)
        bad = np.argwhere((got != want).any(axis=1)).reshape(-1)
        assert bad.size == 0, (name, fmt, len(bad), bad[:4], px[bad[:4]], got[bad[:4]], want[bad[:4]])
        n += count
    assert n > 3000


@pytest.mark.parametrize("fmt", [R.RGBA32F, R.RGB32F, R.RGBA16F])
def test_encode_infinity_is_a_zero_texel(tmp_path, fmt):
    """This project's rule (include/dxtex_amd.h): a texel whose largest channel is +Inf becomes four zero bytes. -Inf counts as 0 like any
    negative, so a texel with -Inf and finite channels encodes as the reference encodes it with 0 there."""
    inf = np.float32(np.inf)
    t = np.array([(inf, 1, 2, 1), (0.5, inf, 0, 1), (1, 2, inf, 1), (inf, inf, inf, 1), (inf, np.nan, -1, 1), (-inf, 1, 2, 1), (-inf, -inf, -inf, 1)], np.float32)
    px = t.astype(np.float16) if fmt == R.RGBA16F else (t[:, :3].copy() if fmt == R.RGB32F else t)
    got = check_encode(str(tmp_path), px, fmt)
    assert not got[:5].any(), got[:5]
    zeroed = t.copy(); zeroed[5:, :3] = np.where(np.isinf(zeroed[5:, :3]), 0, zeroed[5:, :3])
    want = R.ref_rgbe_rows(oracle, R.as_format(zeroed[None, 5:], fmt)[0], 2, 1, fmt).reshape(-1, 4)
    assert np.array_equal(got[5:], want), (got[5:], want)


# ---- LoadFromHDRMemoryRGBE ------------------------------------------------------------------------------------------------------------
def corpus():
    """[file bytes]: valid files of both run-length schemes (with and without an exposure line), then a seeded set of their truncations and
    single-byte mutations."""
    rng = np.random.default_rng(31)
    good = []
    for w, h, imgs in hdr_images(np.random.default_rng(32)):
        for img in imgs[2:]:
            good.append(oracle.ref_save_hdr(img, w, h, R.RGBA32F, w * 16)[1].tobytes())              # new scheme (raw rows below 8 wide)
    for (w, h) in ((20, 3), (600, 2), (9, 4), (1, 1)):
        for k in range(3):
            head = b"#?RADIANCE\n" + (b"EXPOSURE=2.5\n" if k else b"") + b"FORMAT=32-bit_rle_rgbe\n" + (b"EXPOSURE= 0.125\n" if k == 2 else b"")
            good.append(head + f"\n-Y {h} +X {w}\n".encode() + _rows_old_rle(rng, w, h))                # old scheme
    good.append(R.hdr_file(R.random_rgbe(rng, 33, 5), "3.7"))                                          # raw texels
    files = list(good)
    for i in range(900):
        b = bytearray(good[i % len(good)])
        kind = rng.random()
        if kind < 0.35:
            del b[int(rng.integers(0, len(b))):]                                                      # a truncation
        else:
            at = int(rng.integers(0, min(len(b), 90))) if rng.random() < 0.5 else int(rng.integers(0, len(b)))
            b[at] = int(rng.choice([0, 1, 2, 10, 32, 43, 45, 48, 57, 88, 89, 127, 128, 129, 255, int(rng.integers(0, 256))]))
        files.append(bytes(b))
    return good, files


def rgbe_load_many(exe, tmp, files):
    """[(hresult, meta or None, exposure bits or None, (n, 4) uint8 texels or None)] of `exe rgbe_load_many` over the files."""
    paths = []
    for i, data in enumerate(files):
        paths.append(os.path.join(tmp, f"f{i}.hdr"))
        with open(paths[-1], "wb") as f:
            f.write(data)
    lst = os.path.join(tmp, "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(paths) + "\n")
    r = subprocess.run([exe, "rgbe_load_many", lst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-4000:])
    rows = r.stdout.splitlines()
    assert len(rows) == len(files), r.stderr[-2000:]
    out = []
    for i, row in enumerate(rows):
        p = row.split()
        assert int(p[0]) == i
        if len(p) > 2:
            meta = dict(zip(("width", "height", "format", "miscFlags2"), (int(x) for x in p[3:7])))
            out.append((int(p[1], 16), meta, int(p[7], 16), np.fromfile(paths[i] + ".rgbe", np.uint8).reshape(-1, 4)))
        else:
            out.append((int(p[1], 16), None, None, None))
    return out


_corpus = {}


def shared_corpus():
    """The corpus and the oracle's answer to every file of it, computed once."""
    if not _corpus:
        good, files = corpus()
        _corpus["good"], _corpus["files"] = good, files
        _corpus["ref"] = [oracle.ref_load_hdr(f) for f in files]
    return _corpus["good"], _corpus["files"], _corpus["ref"]


def compare_with_oracle(tmp, exe, decode):
    good, files, ref = shared_corpus()
    ours = rgbe_load_many(exe, tmp, files)
    loaded = 0
    for i, ((hr, meta, bits, rgbe), (rhr, rmeta, rpx)) in enumerate(zip(ours, ref)):
        assert hr == rhr, (i, hex(hr), hex(rhr), files[i][:100])
        assert meta == rmeta, (i, meta, rmeta)
        if rpx is None:
            continue
        loaded += 1
        assert rgbe.shape[0] == meta["width"] * meta["height"]
        if decode:
            got = check_decode(tmp, rgbe, bits)
            assert np.array_equal(got.view(np.uint32).reshape(-1), rpx.view(np.uint32)), (i, files[i][:100])
    assert loaded >= len(good) and loaded < len(files)
    return loaded


def test_rgbe_loader_matches_the_reference(tmp_path):
    """HRESULT and metadata equal the reference's for every file; where a file loads, its texels through rgbe_check's decode (with the
    exposure the loader returned) are the reference's floats."""
    assert compare_with_oracle(str(tmp_path), HOST, decode=True) > 40


def test_rgbe_loader_under_sanitizers(tmp_path):
    """The same corpus through the build whose codec and main carry AddressSanitizer and UndefinedBehaviorSanitizer: any report ends the
    program with a non-zero status. Every file is parsed from a heap copy of its exact size."""
    assert os.path.exists(HOST_ASAN)
    compare_with_oracle(str(tmp_path), HOST_ASAN, decode=False)
