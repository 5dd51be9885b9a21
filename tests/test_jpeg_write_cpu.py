"""The JPEG writer of the host layer (host/DirectXTexAMD_JPEG.cpp: SaveJPEGRaw's markers and Huffman coder, the host SaveToJPEGMemory) and
the forward sample rules it shares with the GPU kernels (csrc/dxtex_jpeg.h), against tests/jpeg_write_ref.py, the numpy restatement, and
against tests/golden/jpeg_write, the files libjpeg-turbo wrote at the reference's settings: coefficient for coefficient and byte for byte.
Where Pillow is installed the restatement itself is held to the coefficients of Pillow's files. The host program also runs under
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program. CPU only."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref as R  # noqa: E402
import jpeg_write_ref as W  # noqa: E402
from test_jpeg_cpu import SAMPLINGS, SIZES, load_many, picture  # noqa: E402

LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK, HOST, HOST_ASAN = (os.path.join(LIB, n) for n in ("jpeg_write_check", "jpeg_write_host_test", "jpeg_write_host_test_asan"))
READER = os.path.join(LIB, "jpeg_host_test")
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg_write")
QUALITY_100 = ("grey_1x1", "grey_8x8", "grey_17x23", "colour_1x1", "colour_9x9", "colour_16x16", "colour_24x24", "colour_40x24", "colour_8x24", "colour_23x41", "colour_65x35",
               "extremes_33x17")
QUALITY_75 = ("q75_444", "q75_422", "q75_420", "q75_grey")
E_NOT_SUPPORTED, E_INVALIDARG, E_POINTER, E_FAIL = 0x80070032, 0x80070057, 0x80004003, 0x80004005


def golden(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def source(name):
    """a quality-100 fixture's source: (h, w) grey samples or (h, w, 3) R, G, B; the size is the file's"""
    info = R.decode(golden(name))
    px = np.fromfile(os.path.join(GOLDEN, name + ".bin"), np.uint8)
    return px.reshape(info["height"], info["width"]) if info["colour"] == R.GREY else px.reshape(info["height"], info["width"], 3)


def texels(px, fmt, pad=0, fill=0x5A):
    """grey samples or R, G, B in the rows of `fmt` with `pad` bytes behind each, the fourth byte of a colour texel not 0xff: (bytes, pitch)"""
    h, w = px.shape[:2]
    if fmt == R.R8:
        rows = px.reshape(h, w)
    else:
        rows = np.full((h, w, 4), 0x37, np.uint8)
        rows[..., :3] = px if fmt in (R.RGBA8, R.RGBA8_SRGB) else px[..., ::-1]
        rows = rows.reshape(h, w * 4)
    out = np.full((h, rows.shape[1] + pad), fill, np.uint8)
    out[:, :rows.shape[1]] = rows
    return out.reshape(-1)[:out.size - pad], rows.shape[1] + pad          # the last row ends with its last texel


def save_many(exe, tmp, images, command="save_many", name="save"):
    """[(hresult, None | the file's bytes)] of `exe save_many` over (format, (h, w[, 3]) pixels, pad)"""
    os.makedirs(os.path.join(tmp, name), exist_ok=True)
    lines = []
    for i, (fmt, px, pad) in enumerate(images):
        data, pitch = texels(px, fmt, pad)
        path = os.path.join(tmp, name, f"p{i}.bin")
        data.tofile(path)
        lines.append(f"{fmt} {px.shape[1]} {px.shape[0]} {pitch} {path}")
    listing = os.path.join(tmp, name + ".txt")
    with open(listing, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, command, listing], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == len(images) and [int(p[0]) for p in rows] == list(range(len(images)))
    return rows, [open(f"{listing}.{i}.jpg", "rb").read() if os.path.exists(f"{listing}.{i}.jpg") else None for i in range(len(images))]


# ---- the shared header ------------------------------------------------------------------------------------------------------------------------
def _tables(kind, rng):
    return {"ones": W.ONES, "quality 75": W.quality_tables(75), "random": rng.integers(1, 256, (4, 64)).astype(np.uint16),
            "16-bit": rng.integers(1, 65536, (4, 64)).astype(np.uint16)}[kind]


@pytest.mark.parametrize("tables", ("ones", "quality 75", "random", "16-bit"))
@pytest.mark.parametrize("kind", list(SAMPLINGS))
def test_header_functions_give_the_restatements_coefficients(tmp_path, kind, tables):
    """csrc/dxtex_jpeg.h on the host: colour transform, padding, downsampling, forward DCT, quantiser and dummy blocks at every size of the
    reader's SIZES, from R8G8B8A8, B8G8R8A8 and B8G8R8X8 rows with and without padding"""
    rng = np.random.default_rng(len(kind) * 100 + len(tables))
    sampling = SAMPLINGS[kind]
    for n, (w, h) in enumerate(SIZES):
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if n % 2 else picture(w, h, 300 + n)
        quant = _tables(tables, rng)
        fmt = R.R8 if sampling is None else (R.RGBA8, W.B8G8R8A8, W.B8G8R8X8_SRGB)[n % 3]
        src = px[..., 1] if sampling is None else px
        want = R.coefficients(W.encode(src, sampling, quant, (0, 1, 2)))
        data, pitch = texels(src, fmt, (0, 3, 16)[n % 3])
        data.tofile(tmp_path / "p")
        quant.astype("<u2").tofile(tmp_path / "q")
        hmax, vmax = sampling or (1, 1)
        r = subprocess.run([CHECK, "coefficients", str(w), str(h), str(fmt), str(pitch), str(hmax), str(vmax), str(tmp_path / "q"), str(tmp_path / "p"), str(tmp_path / "o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(np.fromfile(tmp_path / "o", "<i2"), want), (kind, tables, w, h, fmt)


def test_the_restatement_gives_the_fixtures_coefficients():
    """without Pillow: the files it wrote, parsed by the reader's restatement, hold the coefficients the writer's restatement makes"""
    for name in QUALITY_100:
        info, px = R.decode(golden(name)), source(name)
        grey = px.ndim == 2
        assert [(c["h"], c["v"], c["tq"]) for c in info["comps"]] == ([(1, 1, 0)] if grey else [(2, 2, 0), (1, 1, 1), (1, 1, 1)]), name
        assert all((q == 1).all() for q in info["quant"][:1 if grey else 2]), name
        assert np.array_equal(R.coefficients(W.encode(px, None if px.ndim == 2 else (2, 2))), R.coefficients(info)), name


# ---- the host saver ---------------------------------------------------------------------------------------------------------------------------
def fixture_images():
    images, wants = [], []
    for n, name in enumerate(QUALITY_100):
        px = source(name)
        formats = (R.R8,) if px.ndim == 2 else (R.RGBA8, W.B8G8R8A8, W.B8G8R8X8, R.RGBA8_SRGB, W.B8G8R8A8_SRGB, W.B8G8R8X8_SRGB)
        for k, fmt in enumerate(formats):
            images.append((fmt, px, (0, 5, 16)[(n + k) % 3]))
            wants.append((name, fmt))
    return images, wants


@pytest.mark.parametrize("exe", (HOST, HOST_ASAN), ids=("plain", "sanitized"))
def test_host_saver_writes_the_fixtures_bytes(tmp_path, exe):
    """every quality-100 fixture from R8G8B8A8, B8G8R8A8 and B8G8R8X8 texels and their _SRGB twins, on tight and padded pitches: libjpeg-turbo's
    file, byte for byte"""
    images, wants = fixture_images()
    rows, files = save_many(exe, str(tmp_path), images)
    for p, data, (name, fmt) in zip(rows, files, wants):
        assert int(p[1], 16) == 0 and data == golden(name), (name, fmt, p)


@pytest.mark.parametrize("exe", (HOST, HOST_ASAN), ids=("plain", "sanitized"))
def test_raw_loader_then_raw_writer_reproduces_every_fixture(tmp_path, exe):
    """LoadFromJPEGMemoryRaw then SaveJPEGRaw: the quality-75 files at 4:4:4, 4:2:2, 4:2:0 and grey included, whose tables and factors are
    not the saver's"""
    names = QUALITY_100 + QUALITY_75
    listing = tmp_path / "list.txt"
    listing.write_text("\n".join(os.path.join(GOLDEN, n + ".jpg") for n in names) + "\n")
    r = subprocess.run([exe, "resave_many", str(listing)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [line.split() for line in r.stdout.splitlines()]
    assert len(rows) == len(names)
    for i, (p, name) in enumerate(zip(rows, names)):
        assert (int(p[1], 16), int(p[2], 16)) == (0, 0), (name, p)
        assert open(f"{listing}.{i}.jpg", "rb").read() == golden(name), name


def test_written_files_load_to_the_restatements_pixels(tmp_path):
    """the host saver's files of random images at the reader's SIZES, through the host loader: the pixels jpeg_ref gives for the file, and
    the coefficients the writer's restatement gives for the image"""
    rng = np.random.default_rng(9)
    images = []
    for n, (w, h) in enumerate(SIZES):
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        images += [(R.R8, px[..., 0], n % 2), ((R.RGBA8, W.B8G8R8X8)[n % 2], px, (n % 3) * 4)]
    rows, files = save_many(HOST, str(tmp_path), images)
    assert all(int(p[1], 16) == 0 for p in rows), rows
    for (fmt, px, _), result, data in zip(images, load_many(READER, str(tmp_path), [(0, d) for d in files]), files):
        info = R.decode(data)
        assert result[:3] == (0, 0, 0) and np.array_equal(result[3]["pixels"], R.pixels(info).reshape(-1)), (fmt, px.shape)
        assert np.array_equal(result[3]["coef"], R.coefficients(W.encode(px, None if fmt == R.R8 else (2, 2)))), (fmt, px.shape)
        assert (result[3]["width"], result[3]["height"], result[3]["format"]) == (px.shape[1], px.shape[0], R.R8 if fmt == R.R8 else R.RGBA8_SRGB)


@pytest.mark.parametrize("exe", (HOST, HOST_ASAN), ids=("plain", "sanitized"))
def test_refusals(tmp_path, exe):
    r = subprocess.run([exe, "errors", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {line.split()[0]: line.split()[1:] for line in r.stdout.splitlines()}
    assert int(got["file_null"][0], 16) == E_INVALIDARG and int(got["file_null_bad_format"][0], 16) == E_INVALIDARG
    others = [k for k in got if k.startswith("format_")]
    assert len(others) == 10
    for k in others:          # every other format: NOT_SUPPORTED, the blob emptied, no file
        assert int(got[k][0], 16) == E_NOT_SUPPORTED and got[k][1:] == ["held", "0"] and int(got["file_" + k][0], 16) == E_NOT_SUPPORTED, (k, got[k])
    want = dict(pixels_null=E_POINTER, width_0=E_INVALIDARG, width_65536=E_INVALIDARG, pitch_short=E_INVALIDARG, raw_dc_2048=E_FAIL, raw_ac_1024=E_FAIL, raw_ac_minus_1024=E_FAIL,
                raw_quant_0=E_INVALIDARG, raw_blocks=E_INVALIDARG, raw_short=E_INVALIDARG, raw_rgb=E_NOT_SUPPORTED, raw_null=E_INVALIDARG)
    for k, hr in want.items():
        assert int(got[k][0], 16) == hr and got[k][1:] == ["held", "0"], (k, got[k])
    # 11 bits of DC difference and 10 of AC are the most the standard tables code; a table with an entry above 255 goes out in 16 bits under
    # SOF1 and comes back as it was
    assert int(got["raw_ok"][0], 16) == 0 and int(got["raw_dc_2047_ac_1023"][0], 16) == 0
    assert got["raw_wide_table"] == ["00000000", "00000000", "same", "1", "sof", "c1"]
    assert got["file_ok"] == ["00000000", "00000000", "9", "7", str(R.RGBA8_SRGB)]
    assert R.decode(open(tmp_path / "x.jpg", "rb").read())["width"] == 9          # no refusal left a file behind: this is file_ok's


def test_every_size_to_17x17_under_the_sanitizers():
    """the stand-alone program built with -fsanitize=address,undefined: grey, padded RGBA and BGRX at every size from 1x1 to 17x17 through the
    saver, the loader and the raw pair, from and into exact-size heap blocks"""
    r = subprocess.run([HOST_ASAN, "sweep"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.split() == ["sweep", "ok", str(17 * 17 * 3)], (r.stdout[-500:], r.stderr[-3000:])


# ---- against Pillow -------------------------------------------------------------------------------------------------------------------------
def _pillow_file(Image, px, **options):
    buf = io.BytesIO()
    Image.fromarray(px).save(buf, "JPEG", **options)
    return buf.getvalue()


def test_restatement_gives_pillows_coefficients():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(31)
    for n in range(40):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 50))
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if n % 4 else picture(w, h, n)
        quality = (100, 75, 30)[n % 3]
        for kind, sampling in SAMPLINGS.items():
            options = dict(quality=quality) if sampling is None else dict(quality=quality, subsampling={"444": 0, "422": 1, "420": 2}[kind])
            info = R.decode(_pillow_file(Image, px[..., 0] if sampling is None else px, **options))
            quant = np.array([q if q is not None else np.ones(64) for q in info["quant"]], np.uint16)
            mine = W.encode(px[..., 0] if sampling is None else px, sampling, quant)
            assert np.array_equal(R.coefficients(mine), R.coefficients(info)), (w, h, kind, quality)
            if quality != 100:
                assert np.array_equal(quant[:1 if sampling is None else 2], W.quality_tables(quality)[:1 if sampling is None else 2])


def test_pillow_writes_the_savers_files_and_decodes_them_to_the_readers_pixels(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(32)
    images = []
    for n, (w, h) in enumerate(SIZES):
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        images += [(R.R8, px[..., 2], 0), (W.B8G8R8A8, px, 0)]
    rows, files = save_many(HOST, str(tmp_path), images)
    for (fmt, px, _), data in zip(images, files):
        assert data == _pillow_file(Image, px, quality=100), (fmt, px.shape)
        decoded = np.asarray(Image.open(io.BytesIO(data)))
        mine = R.pixels(R.decode(data)).reshape(px.shape[0], px.shape[1], -1)
        assert np.array_equal(decoded.reshape(px.shape[0], px.shape[1], -1), mine[..., :3]), (fmt, px.shape)


def test_format_table_over_the_whole_domain():
    """The table the C ABI and the host saver share (csrc/dxtex_jpeg.h, jpeg_texel_of) for every format 0..191: R8_UNORM is grey, R8G8B8A8
    [_SRGB] colour, B8G8R8A8 / B8G8R8X8 [_SRGB] colour with B before R, everything else refused."""
    r = subprocess.run([CHECK, "formats"], capture_output=True, text=True, check=True, timeout=60)
    table = {int(p[1]): int(p[2]) for p in (line.split() for line in r.stdout.splitlines()) if p[0] == "texel"}
    written = {R.R8: 0, R.RGBA8: 1, R.RGBA8_SRGB: 1, W.B8G8R8A8: 2, W.B8G8R8A8_SRGB: 2, W.B8G8R8X8: 2, W.B8G8R8X8_SRGB: 2}
    assert table == {f: written.get(f, -1) for f in range(192)}
