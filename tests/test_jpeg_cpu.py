"""The JPEG reader of the host layer (host/DirectXTexAMD_JPEG.cpp: the marker walk, the Huffman decoder, the progressive passes) and the
sample rules it shares with the GPU kernels (csrc/dxtex_jpeg.h), against tests/jpeg_ref.py, the numpy restatement: HRESULT, metadata, the raw
loader's frame and coefficients, and the pixels, byte for byte; every refusal, every truncation of a file and a seeded fuzz. Where Pillow is
installed the restatement itself is held to Pillow's decode (libjpeg-turbo, the library the reference calls). The host program also runs
under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program. CPU only."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_ref as R  # noqa: E402

LIB = os.path.join(ROOT, "directxtex_amd", "lib")
CHECK, HOST, HOST_ASAN = (os.path.join(LIB, n) for n in ("jpeg_check", "jpeg_host_test", "jpeg_host_test_asan"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "jpeg")
# they straddle the dw <= 2 switch of the upsampler, its first and last column, one and several MCU rows, and sizes that are no multiple of
# the MCU
SIZES = ((1, 1), (2, 2), (3, 5), (4, 1), (5, 2), (6, 3), (7, 9), (16, 16), (17, 33), (33, 18), (40, 24), (65, 35))
SAMPLINGS = {"grey": None, "444": (1, 1), "422": (2, 1), "420": (2, 2)}
OK_SET = (R.S_OK, R.E_FAIL, R.E_NOT_SUPPORTED)


def picture(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(w + h - 2, 1)], axis=-1)
    return np.clip(base + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)


def pillow_file(Image, px, kind, quality, progressive, restart):
    im = Image.fromarray(px[..., 0] if kind == "grey" else px)
    options = dict(quality=quality, progressive=progressive)
    if kind != "grey":
        options["subsampling"] = {"444": 0, "422": 1, "420": 2}[kind]
    if restart:
        options["restart_marker_blocks"] = 2
    buf = io.BytesIO()
    im.save(buf, "JPEG", **options)
    return buf.getvalue()


def own_files():
    """files of the restatement's own writer at every size and sampling, half of them with restart intervals: [(name, data)]"""
    out = []
    for n, (w, h) in enumerate(SIZES):
        px = picture(w, h, 100 + n)
        for kind, sampling in SAMPLINGS.items():
            for restart in (0, 3):
                data = R.encode(px[..., 0], restart=restart) if sampling is None else R.encode(px, sampling, restart=restart, quality_scale=0.5 + n % 3)
                out.append((f"own {kind} {w}x{h} restart {restart}", data))
    return out


def golden_cases():
    return sorted(n[:-4] for n in os.listdir(GOLDEN) if n.endswith(".jpg")) if os.path.isdir(GOLDEN) else []


def golden(name):
    with open(os.path.join(GOLDEN, name + ".jpg"), "rb") as f:
        return f.read()


def load_many(exe, tmp, files, name="list"):
    """[(raw hresult, host hresult, metadata hresult, None | dict of the line's fields with pixels, coefficients and quant)] of
    `exe load_many` over (flags, data)"""
    os.makedirs(os.path.join(tmp, name), exist_ok=True)
    lines = []
    for i, (flags, data) in enumerate(files):
        path = os.path.join(tmp, name, f"f{i}.jpg")
        with open(path, "wb") as f:
            f.write(data)
        lines.append(f"{flags} {path}")
    listing = os.path.join(tmp, name + ".txt")
    with open(listing, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, "load_many", listing], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    with open(listing + ".out", "rb") as f:
        blob = f.read()
    keys = ("width", "height", "format", "depth", "arraySize", "mipLevels", "miscFlags", "miscFlags2", "dimension", "colour", "components", "count", "offset", "bytes")
    rows = r.stdout.splitlines()
    assert len(rows) == len(files)
    out = []
    for i, line in enumerate(rows):
        p = line.split()
        assert int(p[0]) == i
        hrs = tuple(int(x, 16) for x in p[1:4])
        if len(p) > 4:
            assert p[4] == "ok"
            d = dict(zip(keys, map(int, p[5:5 + len(keys)])))
            rest = list(map(int, p[5 + len(keys):]))
            d["comps"] = [tuple(rest[6 * c:6 * c + 6]) for c in range(d["components"])]
            at = d["offset"]
            d["pixels"] = np.frombuffer(blob[at:at + d["bytes"]], np.uint8)
            at += d["bytes"]
            d["coef"] = np.frombuffer(blob[at:at + 2 * d["count"]], "<i2")
            at += 2 * d["count"]
            d["quant"] = np.frombuffer(blob[at:at + 512], "<u2").reshape(4, 64)
            out.append(hrs + (d,))
        else:
            out.append(hrs + (None,))
    return out


def check_loaded(result, data, flags, where):
    """a loaded file against the restatement's decode of the same bytes: HRESULTs, metadata, frame, coefficients, pixels"""
    raw_hr, hr, meta_hr, d = result
    info = R.decode(data)
    fmt, misc2 = R.metadata(info, flags)
    assert (raw_hr, hr, meta_hr) == (0, 0, 0) and d is not None, (where, hex(raw_hr), hex(hr), hex(meta_hr))
    assert (d["width"], d["height"], d["format"], d["miscFlags2"]) == (info["width"], info["height"], fmt, misc2), (where, d)
    assert (d["depth"], d["arraySize"], d["mipLevels"], d["miscFlags"], d["dimension"]) == (1, 1, 1, 0, 3), (where, d)
    assert (d["colour"], d["components"]) == (info["colour"], len(info["comps"])), (where, d)
    at = 0
    for got, c in zip(d["comps"], info["comps"]):
        assert got == (c["h"], c["v"], c["tq"], c["bw"], c["bh"], at), (where, got)
        assert np.array_equal(d["quant"][c["tq"]], info["quant"][c["tq"]]), where
        at += c["bw"] * c["bh"] * 64
    assert d["count"] == at and np.array_equal(d["coef"], R.coefficients(info)), where
    assert np.array_equal(d["pixels"], R.pixels(info).reshape(-1)), where


# ---- the restatement against Pillow ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SAMPLINGS))
def test_restatement_decodes_like_pillow(kind):
    """every size x quality 30, 75, 100 x baseline and progressive x with and without restart intervals: byte for byte"""
    Image = pytest.importorskip("PIL.Image")
    for n, (w, h) in enumerate(SIZES):
        px = picture(w, h, n)
        for quality in (30, 75, 100):
            for progressive in (False, True):
                for restart in (False, True):
                    data = pillow_file(Image, px, kind, quality, progressive, restart)
                    want = np.asarray(Image.open(io.BytesIO(data)))
                    info = R.decode(data)
                    got = R.pixels(info)
                    where = (kind, w, h, quality, progressive, restart)
                    assert info["progressive"] == progressive, where
                    if kind == "grey":
                        assert np.array_equal(got, want), where
                    else:
                        got = got.reshape(h, w, 4)
                        assert np.array_equal(got[..., :3], want) and (got[..., 3] == 255).all(), where


def test_restatements_writer_is_read_by_pillow_as_by_itself():
    """the writer's files - its own Huffman tables, every sampling, restart intervals, the three ways to say RGB or YCbCr - decode in
    Pillow to what the restatement makes of them"""
    Image = pytest.importorskip("PIL.Image")
    for name, data in own_files():
        want = np.asarray(Image.open(io.BytesIO(data)))
        got = R.pixels(R.decode(data))
        assert np.array_equal(got if want.ndim == 2 else got.reshape(want.shape[0], want.shape[1], 4)[..., :3], want), name
    px = picture(9, 7, 5)
    for options, colour in ((dict(jfif=True), R.YCBCR), (dict(jfif=False, adobe=0), R.RGB), (dict(jfif=True, adobe=0), R.YCBCR), (dict(jfif=False, adobe=1), R.YCBCR),
                            (dict(jfif=False, ids=[82, 71, 66]), R.RGB), (dict(jfif=False), R.YCBCR), (dict(jfif=False, ids=[82, 71, 67]), R.YCBCR)):
        data = R.encode(px, (2, 2), **options)
        info = R.decode(data)
        assert info["colour"] == colour, options
        want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        assert np.array_equal(R.pixels(info).reshape(7, 9, 4)[..., :3], want), options


# ---- the loaders against the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(SAMPLINGS))
def test_loaders_match_the_restatement_on_pillows_files(tmp_path, kind):
    Image = pytest.importorskip("PIL.Image")
    files, wheres = [], []
    for n, (w, h) in enumerate(SIZES):
        px = picture(w, h, 50 + n)
        for quality in (30, 75, 100):
            for progressive in (False, True):
                for restart in (False, True):
                    files.append((n % 2, pillow_file(Image, px, kind, quality, progressive, restart)))
                    wheres.append((kind, w, h, quality, progressive, restart))
    for result, (flags, data), where in zip(load_many(HOST, str(tmp_path), files), files, wheres):
        check_loaded(result, data, flags, where)


def test_loaders_match_the_restatement_on_its_own_files_and_the_golden_ones(tmp_path):
    files = [(n % 2, data) for n, (_, data) in enumerate(own_files())]
    names = [name for name, _ in own_files()]
    px = picture(9, 7, 5)
    for options in (dict(jfif=False, adobe=0), dict(jfif=True, adobe=0), dict(jfif=False, adobe=1), dict(jfif=False, ids=[82, 71, 66]), dict(jfif=False), dict(jfif=False, ids=[82, 71, 67])):
        files.append((0, R.encode(px, (2, 1), **options)))
        names.append(str(options))
    for name in golden_cases():
        if name != "cmyk":
            files.append((0, golden(name)))
            names.append(name)
    assert len(files) > 100
    for result, (flags, data), where in zip(load_many(HOST_ASAN, str(tmp_path), files), files, names):
        check_loaded(result, data, flags, where)
    # what the list must have covered: both flags, every colour kind
    assert R.metadata(dict(colour=R.YCBCR), R.FLAGS_DEFAULT_LINEAR) == (R.RGBA8, R.ALPHA_MODE_OPAQUE) and R.metadata(dict(colour=R.GREY), 1) == (R.R8, 0)


def test_golden_files_written_by_pillow_load_to_pillows_texels(tmp_path):
    """tests/golden/jpeg: files Pillow wrote, each beside Pillow's decode (<name>.bin) and "<format> <miscFlags2> <width> <height>"
    (<name>.txt); cmyk.jpg is refused"""
    names = golden_cases()
    assert {"grey", "c444", "c422", "c420", "c420_progressive", "c420_optimize", "c420_restart", "cmyk"} <= set(names)
    files = [(0, golden(n)) for n in names]
    assert all(len(d) <= 4096 for _, d in files)
    for n, (flags, data), result in zip(names, files, load_many(HOST_ASAN, str(tmp_path), files)):
        if n == "cmyk":
            assert result[:3] == (R.E_FAIL, R.E_FAIL, R.E_FAIL) and result[3] is None
            with pytest.raises(R.Refused) as e:
                R.decode(data)
            assert e.value.hr == R.E_FAIL
            continue
        check_loaded(result, data, flags, n)
        fmt, misc2, w, h = map(int, open(os.path.join(GOLDEN, n + ".txt")).read().split())
        d = result[3]
        assert (d["format"], d["miscFlags2"], d["width"], d["height"]) == (fmt, misc2, w, h), n
        assert np.array_equal(d["pixels"], np.fromfile(os.path.join(GOLDEN, n + ".bin"), np.uint8)), n
    info = R.decode(golden("c420_progressive"))
    assert info["progressive"] and R.decode(golden("c420_restart"))["comps"][0]["h"] == 2


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def crafted_scan(bits):
    """an 8 x 8 grey file of the restatement's writer whose entropy-coded segment is replaced: bits(w) writes it into a BitWriter"""
    data = R.encode(np.full((8, 8), 128, np.uint8))
    sos = data.index(b"\xFF\xDA")
    w = R.BitWriter()
    bits(w)
    w.flush()
    return data[:sos + 10] + bytes(w.out) + b"\xFF\xD9"


def damaged_files():
    """name -> (file, expected HRESULT): every refusal, one at a time, made by editing bytes of good files"""
    px = picture(21, 13, 9)
    good = R.encode(px, (2, 2), restart=1)
    grey = R.encode(px[..., 0])
    sof = good.index(b"\xFF\xC0")
    gsof = grey.index(b"\xFF\xC0")

    def put(data, at, *values):
        return data[:at] + bytes(values) + data[at + len(values):]

    out = {}
    for m in (0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
        out[f"SOF marker {m:#x}"] = (put(good, sof + 1, m), R.E_NOT_SUPPORTED)
    out["12-bit precision"] = (put(good, sof + 4, 12), R.E_NOT_SUPPORTED)
    out["16-bit precision"] = (put(good, sof + 4, 16), R.E_FAIL)
    out["a DNL height"] = (put(good, sof + 5, 0, 0), R.E_NOT_SUPPORTED)
    out["width 0"] = (put(good, sof + 7, 0, 0), R.E_FAIL)
    out["luma 1x2"] = (put(good, sof + 11, 0x12), R.E_NOT_SUPPORTED)
    out["luma 4x1"] = (put(good, sof + 11, 0x41), R.E_NOT_SUPPORTED)
    out["luma 2x4"] = (put(good, sof + 11, 0x24), R.E_NOT_SUPPORTED)
    out["chroma 2x1"] = (put(good, sof + 14, 0x21), R.E_NOT_SUPPORTED)
    out["second chroma 1x2"] = (put(good, sof + 17, 0x12), R.E_NOT_SUPPORTED)
    out["sampling factor 0"] = (put(good, sof + 11, 0x20), R.E_FAIL)
    out["sampling factor 5"] = (put(good, sof + 11, 0x51), R.E_FAIL)
    out["quantiser index 4"] = (put(good, sof + 12, 4), R.E_FAIL)
    out["a missing quantiser table"] = (put(good, sof + 12, 1), R.E_FAIL)
    out["two components"] = (put(good, sof + 9, 2), R.E_FAIL)
    out["four components"] = (golden("cmyk"), R.E_FAIL)
    out["equal component ids"] = (put(good, sof + 13, 1), R.E_FAIL)
    out["no SOI"] = (b"\xFF\xD9" + good[2:], R.E_FAIL)
    out["empty"] = (b"", R.E_FAIL)
    out["SOI only"] = (good[:2], R.E_FAIL)
    out["no frame"] = (good[:sof] + good[sof + 19:], R.E_FAIL)
    out["two frames"] = (good[:sof] + good[sof:sof + 19] + good[sof:], R.E_FAIL)
    out["a segment length past the file"] = (put(good, sof + 2, 0xFF, 0xFF), R.E_FAIL)
    out["a segment length of 1"] = (put(good, 4, 0, 1), R.E_FAIL)
    dht = good.index(b"\xFF\xC4")
    out["an over-subscribed Huffman table"] = (put(good, dht + 5, 3), R.E_FAIL)
    out["a missing Huffman table"] = (put(good, dht + 4, 0x01), R.E_FAIL)
    dqt = good.index(b"\xFF\xDB")
    out["a quantiser table with precision 2"] = (put(good, dqt + 4, 0x20), R.E_FAIL)
    sos = good.index(b"\xFF\xDA")
    out["a scan of an unknown component"] = (put(good, sos + 5, 9), R.E_FAIL)
    out["a scan of four components"] = (put(good, sos + 4, 4), R.E_FAIL)
    out["a scan with table 4"] = (put(good, sos + 6, 0x40), R.E_FAIL)
    # departure 3: the entropy-coded segment
    rst = good.index(b"\xFF\xD0", sos)
    out["a wrong RSTn"] = (put(good, rst + 1, 0xD1), R.E_FAIL)
    out["an RSTn too early"] = (good[:rst - 1] + good[rst:], R.E_FAIL)
    out["data that end before the last MCU"] = (good[:rst + 2] + b"\xFF\xD9", R.E_FAIL)
    out["no EOI"] = (good[:-2], R.E_FAIL)
    out["no EOI and half the data"] = (good[:(sos + len(good)) // 2], R.E_FAIL)
    ac = {s: k for k, s in enumerate(R.AC_SYMBOLS)}
    out["a bad Huffman code"] = (crafted_scan(lambda w: (w.put(0, 4), w.put(0xFE, 8))), R.E_FAIL)
    out["a run past coefficient 63"] = (crafted_scan(lambda w: (w.put(0, 4), [(w.put(ac[0xF1], 8), w.put(1, 1)) for _ in range(4)])), R.E_FAIL)
    out["zero runs past coefficient 63"] = (crafted_scan(lambda w: (w.put(0, 4), [w.put(ac[0xF0], 8) for _ in range(4)])), R.E_FAIL)
    out["a DC size of 11 and four bits"] = (crafted_scan(lambda w: w.put(11, 4)), R.E_FAIL)
    # a progressive file cut behind each of its scans but the last: coefficients that never reach Al = 0
    prog = golden("c420_progressive")
    scans = [i for i in range(len(prog) - 1) if prog[i] == 0xFF and prog[i + 1] == 0xDA]
    assert len(scans) >= 4
    for k, at in enumerate(scans[1:]):
        out[f"a progressive file of {k + 1} scans"] = (prog[:at] + b"\xFF\xD9", R.E_NOT_SUPPORTED)
    out["a progressive scan repeated"] = (prog[:scans[1]] + prog[scans[0]:], R.E_FAIL)
    return out


def good_edits():
    """edits that leave a file good: grey with sampling factors (1 x 1 whatever the file says), fill bytes in front of a marker, an
    unknown APPn and a COM segment"""
    px = picture(21, 13, 9)
    grey = R.encode(px[..., 0])
    sof = grey.index(b"\xFF\xC0")
    out = {"plain": grey}
    for hv in (0x22, 0x41, 0x13):
        out[f"grey with factors {hv:#x}"] = grey[:sof + 11] + bytes([hv]) + grey[sof + 12:]
    out["fill bytes"] = grey[:sof] + b"\xFF\xFF\xFF" + grey[sof:]
    out["APP5 and COM"] = grey[:sof] + R.segment(0xE5, b"Exif\0\0MM") + R.segment(0xFE, b"a comment \xFF\xD9") + R.segment(0xE2, b"ICC_PROFILE\0") + grey[sof:]
    return out


@pytest.mark.parametrize("exe", (HOST, HOST_ASAN), ids=("plain", "sanitizers"))
def test_damaged_files_are_refused_with_the_stated_hresult(tmp_path, exe):
    cases = damaged_files()
    files = [(0, data) for data, _ in cases.values()]
    for (name, (data, want)), (raw_hr, hr, meta_hr, d) in zip(cases.items(), load_many(exe, str(tmp_path), files)):
        assert (raw_hr, hr) == (want, want) and d is None, (name, hex(raw_hr), hex(hr), hex(want))
        with pytest.raises(R.Refused) as e:
            R.decode(data)
        assert e.value.hr == want, (name, hex(e.value.hr))
    edits = good_edits()
    plain = R.pixels(R.decode(edits["plain"]))
    files = [(0, data) for data in edits.values()]
    for (name, data), result in zip(edits.items(), load_many(exe, str(tmp_path), files, "good")):
        check_loaded(result, data, 0, name)
        assert np.array_equal(result[3]["pixels"], plain.reshape(-1)), name


def test_every_truncation_returns_the_restatements_hresult(tmp_path):
    """every prefix of a baseline and of a progressive file, through the sanitizer build: an HRESULT each, the restatement's"""
    for name in ("grey", "c420_progressive"):
        data = golden(name)
        files = [(0, data[:k]) for k in range(len(data) + 1)]
        results = load_many(HOST_ASAN, str(tmp_path), files, name)
        for k, ((raw_hr, hr, meta_hr, d), (flags, cut)) in enumerate(zip(results, files)):
            try:
                R.decode(cut)
                want = R.S_OK
            except R.Refused as e:
                want = e.hr
            assert raw_hr == hr == want, (name, k, hex(raw_hr), hex(hr), hex(want))
        assert results[-1][3] is not None and all(r[3] is None for r in results[:-1])


def test_null_arguments_and_missing_files(tmp_path):
    path = os.path.join(str(tmp_path), "one.jpg")
    with open(path, "wb") as f:
        f.write(R.encode(np.full((1, 1), 77, np.uint8)))
    r = subprocess.run([HOST_ASAN, "errors", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = {k: int(v, 16) for k, v in (line.split() for line in r.stdout.splitlines())}
    nulls = {k: v for k, v in got.items() if k.endswith("_null")}
    assert len(nulls) == 6 and set(nulls.values()) == {R.E_INVALIDARG}, nulls
    missing = {k: v for k, v in got.items() if k.endswith("_missing")}
    assert len(missing) == 3 and set(missing.values()) == {R.E_FILE_NOT_FOUND}, missing
    assert got["load_file"] == 0 and got["metadata_file"] == 0 and got["raw_file"] == 0


def test_fuzz_never_trips_a_sanitizer_or_gives_wrong_pixels(tmp_path):
    """2 000 seeded byte mutations of valid files through the sanitizer build in one process of its own: S_OK, E_FAIL or
    HRESULT_E_NOT_SUPPORTED and nothing else; a sanitizer report (a non-zero exit) fails, and so does a success whose frame, coefficients
    or pixels differ from the restatement's wherever the restatement decodes the same bytes"""
    rng = np.random.default_rng(2026)
    bases = [golden(n) for n in golden_cases() if n != "c420_wide"]
    px = picture(17, 11, 3)
    bases += [R.encode(px, s, restart=r) for s in ((1, 1), (2, 1), (2, 2)) for r in (0, 2)] + [R.encode(px[..., 0], restart=1)]
    files = []
    for n in range(2000):
        target = bytearray(bases[n % len(bases)])
        for _ in range(int(rng.choice((1, 1, 2, 5)))):
            i = int(rng.integers(0, len(target)))
            target[i] = int(rng.integers(0, 256)) if rng.integers(0, 2) else target[i] ^ (1 << int(rng.integers(0, 8)))
        files.append((0, bytes(target)))
    results = load_many(HOST_ASAN, str(tmp_path), files)
    loaded = both = 0
    for n, ((raw_hr, hr, meta_hr, d), (flags, data)) in enumerate(zip(results, files)):
        assert raw_hr == hr and hr in OK_SET, (n, hex(raw_hr), hex(hr))
        if d is None:
            continue
        loaded += 1
        try:
            R.decode(data)
        except R.Refused:
            continue
        both += 1
        check_loaded((raw_hr, hr, meta_hr, d), data, flags, n)
    assert 0 < both <= loaded < 2000          # some damages are harmless (a quantiser entry, a coefficient), many are not


# ---- the sample rules alone (jpeg_check) --------------------------------------------------------------------------------------------------
def run_check(*args):
    r = subprocess.run([CHECK] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, (args, r.stderr)


def test_idct_matches_the_restatement_up_to_the_wrap_of_the_range_limit(tmp_path):
    """blocks an encoder writes, blocks that drive the output through the 10-bit wrap of libjpeg's range-limit table, and any int16 at all
    times any uint16 (32-bit wraparound in both passes): the same samples"""
    rng = np.random.default_rng(8)
    tmp = str(tmp_path)
    cases = {
        "an encoder's": (rng.integers(-40, 41, (300, 64)).astype(np.int16) * (rng.integers(0, 4, (300, 64)) == 0), rng.integers(1, 64, 64)),
        "DC only": (np.concatenate([np.arange(-1024, 1024, 7).reshape(-1, 1), np.zeros((293, 63), np.int64)], axis=1).astype(np.int16), np.full(64, 16)),
        "through the wrap": (rng.integers(-2048, 2048, (300, 64)).astype(np.int16), rng.integers(1, 256, 64)),
        "any int16, any uint16": (rng.integers(-32768, 32768, (300, 64)).astype(np.int16), rng.integers(0, 65536, 64)),
    }
    for name, (coef, quant) in cases.items():
        coef = np.ascontiguousarray(coef, np.int16)
        quant = quant.astype(np.uint16)
        quant.astype("<u2").tofile(os.path.join(tmp, "q"))
        coef.astype("<i2").tofile(os.path.join(tmp, "c"))
        run_check("idct", os.path.join(tmp, "q"), os.path.join(tmp, "c"), os.path.join(tmp, "o"))
        got = np.fromfile(os.path.join(tmp, "o"), np.uint8).reshape(-1, 8, 8)
        want = R.idct(coef, quant)
        assert np.array_equal(got, want), name
    # the wrap is there to be met: a block whose first sample lies past +511 comes out low, not 255
    wrapped = R.idct(np.array([[600 * 8] + [0] * 63], np.int16), np.ones(64, np.uint16))
    assert (600 + 512) % 1024 - 512 + 128 < 0 and wrapped[0, 0, 0] == 0


def frame_comps(w, h, sampling, rng, spread):
    """components with random coefficients for a frame of this size: the restatement's dicts (component c uses table c)"""
    hmax, vmax = sampling or (1, 1)
    comps = []
    for k in range(1 if sampling is None else 3):
        ch, cv = (hmax, vmax) if k == 0 else (1, 1)
        bw, bh = R.ceil_div(w, 8 * hmax) * ch, R.ceil_div(h, 8 * vmax) * cv
        coef = (rng.integers(-spread, spread + 1, (bh, bw, 64)) * (rng.integers(0, 3, (bh, bw, 64)) == 0)).astype(np.int16)
        coef[..., 0] = rng.integers(-spread, spread + 1, (bh, bw))
        comps.append(dict(h=ch, v=cv, tq=k, bw=bw, bh=bh, dw=R.ceil_div(w * ch, hmax), dh=R.ceil_div(h * cv, vmax), coef=coef))
    return comps


@pytest.mark.parametrize("kind", list(SAMPLINGS))
def test_pixel_stage_matches_the_restatement(tmp_path, kind):
    """upsampling and colour on coefficients drawn at random, at every size, for YCbCr and RGB-coded frames"""
    rng = np.random.default_rng(30 + len(kind))
    tmp = str(tmp_path)
    sampling = SAMPLINGS[kind]
    for w, h in SIZES:
        for colour in ((R.GREY,) if sampling is None else (R.YCBCR, R.RGB)):
            comps = frame_comps(w, h, sampling, rng, 60)
            quant = rng.integers(1, 40, (4, 64)).astype(np.uint16)
            quant.astype("<u2").tofile(os.path.join(tmp, "q"))
            np.concatenate([c["coef"].reshape(-1) for c in comps]).astype("<i2").tofile(os.path.join(tmp, "c"))
            hmax, vmax = sampling or (1, 1)
            run_check("pixels", w, h, colour, hmax, vmax, os.path.join(tmp, "q"), os.path.join(tmp, "c"), os.path.join(tmp, "o"))
            got = np.fromfile(os.path.join(tmp, "o"), np.uint8)
            assert np.array_equal(got, R.pixels_from(w, h, colour, comps, quant).reshape(-1)), (kind, w, h, colour)


def test_upsampling_switches_to_replication_at_two_columns():
    """what the restatement itself must say about the one surprise: a chroma plane of one or two columns is replicated, one of three is
    filtered"""
    p = np.array([[10, 200]], np.uint8)
    assert R.upsample(p, 2, 1, 2, 1).tolist() == [[10, 10, 200, 200]]
    assert R.upsample(p, 2, 1, 2, 2).tolist() == [[10, 10, 200, 200]] * 2
    q = np.array([[10, 200, 50]], np.uint8)
    assert R.upsample(q, 3, 1, 2, 1).tolist() == [[10, (30 + 200 + 2) >> 2, (600 + 10 + 1) >> 2, (600 + 50 + 2) >> 2, (150 + 200 + 1) >> 2, 50]]
    assert R.colour_texels(R.YCBCR, np.array([[128]]), np.array([[128]]), np.array([[255]])).tolist() == [[[255, 37, 128, 255]]]


# ---- dxtexconv's options ------------------------------------------------------------------------------------------------------------------
def test_dxtexconv_refuses_jpeg_output_and_lists_jpeg_input():
    conv = os.path.join(LIB, "dxtexconv")
    for args in (["-ft", "jpg", "-o", "out", "in.dds"], ["-ft", "jpeg", "-o", "out", "in.dds"], ["-o", "x.jpg", "in.dds"], ["-o", "x.JPEG", "in.dds"]):
        r = subprocess.run([conv, "-nologo"] + args, capture_output=True, text=True)
        assert r.returncode == 1 and "usage: dxtexconv" in r.stderr and "JPEG output is not written yet" in r.stderr, (args, r.stderr)
    r = subprocess.run([conv], capture_output=True, text=True)
    assert "in.jpg" in r.stderr, r.stderr
