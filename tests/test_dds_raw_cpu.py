"""LoadFromDDSMemoryRaw, the byte-serial half of the .dds reader (host layer, no device), over the LEGACY x FLAG_SETS matrix of
test_dds_legacy_cpu.py: HRESULT and metadata are the reference's LoadFromDDSMemory's (oracle/_ref), op and opaque flag are what
test_dds_texel_cpu.py's CASES name for the files it lists, the payload starts behind the header (and the palette), and every image's offset
and pitches are the file's pitch rule (the reference's ComputePitch under the CP_FLAGS the reader derives). Where the reference refuses a
file the Raw function answers the same HRESULT and hands out no payload pointer. CPU only."""
import os
import subprocess
import sys

import numpy as np

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dds_legacy_cpu import FLAG_SETS, LEGACY, header  # noqa: E402
from test_dds_texel_cpu import CASES, FILE_BYTES, ROW_COPY, ROW_L8U8V8, ROW_SWIZZLE, ROW_WUV10  # noqa: E402

EXE = os.path.join(ROOT, "directxtex_amd", "lib", "dds_host_test")
CP_LEGACY_DWORD, CP_BAD_DXTN_TAILS, CP_24BPP, CP_16BPP, CP_8BPP = 0x1, 0x1000, 0x10000, 0x20000, 0x40000


def run_raw(tmp, cases):
    lines = []
    for i, (data, flags) in enumerate(cases):
        path = os.path.join(tmp, f"c{i}.dds")
        with open(path, "wb") as f:
            f.write(data)
        lines.append(f"{path} {flags}")
    lst = os.path.join(tmp, "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([EXE, "raw_many", lst], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [row.split() for row in r.stdout.splitlines()]
    assert len(rows) == len(cases)
    return rows


def file_layout(meta, cp):
    """[(offset, row pitch, slice pitch)] of the file's images in the reference's order, from the reference's ComputePitch"""
    out, total = [], 0
    volume = meta["dimension"] == 4
    for _ in range(1 if volume else meta["arraySize"]):
        w, h, d = meta["width"], meta["height"], meta["depth"] if volume else 1
        for _ in range(meta["mipLevels"]):
            hr, rp, sp, _ = oracle.ref_compute_pitch(meta["format"], w, h, cp)
            assert hr == 0
            for _ in range(d):
                out.append((total, rp, sp))
                total += sp
            w, h, d = max(1, w >> 1), max(1, h >> 1), max(1, d >> 1)
    return out, total


def test_raw_over_the_legacy_matrix(tmp_path):
    payload = np.random.default_rng(3).integers(0, 256, 1 << 14, dtype=np.uint8).tobytes()
    known = {(pf, flags): (op, opaque) for (pf, dx10, flags, op, opaque, fmt) in CASES.values() if dx10 is None}
    cases = [(header(5, 3, pf, mips=3) + payload, fl) for pf in LEGACY for fl in FLAG_SETS]
    pfs = [pf for pf in LEGACY for _ in FLAG_SETS]
    loaded = refused = named = 0
    for (data, flags), pf, row in zip(cases, pfs, run_raw(str(tmp_path), cases)):
        rhr, rmeta, rpx = oracle.ref_load_dds_ex(np.frombuffer(data, np.uint8), flags, capacity=1 << 20)
        where = (pf, hex(flags), row[:4])
        assert int(row[1], 16) == rhr and int(row[2], 16) == rhr, where
        if rmeta is None:
            assert row[3:] == ["fail", "1"], where          # released: no payload pointer, no images
            refused += 1
            continue
        loaded += 1
        assert row[3] == "ok"
        assert dict(zip(oracle.DDS_META_KEYS, (int(v) for v in row[4:13]))) == rmeta, where
        op, opaque, paletted, direct, at, nbytes, same = (int(v) for v in row[13:20])
        assert same == 1 and opaque == int((rmeta["miscFlags2"] & 7) == 3), where
        assert at == 128 + (1024 if paletted else 0) and paletted == int(bool(pf[1] & 0x20)), where
        if (pf, flags & ~0x1) in known:          # LEGACY_DWORD changes pitches, not the conversion
            assert (op, bool(opaque)) == known[(pf, flags & ~0x1)], where
            named += 1
        expands = op not in (ROW_COPY, ROW_SWIZZLE, ROW_L8U8V8, ROW_WUV10)
        cp = ({1: CP_8BPP, 2: CP_16BPP, 3: CP_24BPP}[FILE_BYTES[op]] if expands else 0) | (CP_LEGACY_DWORD if flags & 0x1 else 0) | (CP_BAD_DXTN_TAILS if flags & 0x40 else 0)
        want, total = file_layout(rmeta, cp)
        got = [tuple(int(v) for v in s.split(":")) for s in row[20:]]
        if flags & 0x40 and (70 <= rmeta["format"] <= 84 or 94 <= rmeta["format"] <= 99):
            # the 2 x 1 and 1 x 1 levels of a block-compressed chain were not stored: they point at level 0's bytes
            assert got[0] == want[0] and got[1:] == [want[0]] * 2 and not direct, where
        else:
            assert got == want, (where, got, want)
            tight, _ = file_layout(rmeta, 0)
            assert direct == int(op == ROW_COPY and not opaque and want == tight), where
        assert nbytes == total, where
    assert loaded > len(cases) // 2 and refused > 50 and named > 30, (loaded, refused, named)
