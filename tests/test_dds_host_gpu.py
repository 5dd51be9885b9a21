"""The resident .dds loaders and writers of the host layer (LoadFromDDSMemory(Device&) / SaveToDDSMemory(Device&)) against the host forms
and the reference (oracle), through tests/cpp/dds_device_test.cpp: same HRESULTs, metadata, pixels and files; the result released on
failure; and the bytes that cross PCIe, as the staging path counts them - a file goes up at the size its payload has on disk."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dds_legacy_cpu import FLAG_SETS, LEGACY, LUM, RGB, RGBA, four, header, masks  # noqa: E402

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "directxtex_amd", "lib", "dds_device_test")
DX10 = four("DX10")
R8G8B8, X8R8G8B8, A8B8G8R8, L8 = (masks(RGB, 24, 0xff0000, 0x00ff00, 0x0000ff, 0), masks(RGB, 32, 0x00ff0000, 0x0000ff00, 0x000000ff, 0),
                                  masks(RGBA, 32, 0x000000ff, 0x0000ff00, 0x00ff0000, 0xff000000), masks(LUM, 8, 0xff, 0, 0, 0))
EXPAND_LUMINANCE, FORCE_DX10_EXT, FORCE_24BPP_RGB = 0x20, 0x10000, 0x100000
PAYLOAD = np.random.default_rng(11).integers(0, 256, 1 << 17, dtype=np.uint8).tobytes()


def run(tmp, command, cases):
    """cases: [(file bytes, flags, ...)] -> the driver's rows, split"""
    lines = []
    for i, case in enumerate(cases):
        path = os.path.join(tmp, f"c{i}.dds")
        with open(path, "wb") as f:
            f.write(case[0])
        lines.append(" ".join([path] + [str(v) for v in case[1:]]))
    lst = os.path.join(tmp, "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([EXE, command, lst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [row.split() for row in r.stdout.splitlines()]
    assert len(rows) == len(cases), r.stdout[-2000:]
    return rows


def test_resident_load_over_the_legacy_matrix(tmp_path, oracle):
    """Every legacy pixel format under every reader flag, on the 5 x 3 chain: where the reference loads, the resident loader's download is
    the host loader's ScratchImage and metadata byte for byte; where it refuses, the same HRESULT and an empty result."""
    cases = [(header(5, 3, pf, mips=3) + PAYLOAD[:1 << 14], fl) for pf in LEGACY for fl in FLAG_SETS]
    loaded = 0
    for (data, flags), row in zip(cases, run(str(tmp_path), "load_many", cases)):
        rhr, rmeta, _ = oracle.ref_load_dds_ex(np.frombuffer(data, np.uint8), flags, capacity=1 << 20)
        where = (data[76:128].hex(), hex(flags), row)
        assert int(row[1], 16) == rhr and int(row[2], 16) == rhr, where
        if rmeta is None:
            assert row[3:] == ["fail", "released"], where
        else:
            assert row[3:6] == ["ok", "1", "1"], where
            loaded += 1
    assert loaded > len(cases) // 2


# (what, 'DX10' extension, width, height, header flags, depth)
NATIVE = (("rgba8 chain", (28, 3, 0, 1, 0), 5, 3, 0x1007 | 0x20000, 0), ("bc7", (98, 3, 0, 1, 0), 16, 8, 0x1007 | 0x20000, 0),
          ("rgba32f", (2, 3, 0, 1, 0), 5, 3, 0x1007 | 0x20000, 0), ("nv12", (103, 3, 0, 1, 0), 8, 4, 0x1007, 0),
          ("cube array", (28, 3, 4, 2, 0), 4, 4, 0x1007 | 0x20000, 0), ("volume", (28, 4, 0, 1, 0), 4, 4, 0x1007 | 0x20000 | 0x800000, 4))


def test_resident_save_equals_the_host_writer_and_round_trips(tmp_path):
    cases = []
    for what, ext, w, h, hflags, depth in NATIVE:
        mips = 1 if what == "nv12" else 3
        cases.append((header(w, h, DX10, flags=hflags, mips=mips, depth=depth, dx10=ext) + PAYLOAD, 0, 0))
    for (what, *_), row in zip(NATIVE, run(str(tmp_path), "save_many", cases)):
        assert row[1:4] == ["00000000", "00000000", "1"] and row[6] == "1", (what, row)
        assert int(row[7]) - int(row[5]) in (128, 148), (what, row)          # down: the payload, once; the rest of the blob is the header


def test_force_24bpp_with_and_without_the_dx10_header(tmp_path):
    """DDS_FLAGS_FORCE_24BPP_RGB packs on the device and comes down at 3 bytes a texel; with FORCE_DX10_EXT there is no 24-bit output."""
    bgrx = header(64, 64, X8R8G8B8) + PAYLOAD
    chain = header(5, 3, X8R8G8B8, flags=0x1007 | 0x20000, mips=3) + PAYLOAD
    rows = run(str(tmp_path), "save_many", [(bgrx, 0, FORCE_24BPP_RGB), (bgrx, 0, FORCE_24BPP_RGB | FORCE_DX10_EXT), (chain, 0, FORCE_24BPP_RGB), (bgrx, 0, 0)])
    for row in rows:
        assert row[1:4] == ["00000000", "00000000", "1"], row
    assert (int(rows[0][5]), int(rows[0][7])) == (64 * 64 * 3, 128 + 64 * 64 * 3)          # a 24-bit save downloads exactly 12 288 bytes
    assert (int(rows[1][5]), int(rows[1][7])) == (64 * 64 * 4, 148 + 64 * 64 * 4) and rows[1][6] == "1"
    assert int(rows[2][5]) == (5 * 3 + 2 * 1 + 1) * 3
    assert int(rows[3][5]) == 64 * 64 * 4 and rows[3][6] == "1"


def test_a_file_goes_up_at_the_size_it_has_on_disk(tmp_path):
    cases = [(header(64, 64, R8G8B8) + PAYLOAD, 0), (header(64, 64, L8) + PAYLOAD, EXPAND_LUMINANCE), (header(64, 64, L8) + PAYLOAD, 0),
             (header(64, 64, A8B8G8R8, flags=0x1007 | 0x20000, mips=7) + PAYLOAD, 0), (header(64, 64, DX10, dx10=(98, 3, 0, 1, 0)) + PAYLOAD, 0),
             (header(63, 5, A8B8G8R8) + PAYLOAD, 0x1), (header(63, 5, L8) + PAYLOAD, 0x1)]
    rows = run(str(tmp_path), "load_many", cases)
    for row in rows:
        assert row[1:6] == ["00000000", "00000000", "ok", "1", "1"], row
    up = [int(r[6]) for r in rows]
    launches = [int(r[8]) for r in rows]
    chain = sum(max(1, 64 >> k) ** 2 * 4 for k in range(7))
    assert up == [12288, 4096, 4096, chain, 64 * 64, 63 * 5 * 4, 64 * 5], up
    # 24-bit texels and expanded luminance take one unpack launch; a native file - a chain and a block-compressed one included, and one
    # whose LEGACY_DWORD pitch is the image's - takes no kernel at all; an L8 file with padded rows takes the copy kernel
    assert launches == [1, 1, 0, 0, 0, 0, 1], launches
    assert all(int(r[7]) == 0 for r in rows)          # nothing comes down during a load
