#!/usr/bin/env python3
"""Generates tests/golden/normalmap.json: SHA-256 digests of what THE REFERENCE's ComputeNormalMap (DirectXTexNormalMaps.cpp) returns
for a fixed, seeded list of height maps, flags, amplitudes and destination formats - HRESULT and the destination's bytes.

The oracle cannot compile DirectXTexNormalMaps.cpp (its DirectXMath shim lacks the vector leaves that file needs), so the digests come
from a program built outside this repository: DirectXTexNormalMaps.cpp compiled in place with oracle/Makefile's CXXFLAGS against
oracle/shim plus the missing DirectXMath leaves (XMVector3Cross, XMVector3Normalize, XMVectorSetZ, g_XMNegIdentityR0 / R1,
g_XMNegativeOneHalf, each in its SSE2 shape), linked with oracle/_ref/libdxtex_ref.so, and driven as

    <program> <in.bin> <width> <height> <src format> <src row pitch> <flags> <amplitude as fp32 bits, hex> <dst format> <out.bin>

printing the HRESULT (8 hex digits) and writing the destination's pixels on success. Run:

    python tests/golden/make_golden_normalmap.py <program>

The sources are regenerated from the seeds by the tests (source_bytes(), imported from here), so only digests are stored.

Under CNMAP_MIRROR_V the reference builds the row above row 0 with memcpy(row0, row1, rowPitch) - rowPitch BYTES into a row of
16-byte XMVECTORs - which is defined only for 16-byte texels with a tight pitch. Every MIRROR_V case here has an R32G32B32A32_FLOAT
source with a tight pitch."""
import hashlib, json, os, struct, subprocess, sys, tempfile
import numpy as np

RGBA32F, RGBA16F, RGBA8, BGRA8, R8, R16F, R32F, A8 = 2, 10, 28, 87, 61, 54, 41, 65
BPP_BYTES = {RGBA32F: 16, RGBA16F: 8, RGBA8: 4, BGRA8: 4, R8: 1, R16F: 2, R32F: 4, A8: 1}
# destination formats: UNORM, SNORM and FLOAT; the tests' restatement covers all of them (tests/nmap_ref.py IDENTITY_DESTINATIONS)
DST_UNORM = (28, 87, 11, 24, 49, 61, 65, 85, 86)
DST_SNORM = (31, 13, 51, 63)
DST_FLOAT = (2, 10, 6, 41, 54)
MIRROR_U, MIRROR_V, INVERT, OCCLUSION = 0x1000, 0x2000, 0x4000, 0x8000


def source_bytes(fmt, w, h, seed, pitch=None):
    """The seeded height map: smooth-ish random content (a low-frequency field plus noise) in the source format, rows `pitch` apart
    (padding bytes seeded too)."""
    rng = np.random.default_rng(seed)
    bpp = BPP_BYTES[fmt]
    pitch = pitch or w * bpp
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.stack([0.5 + 0.4 * np.sin(xx * (0.3 + 0.1 * c) + yy * (0.2 + 0.07 * c) + c) for c in range(4)], -1)
    v = np.clip(base + rng.normal(0.0, 0.08, (h, w, 4)), 0.0, 1.0).astype(np.float32)
    if fmt == RGBA32F:
        texels = (v * np.float32(1.5) - np.float32(0.25)).astype(np.float32).view(np.uint8).reshape(h, w * 16)
    elif fmt == RGBA16F:
        texels = (v * 2.0 - 0.5).astype(np.float16).view(np.uint8).reshape(h, w * 8)
    elif fmt in (RGBA8, BGRA8):
        texels = np.round(v * 255).astype(np.uint8).reshape(h, w * 4)
    elif fmt in (R8, A8):
        texels = np.round(v[..., 0] * 255).astype(np.uint8).reshape(h, w)
    elif fmt == R16F:
        texels = (v[..., 0] * 3.0).astype(np.float16).view(np.uint8).reshape(h, w * 2)
    elif fmt == R32F:
        texels = (v[..., 0] * np.float32(4.0) - np.float32(1.0)).astype(np.float32).view(np.uint8).reshape(h, w * 4)
    else:
        raise NotImplementedError(fmt)
    out = rng.integers(0, 256, (h, pitch), dtype=np.uint8)
    out[:, :w * bpp] = texels
    return out.reshape(-1)


def cases():
    """[(name, src format, dst format, width, height, flags, amplitude, seed)]: every channel selector, wrap / clamp on each axis, invert,
    occlusion, amplitudes {0, 1, 3.7, -2, 100}, eight source formats, UNORM / SNORM / FLOAT destinations, sizes 1x1 .. 67x45."""
    out = []
    srcs = (RGBA8, BGRA8, RGBA16F, RGBA32F, R8, R16F, R32F, A8)
    sizes = ((1, 1), (1, 9), (9, 1), (2, 2), (67, 45))
    amps = (0.0, 1.0, 3.7, -2.0, 100.0)
    dsts = DST_UNORM + DST_SNORM + DST_FLOAT
    k = 0
    for i, src in enumerate(srcs):
        for j in range(6):                      # every channel selector 0..5 over the sources
            w, h = sizes[(i + j) % len(sizes)]
            flags = j
            if (i + j) % 3 == 1: flags |= MIRROR_U
            if (i + j) % 4 == 2: flags |= INVERT
            if (i + j) % 2 == 0: flags |= OCCLUSION
            if src == A8: flags = (flags & ~0xF) | 4          # an A8 height map lives in alpha
            dst = dsts[k % len(dsts)]
            amp = amps[k % len(amps)]
            out.append((f"c{k:02d}", src, dst, w, h, flags, amp, 1000 + k))
            k += 1
    # MIRROR_V (and both axes): R32G32B32A32_FLOAT sources with a tight pitch, where the reference's row -1 is defined
    for m, flags in enumerate((MIRROR_V, MIRROR_U | MIRROR_V, MIRROR_V | OCCLUSION | 5, MIRROR_U | MIRROR_V | INVERT | 2, MIRROR_V | INVERT | OCCLUSION | 3)):
        for n, (w, h) in enumerate(((67, 45), (1, 9), (9, 1))):
            dst = (28, 13, 10)[n]
            out.append((f"v{m}{n}", RGBA32F, dst, w, h, flags, amps[(m + n) % len(amps)], 2000 + 10 * m + n))
    # argument checks: a bad channel, a UINT destination, a BC destination, same source and destination format
    out.append(("e_channel", RGBA8, RGBA8, 4, 4, 6, 1.0, 3000))
    out.append(("e_uint", RGBA8, 30, 4, 4, 0, 1.0, 3001))
    out.append(("e_bc", RGBA8, 83, 4, 4, 0, 1.0, 3002))
    out.append(("same_format", RGBA8, RGBA8, 67, 45, 5 | OCCLUSION, 2.5, 3003))
    return out


def main(program):
    res = {"_generator": "tests/golden/make_golden_normalmap.py <program>: the reference's DirectXTexNormalMaps.cpp compiled in place with "
                         "oracle/Makefile's CXXFLAGS (g++ -O2 -msse2 -mfpmath=sse -ffp-contract=off -fno-fast-math) against oracle/shim plus "
                         "SSE2-shaped XMVector3Cross / XMVector3Normalize / XMVectorSetZ / g_XMNegIdentityR0 / R1 / g_XMNegativeOneHalf, "
                         "linked with oracle/_ref/libdxtex_ref.so; nothing of it is in this repository",
           "cases": []}
    with tempfile.TemporaryDirectory() as tmp:
        for name, src, dst, w, h, flags, amp, seed in cases():
            pix = source_bytes(src, w, h, seed)
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            pix.tofile(fin)
            if os.path.exists(fout): os.remove(fout)
            amp_bits = struct.unpack("<I", struct.pack("<f", amp))[0]
            r = subprocess.run([program, fin, str(w), str(h), str(src), str(w * BPP_BYTES[src]), hex(flags), f"{amp_bits:08x}", str(dst), fout],
                               check=True, capture_output=True, text=True)
            hr = int(r.stdout.strip(), 16)
            digest = hashlib.sha256(open(fout, "rb").read()).hexdigest() if hr == 0 else None
            res["cases"].append({"name": name, "src": src, "dst": dst, "width": w, "height": h, "flags": flags, "amplitude": amp, "seed": seed,
                                 "hr": hr, "sha256": digest})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "normalmap.json")
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {len(res['cases'])} cases to {path}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
