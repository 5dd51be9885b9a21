"""TEST INFRASTRUCTURE ONLY. What the ConvertToSinglePlane tests compare against.

- convert() / convert_array(): the reference's own DirectX::ConvertToSinglePlane overloads, called live in oracle/_ref/libdxtex_ref.so.
  The mangled names are looked up in the library's dynamic symbols by their demangled text (as assemble_ref does for CopyRectangle).
  Image and TexMetadata are plain structs; a zero-filled 88-byte buffer is a default-constructed ScratchImage (m_nimages, m_size,
  m_metadata, m_image, m_memory: DirectXTex.h:493-497), whose images are copied out before ScratchImage::Release() frees them.
- written_mask(): the written-element rule (the reference's end guard, `if ((sPtrUV + 1) >= sourceE) break;`) as a numpy mask over a
  destination with any row pitch. Used only where a caller-supplied destination starts non-zero: the reference's own destination is a
  fresh ScratchImage, zero where nothing was written.
"""
import ctypes
import os
import subprocess

import numpy as np

NV12, P010, P016, OPAQUE420, YUY2, Y210, Y216, NV11, P208, V208, V408 = 103, 104, 105, 106, 107, 108, 109, 110, 130, 131, 132
S_OK, E_INVALIDARG, E_POINTER, E_FAIL, E_NOT_SUPPORTED = 0, -2147024809, -2147467261, -2147467259, -2147024846

_SIG_ONE = "DirectX::ConvertToSinglePlane(DirectX::Image const&, DirectX::ScratchImage&)"
_SIG_ARRAY = "DirectX::ConvertToSinglePlane(DirectX::Image const*, unsigned long, DirectX::TexMetadata const&, DirectX::ScratchImage&)"
_SIG_RELEASE = "DirectX::ScratchImage::Release()"


class RefImage(ctypes.Structure):
    """DirectX::Image (DirectXTex.h:437-445)."""
    _fields_ = [("width", ctypes.c_size_t), ("height", ctypes.c_size_t), ("format", ctypes.c_int32), ("rowPitch", ctypes.c_size_t),
                ("slicePitch", ctypes.c_size_t), ("pixels", ctypes.c_void_p)]


class RefMetadata(ctypes.Structure):
    """DirectX::TexMetadata (DirectXTex.h:199-240)."""
    _fields_ = [("width", ctypes.c_size_t), ("height", ctypes.c_size_t), ("depth", ctypes.c_size_t), ("arraySize", ctypes.c_size_t),
                ("mipLevels", ctypes.c_size_t), ("miscFlags", ctypes.c_uint32), ("miscFlags2", ctypes.c_uint32), ("format", ctypes.c_int32),
                ("dimension", ctypes.c_int32)]


class RefScratchImage(ctypes.Structure):
    """DirectX::ScratchImage's members (DirectXTex.h:493-497); all zero = default-constructed."""
    _fields_ = [("nimages", ctypes.c_size_t), ("size", ctypes.c_size_t), ("metadata", RefMetadata), ("image", ctypes.POINTER(RefImage)),
                ("memory", ctypes.c_void_p)]


assert ctypes.sizeof(RefImage) == 48 and ctypes.sizeof(RefMetadata) == 56 and ctypes.sizeof(RefScratchImage) == 88

_fns = None


def _functions(oracle):
    global _fns
    if _fns is None:
        path = oracle.dxtex_oracle._REF_PATH
        found = {}
        for line in subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout.splitlines():
            name = line.split()[-1]
            if "ConvertToSinglePlane" in name or "ScratchImage7Release" in name:
                found[subprocess.run(["c++filt", name], check=True, capture_output=True, text=True).stdout.strip()] = name
        for sig in (_SIG_ONE, _SIG_ARRAY, _SIG_RELEASE):
            assert sig in found, f"{sig} is not exported by {os.path.basename(path)}"
        lib = oracle.dxtex_oracle._load_ref()
        # lib[name], not getattr: a function object of this module's own, so that its argtypes do not reach the oracle's own callers
        one, many, release = (lib[found[s]] for s in (_SIG_ONE, _SIG_ARRAY, _SIG_RELEASE))
        one.argtypes = [ctypes.POINTER(RefImage), ctypes.POINTER(RefScratchImage)]
        one.restype = ctypes.c_int32
        many.argtypes = [ctypes.POINTER(RefImage), ctypes.c_size_t, ctypes.POINTER(RefMetadata), ctypes.POINTER(RefScratchImage)]
        many.restype = ctypes.c_int32
        release.argtypes = [ctypes.POINTER(RefScratchImage)]
        release.restype = None
        _fns = (one, many, release)
    return _fns


def _take(scratch, release):
    """-> [(format, rowPitch, (height, rowPitch) uint8 copy)] of the ScratchImage's images, then Release()."""
    out = []
    for i in range(scratch.nimages):
        im = scratch.image[i]
        rows = np.ctypeslib.as_array(ctypes.cast(im.pixels, ctypes.POINTER(ctypes.c_uint8)), shape=(im.height, im.rowPitch)).copy()
        out.append((int(im.format), int(im.rowPitch), rows))
    release(ctypes.byref(scratch))
    return out


def natural(fmt, width, height):
    """ComputePitch (DirectXTexUtil.cpp:1054-1112) of the planar formats converted here, and of their single-plane forms."""
    if fmt == NV12:
        row = ((width + 1) >> 1) * 2
        return row, row * (height + ((height + 1) >> 1))
    if fmt in (P010, P016):
        row = ((width + 1) >> 1) * 4
        return row, row * (height + ((height + 1) >> 1))
    if fmt == NV11:
        row = ((width + 3) >> 2) * 4
        return row, row * height * 2
    row = ((width + 1) >> 1) * (4 if fmt == YUY2 else 8)
    return row, row * height


def planar_to_single(fmt):
    return {NV12: YUY2, NV11: YUY2, P010: Y210, P016: Y216}.get(fmt, 0)


def sample_bytes(fmt):
    return 2 if fmt in (P010, P016) else 1


def convert(oracle, src, width, height, fmt, row_pitch, slice_pitch):
    """The reference's image overload on `src` (uint8 array of at least slice_pitch bytes, or None for null pixels).
    -> (HRESULT, destination format, destination rowPitch, (height, rowPitch) uint8 rows), the last three None on failure."""
    one, _, release = _functions(oracle)
    buf = None if src is None else np.ascontiguousarray(src, np.uint8)
    image = RefImage(width, height, fmt, row_pitch, slice_pitch, None if buf is None else buf.ctypes.data)
    scratch = RefScratchImage()
    hr = int(one(ctypes.byref(image), ctypes.byref(scratch)))
    if hr != S_OK:
        assert scratch.nimages == 0 and not scratch.memory, "the reference releases its result on failure"
        return hr, None, None, None
    (dfmt, pitch, rows), = _take(scratch, release)
    return hr, dfmt, pitch, rows


def convert_array(oracle, images, width, height, array_size, mip_levels, fmt, dimension=3, depth=1):
    """The reference's array overload. images: [(uint8 array, width, height, rowPitch, slicePitch)] in ScratchImage's order (item-major).
    -> (HRESULT, [(format, rowPitch, rows)] or None)."""
    _, many, release = _functions(oracle)
    keep = [np.ascontiguousarray(im[0], np.uint8) for im in images]
    arr = (RefImage * max(1, len(images)))(*[RefImage(w, h, fmt, rp, sp, b.ctypes.data) for b, (_, w, h, rp, sp) in zip(keep, images)])
    meta = RefMetadata(width, height, depth, array_size, mip_levels, 0, 0, fmt, dimension)
    scratch = RefScratchImage()
    hr = int(many(arr, len(images), ctypes.byref(meta), ctypes.byref(scratch)))
    if hr != S_OK:
        if scratch.memory:
            release(ctypes.byref(scratch))
        return hr, None
    return hr, _take(scratch, release)


def written_mask(width, height, fmt, row_pitch, slice_pitch, dst_pitch):
    """(height, dst_pitch) bool: the destination bytes ConvertToSinglePlane writes for this source."""
    ss = sample_bytes(fmt)
    mask = np.zeros((height, dst_pitch), bool)
    chroma = slice_pitch - height * row_pitch                    # bytes the guard lets the chroma plane hold
    for y in range(height):
        if fmt == NV11:
            fit = max(0, chroma - y * (row_pitch >> 1)) // 2     # chroma pairs wholly below slicePitch
            elems = 2 * min(width // 4, fit)
        else:
            fit = max(0, chroma - (y // 2) * row_pitch) // (2 * ss)
            elems = min(width // 2, fit)
        mask[y, :elems * 4 * ss] = True
    return mask


def expected(dst_start, ref_rows, mask):
    """`dst_start` ((height, dst_pitch) uint8) with the masked bytes taken from the reference's tight rows."""
    out = np.array(dst_start, np.uint8, copy=True)
    tight = np.zeros_like(out)
    n = min(out.shape[1], ref_rows.shape[1])
    tight[:, :n] = ref_rows[:, :n]
    out[mask] = tight[mask]
    return out


# ---- the case matrix the CPU and GPU tests share -------------------------------------------------------------------------------------------
# The smallest shapes at which the kernel can go wrong: one element (below any vector), a tail only, whole 16-byte groups with a tail
# element and three row pairs, a full workgroup's worth, and a width that needs a second workgroup in x (256 lanes x 8 texels = 2048).
SHAPES_420 = [(2, 2), (6, 2), (34, 6), (258, 4), (2056, 2)]
SHAPES_NV11 = [(4, 1), (8, 3), (36, 5), (260, 4), (2056, 2)]
FORMATS = [NV12, P010, P016, NV11]


def shapes(fmt):
    return SHAPES_NV11 if fmt == NV11 else SHAPES_420


def source_pads(fmt, tight):
    """Extra bytes of source rowPitch: tight, +16 (the wide route with padding where tight is 8-byte aligned), +6 (2-byte alignment only),
    +3 (none; 8-bit formats), and up to the next multiple of 8 (the wide route for the shapes whose tight pitch is not aligned: 34 x 6,
    258 x 4, 36 x 5 then have whole 16-byte groups AND tail elements on it)."""
    pads = [0, 16, 6] + ([3] if sample_bytes(fmt) == 1 else [])
    return pads + ([(-tight) % 8] if tight % 8 else [])


def dest_pads(dst_tight):
    """Extra bytes of destination rowPitch: tight, +4, and up to the next multiple of 16 (the wide route's stores) where neither of
    the two is one already."""
    return [0, 4] + ([(-dst_tight) % 16] if dst_tight % 16 and (-dst_tight) % 16 != 4 else [])


def data_end(fmt, width, height, row_pitch):
    """The byte after the last chroma sample: the smallest slicePitch under which the end guard never fires."""
    ss = sample_bytes(fmt)
    if fmt == NV11:
        return height * row_pitch + (height - 1) * (row_pitch >> 1) + width // 2
    return height * row_pitch + (height // 2 - 1) * row_pitch + width * ss


def slice_pitches(fmt, width, height, row_pitch):
    """[(label, slicePitch)]: the layout's own, then short of the chroma data's end by 1, 2 and 5 samples and by one whole chroma row."""
    ss = sample_bytes(fmt)
    rows = height * 2 if fmt == NV11 else height + height // 2
    end = data_end(fmt, width, height, row_pitch)
    low = height * row_pitch
    chroma_pitch = row_pitch >> 1 if fmt == NV11 else row_pitch
    out = [("full", rows * row_pitch)]
    out += [(f"short{k}", max(low, end - k * ss)) for k in (1, 2, 5)]
    out.append(("shortrow", max(low, end - chroma_pitch)))
    return out


def source(fmt, width, height, row_pitch, slice_pitch, seed):
    """slice_pitch seeded random bytes, none of them zero (so that an element the reference leaves at zero is told from a written one)."""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 256, slice_pitch, dtype=np.uint8)


def matrix(fmt):
    """Every case of one format: dicts with the source geometry, the destination pitch, where the two images start relative to a 16-byte
    boundary (an image off the grid never takes the wide route) and a seed."""
    cases = []
    ss = sample_bytes(fmt)
    for (w, h) in shapes(fmt):
        tight = natural(fmt, w, h)[0]
        dst_tight = natural(planar_to_single(fmt), w, h)[0]
        for pad in source_pads(fmt, tight):
            for label, sp in slice_pitches(fmt, w, h, tight + pad):
                for dpad in dest_pads(dst_tight):
                    i = len(cases)
                    cases.append(dict(fmt=fmt, w=w, h=h, row_pitch=tight + pad, slice_pitch=sp, label=label, dst_pitch=dst_tight + dpad,
                                      src_shift=0 if i % 7 else (2 if ss == 2 else 1), dst_shift=8 if i % 11 == 10 else 0, seed=i + 1000 * fmt))
    return cases


def takes_wide_route(c):
    """The route rule of dxtex_plane.h restated for the tests' bookkeeping (the CPU test checks it against what plane_check resolved)."""
    multi = c["h"] > 1
    return (c["src_shift"] == 0 and c["row_pitch"] % 8 == 0 and c["dst_shift"] == 0 and (not multi or c["dst_pitch"] % 16 == 0))


# ---- the HRESULT table: the reference's checks in its order, then the ones added here ------------------------------------------------------
_I, _P, _F, _N = E_INVALIDARG, E_POINTER, E_FAIL, E_NOT_SUPPORTED
# (name, source (fmt, w, h, rowPitch, slicePitch), source shift, destination (fmt, w, h, rowPitch), destination shift, flags, HRESULT)
HRESULT_TABLE = [
    ("not planar", (YUY2, 4, 2, 8, 16), 0, (YUY2, 4, 2, 8), 0, 0, _I),
    ("not planar before null pixels", (28, 4, 2, 16, 32), 0, (YUY2, 4, 2, 8), 0, 1, _I),
    ("null source", (NV12, 4, 2, 4, 12), 0, (YUY2, 4, 2, 8), 0, 1, _P),
    ("null destination", (NV12, 4, 2, 4, 12), 0, (YUY2, 4, 2, 8), 0, 2, _P),
    ("null pixels before no single-plane form", (OPAQUE420, 4, 2, 4, 12), 0, (YUY2, 4, 2, 8), 0, 1, _P),
    ("420_OPAQUE", (OPAQUE420, 4, 2, 4, 12), 0, (YUY2, 4, 2, 8), 0, 0, _N),
    ("P208", (P208, 4, 2, 4, 16), 0, (YUY2, 4, 2, 8), 0, 0, _N),
    ("V208", (V208, 4, 2, 4, 16), 0, (YUY2, 4, 2, 8), 0, 0, _N),
    ("V408", (V408, 4, 2, 4, 24), 0, (YUY2, 4, 2, 8), 0, 0, _N),
    ("Xbox depth plane", (118, 4, 2, 8, 24), 0, (YUY2, 4, 2, 8), 0, 0, _N),
    ("no single-plane form before odd size", (OPAQUE420, 3, 2, 4, 12), 0, (YUY2, 3, 2, 8), 0, 0, _N),
    ("NV12 odd width", (NV12, 3, 2, 4, 12), 0, (YUY2, 3, 2, 8), 0, 0, _I),
    ("NV12 odd height", (NV12, 4, 3, 4, 20), 0, (YUY2, 4, 3, 8), 0, 0, _I),
    ("P010 odd width", (P010, 3, 2, 8, 24), 0, (Y210, 3, 2, 16), 0, 0, _I),
    ("P016 odd height", (P016, 4, 3, 8, 40), 0, (Y216, 4, 3, 16), 0, 0, _I),
    ("NV11 width 6", (NV11, 6, 2, 8, 32), 0, (YUY2, 6, 2, 12), 0, 0, _I),
    ("NV11 odd height is fine", (NV11, 4, 3, 4, 24), 0, (YUY2, 4, 3, 8), 0, 0, 0),
    # added here
    ("destination format", (NV12, 4, 2, 4, 12), 0, (Y210, 4, 2, 16), 0, 0, _I),
    ("P010 into Y216", (P010, 4, 2, 8, 24), 0, (Y216, 4, 2, 16), 0, 0, _I),
    ("destination size", (NV12, 4, 2, 4, 12), 0, (YUY2, 4, 4, 8), 0, 0, _F),
    ("odd size before destination size", (NV12, 3, 2, 4, 12), 0, (YUY2, 4, 2, 8), 0, 0, _I),
    ("source rowPitch below the row", (NV12, 4, 2, 3, 12), 0, (YUY2, 4, 2, 8), 0, 0, _I),
    ("P010 rowPitch below the row", (P010, 4, 2, 6, 24), 0, (Y210, 4, 2, 16), 0, 0, _I),
    ("slicePitch below the luma plane", (NV12, 4, 2, 4, 7), 0, (YUY2, 4, 2, 8), 0, 0, _I),
    ("slicePitch of the luma plane alone is fine", (NV12, 4, 2, 4, 8), 0, (YUY2, 4, 2, 8), 0, 0, 0),
    ("odd source pointer, 16-bit", (P010, 4, 2, 8, 24), 1, (Y210, 4, 2, 16), 0, 0, _I),
    ("odd source rowPitch, 16-bit", (P016, 4, 2, 9, 27), 0, (Y216, 4, 2, 16), 0, 0, _I),
    ("odd slicePitch, 16-bit", (P016, 4, 2, 8, 23), 0, (Y216, 4, 2, 16), 0, 0, _I),
    ("odd destination pointer, 16-bit", (P010, 4, 2, 8, 24), 0, (Y210, 4, 2, 16), 3, 0, _I),
    ("odd destination rowPitch, 16-bit", (P010, 4, 2, 8, 24), 0, (Y210, 4, 2, 17), 0, 0, _I),
    ("odd source pointer and rowPitch, 8-bit, are fine", (NV12, 4, 2, 5, 15), 1, (YUY2, 4, 2, 9), 1, 0, 0),
    ("destination rowPitch below the row", (NV12, 4, 2, 4, 12), 0, (YUY2, 4, 2, 7), 0, 0, _I),
    ("overlap", (NV12, 4, 2, 4, 12), 0, (YUY2, 4, 2, 8), 0, 4, _I),
]
