"""TEST INFRASTRUCTURE ONLY. CPU oracle for Compress / Decompress (see oracle/__init__.py).

Parity status: the block codecs, the image drivers and the scanline layer are the reference itself
(oracle/_ref). The packed-vector conventions that live in DirectXMath (XMLoadUByteN4 = float(b) * (1/255.f),
XMLoadHalf4 exact, ...) are stated leaf by leaf in oracle/shim from its published SSE2 behaviour -
DirectXMath is not vendored in /root/reference and no reference test pins them: PARITY UNPINNED at that
leaf boundary; the numpy functions below repeat the same conventions.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_REF_PATH = os.path.join(_HERE, "_ref", "libdxtex_ref.so")

BC_BLOCK_BYTES = {71: 8, 72: 8, 80: 8, 81: 8, 74: 16, 75: 16, 77: 16, 78: 16, 83: 16, 84: 16, 95: 16, 96: 16, 98: 16, 99: 16}

_ref = None


class _RefImage(ctypes.Structure):
    """DirectX::Image (DirectXTex.h)."""
    _fields_ = [("width", ctypes.c_size_t), ("height", ctypes.c_size_t), ("format", ctypes.c_int32), ("rowPitch", ctypes.c_size_t),
                ("slicePitch", ctypes.c_size_t), ("pixels", ctypes.c_void_p)]


def have_ref():
    return os.path.exists(_REF_PATH)


def _load_ref():
    global _ref
    if _ref is None:
        if not have_ref():
            raise RuntimeError(f"{_REF_PATH} missing: run `make -C oracle ref` where /root/reference exists")
        lib = ctypes.CDLL(_REF_PATH)
        lib.dxtex_ref_encode_blocks.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p,
                                                ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
        lib.dxtex_ref_encode_blocks.restype = ctypes.c_int
        lib.dxtex_ref_decode_blocks.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.dxtex_ref_decode_blocks.restype = ctypes.c_int
        lib.dxtex_ref_num_threads.restype = ctypes.c_int
        vp, sz, i32p = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int32)
        lib.dxtex_ref_compress.argtypes = [vp, sz, sz, ctypes.c_int, sz, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, vp, sz, i32p]
        lib.dxtex_ref_decompress.argtypes = [vp, sz, sz, ctypes.c_int, ctypes.c_int, vp, sz, i32p]
        lib.dxtex_ref_generate_mips.argtypes = [vp, sz, sz, ctypes.c_int, sz, ctypes.c_uint32, sz, vp, sz, i32p]
        lib.dxtex_ref_resize.argtypes = [vp, sz, sz, ctypes.c_int, sz, sz, sz, ctypes.c_uint32, vp, sz, i32p]
        lib.dxtex_ref_convert.argtypes = [vp, sz, sz, ctypes.c_int, sz, ctypes.c_int, ctypes.c_uint32, ctypes.c_float, vp, sz, i32p]
        lib.dxtex_ref_save_dds_volume.argtypes = [vp, sz, sz, sz, ctypes.c_int, sz, ctypes.c_uint32, vp, sz, i32p]
        lib.dxtex_ref_save_dds_volume.restype = ctypes.c_int64
        lib.dxtex_ref_generate_mips3d.argtypes = [vp, sz, sz, sz, ctypes.c_int, ctypes.c_uint32, sz, vp, sz, i32p]
        lib.dxtex_ref_generate_mips3d.restype = ctypes.c_int64
        lib.dxtex_ref_premultiply_alpha.argtypes = [vp, sz, sz, ctypes.c_int, sz, ctypes.c_uint32, vp, sz, i32p]
        lib.dxtex_ref_scale_mips_alpha.argtypes = [vp, sz, sz, ctypes.c_int, sz, ctypes.c_float, vp, sz, i32p]
        for f in (lib.dxtex_ref_compress, lib.dxtex_ref_decompress, lib.dxtex_ref_generate_mips, lib.dxtex_ref_resize, lib.dxtex_ref_convert,
                  lib.dxtex_ref_premultiply_alpha, lib.dxtex_ref_scale_mips_alpha):
            f.restype = ctypes.c_int64
        lib.dxtex_ref_compute_mse.argtypes = [vp, ctypes.c_int, vp, ctypes.c_int, sz, sz, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        lib.dxtex_ref_compute_mse.restype = ctypes.c_int
        # the reference's own ScratchImage members, as the library exports them (ref_image.cpp compiles DirectXTexImage.cpp in place)
        lib._ZN7DirectX12ScratchImage12Initialize2DE11DXGI_FORMATmmmmNS_8CP_FLAGSE.argtypes = [vp, ctypes.c_int, sz, sz, sz, sz, ctypes.c_uint32]
        lib._ZN7DirectX12ScratchImage12Initialize2DE11DXGI_FORMATmmmmNS_8CP_FLAGSE.restype = ctypes.c_int32
        lib._ZNK7DirectX12ScratchImage8GetImageEmmm.argtypes = [vp, sz, sz, sz]
        lib._ZNK7DirectX12ScratchImage8GetImageEmmm.restype = ctypes.POINTER(_RefImage)
        lib._ZNK7DirectX12ScratchImage16IsAlphaAllOpaqueEv.argtypes = [vp]
        lib._ZNK7DirectX12ScratchImage16IsAlphaAllOpaqueEv.restype = ctypes.c_bool
        lib._ZN7DirectX12ScratchImage7ReleaseEv.argtypes = [vp]
        lib._ZN7DirectX12ScratchImage7ReleaseEv.restype = None
        lib.dxtex_ref_save_dds.argtypes = [vp, sz, sz, ctypes.c_int, sz, sz, ctypes.c_uint32, ctypes.c_uint32, vp, sz, i32p]
        lib.dxtex_ref_save_dds.restype = ctypes.c_int64
        lib.dxtex_ref_load_dds.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint64), vp, sz, i32p]
        lib.dxtex_ref_load_dds.restype = ctypes.c_int64
        lib.dxtex_ref_load_dds_ex.argtypes = [vp, sz, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), vp, sz, i32p]
        lib.dxtex_ref_load_dds_ex.restype = ctypes.c_int64
        lib.dxtex_ref_save_dds_ex.argtypes = [vp, sz, sz, sz, ctypes.c_int, sz, sz, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, sz, i32p]
        lib.dxtex_ref_save_dds_ex.restype = ctypes.c_int64
        szp = ctypes.POINTER(ctypes.c_size_t)
        lib.dxtex_ref_format_facts.argtypes = [ctypes.c_int, szp]
        lib.dxtex_ref_format_facts.restype = ctypes.c_int
        lib.dxtex_ref_compute_pitch_ex.argtypes = [ctypes.c_int, sz, sz, ctypes.c_uint32, szp, szp, szp]
        lib.dxtex_ref_compute_pitch_ex.restype = ctypes.c_int
        lib.dxtex_ref_format_facts2.argtypes = [ctypes.c_int, szp]
        lib.dxtex_ref_format_facts2.restype = ctypes.c_int
        lib.dxtex_ref_tile_shape.argtypes = [ctypes.c_int, ctypes.c_uint32, szp]
        lib.dxtex_ref_tile_shape.restype = ctypes.c_int
        lib.dxtex_ref_triangle_filter.argtypes = [sz, sz, ctypes.c_int, vp, vp, vp, sz]
        lib.dxtex_ref_triangle_filter.restype = ctypes.c_int64
        lib.dxtex_ref_load_hdr.argtypes = [vp, sz, ctypes.POINTER(ctypes.c_uint64), vp, sz, i32p]
        lib.dxtex_ref_load_hdr.restype = ctypes.c_int64
        lib.dxtex_ref_save_hdr.argtypes = [vp, sz, sz, ctypes.c_int, sz, vp, sz, i32p]
        lib.dxtex_ref_save_hdr.restype = ctypes.c_int64
        lib.dxtex_ref_load_tga.argtypes = [vp, sz, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64), vp, sz, i32p]
        lib.dxtex_ref_load_tga.restype = ctypes.c_int64
        lib.dxtex_ref_save_tga.argtypes = [vp, sz, sz, ctypes.c_int, sz, ctypes.c_uint32, ctypes.c_int, vp, sz, i32p]
        lib.dxtex_ref_save_tga.restype = ctypes.c_int64
        _ref = lib
    return _ref


def ref_num_threads():
    return int(_load_ref().dxtex_ref_num_threads())


def ref_encode_blocks(bc_format, rgba, flags=0, threshold=0.5, threads=0):
    """D3DXEncodeBC* of the reference (BC.h:332-343) on (n,16,4) float32 tiles -> (n, 8|16) uint8."""
    rgba = np.ascontiguousarray(rgba, np.float32).reshape(-1, 16, 4)
    n = rgba.shape[0]
    out = np.zeros((n, BC_BLOCK_BYTES[bc_format]), np.uint8)
    rc = _load_ref().dxtex_ref_encode_blocks(bc_format, flags & 0x1F0000, threshold, rgba.ctypes.data, n, out.ctypes.data, threads)
    assert rc == 0
    return out


def ref_decode_blocks(bc_format, blocks):
    """D3DXDecodeBC* of the reference (BC.h:321-330): (n, 8|16) uint8 -> (n,16,4) float32."""
    blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, BC_BLOCK_BYTES[bc_format])
    n = blocks.shape[0]
    out = np.zeros((n, 16, 4), np.float32)
    rc = _load_ref().dxtex_ref_decode_blocks(bc_format, blocks.ctypes.data, n, out.ctypes.data)
    assert rc == 0
    return out


# ---- LoadScanline restatement (DirectXTexConvert.cpp:779-1619) -----------------------------------------

_F = np.float32


def load_image(pixels, width, height, fmt, row_pitch=None):
    """-> (H, W, 4) float32, exactly what LoadScanline puts in the XMVECTOR row buffer."""
    raw = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    if fmt == 68:              # R8G8_B8G8_UNORM: one XMLoadUByteN4 per two texels, (r, g0, b, 1) and (r, g1, b, 1), :1192-1205
        ne = (width + 1) // 2
        rp = row_pitch or ne * 4
        v = np.stack([raw[y * rp: y * rp + ne * 4] for y in range(height)]).reshape(height, ne, 4).astype(np.float32) * _F(1.0 / 255.0)
        out = np.ones((height, ne * 2, 4), np.float32)
        out[:, 0::2, :3] = v[..., :3]
        out[:, 1::2, :3] = v[..., [0, 3, 2]]
        return out[:, :width].copy()
    bpp = {2: 16, 10: 8, 28: 4, 29: 4, 87: 4, 88: 4, 91: 4, 93: 4, 49: 2, 61: 1, 63: 1, 65: 1, 41: 4, 54: 2}[fmt]
    rp = row_pitch or width * bpp
    rows = np.stack([raw[y * rp: y * rp + width * bpp] for y in range(height)])
    out = np.zeros((height, width, 4), np.float32)
    out[..., 3] = 1.0
    if fmt in (28, 29):        # R8G8B8A8_UNORM: XMLoadUByteN4, :909-911
        out[:] = rows.reshape(height, width, 4).astype(np.float32) * _F(1.0 / 255.0)
    elif fmt in (87, 91):      # B8G8R8A8: XMLoadUByteN4 + swizzle<2,1,0,3>, :1260-1273
        v = rows.reshape(height, width, 4).astype(np.float32) * _F(1.0 / 255.0)
        out[:] = v[..., [2, 1, 0, 3]]
    elif fmt in (88, 93):      # B8G8R8X8: alpha forced to 1, :1275-1289
        v = rows.reshape(height, width, 4).astype(np.float32) * _F(1.0 / 255.0)
        out[..., :3] = v[..., [2, 1, 0]]
    elif fmt == 10:            # R16G16B16A16_FLOAT: XMLoadHalf4 (exact), :820-821
        out[:] = rows.view(np.float16).reshape(height, width, 4).astype(np.float32)
    elif fmt == 2:             # R32G32B32A32_FLOAT: memcpy, :798-803
        out[:] = rows.view(np.float32).reshape(height, width, 4)
    elif fmt == 61:            # R8_UNORM: float(b) / 255.f (true division), :1106-1117
        out[..., 0] = rows.reshape(height, width).astype(np.float32) / _F(255.0)
        out[..., 1:3] = 0
    elif fmt == 63:            # R8_SNORM: float(b) / 127.f, :1132-1143
        out[..., 0] = rows.view(np.int8).reshape(height, width).astype(np.float32) / _F(127.0)
        out[..., 1:3] = 0
    elif fmt == 65:            # A8_UNORM: (0,0,0,a/255.f), :1158-1169
        out[..., :3] = 0
        out[..., 3] = rows.reshape(height, width).astype(np.float32) / _F(255.0)
    elif fmt == 49:            # R8G8_UNORM: XMLoadUByteN2 -> (x,y,0,1), :1028-1029
        v = rows.reshape(height, width, 2).astype(np.float32) * _F(1.0 / 255.0)
        out[..., :2] = v
        out[..., 2] = 0
    elif fmt == 41:            # R32_FLOAT
        out[..., 0] = rows.view(np.float32).reshape(height, width)
        out[..., 1:3] = 0
    elif fmt == 54:            # R16_FLOAT: XMConvertHalfToFloat, :1040-1051
        out[..., 0] = rows.view(np.float16).reshape(height, width).astype(np.float32)
        out[..., 1:3] = 0
    else:
        raise NotImplementedError(fmt)
    return out


_UNORM_SRC = {28, 29, 87, 88, 91, 93, 49, 61, 65}
_FLOAT_SRC = {2, 10, 41, 54}
_SNORM_SRC = {63}
_R_ONLY_SRC = {61, 63, 41, 54}


def convert_tiles(tiles, src_fmt, dst_fmt):
    """ConvertScanline on the compress path (DirectXTexConvert.cpp:3080-3854; branches at :3453-3530 and
    :3650-3695). tiles: (..., 4) float32, returns a new array."""
    t = tiles.astype(np.float32, copy=True)
    out_unorm = dst_fmt in (71, 72, 74, 75, 77, 78, 80, 83, 98, 99)
    out_snorm = dst_fmt in (81, 84)
    if out_unorm:
        if src_fmt in _SNORM_SRC:
            t = t * _F(0.5) + _F(0.5)
        elif src_fmt in _FLOAT_SRC:
            t = np.minimum(np.maximum(t, _F(0)), _F(1))           # XMVectorSaturate
    elif out_snorm:
        if src_fmt in _UNORM_SRC:
            t = t * _F(2.0) + _F(-1.0)                             # XMVectorMultiplyAdd(v, 2, -1), unfused
        elif src_fmt in _FLOAT_SRC:
            t = np.minimum(np.maximum(t, _F(-1)), _F(1))
    out_rgb = dst_fmt in (71, 72, 74, 75, 77, 78, 95, 96, 98, 99)
    out_rg = dst_fmt in (83, 84)
    out_has_a = out_rgb
    if src_fmt == 65 and not out_has_a:
        t[..., 0] = t[..., 3]; t[..., 1] = t[..., 3]; t[..., 2] = t[..., 3]   # splat W, :3657-3666
    elif src_fmt in _R_ONLY_SRC:
        if out_rgb:
            t[..., 1] = t[..., 0]; t[..., 2] = t[..., 0]                      # :3670-3680
        elif out_rg:
            t[..., 1] = t[..., 0]                                            # :3683-3693
    return t


def gather_tiles(img):
    """(H, W, 4) float32 -> (nbh*nbw, 16, 4) tiles temp[y*4+x], replicating partial blocks with
    uSrc = {0,0,0,1} exactly as CompressBC does (DirectXTexCompress.cpp:315-341)."""
    h, w = img.shape[:2]
    nbw, nbh = (w + 3) // 4, (h + 3) // 4

    def src_index(n, extent_total):
        idx = np.zeros((n, 4), np.int64)
        for b in range(n):
            ext = min(4, extent_total - b * 4)
            for s in range(4):
                if s < ext:
                    k = s
                else:
                    k = 1 if (s == 3 and ext > 1) else 0
                idx[b, s] = b * 4 + k
        return idx

    xi = src_index(nbw, w)      # (nbw, 4)
    yi = src_index(nbh, h)      # (nbh, 4)
    t = img[yi[:, None, :, None], xi[None, :, None, :]]     # (nbh, nbw, 4y, 4x, 4)
    return np.ascontiguousarray(t.reshape(nbh * nbw, 16, 4))


def compress_image(pixels, width, height, src_fmt, dst_fmt, flags=0, threshold=0.5, row_pitch=None, threads=0):
    """Oracle for DirectX::Compress on one image: CompressBC (DirectXTexCompress.cpp:72-205) with the
    reference's block encoders. Returns the tight-pitch BC payload as uint8."""
    if ((src_fmt in (29, 91, 93)) or bool(flags & 0x1000000)) != ((dst_fmt in (72, 75, 78, 99)) or bool(flags & 0x2000000)):
        raise NotImplementedError("one-sided sRGB")
    img = load_image(pixels, width, height, src_fmt, row_pitch)
    tiles = convert_tiles(gather_tiles(img), src_fmt, dst_fmt)
    return ref_encode_blocks(dst_fmt, tiles, flags, threshold, threads).reshape(-1)


def decode_image(payload, width, height, bc_fmt):
    """BC payload -> (H, W, 4) float32 via the reference decoders (DecompressBC, DirectXTexCompress.cpp:425-535)."""
    nbw, nbh = (width + 3) // 4, (height + 3) // 4
    t = ref_decode_blocks(bc_fmt, payload).reshape(nbh, nbw, 4, 4, 4)
    img = t.transpose(0, 2, 1, 3, 4).reshape(nbh * 4, nbw * 4, 4)
    return img[:height, :width]


# ---- StoreScanline restatement (DirectXTexConvert.cpp:1629-2533) ------------------------------------------
# Packed stores are DirectXMath's (SSE2 flavour): see the header of directxtex_amd/csrc/dxtex_store.h for the
# behaviours assumed; PARITY UNPINNED at that boundary.

def _trunc_u8_biased(v):
    s = (v.astype(np.float32) + _F(0.5 / 255.0)).astype(np.float32)
    s = np.minimum(np.maximum(s, _F(0)), _F(1))
    return (s * _F(255.0)).astype(np.float32).astype(np.uint8)       # truncation


def _half_clamped(v):
    s = np.minimum(np.maximum(v.astype(np.float32), _F(-65504.0)), _F(65504.0))
    return s.astype(np.float16)                                        # IEEE round to nearest even


def store_image(img, fmt):
    """(H, W, 4) float32 -> tight-pitch bytes of `fmt`, exactly what StoreScanline writes."""
    img = np.ascontiguousarray(img, np.float32)
    h, w = img.shape[:2]
    if fmt == 2:
        return img.reshape(-1).view(np.uint8).copy()
    if fmt == 10:
        return _half_clamped(img).reshape(-1).view(np.uint8).copy()
    if fmt in (28, 29):
        return _trunc_u8_biased(img).reshape(-1)
    if fmt in (87, 91):
        return _trunc_u8_biased(img[..., [2, 1, 0, 3]]).reshape(-1)
    if fmt in (88, 93):
        t = img[..., [2, 1, 0, 3]].copy(); t[..., 3] = 1.0
        return _trunc_u8_biased(t).reshape(-1)
    if fmt == 61:       # R8_UNORM (:1958-1971)
        s = np.maximum(np.minimum((img[..., 0] + _F(0.5 / 255.0)).astype(np.float32), _F(1)), _F(0))
        return (s * _F(255.0)).astype(np.float32).astype(np.uint8).reshape(-1)
    if fmt == 65:       # A8_UNORM
        s = np.maximum(np.minimum((img[..., 3] + _F(0.5 / 255.0)).astype(np.float32), _F(1)), _F(0))
        return (s * _F(255.0)).astype(np.float32).astype(np.uint8).reshape(-1)
    if fmt == 49:       # R8G8_UNORM: XMStoreUByteN2 = saturate, *255 + 0.5, truncate
        s = np.minimum(np.maximum(img[..., :2], _F(0)), _F(1))
        return ((s * _F(255.0)).astype(np.float32) + _F(0.5)).astype(np.float32).astype(np.uint8).reshape(-1)
    if fmt == 63:       # R8_SNORM: lroundf(clamp(v) * 127) (:1988-2001)
        s = np.maximum(np.minimum(img[..., 0], _F(1)), _F(-1))
        p = (s * _F(127.0)).astype(np.float32)
        r = np.where(p >= 0, np.floor(p + _F(0.5)), np.ceil(p - _F(0.5)))       # half away from zero
        return r.astype(np.int8).view(np.uint8).reshape(-1)
    if fmt == 51:       # R8G8_SNORM: XMStoreByteN2 = clamp, *127, round to nearest even
        s = np.minimum(np.maximum(img[..., :2], _F(-1)), _F(1))
        return np.rint((s * _F(127.0)).astype(np.float32)).astype(np.int8).view(np.uint8).reshape(-1)
    if fmt == 41:
        return np.ascontiguousarray(img[..., 0]).reshape(-1).view(np.uint8).copy()
    if fmt == 54:
        return _half_clamped(img[..., 0]).reshape(-1).view(np.uint8).copy()
    raise NotImplementedError(fmt)


def decompress_image(payload, width, height, bc_fmt, dst_fmt):
    """Oracle for DirectX::Decompress on one image (DecompressBC, DirectXTexCompress.cpp:425-535): reference block
    decoder + ConvertScanline (a no-op for the default target formats) + StoreScanline."""
    return store_image(decode_image(payload, width, height, bc_fmt), dst_fmt)


def compute_mse(a, b):
    """ComputeMSE (DirectXTexMisc.cpp:27-176): per-channel sum of squared differences / (w*h), on floats."""
    d = a.astype(np.float64) - b.astype(np.float64)
    return (d * d).reshape(-1, a.shape[-1]).mean(axis=0)


def psnr_rgb(a, b):
    """texdiag's PSNR: 10*log10(3 / (mseR + mseG + mseB)) (Texdiag/texdiag.cpp:3531-3532)."""
    m = compute_mse(a, b)
    s = float(m[0] + m[1] + m[2])
    return float("inf") if s == 0 else 10.0 * np.log10(3.0 / s)


# ---- the reference's own image drivers (oracle/_ref: DirectXTexCompress / Mipmaps / Resize / Misc.cpp compiled in place) ----

class RefError(RuntimeError):
    def __init__(self, hr):
        self.hresult = hr & 0xFFFFFFFF
        super().__init__(f"reference returned HRESULT 0x{self.hresult:08X}")


BPP = {2: 128, 6: 96, 13: 64, 24: 32, 26: 32, 37: 32, 58: 16, 67: 32, 85: 16, 86: 16, 115: 16, 10: 64, 11: 64, 16: 64, 28: 32, 29: 32, 31: 32, 34: 32, 35: 32, 41: 32, 49: 16, 51: 16, 54: 16, 56: 16, 61: 8, 63: 8, 65: 8,
       87: 32, 88: 32, 91: 32, 93: 32,
       # integer, extended-range and 4:4:4 video formats
       3: 128, 4: 128, 7: 96, 8: 96, 12: 64, 14: 64, 17: 64, 18: 64, 25: 32, 30: 32, 32: 32, 36: 32, 38: 32, 42: 32, 43: 32, 50: 16, 52: 16, 57: 16, 59: 16, 62: 8, 64: 8,
       89: 32, 100: 32, 101: 32, 102: 64,
       # depth / stencil
       20: 64, 40: 32, 45: 32, 55: 16,
       # several texels per element: R1 (8 per byte); R8G8_B8G8 / G8R8_G8B8 / YUY2 (2 per dword); Y210 / Y216 (2 per qword)
       66: 1, 68: 16, 69: 16, 107: 16, 108: 32, 109: 32, 191: 16}
PAIRED = {68: 4, 69: 4, 107: 4, 108: 8, 109: 8}      # bytes of an element of two texels: rows are ((w + 1) >> 1) elements (ComputePitch)


def image_bytes(fmt, w, h):
    if fmt in BC_BLOCK_BYTES:
        return max(1, (w + 3) // 4) * max(1, (h + 3) // 4) * BC_BLOCK_BYTES[fmt]
    if fmt in PAIRED:
        return ((w + 1) >> 1) * PAIRED[fmt] * h
    return (w * BPP[fmt] + 7) // 8 * h


def _run(fn, out_bytes, *args):
    out = np.zeros(out_bytes, np.uint8)
    hr = ctypes.c_int32(0)
    n = fn(*args, out.ctypes.data, out.nbytes, ctypes.byref(hr))
    if n < 0:
        raise RefError(hr.value if n == -1 else 0x8007000E)
    return out[:n]


def ref_compress_image(pixels, width, height, src_fmt, dst_fmt, flags=0, threshold=0.5, row_pitch=0):
    """DirectX::Compress of the reference (DirectXTexCompress.cpp:643-760) -> tight BC payload."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    return _run(_load_ref().dxtex_ref_compress, image_bytes(dst_fmt, width, height), px.ctypes.data, width, height, src_fmt, row_pitch, dst_fmt, flags, threshold)


def ref_decompress_image(payload, width, height, bc_fmt, dst_fmt):
    """DirectX::Decompress of the reference (DirectXTexCompress.cpp:852-910)."""
    px = np.ascontiguousarray(payload, np.uint8).reshape(-1)
    return _run(_load_ref().dxtex_ref_decompress, image_bytes(dst_fmt, width, height), px.ctypes.data, width, height, bc_fmt, dst_fmt)


def mip_sizes(width, height, levels):
    out = []
    for _ in range(levels):
        out.append((width, height))
        width, height = max(1, width >> 1), max(1, height >> 1)
    return out


def ref_generate_mips(pixels, width, height, fmt, filter_flags, levels):
    """DirectX::GenerateMipMaps (DirectXTexMipmaps.cpp:2828-3017, custom filters) -> list of tight per-level buffers."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    sizes = mip_sizes(width, height, levels)
    blob = _run(_load_ref().dxtex_ref_generate_mips, sum(image_bytes(fmt, w, h) for w, h in sizes), px.ctypes.data, width, height, fmt, 0, filter_flags, levels)
    res, at = [], 0
    for w, h in sizes:
        n = image_bytes(fmt, w, h)
        res.append(blob[at:at + n].copy()); at += n
    return res


def ref_resize(pixels, width, height, fmt, new_width, new_height, filter_flags):
    """DirectX::Resize (DirectXTexResize.cpp:854-930, custom filters)."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    return _run(_load_ref().dxtex_ref_resize, image_bytes(fmt, new_width, new_height), px.ctypes.data, width, height, fmt, 0, new_width, new_height, filter_flags)


def ref_convert(pixels, width, height, src_fmt, dst_fmt, filter_flags=0, threshold=0.5):
    """The reference's own Convert (DirectXTexConvert.cpp:5091-5180 -> ConvertCustom :4804-4913), compiled in place."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    return _run(_load_ref().dxtex_ref_convert, image_bytes(dst_fmt, width, height), px.ctypes.data, width, height, src_fmt, 0, dst_fmt, filter_flags, threshold)


def mip_sizes3d(width, height, depth, levels):
    out = []
    for _ in range(levels):
        out.append((width, height, depth))
        width, height, depth = max(1, width >> 1), max(1, height >> 1), max(1, depth >> 1)
    return out


def ref_generate_mips3d(volume, width, height, depth, fmt, filter_flags, levels):
    """DirectX::GenerateMipMaps3D (DirectXTexMipmaps.cpp:3254-3361) -> list of per-level buffers (slices consecutive, tight)."""
    px = np.ascontiguousarray(volume).view(np.uint8).reshape(-1)
    sizes = mip_sizes3d(width, height, depth, levels)
    blob = _run(_load_ref().dxtex_ref_generate_mips3d, sum(image_bytes(fmt, w, h) * d for w, h, d in sizes), px.ctypes.data, width, height, depth, fmt, filter_flags, levels)
    res, at = [], 0
    for w, h, d in sizes:
        n = image_bytes(fmt, w, h) * d
        res.append(blob[at:at + n].copy()); at += n
    return res


def ref_premultiply_alpha(pixels, width, height, fmt, flags=0):
    """DirectX::PremultiplyAlpha (DirectXTexPMAlpha.cpp:214-262); flags = TEX_PMALPHA_* (0x1 IGNORE_SRGB, 0x2 REVERSE, SRGB_IN/OUT)."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    return _run(_load_ref().dxtex_ref_premultiply_alpha, image_bytes(fmt, width, height), px.ctypes.data, width, height, fmt, 0, flags)


def ref_scale_mips_alpha_for_coverage(levels, width, height, fmt, alpha_reference):
    """DirectX::ScaleMipMapsAlphaForCoverage (DirectXTexMipmaps.cpp:3483-3556) on a list of tight per-level buffers."""
    chain = np.concatenate([np.ascontiguousarray(l).view(np.uint8).reshape(-1) for l in levels])
    sizes = mip_sizes(width, height, len(levels))
    blob = _run(_load_ref().dxtex_ref_scale_mips_alpha, chain.size, chain.ctypes.data, width, height, fmt, len(levels), alpha_reference)
    res, at = [], 0
    for w, h in sizes:
        n = image_bytes(fmt, w, h)
        res.append(blob[at:at + n].copy()); at += n
    return res


def ref_compute_mse(a, fmt_a, b, fmt_b, width, height):
    """DirectX::ComputeMSE (DirectXTexMisc.cpp:27-176, fp32 accumulation) -> per-channel MSE (4,) float32."""
    pa = np.ascontiguousarray(a).view(np.uint8).reshape(-1); pb = np.ascontiguousarray(b).view(np.uint8).reshape(-1)
    m = ctypes.c_float(0); v = (ctypes.c_float * 4)()
    hr = _load_ref().dxtex_ref_compute_mse(pa.ctypes.data, fmt_a, pb.ctypes.data, fmt_b, width, height, ctypes.byref(m), v)
    if hr != 0:
        raise RefError(hr)
    return np.array(list(v), np.float32)


def ref_alpha_all_opaque(images, fmt, width, height):
    """ScratchImage::IsAlphaAllOpaque (DirectXTexImage.cpp:800-852; IsAlphaAllOpaqueBC, DirectXTexCompress.cpp:539-621) over a list of
    tight images of one size and format (a texture array; block-compressed formats included) -> bool.

    The function is a member of ScratchImage, so the oracle drives the reference's own exported members: Initialize2D on a zeroed
    object (the state its constructor leaves, DirectXTex.h: every member 0 / nullptr; 256 bytes hold its 88), GetImage for each item's
    pixels, IsAlphaAllOpaque, Release. Nothing of the function is restated here, and any build of oracle/_ref answers."""
    images = [np.ascontiguousarray(i).view(np.uint8).reshape(-1) for i in images]
    nbytes = image_bytes(fmt, width, height)
    assert all(i.size == nbytes for i in images), ([i.size for i in images], fmt, width, height)
    lib = _load_ref()
    si = ctypes.create_string_buffer(256)
    hr = lib._ZN7DirectX12ScratchImage12Initialize2DE11DXGI_FORMATmmmmNS_8CP_FLAGSE(si, fmt, width, height, len(images), 1, 0)
    if hr < 0:
        raise RefError(hr)
    try:
        for item, px in enumerate(images):
            im = lib._ZNK7DirectX12ScratchImage8GetImageEmmm(si, 0, item, 0).contents
            rows = im.slicePitch // im.rowPitch
            assert nbytes % rows == 0 and nbytes // rows <= im.rowPitch, (nbytes, rows, im.rowPitch)
            for y, row in enumerate(px.reshape(rows, -1)):
                ctypes.memmove(im.pixels + y * im.rowPitch, row.ctypes.data, row.size)
        return bool(lib._ZNK7DirectX12ScratchImage16IsAlphaAllOpaqueEv(si))
    finally:
        lib._ZN7DirectX12ScratchImage7ReleaseEv(si)


def texture_bytes(fmt, width, height, array_size, mip_levels):
    return array_size * sum(image_bytes(fmt, w, h) for w, h in mip_sizes(width, height, mip_levels))


def ref_save_dds(pixels, width, height, fmt, array_size=1, mip_levels=1, misc_flags=0, dds_flags=0):
    """DirectX::SaveToDDSMemory (DirectXTexDDS.cpp:2403-2698) of a texture given in ScratchImage order with tight pitches."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    assert px.size == texture_bytes(fmt, width, height, array_size, mip_levels)
    return _run(_load_ref().dxtex_ref_save_dds, px.size + 256, px.ctypes.data, width, height, fmt, array_size, mip_levels, misc_flags, dds_flags)


def ref_save_dds_volume(pixels, width, height, depth, fmt, mip_levels=1, dds_flags=0):
    """DirectX::SaveToDDSMemory of a volume texture given in ScratchImage order with tight pitches."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    return _run(_load_ref().dxtex_ref_save_dds_volume, px.size + 256, px.ctypes.data, width, height, depth, fmt, mip_levels, dds_flags)


def ref_load_dds(data, dds_flags=0):
    """DirectX::LoadFromDDSMemory (DirectXTexDDS.cpp:2008-2107) -> (metadata dict, pixel blob); raises RefError on failure."""
    hr, meta, px = ref_load_dds_ex(data, dds_flags)
    if meta is None:
        raise RefError(hr - (1 << 32) if hr & 0x80000000 else hr)
    return meta, px


DDS_META_KEYS = ("width", "height", "depth", "format", "arraySize", "mipLevels", "miscFlags", "miscFlags2", "dimension")


def ref_load_dds_ex(data, dds_flags=0, capacity=None):
    """DirectX::LoadFromDDSMemory with DDS_FLAGS -> (hr, metadata dict or None, pixel blob or None). Never raises on a bad
    file: the HRESULT is the result to compare."""
    d = np.ascontiguousarray(data, np.uint8)
    meta = (ctypes.c_uint64 * 9)()
    out = np.zeros(capacity if capacity is not None else d.size * 16 + 4096, np.uint8)
    hr = ctypes.c_int32(0)
    n = _load_ref().dxtex_ref_load_dds_ex(d.ctypes.data, d.size, dds_flags, meta, out.ctypes.data, out.nbytes, ctypes.byref(hr))
    if n == -2:
        raise MemoryError("ref_load_dds_ex: capacity too small")
    if n < 0:
        return hr.value & 0xFFFFFFFF, None, None
    return hr.value & 0xFFFFFFFF, {k: int(v) for k, v in zip(DDS_META_KEYS, meta)}, out[:n].copy()


def ref_save_dds_ex(pixels, width, height, depth, fmt, array_size, mip_levels, misc_flags, misc_flags2, dimension, dds_flags):
    """DirectX::SaveToDDSMemory of any texture -> (hr, file bytes or None)."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    out = np.zeros(px.size + 4096, np.uint8)
    hr = ctypes.c_int32(0)
    n = _load_ref().dxtex_ref_save_dds_ex(px.ctypes.data, width, height, depth, fmt, array_size, mip_levels, misc_flags, misc_flags2, dimension, dds_flags,
                                          out.ctypes.data, out.nbytes, ctypes.byref(hr))
    if n < 0:
        return hr.value & 0xFFFFFFFF, None
    return hr.value & 0xFFFFFFFF, out[:n].copy()


def ref_format_facts(fmt):
    """-> (bits per pixel, predicate bits: 1 compressed, 2 packed, 4 planar, 8 palettised, 16 sRGB, 32 valid)."""
    bpp = ctypes.c_size_t(0)
    bits = _load_ref().dxtex_ref_format_facts(fmt, ctypes.byref(bpp))
    return bpp.value, bits


def ref_compute_pitch(fmt, width, height, cp_flags=0):
    """DirectX::ComputePitch / ComputeScanlines -> (hr, rowPitch, slicePitch, scanlines)."""
    rp, sp, sl = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    hr = _load_ref().dxtex_ref_compute_pitch_ex(fmt, width, height, cp_flags, ctypes.byref(rp), ctypes.byref(sp), ctypes.byref(sl))
    return hr & 0xFFFFFFFF, rp.value, sp.value, sl.value


def ref_format_facts2(fmt):
    """-> ([BitsPerColor, BytesPerBlock, MakeSRGB, MakeLinear, MakeTypeless, MakeTypelessUNORM, MakeTypelessFLOAT], predicate bits:
    1 video, 2 depth-stencil, 4 BGR, 8 typeless incl. partially typeless, 16 fully typeless)."""
    out = (ctypes.c_size_t * 7)()
    bits = _load_ref().dxtex_ref_format_facts2(fmt, out)
    return [int(v) for v in out], bits


def ref_load_hdr(data):
    """DirectX::LoadFromHDRMemory -> (hr, {width, height, format, miscFlags2} or None, RGBA32F bytes or None)."""
    d = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
    meta = (ctypes.c_uint64 * 4)()
    out = np.zeros(1 << 22, np.uint8)
    hr = ctypes.c_int32(0)
    n = _load_ref().dxtex_ref_load_hdr(d.ctypes.data, d.size, meta, out.ctypes.data, out.nbytes, ctypes.byref(hr))
    if n == -2:
        raise MemoryError("ref_load_hdr: capacity")
    if n < 0:
        return hr.value & 0xFFFFFFFF, None, None
    return hr.value & 0xFFFFFFFF, dict(zip(("width", "height", "format", "miscFlags2"), (int(v) for v in meta))), out[:n].copy()


def ref_save_hdr(pixels, width, height, fmt, row_pitch):
    """DirectX::SaveToHDRMemory -> (hr, file bytes or None)."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    out = np.zeros(width * height * 4 + 4096, np.uint8)
    hr = ctypes.c_int32(0)
    n = _load_ref().dxtex_ref_save_hdr(px.ctypes.data, width, height, fmt, row_pitch, out.ctypes.data, out.nbytes, ctypes.byref(hr))
    if n < 0:
        return hr.value & 0xFFFFFFFF, None
    return hr.value & 0xFFFFFFFF, out[:n].copy()


TGA_META_KEYS = ("width", "height", "format", "miscFlags2", "imageFormat", "queryHr", "queryFormat", "queryMiscFlags2")


def ref_load_tga(data, flags=0):
    """DirectX::LoadFromTGAMemory (+ GetMetadataFromTGAMemory) -> (hr, dict of TGA_META_KEYS or None, pixel bytes or None)."""
    d = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
    meta = (ctypes.c_uint64 * 8)()
    out = np.zeros(1 << 22, np.uint8)
    hr = ctypes.c_int32(0)
    n = _load_ref().dxtex_ref_load_tga(d.ctypes.data, d.size, flags, meta, out.ctypes.data, out.nbytes, ctypes.byref(hr))
    if n == -2:
        raise MemoryError("ref_load_tga: capacity")
    if n < 0:
        return hr.value & 0xFFFFFFFF, None, None
    return hr.value & 0xFFFFFFFF, dict(zip(TGA_META_KEYS, (int(v) for v in meta))), out[:n].copy()


def ref_save_tga(pixels, width, height, fmt, row_pitch, flags=0, alpha_mode=-1):
    """DirectX::SaveToTGAMemory -> (hr, file bytes or None); alpha_mode >= 0 passes metadata (TGA 2.0 extension area)."""
    px = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
    out = np.zeros(width * height * 4 + 4096, np.uint8)
    hr = ctypes.c_int32(0)
    n = _load_ref().dxtex_ref_save_tga(px.ctypes.data, width, height, fmt, row_pitch, flags, alpha_mode, out.ctypes.data, out.nbytes, ctypes.byref(hr))
    if n < 0:
        return hr.value & 0xFFFFFFFF, None
    return hr.value & 0xFFFFFFFF, out[:n].copy()


def ref_tile_shape(fmt, dimension):
    """DirectX::ComputeTileShape -> (hr, width, height, depth)."""
    out = (ctypes.c_size_t * 3)()
    hr = _load_ref().dxtex_ref_tile_shape(fmt, dimension, out)
    return hr & 0xFFFFFFFF, int(out[0]), int(out[1]), int(out[2])


def ref_triangle_filter(source, dest, wrap):
    """The reference's CreateTriangleFilter (filters.h:249-419) -> arrays (src, dst, weight bits as uint32), source-major."""
    cap = 4 * (source + dest) + 64
    s = np.zeros(cap, np.uint32); d = np.zeros(cap, np.uint32); w = np.zeros(cap, np.float32)
    n = _load_ref().dxtex_ref_triangle_filter(source, dest, 1 if wrap else 0, s.ctypes.data, d.ctypes.data, w.ctypes.data, cap)
    assert n >= 0, n
    return s[:n].copy(), d[:n].copy(), w[:n].view(np.uint32).copy()
