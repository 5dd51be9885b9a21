"""ctypes binding of include/dxtex_amd.h. One-to-one with the C ABI; numpy arrays carry host pixels,
integers carry device pointers (e.g. ``torch.Tensor.data_ptr()``)."""
import ctypes
import os

import numpy as np

from . import formats as F

_HERE = os.path.dirname(os.path.abspath(__file__))


_loaded = {"path": None, "dev": False}


def library_path(dev=None):
    """Path of the loaded library (dev=None), of the product library (dev=False) or of the development build (dev=True)."""
    if dev is None:
        return _loaded["path"]
    return os.path.join(_HERE, "lib", "libdxtex_amd_dev.so" if dev else "libdxtex_amd.so")


def _open(dev):
    path = library_path(dev)
    if not os.path.exists(path):
        raise ImportError(
            f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the MI355X path)")
    try:
        # Share PyTorch's HIP runtime when PyTorch is in the process (same SONAME libamdhip64.so.7), so that
        # torch device pointers and streams are valid in this library.
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI itself
        pass
    # RTLD_LOCAL: the product and the development build export the same C++ symbols (dxtex::launch_*); with both in the global scope the
    # second one's internal calls would bind to the first one's definitions and a development knob would silently do nothing. (The libraries
    # are also linked with -Bsymbolic-functions, so each binds its own calls whatever the loader is told.) libamdhip64 is shared with
    # PyTorch by its SONAME, not through this handle's visibility.
    return ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL), path


class Volume(ctypes.Structure):
    """dxtex_volume (include/dxtex_amd.h): one mip level of a volume texture."""
    _fields_ = [("width", ctypes.c_size_t), ("height", ctypes.c_size_t), ("depth", ctypes.c_size_t), ("format", ctypes.c_int32),
                ("rowPitch", ctypes.c_size_t), ("slicePitch", ctypes.c_size_t), ("pixels", ctypes.c_void_p)]


class Image(ctypes.Structure):
    """Mirrors ``dxtex_image`` / ``DirectX::Image`` (DirectXTex.h:437-445)."""
    _fields_ = [("width", ctypes.c_size_t), ("height", ctypes.c_size_t), ("format", ctypes.c_int32),
                ("rowPitch", ctypes.c_size_t), ("slicePitch", ctypes.c_size_t), ("pixels", ctypes.c_void_p)]


class JpegComponent(ctypes.Structure):
    """dxtex_jpeg_component (include/dxtex_amd.h): one component of a JPEG frame."""
    _fields_ = [("h", ctypes.c_uint32), ("v", ctypes.c_uint32), ("quant", ctypes.c_uint32), ("blocksPerRow", ctypes.c_uint32), ("blockRows", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("offset", ctypes.c_uint64)]


class JpegFrame(ctypes.Structure):
    """dxtex_jpeg_frame (include/dxtex_amd.h): a JPEG frame, its components and quantiser tables in natural order."""
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("components", ctypes.c_uint32), ("colour", ctypes.c_uint32),
                ("component", JpegComponent * 3), ("quant", (ctypes.c_uint16 * 64) * 4)]


class ExrChunk(ctypes.Structure):
    """dxtex_exr_chunk (include/dxtex_amd.h): one chunk of an .exr file's expanded stream."""
    _fields_ = [("offset", ctypes.c_uint64), ("bytes", ctypes.c_uint32), ("firstRow", ctypes.c_uint32), ("rows", ctypes.c_uint32), ("coded", ctypes.c_uint32)]


class ExrChannel(ctypes.Structure):
    """dxtex_exr_channel (include/dxtex_amd.h): where one of R, G, B, A lies in a scanline, and its type."""
    _fields_ = [("offset", ctypes.c_uint32), ("type", ctypes.c_uint32)]


class TiffSegment(ctypes.Structure):
    """dxtex_tiff_segment (include/dxtex_amd.h): one strip or tile of a .tif file's expanded stream."""
    _fields_ = [("offset", ctypes.c_uint64), ("firstRow", ctypes.c_uint32), ("rows", ctypes.c_uint32), ("firstCol", ctypes.c_uint32), ("cols", ctypes.c_uint32),
                ("rowBytes", ctypes.c_uint32), ("plane", ctypes.c_uint32)]


class TiffLayout(ctypes.Structure):
    """dxtex_tiff_layout (include/dxtex_amd.h): the file as the kernels see it."""
    _fields_ = [(n, ctypes.c_uint32) for n in ("width", "height", "bits", "samples", "kind", "predictor", "bigEndian", "planar", "whiteIsZero", "opaque")]


def _tiff_tables(segments, layout, palette):
    """(TiffSegment array or None, count, TiffLayout or None, 256 words or None) from segments = [(offset, first row, rows, first column,
    columns, row bytes, plane)], layout = the ten fields of TiffLayout in order and palette = up to 256 words; None stays a null pointer."""
    seg = None if segments is None else (TiffSegment * max(1, len(segments)))(*[TiffSegment(*s) for s in segments])
    lay = None if layout is None else TiffLayout(*layout)
    pal = None if palette is None else (ctypes.c_uint32 * 256)(*[int(w) for w in palette])
    return seg, (0 if segments is None else len(segments)), lay, pal


def _exr_tables(chunks, channels):
    """(ExrChunk array or None, count, ExrChannel[4] or None) from chunks = [(offset, bytes, first row, rows, coded)] and channels =
    [(offset, type)] * 4 for R, G, B, A; None stays a null pointer."""
    ch = None if chunks is None else (ExrChunk * max(1, len(chunks)))(*[ExrChunk(*c) for c in chunks])
    tab = None if channels is None else (ExrChannel * 4)(*[ExrChannel(*c) for c in channels])
    return ch, (0 if chunks is None else len(chunks)), tab


def jpeg_frame(width, height, colour, sampling=(1, 1), quant=None, quant_of=(0, 1, 1)):
    """The JpegFrame of an image whose luma is sampling = (h, v) over 1 x 1 chroma (grey: 1 x 1), laid out as dxtex_jpeg_decode takes the
    coefficients: blocks padded to whole MCUs, one component after another. quant = up to four tables of 64 entries in natural order;
    quant_of = the table of each component."""
    f = JpegFrame()
    f.width, f.height, f.colour = width, height, colour
    f.components = 1 if colour == 0 else 3
    hmax, vmax = sampling if f.components == 3 else (1, 1)
    at = 0
    for c in range(f.components):
        h, v = (hmax, vmax) if c == 0 else (1, 1)
        k = f.component[c]
        k.h, k.v, k.quant = h, v, quant_of[c]
        k.blocksPerRow, k.blockRows, k.offset = -(-width // (8 * hmax)) * h, -(-height // (8 * vmax)) * v, at
        at += k.blocksPerRow * k.blockRows * 64
    for t, table in enumerate(quant if quant is not None else ()):
        for i, q in enumerate(table):
            f.quant[t][i] = int(q)
    return f


def jpeg_coefficient_count(frame):
    """the int16 coefficients a JpegFrame takes"""
    return sum(frame.component[c].blocksPerRow * frame.component[c].blockRows * 64 for c in range(frame.components))


class Rect(ctypes.Structure):
    """dxtex_rect / DirectX::Rect: a rectangle of texels."""
    _fields_ = [("x", ctypes.c_size_t), ("y", ctypes.c_size_t), ("w", ctypes.c_size_t), ("h", ctypes.c_size_t)]


class ImageStats(ctypes.Structure):
    """dxtex_image_stats (include/dxtex_amd.h): Analyze's figures for one image, per channel r, g, b, a."""
    _fields_ = [("min", ctypes.c_float * 4), ("max", ctypes.c_float * 4), ("avg", ctypes.c_double * 4), ("variance", ctypes.c_double * 4),
                ("luminance", ctypes.c_float), ("specials", ctypes.c_uint64 * 4)]


class Transform(ctypes.Structure):
    """dxtex_transform (include/dxtex_amd.h): one of texconv's per-texel ops for TransformImage."""
    _fields_ = [("op", ctypes.c_uint32), ("swizzle", ctypes.c_uint32 * 4), ("zero", ctypes.c_uint32 * 4), ("one", ctypes.c_uint32 * 4),
                ("colorKey", ctypes.c_uint32)]


def make_transform(op, swizzle=(0, 1, 2, 3), zero=(0, 0, 0, 0), one=(0, 0, 0, 0), color_key=0):
    """A Transform; `swizzle` may also be a texconv mask string such as "bgr1" (parse_swizzle_mask)."""
    if isinstance(swizzle, str):
        swizzle, zero, one = parse_swizzle_mask(swizzle)
    return Transform(op, (ctypes.c_uint32 * 4)(*swizzle), (ctypes.c_uint32 * 4)(*zero), (ctypes.c_uint32 * 4)(*one), color_key)


def parse_swizzle_mask(mask):
    """texconv's ParseSwizzleMask (texconv.cpp:1157-1248) -> (swizzle, zero, one), or None for a bad mask: 1 to 4 characters of
    rgbaxyzw01 (either case for the letters), the last repeated into the remaining channels."""
    if not 1 <= len(mask) <= 4:
        return None
    swz, zero, one = [0, 1, 2, 3], [0] * 4, [0] * 4
    for j, ch in enumerate(mask):
        c = ch.lower()
        for k in range(j, 4):
            if c in "rgbaxyzw":
                swz[k], zero[k], one[k] = "rgba".index(c) if c in "rgba" else "xyzw".index(c), 0, 0
            elif ch == "0":
                swz[k], zero[k], one[k] = k, 1, 0
            elif ch == "1":
                swz[k], zero[k], one[k] = k, 0, 1
            else:
                return None
    return swz, zero, one


_lib = None
_P = ctypes.POINTER
_ctx_p = ctypes.c_void_p

_SIGS = {
    "dxtex_ctx_create": (ctypes.c_int32, [ctypes.c_int, _P(_ctx_p)]),
    "dxtex_ctx_destroy": (None, [_ctx_p]),
    "dxtex_ctx_set_stream": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p]),
    "dxtex_ctx_get_stream": (ctypes.c_void_p, [_ctx_p]),
    "dxtex_ctx_synchronize": (ctypes.c_int32, [_ctx_p]),
    "dxtex_ctx_last_error": (ctypes.c_char_p, [_ctx_p]),
    "dxtex_ctx_last_kernel_ms": (ctypes.c_float, [_ctx_p]),
    "dxtex_ctx_profile_begin": (ctypes.c_int32, [_ctx_p]),
    "dxtex_ctx_profile_end": (ctypes.c_int32, [_ctx_p, ctypes.c_char_p, ctypes.c_size_t, _P(ctypes.c_float), _P(ctypes.c_uint32), ctypes.c_size_t, _P(ctypes.c_size_t)]),
    "dxtex_is_compressed": (ctypes.c_int, [ctypes.c_int32]),
    "dxtex_bits_per_pixel": (ctypes.c_size_t, [ctypes.c_int32]),
    "dxtex_compute_pitch": (ctypes.c_int32, [ctypes.c_int32, ctypes.c_size_t, ctypes.c_size_t, _P(ctypes.c_size_t), _P(ctypes.c_size_t)]),
    "dxtex_ctx_prepare": (ctypes.c_int32, [_ctx_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32, ctypes.c_size_t, _P(ctypes.c_size_t)]),
    "dxtex_compress": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_compress_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_compress_many_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_size_t, ctypes.c_uint32, ctypes.c_float]),
    "dxtex_decompress": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image)]),
    "dxtex_decompress_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image)]),
    "dxtex_encode_blocks": (ctypes.c_int32, [_ctx_p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dxtex_decode_blocks": (ctypes.c_int32, [_ctx_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]),
    "dxtex_generate_mips": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_size_t, ctypes.c_uint32]),
    "dxtex_compress_multi": (ctypes.c_int32, [_P(_ctx_p), ctypes.c_size_t, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_generate_mips_multi": (ctypes.c_int32, [_P(_ctx_p), ctypes.c_size_t, _P(Image), ctypes.c_size_t, ctypes.c_uint32]),
    "dxtex_generate_mips_device": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_size_t, ctypes.c_uint32]),
    "dxtex_compress_many": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_size_t, ctypes.c_uint32, ctypes.c_float]),
    "dxtex_convert": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_convert_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_convert_slice": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float, ctypes.c_uint32]),
    "dxtex_convert_slice_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float, ctypes.c_uint32]),
    "dxtex_convert_dither_stats": (ctypes.c_int32, [_ctx_p, _P(ctypes.c_uint64), _P(ctypes.c_uint64)]),
    "dxtex_compute_normal_map": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_compute_normal_map_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_transform_image": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), _P(Transform)]),
    "dxtex_transform_images_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_size_t, _P(Transform)]),
    "dxtex_rotate_color": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_rotate_color_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_size_t, ctypes.c_uint32, ctypes.c_float]),
    "dxtex_rgbe_decode": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_float]),
    "dxtex_rgbe_decode_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_float]),
    "dxtex_rgbe_encode": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image)]),
    "dxtex_rgbe_encode_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image)]),
    "dxtex_tga_unpack": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, _P(Image), _P(ctypes.c_uint32)]),
    "dxtex_tga_unpack_device": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, _P(Image), ctypes.c_void_p]),
    "dxtex_tga_pack": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_tga_pack_device": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_dds_unpack": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, _P(Image), _P(ctypes.c_size_t), _P(ctypes.c_size_t), ctypes.c_size_t]),
    "dxtex_dds_unpack_device": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, _P(Image), _P(ctypes.c_size_t), _P(ctypes.c_size_t), ctypes.c_size_t]),
    "dxtex_dds_pack24": (ctypes.c_int32, [_ctx_p, _P(Image), _P(ctypes.c_size_t), _P(ctypes.c_size_t), ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_dds_pack24_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(ctypes.c_size_t), _P(ctypes.c_size_t), ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_pnm_unpack": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P(Image)]),
    "dxtex_pnm_unpack_device": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, _P(Image)]),
    "dxtex_pnm_pack": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_pnm_pack_device": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_png_unpack": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, _P(Image)]),
    "dxtex_png_unpack_device": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32, _P(Image)]),
    "dxtex_png_pack": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_png_pack_device": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_jpeg_decode": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, _P(JpegFrame), _P(Image)]),
    "dxtex_jpeg_decode_device": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, _P(JpegFrame), _P(Image)]),
    "dxtex_jpeg_encode": (ctypes.c_int32, [_ctx_p, _P(Image), _P(JpegFrame), ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_jpeg_encode_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(JpegFrame), ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_exr_unpack": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_exr_unpack_device": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_exr_pack": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_exr_pack_device": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_tiff_unpack": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, _P(Image)]),
    "dxtex_tiff_unpack_device": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, _P(Image)]),
    "dxtex_tiff_pack": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_tiff_pack_device": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_generate_mips3d": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32]),
    "dxtex_generate_mips3d_device": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32]),
    "dxtex_premultiply_alpha": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32]),
    "dxtex_premultiply_alpha_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32]),
    "dxtex_scale_mips_alpha_for_coverage": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_size_t, ctypes.c_float]),
    "dxtex_scale_mips_alpha_for_coverage_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_size_t, ctypes.c_float]),
    "dxtex_resize": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32]),
    "dxtex_resize_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32]),
    "dxtex_compute_mse_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), _P(ctypes.c_double)]),
    "dxtex_compute_mse_flags_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32, _P(ctypes.c_double)]),
    "dxtex_analyze": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_size_t, _P(ImageStats)]),
    "dxtex_analyze_device": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_size_t, _P(ImageStats)]),
    "dxtex_analyze_bc": (ctypes.c_int32, [_ctx_p, _P(Image), _P(ctypes.c_uint64), _P(ctypes.c_uint64)]),
    "dxtex_analyze_bc_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(ctypes.c_uint64), _P(ctypes.c_uint64)]),
    "dxtex_difference": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_difference_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), _P(Image), ctypes.c_uint32, ctypes.c_float]),
    "dxtex_copy_rectangle": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Rect), _P(Image), ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t]),
    "dxtex_copy_rectangles_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Rect), _P(Image), _P(ctypes.c_size_t), _P(ctypes.c_size_t), ctypes.c_size_t, ctypes.c_uint32]),
    "dxtex_planar_to_single": (ctypes.c_int32, [ctypes.c_int32]),
    "dxtex_flip_rotate": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_uint32]),
    "dxtex_flip_rotate_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_size_t, ctypes.c_uint32]),
    "dxtex_convert_to_single_plane": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image)]),
    "dxtex_convert_to_single_plane_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), ctypes.c_size_t]),
    "dxtex_merge_image": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), _P(Image), _P(ctypes.c_uint32), _P(ctypes.c_uint32), _P(ctypes.c_uint32)]),
    "dxtex_merge_image_device": (ctypes.c_int32, [_ctx_p, _P(Image), _P(Image), _P(Image), _P(ctypes.c_uint32), _P(ctypes.c_uint32), _P(ctypes.c_uint32)]),
    "dxtex_device_alloc": (ctypes.c_int32, [_ctx_p, ctypes.c_size_t, _P(ctypes.c_void_p)]),
    "dxtex_device_free": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p]),
    "dxtex_memcpy_h2d": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_memcpy_d2h": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_device_memset": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]),
    "dxtex_copy_rows_device": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]),
    "dxtex_memcpy_h2d_async": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_memcpy_d2h_async": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]),
    "dxtex_memcpy_rows_d2h_async": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t]),
    "dxtex_host_alloc": (ctypes.c_int32, [_ctx_p, ctypes.c_size_t, _P(ctypes.c_void_p)]),
    "dxtex_host_free": (ctypes.c_int32, [_ctx_p, ctypes.c_void_p]),
    "dxtex_alpha_all_opaque_device": (ctypes.c_int32, [_ctx_p, _P(Image), ctypes.c_size_t, _P(ctypes.c_int)]),
    "dxtex_ctx_transfer_bytes": (ctypes.c_int32, [_ctx_p, _P(ctypes.c_uint64), _P(ctypes.c_uint64), ctypes.c_int]),
}
def load(dev=False):
    """Binds this module to the product library (the default, done at import) or - dev=True - to libdxtex_amd_dev.so: the same sources
    compiled with -DDXTEX_DEV, the only build that reads DXTEX_* development knobs from the environment. The choice is this explicit
    call, made by the tests and tools that need knobs before they create a Context; no environment variable selects a library, so
    nothing in a user's shell changes what `import directxtex_amd` runs. A Context keeps the library that created it (its handle belongs to
    that library's statics), so contexts of both builds can live side by side; module-level helpers follow the latest load()."""
    global _lib
    lib, path = _open(dev)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)     # AttributeError here == the .so does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    _loaded["path"], _loaded["dev"] = path, bool(dev)
    return path


load(False)

EXPORTED_SYMBOLS = tuple(_SIGS)


class DxtexError(RuntimeError):
    def __init__(self, hr, msg=""):
        self.hresult = hr
        super().__init__(f"HRESULT 0x{hr & 0xFFFFFFFF:08X} {msg}".strip())


def compute_pitch(fmt, width, height):
    rp, sp = ctypes.c_size_t(), ctypes.c_size_t()
    hr = _lib.dxtex_compute_pitch(fmt, width, height, ctypes.byref(rp), ctypes.byref(sp))
    if hr != 0:
        raise DxtexError(hr, "compute_pitch")
    return rp.value, sp.value


def planar_to_single(fmt):
    """PlanarToSingle: the single-plane format ConvertToSinglePlane gives a planar one (NV12, NV11 -> YUY2; P010 -> Y210; P016 -> Y216),
    0 where there is none."""
    return int(_lib.dxtex_planar_to_single(fmt))


def _planar_pitches(fmt, width, height):
    """ComputePitch (DirectXTexUtil.cpp:1054-1112) of the planar formats ConvertToSinglePlane takes: (rowPitch, slicePitch). Only the
    default layout of Context.convert_to_single_plane; the C ABI takes both pitches from the caller."""
    if fmt == 110:                      # NV11
        row = ((width + 3) >> 2) * 4
        return row, row * height * 2
    if fmt not in (103, 104, 105):      # NV12, P010, P016
        raise DxtexError(-2147024846, "no single-plane form")
    row = ((width + 1) >> 1) * (2 if fmt == 103 else 4)
    return row, row * (height + ((height + 1) >> 1))


def is_compressed(fmt):
    return bool(_lib.dxtex_is_compressed(fmt))


def bits_per_pixel(fmt):
    return int(_lib.dxtex_bits_per_pixel(fmt))


def _host_image(arr, width, height, fmt, row_pitch=None):
    """numpy buffer -> dxtex_image (host pointer). `arr` must be C-contiguous."""
    assert arr.flags["C_CONTIGUOUS"]
    rp, sp = compute_pitch(fmt, width, height)
    if row_pitch is not None:
        rows = sp // rp
        rp, sp = row_pitch, row_pitch * rows
    assert arr.nbytes >= sp, (arr.nbytes, sp)
    return Image(width, height, fmt, rp, sp, arr.ctypes.data)


def device_image(ptr, width, height, fmt, row_pitch=None, slice_pitch=None):
    """A dxtex_image on device memory. The pitches default to compute_pitch's; a planar source (convert_to_single_plane_device), which
    compute_pitch does not take, is described by both row_pitch and slice_pitch."""
    if row_pitch is not None and slice_pitch is not None:
        return Image(width, height, fmt, row_pitch, slice_pitch, ptr)
    rp, sp = compute_pitch(fmt, width, height)
    if row_pitch is not None:
        rows = sp // rp
        rp, sp = row_pitch, row_pitch * rows
    if slice_pitch is not None:
        sp = slice_pitch
    return Image(width, height, fmt, rp, sp, ptr)


def _ctx_array(contexts):
    libs = {id(c._lib) for c in contexts}
    assert len(libs) == 1, "the contexts of one call must come from one library"
    return (_ctx_p * len(contexts))(*[c._h for c in contexts])


def compress_multi(contexts, pixels, width, height, src_format, dst_format, flags=0, threshold=0.5, out=None):
    """ONE host image over several contexts (dxtex_compress_multi: stripes of block rows, a thread per context) -> the BC payload,
    byte for byte what contexts[0].compress returns."""
    pixels = np.ascontiguousarray(pixels)
    src = _host_image(pixels, width, height, src_format)
    rp, sp = compute_pitch(dst_format, width, height)
    if out is None:
        out = np.zeros(sp, np.uint8)
    dst = Image(width, height, dst_format, rp, sp, out.ctypes.data)
    c0 = contexts[0]
    c0._check(c0._lib.dxtex_compress_multi(_ctx_array(contexts), len(contexts), ctypes.byref(src), ctypes.byref(dst), flags, threshold), "compress_multi")
    return out


def generate_mips_multi(contexts, level0, width, height, fmt, nlevels, filter_flags=0):
    """dxtex_generate_mips_multi: the chain of a host image with its large levels cut into stripes of rows over the contexts; returns the
    levels as uint8 arrays (tight pitch), identical to contexts[0].generate_mips."""
    bufs, levels = [], []
    w, h = width, height
    for i in range(nlevels):
        rp, sp = compute_pitch(fmt, w, h)
        buf = np.zeros(sp, np.uint8)
        if i == 0:
            buf[:] = np.ascontiguousarray(level0).view(np.uint8).reshape(-1)[:sp]
        bufs.append(buf)
        levels.append(Image(w, h, fmt, rp, sp, buf.ctypes.data))
        w, h = max(1, w >> 1), max(1, h >> 1)
    arr = (Image * nlevels)(*levels)
    c0 = contexts[0]
    c0._check(c0._lib.dxtex_generate_mips_multi(_ctx_array(contexts), len(contexts), arr, nlevels, filter_flags), "generate_mips_multi")
    return bufs


class Context:
    """One context per GPU (``dxtex_ctx``)."""

    def __init__(self, device=0):
        self._h = _ctx_p()
        self._lib = _lib            # the library that creates the handle serves it for life, whatever load() binds the module to later
        hr = self._lib.dxtex_ctx_create(device, ctypes.byref(self._h))
        if hr != 0:
            raise DxtexError(hr, "dxtex_ctx_create: no usable gfx950 device (this library has no CPU path)")
        self.device = device

    def close(self):
        if self._h:
            self._lib.dxtex_ctx_destroy(self._h)
            self._h = _ctx_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, hr, what):
        if hr != 0:
            raise DxtexError(hr, f"{what}: {self._lib.dxtex_ctx_last_error(self._h).decode()}")

    # -- plumbing ---------------------------------------------------------------------------------
    def set_stream(self, stream_ptr):
        self._check(self._lib.dxtex_ctx_set_stream(self._h, stream_ptr), "set_stream")

    def stream(self):
        return self._lib.dxtex_ctx_get_stream(self._h)

    def synchronize(self):
        self._check(self._lib.dxtex_ctx_synchronize(self._h), "synchronize")

    def last_kernel_ms(self):
        return float(self._lib.dxtex_ctx_last_kernel_ms(self._h))

    def profile_begin(self):
        self._check(self._lib.dxtex_ctx_profile_begin(self._h), "profile_begin")

    def profile_end(self):
        """-> {kernel name: (total ms, launches)} since profile_begin (synchronises the stream)."""
        cap = 256
        names = ctypes.create_string_buffer(16384)
        ms = (ctypes.c_float * cap)()
        n = (ctypes.c_uint32 * cap)()
        cnt = ctypes.c_size_t()
        self._check(self._lib.dxtex_ctx_profile_end(self._h, names, 16384, ms, n, cap, ctypes.byref(cnt)), "profile_end")
        keys = names.value.decode().split("\n")[:cnt.value]
        return {k: (float(ms[i]), int(n[i])) for i, k in enumerate(keys)}

    # -- device-resident pipeline helpers -----------------------------------------------------------
    def device_alloc(self, nbytes, zero=False):
        p = ctypes.c_void_p()
        self._check(self._lib.dxtex_device_alloc(self._h, nbytes, ctypes.byref(p)), "device_alloc")
        if zero:
            self._check(self._lib.dxtex_device_memset(self._h, p, 0, nbytes), "device_memset")
        return p.value

    def device_free(self, ptr):
        self._check(self._lib.dxtex_device_free(self._h, ptr), "device_free")

    def host_alloc(self, nbytes):
        """Page-locked host memory as a numpy uint8 array (free with host_free(arr.ctypes.data) after the last use)."""
        p = ctypes.c_void_p()
        self._check(self._lib.dxtex_host_alloc(self._h, nbytes, ctypes.byref(p)), "host_alloc")
        return np.ctypeslib.as_array(ctypes.cast(p, _P(ctypes.c_uint8)), shape=(nbytes,))

    def host_free(self, ptr):
        self._check(self._lib.dxtex_host_free(self._h, ptr), "host_free")

    def upload(self, dst_ptr, arr, nbytes=None, sync=False):
        """Stream-ordered host -> device copy of a C-contiguous numpy buffer (keep it alive until synchronize())."""
        n = arr.nbytes if nbytes is None else nbytes
        fn = self._lib.dxtex_memcpy_h2d if sync else self._lib.dxtex_memcpy_h2d_async
        self._check(fn(self._h, dst_ptr, arr.ctypes.data, n), "upload")

    def download(self, arr, src_ptr, nbytes=None, sync=False):
        n = arr.nbytes if nbytes is None else nbytes
        fn = self._lib.dxtex_memcpy_d2h if sync else self._lib.dxtex_memcpy_d2h_async
        self._check(fn(self._h, arr.ctypes.data, src_ptr, n), "download")

    def copy_rows_device(self, dst_ptr, dst_pitch, src_ptr, src_pitch, row_bytes, rows):
        self._check(self._lib.dxtex_copy_rows_device(self._h, dst_ptr, dst_pitch, src_ptr, src_pitch, row_bytes, rows), "copy_rows_device")

    def alpha_all_opaque_device(self, images):
        arr = (Image * len(images))(*images)
        out = ctypes.c_int(0)
        self._check(self._lib.dxtex_alpha_all_opaque_device(self._h, arr, len(images), ctypes.byref(out)), "alpha_all_opaque_device")
        return bool(out.value)

    def transfer_bytes(self, reset=False):
        """(host -> device bytes, device -> host bytes) this context has moved since creation / the last reset."""
        up, down = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.dxtex_ctx_transfer_bytes(self._h, ctypes.byref(up), ctypes.byref(down), 1 if reset else 0), "transfer_bytes")
        return int(up.value), int(down.value)

    # -- Compress -----------------------------------------------------------------------------------
    def prepare(self, width, height, src_format, dst_format, flags=0, count=1):
        """GPUCompressBC::Prepare's role: allocate the search scratch and staging for `count` images of this shape now.
        Returns the bytes of device memory the context holds afterwards."""
        held = ctypes.c_size_t(0)
        self._check(self._lib.dxtex_ctx_prepare(self._h, width, height, src_format, dst_format, flags, count, ctypes.byref(held)), "prepare")
        return held.value

    def compress(self, pixels, width, height, src_format, dst_format, flags=0, threshold=0.5, src_row_pitch=None):
        """Host image (numpy, any dtype, C-contiguous rows) -> numpy uint8 BC payload (tight pitch)."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, src_format, src_row_pitch)
        rp, sp = compute_pitch(dst_format, width, height)
        out = np.zeros(sp, np.uint8)
        dst = Image(width, height, dst_format, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_compress(self._h, ctypes.byref(src), ctypes.byref(dst), flags, threshold), "compress")
        return out

    def compress_into(self, pixels, width, height, src_format, out, dst_format, flags=0, threshold=0.5):
        """dxtex_compress with caller-owned buffers on both sides (e.g. pinned memory): `out` receives the tight BC payload."""
        src = _host_image(pixels, width, height, src_format)
        rp, sp = compute_pitch(dst_format, width, height)
        assert out.flags["C_CONTIGUOUS"] and out.nbytes >= sp
        dst = Image(width, height, dst_format, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_compress(self._h, ctypes.byref(src), ctypes.byref(dst), flags, threshold), "compress")

    def compress_device(self, src_ptr, width, height, src_format, dst_ptr, dst_format, flags=0, threshold=0.5, src_row_pitch=None):
        src = device_image(src_ptr, width, height, src_format, src_row_pitch)
        dst = device_image(dst_ptr, width, height, dst_format)
        self._check(self._lib.dxtex_compress_device(self._h, ctypes.byref(src), ctypes.byref(dst), flags, threshold), "compress_device")

    def compress_many_device(self, srcs, dsts, flags=0, threshold=0.5):
        n = len(srcs)
        a = (Image * n)(*srcs)
        b = (Image * n)(*dsts)
        self._check(self._lib.dxtex_compress_many_device(self._h, a, b, n, flags, threshold), "compress_many_device")

    def compress_many(self, images, width, height, src_format, dst_format, flags=0, threshold=0.5):
        """Array of same-sized host images -> list of BC payloads, through dxtex_compress_many (the cfg5 entry point: chunks of the
        array are staged through pinned memory on copy streams while the previous chunk is searched)."""
        images = [np.ascontiguousarray(im) for im in images]
        n = len(images)
        rp, sp = compute_pitch(dst_format, width, height)
        outs = [np.zeros(sp, np.uint8) for _ in range(n)]
        srcs = (Image * n)(*[_host_image(im, width, height, src_format) for im in images])
        dsts = (Image * n)(*[Image(width, height, dst_format, rp, sp, o.ctypes.data) for o in outs])
        self._check(self._lib.dxtex_compress_many(self._h, srcs, dsts, n, flags, threshold), "compress_many")
        return outs

    def compress_array(self, items, dst_format, flags=0, threshold=0.5):
        """General form of dxtex_compress_many: items = [(pixels, width, height, src_format, src_row_pitch or None), ...] - any mix
        of sizes and source formats, as the images of a DirectX::Compress array call may be. Returns the list of tight BC payloads."""
        keep = [np.ascontiguousarray(it[0]) for it in items]
        n = len(items)
        outs, srcs, dsts = [], [], []
        for arr, (_, w, h, fmt, pitch) in zip(keep, items):
            srcs.append(_host_image(arr, w, h, fmt, pitch))
            rp, sp = compute_pitch(dst_format, w, h)
            o = np.zeros(sp, np.uint8); outs.append(o)
            dsts.append(Image(w, h, dst_format, rp, sp, o.ctypes.data))
        a = (Image * n)(*srcs); b = (Image * n)(*dsts)
        self._check(self._lib.dxtex_compress_many(self._h, a, b, n, flags, threshold), "compress_many")
        return outs

    def encode_blocks(self, bc_format, rgba, flags=0, threshold=0.5):
        rgba = np.ascontiguousarray(rgba, np.float32).reshape(-1, 16, 4)
        n = rgba.shape[0]
        out = np.zeros((n, F.BC_BLOCK_BYTES[bc_format]), np.uint8)
        self._check(self._lib.dxtex_encode_blocks(self._h, bc_format, flags, threshold, rgba.ctypes.data, n, out.ctypes.data), "encode_blocks")
        return out

    def decode_blocks(self, bc_format, blocks):
        blocks = np.ascontiguousarray(blocks, np.uint8).reshape(-1, F.BC_BLOCK_BYTES[bc_format])
        n = blocks.shape[0]
        out = np.zeros((n, 16, 4), np.float32)
        self._check(self._lib.dxtex_decode_blocks(self._h, bc_format, blocks.ctypes.data, n, out.ctypes.data), "decode_blocks")
        return out

    def decompress(self, payload, width, height, bc_format, dst_format):
        payload = np.ascontiguousarray(payload, np.uint8)
        src = _host_image(payload, width, height, bc_format)
        rp, sp = compute_pitch(dst_format, width, height)
        out = np.zeros(sp, np.uint8)
        dst = Image(width, height, dst_format, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_decompress(self._h, ctypes.byref(src), ctypes.byref(dst)), "decompress")
        return out

    def decompress_device(self, src_ptr, width, height, bc_format, dst_ptr, dst_format):
        src = device_image(src_ptr, width, height, bc_format)
        dst = device_image(dst_ptr, width, height, dst_format)
        self._check(self._lib.dxtex_decompress_device(self._h, ctypes.byref(src), ctypes.byref(dst)), "decompress_device")

    def compute_mse_device(self, a_ptr, a_format, b_ptr, b_format, width, height):
        """Per-channel MSE (4 doubles) of two device images of the same size."""
        a = device_image(a_ptr, width, height, a_format)
        b = device_image(b_ptr, width, height, b_format)
        out = (ctypes.c_double * 4)()
        self._check(self._lib.dxtex_compute_mse_device(self._h, ctypes.byref(a), ctypes.byref(b), out), "compute_mse_device")
        return np.array(list(out), np.float64)

    # -- texdiag's diagnostics -------------------------------------------------------------------------
    def compute_mse_flags_device(self, a, b, flags=0):
        """dxtex_compute_mse_flags_device: per-channel MSE (4 doubles) of two device Images (device_image) under CMSE_FLAGS."""
        out = (ctypes.c_double * 4)()
        self._check(self._lib.dxtex_compute_mse_flags_device(self._h, ctypes.byref(a), ctypes.byref(b), flags, out), "compute_mse_flags_device")
        return np.array(list(out), np.float64)

    @staticmethod
    def _stats(s):
        return {"min": np.array(list(s.min), np.float32), "max": np.array(list(s.max), np.float32), "avg": np.array(list(s.avg), np.float64),
                "variance": np.array(list(s.variance), np.float64), "luminance": np.float32(s.luminance),
                "specials": np.array(list(s.specials), np.uint64)}

    def analyze_device(self, images):
        """dxtex_analyze_device: a list of device Images -> one dict per image (min, max, avg, variance, luminance, specials)."""
        n = len(images)
        arr, out = (Image * max(n, 1))(*images), (ImageStats * max(n, 1))()
        self._check(self._lib.dxtex_analyze_device(self._h, arr, n, out), "analyze_device")
        return [self._stats(out[i]) for i in range(n)]

    def analyze(self, items):
        """dxtex_analyze: items = [(pixels, width, height, format, row_pitch or None), ...] in host memory -> one dict per image."""
        keep = [np.ascontiguousarray(it[0]) for it in items]
        n = len(items)
        arr = (Image * max(n, 1))(*[_host_image(k, w, h, f, rp) for k, (_, w, h, f, rp) in zip(keep, items)])
        out = (ImageStats * max(n, 1))()
        self._check(self._lib.dxtex_analyze(self._h, arr, n, out), "analyze")
        return [self._stats(out[i]) for i in range(n)]

    def analyze_bc_device(self, image):
        """dxtex_analyze_bc_device: a device Image of a BC format -> (the 15 bins as uint64, the number of blocks)."""
        hist, blocks = (ctypes.c_uint64 * 15)(), ctypes.c_uint64(0)
        self._check(self._lib.dxtex_analyze_bc_device(self._h, ctypes.byref(image), hist, ctypes.byref(blocks)), "analyze_bc_device")
        return np.array(list(hist), np.uint64), int(blocks.value)

    def analyze_bc(self, payload, width, height, bc_format, row_pitch=None):
        """dxtex_analyze_bc of a BC payload in host memory -> (the 15 bins as uint64, the number of blocks)."""
        payload = np.ascontiguousarray(payload)
        im = _host_image(payload, width, height, bc_format, row_pitch)
        hist, blocks = (ctypes.c_uint64 * 15)(), ctypes.c_uint64(0)
        self._check(self._lib.dxtex_analyze_bc(self._h, ctypes.byref(im), hist, ctypes.byref(blocks)), "analyze_bc")
        return np.array(list(hist), np.uint64), int(blocks.value)

    def difference_device(self, a, b, dst, diff_color=0, threshold=0.25):
        """dxtex_difference_device on device Images: b is R32G32B32A32_FLOAT, dst has a's format; asynchronous on the context's stream."""
        self._check(self._lib.dxtex_difference_device(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(dst), diff_color, threshold), "difference_device")

    def difference(self, a_pixels, b_float, width, height, fmt, diff_color=0, threshold=0.25):
        """dxtex_difference: host image `a_pixels` of `fmt` against `b_float` (R32G32B32A32_FLOAT) -> the map in `fmt` (tight pitch)."""
        a_pixels, b_float = np.ascontiguousarray(a_pixels), np.ascontiguousarray(b_float, np.float32)
        a, b = _host_image(a_pixels, width, height, fmt), _host_image(b_float, width, height, F.DXGI_FORMAT_R32G32B32A32_FLOAT)
        rp, sp = compute_pitch(fmt, width, height)
        out = np.zeros(sp, np.uint8)
        dst = Image(width, height, fmt, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_difference(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(dst), diff_color, threshold), "difference")
        return out

    # -- CopyRectangle and texassemble's merge ---------------------------------------------------------
    def copy_rectangle(self, src, rect, dst, filter_flags=0, x_offset=0, y_offset=0):
        """dxtex_copy_rectangle on host Images (their `pixels` point into numpy buffers the caller keeps alive): the w x h texels at
        rect = (x, y, w, h) of `src` into `dst` at (x_offset, y_offset); returns when the destination's rows have landed."""
        r = Rect(*rect)
        self._check(self._lib.dxtex_copy_rectangle(self._h, ctypes.byref(src), ctypes.byref(r), ctypes.byref(dst), filter_flags, x_offset, y_offset), "copy_rectangle")

    def copy_rectangles_device(self, srcs, rects, dsts, x_offsets, y_offsets, filter_flags=0):
        """dxtex_copy_rectangles_device: lists of device Images, (x, y, w, h) rectangles and offsets, one kernel launch per 32 of them;
        asynchronous on the context's stream. Each rectangle is checked against its own destination only: the rectangles of one call must
        not write bytes that another rectangle of the same call reads or writes (they run in one launch, in no order)."""
        n = len(srcs)
        m = max(n, 1)
        a, b = (Image * m)(*srcs), (Image * m)(*dsts)
        r = (Rect * m)(*[Rect(*q) for q in rects])
        xs, ys = (ctypes.c_size_t * m)(*x_offsets), (ctypes.c_size_t * m)(*y_offsets)
        self._check(self._lib.dxtex_copy_rectangles_device(self._h, a, r, b, xs, ys, n, filter_flags), "copy_rectangles_device")

    # -- FlipRotate ---------------------------------------------------------------------------------------
    def flip_rotate(self, pixels, width, height, fmt, flags, row_pitch=None):
        """dxtex_flip_rotate: the host image `pixels` turned clockwise by the angle of `flags` (TEX_FR_*), then flipped -> the result's
        bytes with tight pitch (height x width texels for ROTATE90 / ROTATE270). Texels move as bytes."""
        pixels = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
        src = _host_image(pixels, width, height, fmt, row_pitch)
        ow, oh = (height, width) if flags & 1 else (width, height)
        rp, sp = compute_pitch(fmt, ow, oh)
        out = np.zeros(max(sp, 1), np.uint8)
        dst = Image(ow, oh, fmt, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_flip_rotate(self._h, ctypes.byref(src), ctypes.byref(dst), flags), "flip_rotate")
        return out[:sp]

    def flip_rotate_device(self, srcs, dsts, flags):
        """dxtex_flip_rotate_device: lists of device Images (a destination may be a cell of a larger image: a pointer into it and its
        pitch), one kernel launch per route per 32 of them; asynchronous on the context's stream."""
        n = len(srcs)
        m = max(n, 1)
        a, b = (Image * m)(*srcs), (Image * m)(*dsts)
        self._check(self._lib.dxtex_flip_rotate_device(self._h, a, b, n, flags), "flip_rotate_device")

    # -- ConvertToSinglePlane ---------------------------------------------------------------------------
    def convert_to_single_plane(self, pixels, width, height, fmt, row_pitch=None, slice_pitch=None):
        """dxtex_convert_to_single_plane: the planar host image `pixels` (NV12, P010, P016, NV11; ComputePitch's layout unless row_pitch /
        slice_pitch say otherwise) -> its single-plane form (planar_to_single(fmt)) as bytes with tight pitch, zero where the reference's
        end guard leaves elements unwritten (a slice_pitch below the layout's)."""
        pixels = np.ascontiguousarray(pixels).view(np.uint8).reshape(-1)
        nrp, nsp = _planar_pitches(fmt, width, height) if planar_to_single(fmt) else (0, 0)
        rp = nrp if row_pitch is None else row_pitch
        sp = slice_pitch if slice_pitch is not None else (nsp // nrp) * rp if nrp else 0
        assert pixels.nbytes >= sp, (pixels.nbytes, sp)
        dfmt = planar_to_single(fmt)
        drp, dsp = compute_pitch(dfmt, width, height) if dfmt else (0, 0)
        out = np.zeros(max(dsp, 1), np.uint8)
        src = Image(width, height, fmt, rp, sp, pixels.ctypes.data)
        dst = Image(width, height, dfmt, drp, dsp, out.ctypes.data)
        self._check(self._lib.dxtex_convert_to_single_plane(self._h, ctypes.byref(src), ctypes.byref(dst)), "convert_to_single_plane")
        return out[:dsp]

    def convert_to_single_plane_device(self, srcs, dsts):
        """dxtex_convert_to_single_plane_device: lists of device Images (device_image with row_pitch and slice_pitch for the planar
        sources), one kernel launch per 32 of them; asynchronous on the context's stream."""
        n = len(srcs)
        m = max(n, 1)
        a, b = (Image * m)(*srcs), (Image * m)(*dsts)
        self._check(self._lib.dxtex_convert_to_single_plane_device(self._h, a, b, n), "convert_to_single_plane_device")

    @staticmethod
    def _merge_args(permute, zero, one):
        return (ctypes.c_uint32 * 4)(*permute), (ctypes.c_uint32 * 4)(*zero), (ctypes.c_uint32 * 4)(*one)

    def merge_image_device(self, a, b, dst, permute, zero=(0, 0, 0, 0), one=(0, 0, 0, 0)):
        """dxtex_merge_image_device on device Images: b is R32G32B32A32_FLOAT, dst has a's format; asynchronous on the context's stream."""
        p, z, o = self._merge_args(permute, zero, one)
        self._check(self._lib.dxtex_merge_image_device(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(dst), p, z, o), "merge_image_device")

    def merge_image(self, a_pixels, b_float, width, height, fmt, permute, zero=(0, 0, 0, 0), one=(0, 0, 0, 0)):
        """dxtex_merge_image: texassemble's merge of host image `a_pixels` of `fmt` with `b_float` (R32G32B32A32_FLOAT): channel k of the
        result is channel permute[k] of a (0..3) or of b (4..7), then 0 / 1 by the masks -> the merged image in `fmt` (tight pitch)."""
        a_pixels, b_float = np.ascontiguousarray(a_pixels), np.ascontiguousarray(b_float, np.float32)
        a, b = _host_image(a_pixels, width, height, fmt), _host_image(b_float, width, height, F.DXGI_FORMAT_R32G32B32A32_FLOAT)
        rp, sp = compute_pitch(fmt, width, height)
        out = np.zeros(sp, np.uint8)
        dst = Image(width, height, fmt, rp, sp, out.ctypes.data)
        p, z, o = self._merge_args(permute, zero, one)
        self._check(self._lib.dxtex_merge_image(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(dst), p, z, o), "merge_image")
        return out

    # -- GenerateMipMaps / Convert / Resize ---------------------------------------------------------
    def generate_mips(self, level0, width, height, fmt, nlevels, filter_flags):
        """Returns [level0, level1, ...] as numpy uint8 buffers with tight pitch."""
        levels, bufs = [], []
        w, h = width, height
        for i in range(nlevels):
            rp, sp = compute_pitch(fmt, w, h)
            buf = np.zeros(sp, np.uint8)
            if i == 0:
                src = np.ascontiguousarray(level0).view(np.uint8).reshape(-1)
                buf[:] = src[:sp]
            bufs.append(buf)
            levels.append(Image(w, h, fmt, rp, sp, buf.ctypes.data))
            w, h = max(1, w >> 1), max(1, h >> 1)
        arr = (Image * nlevels)(*levels)
        self._check(self._lib.dxtex_generate_mips(self._h, arr, nlevels, filter_flags), "generate_mips")
        return bufs

    def generate_mips_device(self, levels, filter_flags):
        """levels: list of device Images (capi.device_image) forming a mip chain; fills levels[1:] from levels[0]."""
        arr = (Image * len(levels))(*levels)
        self._check(self._lib.dxtex_generate_mips_device(self._h, arr, len(levels), filter_flags), "generate_mips_device")

    def convert(self, pixels, width, height, src_format, dst_format, filter_flags=0, threshold=0.5, z=0):
        """DirectX::Convert of one image; filter_flags may carry TEX_FILTER_DITHER (0x10000) / TEX_FILTER_DITHER_DIFFUSION (0x20000).
        z = the slice of a volume (the phase of ordered dithering; dxtex_convert_slice)."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, src_format)
        rp, sp = compute_pitch(dst_format, width, height)
        out = np.zeros(sp, np.uint8)
        dst = Image(width, height, dst_format, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_convert_slice(self._h, ctypes.byref(src), ctypes.byref(dst), filter_flags, threshold, z), "convert")
        return out

    def convert_device(self, src_ptr, width, height, src_format, dst_ptr, dst_format, filter_flags=0, threshold=0.5, z=0, src_row_pitch=None):
        """dxtex_convert_slice_device: device pointers (tight destination pitch), asynchronous on the context's stream."""
        src = device_image(src_ptr, width, height, src_format, src_row_pitch)
        dst = device_image(dst_ptr, width, height, dst_format)
        self._check(self._lib.dxtex_convert_slice_device(self._h, ctypes.byref(src), ctypes.byref(dst), filter_flags, threshold, z), "convert_device")

    def convert_dither_stats(self):
        """(texels the error-diffusion merge re-ran, texels converted with error diffusion), cumulative on this context."""
        rerun, total = ctypes.c_uint64(), ctypes.c_uint64()
        self._check(self._lib.dxtex_convert_dither_stats(self._h, ctypes.byref(rerun), ctypes.byref(total)), "convert_dither_stats")
        return rerun.value, total.value

    # -- ComputeNormalMap ---------------------------------------------------------------------------
    def compute_normal_map(self, pixels, width, height, src_format, dst_format, flags=0, amplitude=1.0, src_row_pitch=None):
        """DirectX::ComputeNormalMap of one height map; flags = CNMAP_* (channel in the low 4 bits). Returns the destination
        (tight pitch) as a numpy uint8 buffer."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, src_format, src_row_pitch)
        rp, sp = compute_pitch(dst_format, width, height)
        out = np.zeros(sp, np.uint8)
        dst = Image(width, height, dst_format, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_compute_normal_map(self._h, ctypes.byref(src), ctypes.byref(dst), flags, amplitude), "compute_normal_map")
        return out

    def compute_normal_map_device(self, src_ptr, width, height, src_format, dst_ptr, dst_format, flags=0, amplitude=1.0, src_row_pitch=None):
        """dxtex_compute_normal_map_device: device pointers (tight destination pitch), asynchronous on the context's stream."""
        src = device_image(src_ptr, width, height, src_format, src_row_pitch)
        dst = device_image(dst_ptr, width, height, dst_format)
        self._check(self._lib.dxtex_compute_normal_map_device(self._h, ctypes.byref(src), ctypes.byref(dst), flags, amplitude), "compute_normal_map_device")

    # -- TransformImage with texconv's per-texel ops -----------------------------------------------------------------------------
    def transform_image(self, pixels, width, height, fmt, transform, row_pitch=None):
        """dxtex_transform_image: one image (host pixels) through a Transform (make_transform). Returns the destination (tight pitch)
        as a numpy uint8 buffer."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt, row_pitch)
        rp, sp = compute_pitch(fmt, width, height)
        out = np.zeros(sp, np.uint8)
        dst = Image(width, height, fmt, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_transform_image(self._h, ctypes.byref(src), ctypes.byref(dst), ctypes.byref(transform)), "transform_image")
        return out

    def transform_images_device(self, srcs, dsts, transform):
        """dxtex_transform_images_device: lists of device Images (device_image) of one format, asynchronous on the context's stream;
        TONEMAP takes its maximum over all of `srcs`."""
        n = len(srcs)
        a, b = (Image * max(n, 1))(*srcs), (Image * max(n, 1))(*dsts)
        self._check(self._lib.dxtex_transform_images_device(self._h, a, b, n, ctypes.byref(transform)), "transform_images_device")

    # -- texconv's HDR colour rotation ----------------------------------------------------------------------------------------------
    def rotate_color(self, pixels, width, height, fmt, rotate, paper_white_nits=200.0, row_pitch=None):
        """dxtex_rotate_color: one image (host pixels) through rotate = ROTATE_* (formats.py). Returns the destination (tight pitch) as
        a numpy uint8 buffer."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt, row_pitch)
        rp, sp = compute_pitch(fmt, width, height)
        out = np.zeros(sp, np.uint8)
        dst = Image(width, height, fmt, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_rotate_color(self._h, ctypes.byref(src), ctypes.byref(dst), rotate, paper_white_nits), "rotate_color")
        return out

    def rotate_color_device(self, srcs, dsts, rotate, paper_white_nits=200.0):
        """dxtex_rotate_color_device: lists of device Images (device_image) of one format, asynchronous on the context's stream."""
        n = len(srcs)
        a, b = (Image * max(n, 1))(*srcs), (Image * max(n, 1))(*dsts)
        self._check(self._lib.dxtex_rotate_color_device(self._h, a, b, n, rotate, paper_white_nits), "rotate_color_device")

    # -- Radiance RGBE texels (the per-texel half of the .hdr codec) ---------------------------------------------------------------------
    def rgbe_decode(self, rgbe_bytes, width, height, exposure=1.0, row_pitch=None):
        """dxtex_rgbe_decode: rows of four-byte shared-exponent texels (host memory, row_pitch bytes apart, default width * 4) ->
        R32G32B32A32_FLOAT with tight pitch, as a numpy uint8 buffer."""
        rgbe_bytes = np.ascontiguousarray(rgbe_bytes)
        src = _host_image(rgbe_bytes, width, height, F.DXGI_FORMAT_R8G8B8A8_UINT, row_pitch)
        out = np.zeros(width * height * 16, np.uint8)
        dst = Image(width, height, F.DXGI_FORMAT_R32G32B32A32_FLOAT, width * 16, width * height * 16, out.ctypes.data)
        self._check(self._lib.dxtex_rgbe_decode(self._h, ctypes.byref(src), ctypes.byref(dst), exposure), "rgbe_decode")
        return out

    def rgbe_encode(self, pixels, width, height, fmt, row_pitch=None):
        """dxtex_rgbe_encode: one R32G32B32A32_FLOAT, R32G32B32_FLOAT or R16G16B16A16_FLOAT image (host pixels) -> its RGBE texels, four
        bytes each with tight pitch, as a numpy uint8 buffer."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt, row_pitch)
        out = np.zeros(width * height * 4, np.uint8)
        dst = Image(width, height, F.DXGI_FORMAT_R8G8B8A8_UINT, width * 4, width * height * 4, out.ctypes.data)
        self._check(self._lib.dxtex_rgbe_encode(self._h, ctypes.byref(src), ctypes.byref(dst)), "rgbe_encode")
        return out

    def rgbe_decode_device(self, src, dst, exposure=1.0):
        """dxtex_rgbe_decode_device on device Images (device_image): R8G8B8A8_UINT -> R32G32B32A32_FLOAT, asynchronous on the stream."""
        self._check(self._lib.dxtex_rgbe_decode_device(self._h, ctypes.byref(src), ctypes.byref(dst), exposure), "rgbe_decode_device")

    def rgbe_encode_device(self, src, dst):
        """dxtex_rgbe_encode_device on device Images (device_image): a float format -> R8G8B8A8_UINT, asynchronous on the stream."""
        self._check(self._lib.dxtex_rgbe_encode_device(self._h, ctypes.byref(src), ctypes.byref(dst)), "rgbe_encode_device")

    # -- Truevision TGA texels (the per-texel half of the .tga codec) --------------------------------------------------------------------
    @staticmethod
    def _tga_palette(palette):
        """256 host words for the palette argument, or None"""
        if palette is None:
            return None
        palette = np.ascontiguousarray(palette, np.uint32)
        assert palette.size == 256
        return palette

    def tga_unpack(self, texels, width, height, bytes_per_texel, fmt, flags=0, palette=None, row_pitch=None):
        """dxtex_tga_unpack: the file-order texel stream (host bytes) -> (pixels of `fmt` as a numpy uint8 buffer with `row_pitch` bytes a
        row, default tight; the alpha answer: 1 = opaque). flags = TGA_RIGHT_TO_LEFT | TGA_TOP_DOWN | TGA_ALLOW_ALL_ZERO_ALPHA."""
        texels = np.ascontiguousarray(texels, np.uint8)
        pal = self._tga_palette(palette)
        pitch = compute_pitch(fmt, width, height)[0] if row_pitch is None else row_pitch
        out = np.zeros(pitch * height, np.uint8)
        dst = Image(width, height, fmt, pitch, pitch * height, out.ctypes.data)
        opaque = ctypes.c_uint32(0xFFFFFFFF)
        self._check(self._lib.dxtex_tga_unpack(self._h, texels.ctypes.data, texels.nbytes, bytes_per_texel, flags, None if pal is None else pal.ctypes.data,
                                               ctypes.byref(dst), ctypes.byref(opaque)), "tga_unpack")
        return out, int(opaque.value)

    def tga_pack(self, pixels, width, height, fmt, bytes_per_texel, row_pitch=None):
        """dxtex_tga_pack: one image (host pixels) -> the width * height * bytes_per_texel bytes of the file's rows, as a numpy uint8 buffer."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt, row_pitch)
        out = np.zeros(width * height * bytes_per_texel, np.uint8)
        self._check(self._lib.dxtex_tga_pack(self._h, ctypes.byref(src), bytes_per_texel, out.ctypes.data, out.nbytes), "tga_pack")
        return out

    def tga_unpack_device(self, texels_ptr, texel_bytes, bytes_per_texel, dst, flags=0, palette=None, opaque_ptr=None):
        """dxtex_tga_unpack_device: the stream at a device pointer -> the device Image `dst` (device_image), asynchronous on the stream; the
        answer goes to the device dword opaque_ptr if given. palette = 256 host words."""
        pal = self._tga_palette(palette)
        self._check(self._lib.dxtex_tga_unpack_device(self._h, texels_ptr, texel_bytes, bytes_per_texel, flags, None if pal is None else pal.ctypes.data,
                                                      ctypes.byref(dst), opaque_ptr), "tga_unpack_device")

    def tga_pack_device(self, src, bytes_per_texel, texels_ptr, texel_bytes):
        """dxtex_tga_pack_device: the device Image `src` -> the file's rows at a device pointer, asynchronous on the stream."""
        self._check(self._lib.dxtex_tga_pack_device(self._h, ctypes.byref(src), bytes_per_texel, texels_ptr, texel_bytes), "tga_pack_device")

    # -- portable pixmap texels (the per-texel half of the .ppm / .pfm / .phm codec) -------------------------------------------------------
    def pnm_unpack(self, samples, width, height, kind, fmt, maxval=255, flags=0, row_pitch=None, out=None):
        """dxtex_pnm_unpack: the samples behind the header (host bytes) -> pixels of `fmt` as a numpy uint8 buffer with `row_pitch` bytes a
        row, default tight. kind = PNM_*; flags = PNM_BIG_ENDIAN. out: the buffer to unpack into (so that a caller can see what is left
        untouched), default a zeroed one."""
        samples = np.ascontiguousarray(samples, np.uint8)
        pitch = compute_pitch(fmt, width, height)[0] if row_pitch is None else row_pitch
        if out is None:
            out = np.zeros(pitch * height, np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.nbytes >= pitch * height
        dst = Image(width, height, fmt, pitch, pitch * height, out.ctypes.data)
        self._check(self._lib.dxtex_pnm_unpack(self._h, samples.ctypes.data, samples.nbytes, kind, maxval, flags, ctypes.byref(dst)), "pnm_unpack")
        return out

    def pnm_pack(self, pixels, width, height, fmt, kind, row_pitch=None, out=None):
        """dxtex_pnm_pack: one image (host pixels) -> the width * height * texel bytes of the file's rows, as a numpy uint8 buffer (or the
        front of `out`)."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt, row_pitch)
        if out is None:
            out = np.zeros(width * height * F.PNM_FILE_BYTES[kind], np.uint8)
        self._check(self._lib.dxtex_pnm_pack(self._h, ctypes.byref(src), kind, out.ctypes.data, out.nbytes), "pnm_pack")
        return out

    def pnm_unpack_device(self, samples_ptr, sample_bytes, kind, dst, maxval=255, flags=0):
        """dxtex_pnm_unpack_device: the samples at a device pointer -> the device Image `dst` (device_image), asynchronous on the stream."""
        self._check(self._lib.dxtex_pnm_unpack_device(self._h, samples_ptr, sample_bytes, kind, maxval, flags, ctypes.byref(dst)), "pnm_unpack_device")

    def pnm_pack_device(self, src, kind, samples_ptr, sample_bytes):
        """dxtex_pnm_pack_device: the device Image `src` -> the file's rows at a device pointer, asynchronous on the stream."""
        self._check(self._lib.dxtex_pnm_pack_device(self._h, ctypes.byref(src), kind, samples_ptr, sample_bytes), "pnm_pack_device")

    # -- PNG texels (the per-texel half of the .png codec) -------------------------------------------------------------------------------
    @staticmethod
    def _png_palette(palette):
        """(pointer or None, count, the array to keep alive) of a palette given as R | G << 8 | B << 16 | A << 24 words"""
        if palette is None:
            return None, 0, None
        words = np.ascontiguousarray(palette, np.uint32)
        return words.ctypes.data, words.size, words

    def png_unpack(self, rows, width, height, kind, fmt, flags=0, palette=None, row_pitch=None, out=None):
        """dxtex_png_unpack: a file's unfiltered rows (host bytes, ceil(width * bits / 8) each) -> pixels of `fmt` as a numpy uint8 buffer
        with `row_pitch` bytes a row, default tight. kind = PNG_*; flags = PNG_BGR; palette = up to 256 words for a palette kind. out: the
        buffer to unpack into (so that a caller can see what is left untouched), default a zeroed one."""
        rows = np.ascontiguousarray(rows, np.uint8)
        pitch = compute_pitch(fmt, width, height)[0] if row_pitch is None else row_pitch
        if out is None:
            out = np.zeros(pitch * height, np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.nbytes >= pitch * height
        dst = Image(width, height, fmt, pitch, pitch * height, out.ctypes.data)
        pal, count, _keep = self._png_palette(palette)
        self._check(self._lib.dxtex_png_unpack(self._h, rows.ctypes.data, rows.nbytes, kind, flags, pal, count, ctypes.byref(dst)), "png_unpack")
        return out

    def png_pack(self, pixels, width, height, fmt, row_pitch=None, out=None):
        """dxtex_png_pack: one image (host pixels) -> the file's rows, tight, as a numpy uint8 buffer (or the front of `out`)."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt, row_pitch)
        if out is None:
            out = np.zeros(width * height * 8, np.uint8)
        self._check(self._lib.dxtex_png_pack(self._h, ctypes.byref(src), out.ctypes.data, out.nbytes), "png_pack")
        return out

    def png_unpack_device(self, rows_ptr, rows_bytes, kind, dst, flags=0, palette=None):
        """dxtex_png_unpack_device: the rows at a device pointer -> the device Image `dst` (device_image), asynchronous on the stream."""
        pal, count, _keep = self._png_palette(palette)
        self._check(self._lib.dxtex_png_unpack_device(self._h, rows_ptr, rows_bytes, kind, flags, pal, count, ctypes.byref(dst)), "png_unpack_device")

    def png_pack_device(self, src, rows_ptr, rows_bytes):
        """dxtex_png_pack_device: the device Image `src` -> the file's rows at a device pointer, asynchronous on the stream."""
        self._check(self._lib.dxtex_png_pack_device(self._h, ctypes.byref(src), rows_ptr, rows_bytes), "png_pack_device")

    # -- JPEG samples (everything behind the Huffman walk of the .jpg reader, everything in front of the writer's Huffman coder) ----------
    def jpeg_decode(self, coefficients, frame, fmt, row_pitch=None, out=None):
        """dxtex_jpeg_decode: a frame's quantised coefficients (host int16, laid out as jpeg_frame states) -> pixels of `fmt` as a numpy
        uint8 buffer with `row_pitch` bytes a row, default tight. out: the buffer to decode into, default a zeroed one."""
        coefficients = np.ascontiguousarray(coefficients, np.int16)
        pitch = compute_pitch(fmt, frame.width, frame.height)[0] if row_pitch is None else row_pitch
        if out is None:
            out = np.zeros(pitch * frame.height, np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.nbytes >= pitch * frame.height
        dst = Image(frame.width, frame.height, fmt, pitch, pitch * frame.height, out.ctypes.data)
        self._check(self._lib.dxtex_jpeg_decode(self._h, coefficients.ctypes.data, coefficients.nbytes, ctypes.byref(frame), ctypes.byref(dst)), "jpeg_decode")
        return out

    def jpeg_decode_device(self, coefficients_ptr, coefficient_bytes, frame, dst):
        """dxtex_jpeg_decode_device: the coefficients at a device pointer -> the device Image `dst` (device_image), asynchronous on the
        stream."""
        self._check(self._lib.dxtex_jpeg_decode_device(self._h, coefficients_ptr, coefficient_bytes, ctypes.byref(frame), ctypes.byref(dst)), "jpeg_decode_device")

    def jpeg_encode(self, pixels, frame, fmt, row_pitch=None, out=None):
        """dxtex_jpeg_encode: host pixels of `fmt` (a numpy uint8 buffer with `row_pitch` bytes a row, default tight) -> the frame's
        quantised coefficients as a numpy int16 array, laid out as jpeg_frame states. out: the array to encode into, default a zeroed one
        of the frame's size."""
        pixels = np.ascontiguousarray(pixels, np.uint8)
        pitch = compute_pitch(fmt, frame.width, frame.height)[0] if row_pitch is None else row_pitch
        if out is None:
            out = np.zeros(jpeg_coefficient_count(frame), np.int16)
        assert out.dtype == np.int16 and out.flags["C_CONTIGUOUS"]
        src = Image(frame.width, frame.height, fmt, pitch, pitch * frame.height, pixels.ctypes.data)
        self._check(self._lib.dxtex_jpeg_encode(self._h, ctypes.byref(src), ctypes.byref(frame), out.ctypes.data, out.nbytes), "jpeg_encode")
        return out

    def jpeg_encode_device(self, src, frame, coefficients_ptr, coefficient_bytes):
        """dxtex_jpeg_encode_device: the device Image `src` (device_image) -> the frame's coefficients at a device pointer, asynchronous on
        the stream."""
        self._check(self._lib.dxtex_jpeg_encode_device(self._h, ctypes.byref(src), ctypes.byref(frame), coefficients_ptr, coefficient_bytes), "jpeg_encode_device")

    # -- OpenEXR chunks (everything behind the inflater of the .exr reader, the writer's scanlines) -------------------------------------------
    def exr_unpack(self, stream, chunks, channels, scanline_bytes, width, height, items=1, row_pitch=None, out=None):
        """dxtex_exr_unpack: the expanded stream (host bytes), its chunks [(offset, bytes, first row, rows, coded)] and the channel table
        [(offset, type)] for R, G, B, A -> `items` R16G16B16A16_FLOAT images of width x height, one behind another in a numpy uint8 buffer
        with `row_pitch` bytes a row, default tight. out: the buffer to unpack into, default a zeroed one."""
        stream = np.ascontiguousarray(stream, np.uint8)
        pitch = width * 8 if row_pitch is None else row_pitch
        if out is None:
            out = np.zeros(pitch * height * items, np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.nbytes >= pitch * height * items
        imgs = (Image * items)(*[Image(width, height, F.DXGI_FORMAT_R16G16B16A16_FLOAT, pitch, pitch * height, out.ctypes.data + i * pitch * height) for i in range(items)])
        ch, count, tab = _exr_tables(chunks, channels)
        self._check(self._lib.dxtex_exr_unpack(self._h, stream.ctypes.data, stream.nbytes, ch, count, tab, scanline_bytes, imgs, items), "exr_unpack")
        return out

    def exr_unpack_device(self, stream_ptr, stream_bytes, chunks, channels, scanline_bytes, items):
        """dxtex_exr_unpack_device: the stream at a device pointer (its coded chunks are undone in place) -> the device Images `items`
        (a list of device_image), asynchronous on the stream."""
        imgs = None if items is None else (Image * max(1, len(items)))(*items)
        ch, count, tab = _exr_tables(chunks, channels)
        self._check(self._lib.dxtex_exr_unpack_device(self._h, stream_ptr, stream_bytes, ch, count, tab, scanline_bytes, imgs, 0 if items is None else len(items)), "exr_unpack_device")

    def exr_pack(self, pixels, width, height, fmt, row_pitch=None, out=None):
        """dxtex_exr_pack: one image (host pixels) -> the writer's scanlines (per row the A, B, G, R half planes), width * height * 8 bytes
        as a numpy uint8 buffer (or the front of `out`)."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt, row_pitch)
        if out is None:
            out = np.zeros(width * height * 8, np.uint8)
        self._check(self._lib.dxtex_exr_pack(self._h, ctypes.byref(src), out.ctypes.data, out.nbytes), "exr_pack")
        return out

    def exr_pack_device(self, src, scanlines_ptr, scanline_bytes):
        """dxtex_exr_pack_device: the device Image `src` -> the writer's scanlines at a device pointer, asynchronous on the stream."""
        self._check(self._lib.dxtex_exr_pack_device(self._h, ctypes.byref(src), scanlines_ptr, scanline_bytes), "exr_pack_device")

    # -- TIFF strips and tiles (everything behind LZW, PackBits and inflate of the .tif reader, the writer's rows) ---------------------------------
    def tiff_unpack(self, stream, segments, layout, fmt, palette=None, row_pitch=None, out=None):
        """dxtex_tiff_unpack: the expanded stream (host bytes), its segments [(offset, first row, rows, first column, columns, row bytes,
        plane)] and the layout (the ten fields of TiffLayout) -> pixels of `fmt` as a numpy uint8 buffer with `row_pitch` bytes a row,
        default tight. out: the buffer to unpack into, default a zeroed one."""
        stream = np.ascontiguousarray(stream, np.uint8)
        width, height = layout[0], layout[1]
        pitch = compute_pitch(fmt, width, height)[0] if row_pitch is None else row_pitch
        if out is None:
            out = np.zeros(pitch * height, np.uint8)
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.nbytes >= pitch * height
        dst = Image(width, height, fmt, pitch, pitch * height, out.ctypes.data)
        seg, count, lay, pal = _tiff_tables(segments, layout, palette)
        self._check(self._lib.dxtex_tiff_unpack(self._h, stream.ctypes.data, stream.nbytes, seg, count, ctypes.byref(lay), pal, ctypes.byref(dst)), "tiff_unpack")
        return out

    def tiff_unpack_device(self, stream_ptr, stream_bytes, segments, layout, dst, palette=None):
        """dxtex_tiff_unpack_device: the stream at a device pointer (its rows are undone in place where the file has a predictor) -> the
        device Image `dst` (device_image), asynchronous on the stream."""
        seg, count, lay, pal = _tiff_tables(segments, layout, palette)
        self._check(self._lib.dxtex_tiff_unpack_device(self._h, stream_ptr, stream_bytes, seg, count, None if lay is None else ctypes.byref(lay), pal,
                                                       None if dst is None else ctypes.byref(dst)), "tiff_unpack_device")

    def tiff_pack(self, pixels, width, height, fmt, row_pitch=None, out=None):
        """dxtex_tiff_pack: one image (host pixels) -> the writer's rows, tight, as a numpy uint8 buffer (or the front of `out`)."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt, row_pitch)
        if out is None:
            out = np.zeros(width * height * 16, np.uint8)
        self._check(self._lib.dxtex_tiff_pack(self._h, ctypes.byref(src), out.ctypes.data, out.nbytes), "tiff_pack")
        return out

    def tiff_pack_device(self, src, rows_ptr, rows_bytes):
        """dxtex_tiff_pack_device: the device Image `src` -> the writer's rows at a device pointer, asynchronous on the stream."""
        self._check(self._lib.dxtex_tiff_pack_device(self._h, ctypes.byref(src), rows_ptr, rows_bytes), "tiff_pack_device")

    # -- DDS texels (the per-texel half of the .dds codec) -------------------------------------------------------------------------------
    @staticmethod
    def _dds_arrays(images, offsets, pitches):
        n = len(images)
        assert len(offsets) == n and len(pitches) == n
        return (Image * max(n, 1))(*images), (ctypes.c_size_t * max(n, 1))(*offsets), (ctypes.c_size_t * max(n, 1))(*pitches), n

    def dds_unpack(self, payload, op, images, offsets, pitches, opaque=False, palette=None):
        """dxtex_dds_unpack: the file's payload (host bytes) -> one numpy uint8 buffer per image. images = [(width, height, fmt, row_pitch or
        None)]; offsets / pitches = where each image's rows lie in the payload. op = DDS_ROW_*."""
        payload = np.ascontiguousarray(payload, np.uint8)
        pal = self._tga_palette(palette)
        outs, ims = [], []
        for (w, h, fmt, rp) in images:
            mrp, msp = compute_pitch(fmt, w, h)
            rows = msp // mrp if mrp else 0
            rp = mrp if rp is None else rp
            outs.append(np.zeros(rp * rows, np.uint8))
            ims.append(Image(w, h, fmt, rp, rp * rows, outs[-1].ctypes.data))
        arr, off, pit, n = self._dds_arrays(ims, offsets, pitches)
        self._check(self._lib.dxtex_dds_unpack(self._h, payload.ctypes.data, payload.nbytes, op, int(bool(opaque)), None if pal is None else pal.ctypes.data,
                                               arr, off, pit, n), "dds_unpack")
        return outs

    def dds_unpack_device(self, payload_ptr, payload_bytes, op, dsts, offsets, pitches, opaque=False, palette=None):
        """dxtex_dds_unpack_device: the payload at a device pointer -> the device Images `dsts` (device_image), asynchronous on the stream."""
        pal = self._tga_palette(palette)
        arr, off, pit, n = self._dds_arrays(dsts, offsets, pitches)
        self._check(self._lib.dxtex_dds_unpack_device(self._h, payload_ptr, payload_bytes, op, int(bool(opaque)), None if pal is None else pal.ctypes.data,
                                                      arr, off, pit, n), "dds_unpack_device")

    def dds_pack24(self, images, offsets, pitches, out_bytes):
        """dxtex_dds_pack24: B8G8R8X8 images [(pixels, width, height, row_pitch or None)] -> out_bytes of 24-bit rows (zero where no row lies)."""
        keep = [np.ascontiguousarray(px) for (px, _, _, _) in images]
        ims = [_host_image(k, w, h, 88, rp) for k, (_, w, h, rp) in zip(keep, images)]
        arr, off, pit, n = self._dds_arrays(ims, offsets, pitches)
        out = np.zeros(out_bytes, np.uint8)
        self._check(self._lib.dxtex_dds_pack24(self._h, arr, off, pit, n, out.ctypes.data, out.nbytes), "dds_pack24")
        return out

    def dds_pack24_device(self, srcs, offsets, pitches, out_ptr, out_bytes):
        """dxtex_dds_pack24_device: the device Images `srcs` -> 24-bit rows at a device pointer, asynchronous on the stream."""
        arr, off, pit, n = self._dds_arrays(srcs, offsets, pitches)
        self._check(self._lib.dxtex_dds_pack24_device(self._h, arr, off, pit, n, out_ptr, out_bytes), "dds_pack24_device")

    def generate_mips3d(self, volume, width, height, depth, fmt, nlevels, filter_flags):
        """DirectX::GenerateMipMaps3D: `volume` = the base slices (tight, consecutive). Returns one uint8 buffer per level."""
        bufs, vols = [], []
        w, h, d = width, height, depth
        for i in range(nlevels):
            rp, sp = compute_pitch(fmt, w, h)
            buf = np.zeros(sp * d, np.uint8)
            if i == 0:
                buf[:] = np.ascontiguousarray(volume).view(np.uint8).reshape(-1)[:sp * d]
            bufs.append(buf)
            vols.append(Volume(w, h, d, fmt, rp, sp, buf.ctypes.data))
            w, h, d = max(1, w >> 1), max(1, h >> 1), max(1, d >> 1)
        arr = (Volume * nlevels)(*vols)
        self._check(self._lib.dxtex_generate_mips3d(self._h, arr, nlevels, filter_flags), "generate_mips3d")
        return bufs

    def premultiply_alpha(self, pixels, width, height, fmt, flags=0):
        """DirectX::PremultiplyAlpha (flags = TEX_PMALPHA_*: 0x1 IGNORE_SRGB, 0x2 REVERSE, 0x1000000 / 0x2000000 SRGB_IN / OUT)."""
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt)
        rp, sp = compute_pitch(fmt, width, height)
        out = np.zeros(sp, np.uint8)
        dst = Image(width, height, fmt, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_premultiply_alpha(self._h, ctypes.byref(src), ctypes.byref(dst), flags), "premultiply_alpha")
        return out

    def scale_mips_alpha_for_coverage(self, levels, width, height, fmt, alpha_reference):
        """DirectX::ScaleMipMapsAlphaForCoverage on a list of tight per-level buffers; returns the new levels."""
        levels = [np.ascontiguousarray(l).view(np.uint8).reshape(-1) for l in levels]
        n = len(levels)
        srcs, dsts, outs = [], [], []
        w, h = width, height
        for l in levels:
            srcs.append(_host_image(l, w, h, fmt))
            rp, sp = compute_pitch(fmt, w, h)
            o = np.zeros(sp, np.uint8); outs.append(o)
            dsts.append(Image(w, h, fmt, rp, sp, o.ctypes.data))
            w, h = max(1, w >> 1), max(1, h >> 1)
        a = (Image * n)(*srcs); b = (Image * n)(*dsts)
        self._check(self._lib.dxtex_scale_mips_alpha_for_coverage(self._h, a, b, n, alpha_reference), "scale_mips_alpha_for_coverage")
        return outs

    def resize(self, pixels, width, height, fmt, new_width, new_height, filter_flags=0):
        pixels = np.ascontiguousarray(pixels)
        src = _host_image(pixels, width, height, fmt)
        rp, sp = compute_pitch(fmt, new_width, new_height)
        out = np.zeros(sp, np.uint8)
        dst = Image(new_width, new_height, fmt, rp, sp, out.ctypes.data)
        self._check(self._lib.dxtex_resize(self._h, ctypes.byref(src), ctypes.byref(dst), filter_flags), "resize")
        return out
