"""TEST INFRASTRUCTURE ONLY. What the CopyRectangle and merge tests compare against.

- copy_rectangle(): the reference's own DirectX::CopyRectangle, called live in oracle/_ref/libdxtex_ref.so (its ref_misc.cpp compiles
  DirectXTexMisc.cpp in place). The mangled name is looked up in the library's dynamic symbols by its demangled text; Image and Rect are
  plain structs that the function takes by reference, i.e. by pointer.
- merge(): texassemble's merge lambda (XMVectorPermute + two XMVectorSelect, Texassemble/texassemble.cpp:2257-2268) as a numpy index
  operation - channels are moved, never computed - between the oracle's compiled LoadScanline and StoreScanline (transform_ref).
"""
import ctypes
import os
import subprocess

import numpy as np

import transform_ref

_SIGNATURE = "DirectX::CopyRectangle(DirectX::Image const&, DirectX::Rect const&, DirectX::Image const&, DirectX::TEX_FILTER_FLAGS, unsigned long, unsigned long)"


class RefImage(ctypes.Structure):
    """DirectX::Image (DirectXTex.h:437-445)."""
    _fields_ = [("width", ctypes.c_size_t), ("height", ctypes.c_size_t), ("format", ctypes.c_int32), ("rowPitch", ctypes.c_size_t),
                ("slicePitch", ctypes.c_size_t), ("pixels", ctypes.c_void_p)]


class RefRect(ctypes.Structure):
    """DirectX::Rect (DirectXTex.h:1007-1016)."""
    _fields_ = [("x", ctypes.c_size_t), ("y", ctypes.c_size_t), ("w", ctypes.c_size_t), ("h", ctypes.c_size_t)]


_fn = None


def _copy_rectangle_fn(oracle):
    global _fn
    if _fn is None:
        path = oracle.dxtex_oracle._REF_PATH
        mangled = None
        for line in subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout.splitlines():
            name = line.split()[-1]
            if "CopyRectangle" in name:
                demangled = subprocess.run(["c++filt", name], check=True, capture_output=True, text=True).stdout.strip()
                if demangled == _SIGNATURE:
                    mangled = name
        assert mangled, f"{_SIGNATURE} is not exported by {os.path.basename(path)}"
        fn = getattr(oracle.dxtex_oracle._load_ref(), mangled)
        fn.argtypes = [ctypes.POINTER(RefImage), ctypes.POINTER(RefRect), ctypes.POINTER(RefImage), ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t]
        fn.restype = ctypes.c_int32
        _fn = fn
    return _fn


def copy_rectangle(oracle, src, src_dims, rect, dst, dst_dims, filter_flags, x_offset, y_offset):
    """The reference's CopyRectangle. src / dst: numpy uint8 buffers or None (null pixels); *_dims = (width, height, format, rowPitch).
    -> (HRESULT as a signed 32-bit int, a copy of `dst` after the call). `dst` itself is not modified."""
    fn = _copy_rectangle_fn(oracle)
    out = None if dst is None else np.array(dst, np.uint8, copy=True)

    def image(buf, dims):
        w, h, fmt, pitch = dims
        return RefImage(w, h, fmt, pitch, pitch * h, None if buf is None else buf.ctypes.data)
    s = None if src is None else np.ascontiguousarray(src, np.uint8)
    a, b, r = image(s, src_dims), image(out, dst_dims), RefRect(*rect)
    hr = fn(ctypes.byref(a), ctypes.byref(r), ctypes.byref(b), filter_flags, x_offset, y_offset)
    return int(hr), out


def merge(oracle, a_raw, b_float, width, height, fmt, row_pitch, permute, zero=(0, 0, 0, 0), one=(0, 0, 0, 0)):
    """texassemble's merge of image 1 (`a_raw` in `fmt`, `row_pitch` bytes per row) with image 2 (`b_float`: (H, W, 4) float32) ->
    the merged image's bytes (row_pitch bytes per row, padding zero)."""
    a = transform_ref.load_rows(oracle, a_raw, width, height, fmt, row_pitch)
    both = np.concatenate([a, np.ascontiguousarray(b_float, np.float32).reshape(height, width, 4)], axis=2)     # XMVectorPermute's eight inputs
    out = both[..., list(permute)].copy()
    for k in range(4):
        if zero[k]:
            out[..., k] = 0.0
        if one[k]:
            out[..., k] = 1.0
    return transform_ref.store_rows(oracle, out, fmt, row_pitch)
