"""CPU-side checks: the C-ABI library loads and exports every symbol include/dxtex_amd.h declares (no
compute calls without a GPU), pitch arithmetic matches ComputePitch (DirectXTexUtil.cpp:961-1186)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "dxtex_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dxtex_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported():
    import ctypes
    import directxtex_amd as dx
    lib = ctypes.CDLL(dx.library_path())
    names = _declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/dxtex_amd.h but not exported"
    from directxtex_amd import capi
    assert set(capi.EXPORTED_SYMBOLS) == set(names)


def test_compute_pitch():
    import directxtex_amd as dx
    assert dx.compute_pitch(dx.DXGI_FORMAT_BC1_UNORM, 256, 256) == (512, 512 * 64)
    assert dx.compute_pitch(dx.DXGI_FORMAT_BC7_UNORM, 4096, 4096) == (16384, 16384 * 1024)
    assert dx.compute_pitch(dx.DXGI_FORMAT_BC3_UNORM, 1, 1) == (16, 16)
    assert dx.compute_pitch(dx.DXGI_FORMAT_BC4_UNORM, 5, 7) == (16, 32)
    assert dx.compute_pitch(dx.DXGI_FORMAT_R8G8B8A8_UNORM, 13, 3) == (52, 156)
    assert dx.compute_pitch(dx.DXGI_FORMAT_R16G16B16A16_FLOAT, 4096, 2) == (32768, 65536)
    assert dx.is_compressed(dx.DXGI_FORMAT_BC6H_UF16) and not dx.is_compressed(dx.DXGI_FORMAT_R8_UNORM)
    assert dx.bits_per_pixel(dx.DXGI_FORMAT_R32G32B32A32_FLOAT) == 128


def test_no_context_without_gpu():
    """Without a gfx950 device the library must refuse to create a context - never fall back to CPU."""
    import torch
    import directxtex_amd as dx
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(dx.DxtexError):
        dx.Context(0)


def test_header_is_plain_c():
    """include/dxtex_amd.h is the FFI boundary: it must compile as C99 (and as C++11) on its own, warnings as errors."""
    import subprocess
    header = os.path.join(ROOT, "include", "dxtex_amd.h")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", "c", header],
                ["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", header]):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr


def test_integration_binding_compiles_against_the_reference_headers(tmp_path):
    """The reference-side binding shown in INTEGRATION.md (DirectXTexCompressMI355X.cpp) is real code: the document's snippet is the
    file oracle/binding/DirectXTexCompressMI355X.cpp character for character, and that file compiles against the reference's own
    headers (in place, with the oracle's stand-ins for its un-vendored dependencies) and include/dxtex_amd.h. build() does that
    compile: oracle/Makefile builds it and oracle/binding/DirectXTexMI355X.cpp (array Compress, Decompress, mips, Resize, Convert)
    against those headers and links them with the reference and the product into oracle/_ref/binding_demo, which
    tests/test_zz_binding_gpu.py runs on a GPU."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = re.search(r"```cpp\n(// DirectXTexCompressMI355X.cpp.*?)```", doc, re.S).group(1)
    path = os.path.join(ROOT, "oracle", "binding", "DirectXTexCompressMI355X.cpp")
    assert open(path).read() == code, "INTEGRATION.md and oracle/binding/DirectXTexCompressMI355X.cpp have drifted apart"
    demo = os.path.join(ROOT, "oracle", "_ref", "binding_demo")
    assert os.path.isfile(demo) and os.access(demo, os.X_OK), f"{demo} missing: the binding did not compile and link in __graft_entry__.build()"


def test_product_library_reads_no_environment():
    """The shipped libraries must not be steerable from a user's shell: neither libdxtex_amd.so nor the C++ host layer imports getenv /
    secure_getenv (development knobs exist only in libdxtex_amd_dev.so, the -DDXTEX_DEV build the tests and tools load explicitly)."""
    import subprocess
    lib = os.path.join(ROOT, "directxtex_amd", "lib")
    for name, expect in (("libdxtex_amd.so", False), ("libdxtex_amd_host.so", False), ("libdxtex_amd_dev.so", True)):
        r = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(lib, name)], capture_output=True, text=True, check=True)
        has = any("getenv" in l for l in r.stdout.splitlines())
        assert has == expect, (name, "imports getenv" if has else "does not import getenv")
