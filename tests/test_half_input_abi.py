"""CPU-side checks of the half-precision input ABI: include/ctcdecode_amd.h declares ctcd_set_input_dtype / ctcd_last_input_dtype and the
CTCD_DTYPE_* constants, the built library exports the functions, and the ctypes binding knows their argument types."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ctcdecode_amd.h")).read()


def test_header_declares_half_input():
    text = _header()
    assert re.search(r"\bint\s+ctcd_set_input_dtype\s*\(\s*ctcd_decoder\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+ctcd_last_input_dtype\s*\(\s*ctcd_decoder\s*\*\s*\w+\s*\)\s*;", text)
    consts = dict((k, int(v)) for k, v in re.findall(r"#define\s+(CTCD_DTYPE_\w+)\s+(\d+)", text))
    assert consts == {"CTCD_DTYPE_F32": 0, "CTCD_DTYPE_F16": 1, "CTCD_DTYPE_BF16": 2}


def test_library_exports_half_input():
    import __graft_entry__ as g

    g.build()
    from ctcdecode_amd import _build

    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in ("ctcd_set_input_dtype", "ctcd_last_input_dtype"):
        assert hasattr(lib, name), name
    # (no decoder object without a device: a NULL decoder is refused, not dereferenced)
    lib.ctcd_set_input_dtype.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_last_input_dtype.argtypes = [ctypes.c_void_p]
    assert lib.ctcd_set_input_dtype(None, 2) == -1
    assert lib.ctcd_last_input_dtype(None) == -1


def test_binding_sets_argtypes():
    from ctcdecode_amd import _native

    assert "ctcd_set_input_dtype" in _native.SYMBOLS and "ctcd_last_input_dtype" in _native.SYMBOLS
    assert _native.lib.ctcd_set_input_dtype.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert _native.lib.ctcd_last_input_dtype.argtypes == [ctypes.c_void_p]
    import ctcdecode_amd

    assert (ctcdecode_amd.DTYPE_F32, ctcdecode_amd.DTYPE_F16, ctcdecode_amd.DTYPE_BF16) == (0, 1, 2)
