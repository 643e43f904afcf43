"""CPU-side checks of the launch-order ABI: include/ctcdecode_amd.h declares ctcd_set_launch_order / ctcd_debug_last_launch_order and the
CTCD_ORDER_* constants, the built library exports the functions, a NULL decoder is refused, and the ctypes binding knows their argument
types."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ctcdecode_amd.h")).read()


def test_header_declares_launch_order():
    text = _header()
    assert re.search(r"\bint\s+ctcd_set_launch_order\s*\(\s*ctcd_decoder\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+ctcd_debug_last_launch_order\s*\(\s*ctcd_decoder\s*\*\s*\w+\s*,\s*int32_t\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    consts = dict((k, int(v)) for k, v in re.findall(r"#define\s+(CTCD_ORDER_\w+)\s+(\d+)", text))
    assert consts == {"CTCD_ORDER_BATCH": 0, "CTCD_ORDER_LENGTH": 1}


def test_library_exports_launch_order():
    import __graft_entry__ as g

    g.build()
    from ctcdecode_amd import _build

    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in ("ctcd_set_launch_order", "ctcd_debug_last_launch_order"):
        assert hasattr(lib, name), name
    # (no decoder object without a device: a NULL decoder is refused, not dereferenced -- whatever the mode)
    lib.ctcd_set_launch_order.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.ctcd_debug_last_launch_order.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    for mode in (0, 1, 2, -1):
        assert lib.ctcd_set_launch_order(None, mode) == -1
    out = (ctypes.c_int32 * 4)()
    assert lib.ctcd_debug_last_launch_order(None, out, 4) == -1
    assert lib.ctcd_debug_last_launch_order(None, None, 0) == -1


def test_binding_sets_argtypes():
    from ctcdecode_amd import _native

    assert "ctcd_set_launch_order" in _native.SYMBOLS and "ctcd_debug_last_launch_order" in _native.SYMBOLS
    assert _native.lib.ctcd_set_launch_order.argtypes == [ctypes.c_void_p, ctypes.c_int]
    assert _native.lib.ctcd_debug_last_launch_order.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]


def test_python_api_present():
    import ctcdecode_amd

    assert callable(getattr(ctcdecode_amd.CTCBeamDecoder, "set_launch_order", None))
    assert callable(getattr(ctcdecode_amd.CTCBeamDecoder, "last_launch_order", None))
    # the mode is checked before the decoder is touched: an unknown name raises ValueError (no device needed)
    dec = ctcdecode_amd.CTCBeamDecoder.__new__(ctcdecode_amd.CTCBeamDecoder)
    dec._handle = None
    with pytest.raises(ValueError):
        dec.set_launch_order("fastest")
