"""CPU-side checks of the stream-commit ABI: include/ctcdecode_amd.h declares ctcd_stream_commit / ctcd_stream_committed, the built
library exports them and refuses bad arguments without a device, the ctypes binding knows their argument types, and the Python
classes have the method and the property."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_stream_commit():
    text = open(os.path.join(ROOT, "include", "ctcdecode_amd.h")).read()
    m = re.search(r"\bint\s+ctcd_stream_commit\s*\(([^;]*)\)\s*;", text)
    assert m, "ctcd_stream_commit is not declared"
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.match(r"\s*ctcd_decoder\s*\*\s*\w+\s*,\s*ctcd_stream\s*\*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*ctcd_result_alloc_fn\s+\w+", args), args
    assert re.search(r"void\s*\*\s*stream\s*$", args.strip()), args
    assert re.search(r"\blong\s+long\s+ctcd_stream_committed\s*\(\s*const\s+ctcd_stream\s*\*\s*\w+\s*\)\s*;", text)


def test_library_exports_stream_commit():
    import __graft_entry__ as g

    g.build()
    from ctcdecode_amd import _build

    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in ("ctcd_stream_commit", "ctcd_stream_committed"):
        assert hasattr(lib, name), name
    # (no decoder object without a device: NULL arguments are refused, not dereferenced)
    lib.ctcd_stream_committed.argtypes = [ctypes.c_void_p]
    lib.ctcd_stream_committed.restype = ctypes.c_longlong
    assert lib.ctcd_stream_committed(None) == -1
    lib.ctcd_stream_commit.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 6
    assert lib.ctcd_stream_commit(None, None, 1, None, None, None, None, None, None) == -1


def test_binding_and_classes_know_stream_commit():
    from ctcdecode_amd import _native

    assert "ctcd_stream_commit" in _native.SYMBOLS and "ctcd_stream_committed" in _native.SYMBOLS
    assert _native.lib.ctcd_stream_commit.argtypes[2] == ctypes.c_int and _native.lib.ctcd_stream_commit.argtypes[3] is _native.RESULT_ALLOC_FN
    assert len(_native.lib.ctcd_stream_commit.argtypes) == 9
    assert _native.lib.ctcd_stream_committed.restype == ctypes.c_longlong
    import ctcdecode
    import ctcdecode_amd

    assert callable(ctcdecode_amd.OnlineCTCBeamDecoder.commit) and ctcdecode.OnlineCTCBeamDecoder is ctcdecode_amd.OnlineCTCBeamDecoder
    assert isinstance(ctcdecode_amd.DecoderState.committed_len, property) and ctcdecode.DecoderState is ctcdecode_amd.DecoderState
