"""ctcd_set_long_keywords' C ABI without a GPU: declared in the header, exported by the library, bound with its two argtypes; a NULL
decoder is refused."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound_and_refuses_null():
    import __graft_entry__ as g

    g.build()
    from ctcdecode_amd import _native as nat

    with open(os.path.join(ROOT, "include", "ctcdecode_amd.h")) as f:
        assert re.search(r"^int ctcd_set_long_keywords\(ctcd_decoder \*dec, int on\);", f.read(), re.M)
    assert "ctcd_set_long_keywords" in nat.SYMBOLS
    assert list(nat.lib.ctcd_set_long_keywords.argtypes) == [ctypes.c_void_p, ctypes.c_int]
    for on in (0, 1, 2):
        assert nat.lib.ctcd_set_long_keywords(None, on) == -1
    assert b"ctcd_set_long_keywords" in nat.lib.ctcd_last_error()
