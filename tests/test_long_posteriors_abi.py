"""The C ABI of long posteriors (include/ctcdecode_amd.h ctcd_set_long_posteriors / ctcd_last_long_posteriors): exported, bound, and
refusing a NULL decoder; tests/test_abi.py holds the header's declarations to _native.SYMBOLS.  No GPU."""
import ctypes

import pytest

CTCD_EINVAL = -1


@pytest.mark.parametrize("name, nargs", [("ctcd_set_long_posteriors", 3), ("ctcd_last_long_posteriors", 3)])
def test_exported_and_bound(name, nargs):
    from ctcdecode_amd import _native

    assert name in _native.SYMBOLS
    assert len(getattr(_native.lib, name).argtypes) == nargs  # (a name the library does not export raises AttributeError)


def test_null_decoder_refused():
    from ctcdecode_amd import _native

    band, block = ctypes.c_int(7), ctypes.c_int(7)
    assert _native.lib.ctcd_set_long_posteriors(None, 4096, 0) == CTCD_EINVAL
    assert _native.lib.ctcd_last_long_posteriors(None, ctypes.byref(band), ctypes.byref(block)) == CTCD_EINVAL
    assert (band.value, block.value) == (7, 7)
