"""The C ABI and the Python setting of the blank-frame filter of live streams, without a GPU: the new entry points are declared in
the header with the documented signatures, exported by the library and bound with argtypes; NULL and bad arguments are refused with
CTCD_EINVAL before the device is touched; ``OnlineCTCBeamDecoder.set_blank_skip`` validates its threshold before it touches the decoder,
and the constructor keeps its parameters."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = {
    "ctcd_set_stream_blank_skip": r"int ctcd_set_stream_blank_skip\(ctcd_decoder \*dec, int on, float cmp_prob, float cmp_log\);",
    "ctcd_stream_frames_seen": r"long long ctcd_stream_frames_seen\(const ctcd_stream \*st\);",
    "ctcd_stream_map_bytes": r"long long ctcd_stream_map_bytes\(const ctcd_stream \*st\);",
    "ctcd_last_stream_blank_skip": r"int ctcd_last_stream_blank_skip\(ctcd_decoder \*dec, long long \*considered, long long \*kept\);",
    "ctcd_last_stream_blank_skip_ms": r"int ctcd_last_stream_blank_skip_ms\(ctcd_decoder \*dec, float \*filter_ms, float \*wait_ms, float \*remap_ms\);",
}


def _native():
    import __graft_entry__ as g

    g.build()
    from ctcdecode_amd import _native

    return _native


def test_symbols_are_declared_exported_and_bound():
    nat = _native()
    with open(os.path.join(ROOT, "include", "ctcdecode_amd.h")) as f:
        header = f.read()
    for name, decl in DECLS.items():
        assert re.search(r"^" + decl, header, re.M), name + " is not declared as documented in include/ctcdecode_amd.h"
        assert name in nat.SYMBOLS, name
        assert getattr(nat.lib, name).argtypes is not None, name + " has no argtypes"
    a = nat.lib.ctcd_set_stream_blank_skip.argtypes
    assert len(a) == 4 and a[2] is ctypes.c_float and a[3] is ctypes.c_float
    assert nat.lib.ctcd_stream_frames_seen.restype is ctypes.c_longlong and nat.lib.ctcd_stream_map_bytes.restype is ctypes.c_longlong
    assert len(nat.lib.ctcd_last_stream_blank_skip.argtypes) == 3 and len(nat.lib.ctcd_last_stream_blank_skip_ms.argtypes) == 4


def test_new_unit_is_outside_the_kernel_list():
    from ctcdecode_amd import _build

    assert "stream_blank_skip.hip" in _build.SOURCES and "stream_blank_skip.h" in _build.HEADERS and "stream_blank_skip.h" not in _build.KERNEL_HEADERS
    for name in ("decode_kernel.h", "decode_kernels.hip", "beam_core.h"):
        with open(os.path.join(ROOT, "ctcdecode_amd", "csrc", name)) as f:
            text = f.read()
        assert "blank_skip" not in text and "ctcsskip" not in text, name


def test_null_and_bad_arguments_are_refused_without_a_device():
    nat = _native()
    lib = nat.lib
    assert lib.ctcd_set_stream_blank_skip(None, 1, 0.5, -0.7) == -1
    assert b"NULL" in lib.ctcd_last_error()
    assert lib.ctcd_stream_frames_seen(None) == -1 and lib.ctcd_stream_map_bytes(None) == -1
    v = ctypes.c_longlong(0)
    f = ctypes.c_float(0)
    assert lib.ctcd_last_stream_blank_skip(None, ctypes.byref(v), ctypes.byref(v)) == -1
    assert lib.ctcd_last_stream_blank_skip_ms(None, ctypes.byref(f), ctypes.byref(f), ctypes.byref(f)) == -1
    with pytest.raises(ValueError):
        nat.check(lib.ctcd_set_stream_blank_skip(None, 0, 0.0, 0.0))
    # a fake non-NULL decoder pointer is never dereferenced: the argument checks come first
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    nan = float("nan")
    for bounds in ((nan, -0.7), (0.5, nan), (nan, nan)):
        assert lib.ctcd_set_stream_blank_skip(p, 1, *bounds) == -1, bounds
        assert b"NaN" in lib.ctcd_last_error()
    for args in ((None, ctypes.byref(v)), (ctypes.byref(v), None), (None, None)):
        assert lib.ctcd_last_stream_blank_skip(p, *args) == -1, args
        assert b"null" in lib.ctcd_last_error()
    for hole in range(3):
        args = [None if i == hole else ctypes.byref(f) for i in range(3)]
        assert lib.ctcd_last_stream_blank_skip_ms(p, *args) == -1, hole
        assert b"null" in lib.ctcd_last_error()


@pytest.mark.parametrize("bad", [0, 0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), "0.5", True, [0.5]])
def test_threshold_validation_raises(bad):
    """The threshold is checked first, by the one-shot class's check: the error does not depend on a device (or a decoder handle) being
    there -- the object here was never initialised."""
    _native()
    import ctcdecode_amd

    dec = ctcdecode_amd.OnlineCTCBeamDecoder.__new__(ctcdecode_amd.OnlineCTCBeamDecoder)
    with pytest.raises(ValueError, match="blank_skip"):
        dec.set_blank_skip(bad)


def test_the_setting_is_a_method_and_the_constructor_keeps_its_parameters():
    """The streaming class's constructor does not take the setting (tests/test_blank_skip_abi.py pins that); DecoderState reports the
    frames a stream has seen."""
    _native()
    import ctcdecode_amd

    sig = inspect.signature(ctcdecode_amd.OnlineCTCBeamDecoder.__init__)
    assert "blank_skip" not in sig.parameters and list(sig.parameters)[-1] == "compact_pool_above"
    assert list(inspect.signature(ctcdecode_amd.OnlineCTCBeamDecoder.set_blank_skip).parameters) == ["self", "thr"]
    assert isinstance(ctcdecode_amd.DecoderState.frames_seen, property) and callable(ctcdecode_amd.OnlineCTCBeamDecoder.last_blank_skip)
