"""The C ABI of the stream images without a device: the three entry points are declared, exported and bound with argument types, refuse
NULL and zero-length arguments before they touch a GPU, and ctcd_snapshot_info reads the committed version-1 image."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("ctcd_stream_save", "ctcd_stream_restore", "ctcd_snapshot_info")


def _image():
    with open(os.path.join(GOLDEN, "stream_snapshot_v1_k4_t30.bin"), "rb") as f:
        return f.read()


def test_snapshot_symbols_are_declared_exported_and_bound():
    from ctcdecode_amd import _native

    with open(os.path.join(ROOT, "include", "ctcdecode_amd.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NAMES + ("ctcd_scorer_fingerprint",):
        assert re.search(r"\b%s\s*\(" % name, text), "%s is not declared" % name
        assert name in _native.SYMBOLS
        fn = getattr(_native.lib, name)
        assert fn.argtypes, "%s is bound without argument types" % name
    assert len(_native.lib.ctcd_stream_save.argtypes) == 7 and len(_native.lib.ctcd_stream_restore.argtypes) == 8
    assert len(_native.lib.ctcd_snapshot_info.argtypes) == 3
    assert _native.lib.ctcd_scorer_fingerprint.restype is ctypes.c_ulonglong


def test_null_and_empty_arguments_are_refused_without_a_device():
    from ctcdecode_amd import _native

    lib = _native.lib
    one = (ctypes.c_void_p * 1)()
    sizes = (ctypes.c_ulonglong * 1)(0)
    cb = _native.BYTES_ALLOC_FN(lambda _u, _n: None)
    info = _native.SnapshotInfo()
    blob = _image()
    buf = ctypes.create_string_buffer(blob, len(blob))
    for rc in (lib.ctcd_stream_save(None, one, 1, cb, None, sizes, None),
               lib.ctcd_stream_restore(None, None, one, sizes, 1, 0, one, None),
               lib.ctcd_snapshot_info(None, 16, ctypes.byref(info)),
               lib.ctcd_snapshot_info(buf, 0, ctypes.byref(info)),
               lib.ctcd_snapshot_info(buf, len(blob), None)):
        assert rc == -1, rc
        assert lib.ctcd_last_error()
    assert _native.lib.ctcd_scorer_fingerprint(None) == 0
    assert lib.ctcd_stream_save(None, None, 0, cb, None, None, None) == -1  # (a NULL decoder is refused for an empty batch too)


def test_snapshot_info_reads_the_committed_image_device_free():
    import ctcdecode_amd

    blob = _image()
    with open(os.path.join(GOLDEN, "stream_snapshot_v1_k4_t30.json")) as f:
        want = json.load(f)["info"]
    got = ctcdecode_amd.snapshot_info(blob)
    assert got == dict((k, want[k]) for k in got), got
    assert got["bytes"] == len(blob) == 4 * (16 + 12 + 14 * 4 + 5 * got["nodes"])
    import torch

    assert ctcdecode_amd.snapshot_info(torch.frombuffer(bytearray(blob), dtype=torch.uint8)) == got
    for bad in (blob[:-1], blob[:60], b"", blob + b"\0", b"\0" * len(blob), blob[:4] + b"\2\0\0\0" + blob[8:]):
        with pytest.raises(ValueError):
            ctcdecode_amd.snapshot_info(bad)
