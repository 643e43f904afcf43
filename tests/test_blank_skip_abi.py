"""The blank-frame filter's C ABI and constructor keyword without a GPU: the four entry points are declared in the header, exported by
the library and bound with argtypes; every NULL or non-positive argument is refused with CTCD_EINVAL before the device is touched; the
host remap works on plain memory; ``blank_skip`` is validated before anything else the constructor does."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ctcd_blank_skip", "ctcd_remap_timesteps", "ctcd_remap_compact", "ctcd_remap_timesteps_host"]


def _native():
    import __graft_entry__ as g

    g.build()
    from ctcdecode_amd import _native

    return _native


def test_symbols_are_declared_exported_and_bound():
    nat = _native()
    with open(os.path.join(ROOT, "include", "ctcdecode_amd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name + " is not declared in include/ctcdecode_amd.h"
        assert name in nat.SYMBOLS, name
        fn = getattr(nat.lib, name)
        assert fn.argtypes is not None, name + " has no argtypes"
    assert len(nat.lib.ctcd_blank_skip.argtypes) == 12 and nat.lib.ctcd_blank_skip.argtypes[7] is ctypes.c_float
    assert len(nat.lib.ctcd_remap_timesteps.argtypes) == 9 and len(nat.lib.ctcd_remap_compact.argtypes) == 10
    assert len(nat.lib.ctcd_remap_timesteps_host.argtypes) == 8


def test_new_unit_is_outside_the_kernel_list_and_the_prepass_table():
    from ctcdecode_amd import _build

    assert "blank_skip.hip" in _build.SOURCES and "blank_skip.h" in _build.HEADERS and "blank_skip.h" not in _build.KERNEL_HEADERS
    for name in ("decode_kernel.h", "decode_kernels.hip"):
        with open(os.path.join(ROOT, "ctcdecode_amd", "csrc", name)) as f:
            text = f.read()
        assert "blank_skip" not in text and "ctcskip" not in text, name


def test_null_and_non_positive_arguments_are_refused_without_a_device():
    """A fake non-NULL decoder pointer is never dereferenced: the argument checks come first."""
    nat = _native()
    lib = nat.lib
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)
    assert lib.ctcd_blank_skip(None, p, p, 1, 1, 1, 0, 0.5, p, p, p, None) == -1
    assert b"null" in lib.ctcd_last_error()
    for args in [(p, None, p, 1, 1, 1, 0, 0.5, p, p, p, None), (p, p, p, 1, 1, 1, 0, 0.5, None, p, p, None),
                 (p, p, p, 1, 1, 1, 0, 0.5, p, None, p, None), (p, p, p, 1, 1, 1, 0, 0.5, p, p, None, None),
                 (p, p, p, 0, 1, 1, 0, 0.5, p, p, p, None), (p, p, p, 1, 0, 1, 0, 0.5, p, p, p, None), (p, p, p, 1, 1, 0, 0, 0.5, p, p, p, None),
                 (p, p, p, -1, 1, 1, 0, 0.5, p, p, p, None), (p, p, p, 1, 1, 4, 4, 0.5, p, p, p, None), (p, p, p, 1, 1, 4, -1, 0.5, p, p, p, None)]:
        assert lib.ctcd_blank_skip(*args) == -1, args
    for fn, n in ((lib.ctcd_remap_timesteps, 5), (lib.ctcd_remap_compact, 6)):
        for hole in range(n):
            ptrs = [None if i == hole else p for i in range(n)]
            assert fn(*ptrs, 1, 1, 1, None) == -1, (fn, hole)
        for dims in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (1, -2, 1)):
            assert fn(*([p] * n), *dims, None) == -1, (fn, dims)
    assert lib.ctcd_remap_compact(*([p] * 6), 1, 1, 65537, None) == -1  # compact records hold frame numbers below 65536
    for hole in range(4):
        assert lib.ctcd_remap_timesteps_host(*[None if i == hole else p for i in range(4)], 1, 1, 1, 1) == -1
    assert lib.ctcd_remap_timesteps_host(p, p, p, p, 0, 1, 1, 1) == -1
    with pytest.raises(ValueError):
        nat.check(lib.ctcd_remap_timesteps_host(p, p, p, p, 1, 1, 0, 1))


@pytest.mark.parametrize("threads", [1, 3, 64])
def test_host_remap_touches_valid_prefixes_only(threads):
    nat = _native()
    rng = np.random.default_rng(threads)
    B, K, T = 5, 3, 11
    n2 = np.asarray([11, 4, 0, 7, 1], np.int32)
    kept = np.zeros((B, T), np.int32)
    for b in range(B):
        kept[b, :n2[b]] = np.sort(rng.choice(50, n2[b], replace=False))
    lens = np.zeros((B, K), np.int32)
    ts = np.full((B, K, T), 9_000_000, np.int32)
    want = ts.copy()
    for b in range(B):
        for p in range(K):
            L = int(rng.integers(0, n2[b] + 1))
            lens[b, p] = L
            ts[b, p, :L] = np.sort(rng.choice(n2[b], L, replace=False)) if L else []
            want[b, p, :L] = kept[b, ts[b, p, :L]]
    ts[0, 0, 0] = -3  # no index of a kept frame: left alone
    want[0, 0, 0] = -3
    lens[0, 0] = max(lens[0, 0], 1)
    rc = nat.lib.ctcd_remap_timesteps_host(ts.ctypes.data, lens.ctypes.data, kept.ctypes.data, n2.ctypes.data, B, K, T, threads)
    assert rc == 0 and np.array_equal(ts, want)


@pytest.mark.parametrize("bad", [0, 0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), "0.5", True, [0.5]])
def test_keyword_validation_raises(bad):
    """The threshold is checked first: the error does not depend on a device being there."""
    _native()
    import ctcdecode_amd

    with pytest.raises(ValueError, match="blank_skip"):
        ctcdecode_amd.CTCBeamDecoder(["_", "a"], blank_skip=bad)


def test_online_decoder_does_not_take_the_keyword():
    _native()
    import ctcdecode_amd

    with pytest.raises(TypeError):
        ctcdecode_amd.OnlineCTCBeamDecoder(["_", "a"], blank_skip=0.5)
