"""The n-best entry points' C ABI without a GPU: the three symbols are declared in the header, exported by the library and bound with
matching argtypes; NULL or invalid arguments -- n_best outside [1, beam] among them -- are refused before the device is touched; the
Python keyword's validation."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ctcd_expand_compact_nbest", "ctcd_beam_decode_nbest", "ctcd_beam_decode_to_host_nbest"]
C_TYPES = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "double": ctypes.c_double}


def _native():
    import __graft_entry__ as g

    g.build()
    from ctcdecode_amd import _native

    return _native


def _declared_argtypes(header, name):
    """The ctypes a declaration of the header asks for: every pointer a c_void_p, scalars by their C type."""
    m = re.search(r"^int %s\((.*?)\);" % name, header, re.M | re.S)
    assert m, name + " is not declared in include/ctcdecode_amd.h"
    out = []
    for arg in m.group(1).replace("\n", " ").split(","):
        arg = arg.strip()
        if "*" in arg:
            out.append(ctypes.c_void_p)
        else:
            out.append(C_TYPES[arg.rsplit(" ", 1)[0].strip()])
    return out


def test_symbols_are_declared_exported_and_bound():
    nat = _native()
    with open(os.path.join(ROOT, "include", "ctcdecode_amd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert name in nat.SYMBOLS, name
        fn = getattr(nat.lib, name)  # (AttributeError: the library does not export it)
        assert fn.argtypes is not None, name + " has no argtypes"
        assert list(fn.argtypes) == _declared_argtypes(header, name), name + ": the ctypes argument types differ from the header's"
    assert len(nat.lib.ctcd_expand_compact_nbest.argtypes) == 13
    assert len(nat.lib.ctcd_beam_decode_nbest.argtypes) == 20 and len(nat.lib.ctcd_beam_decode_to_host_nbest.argtypes) == 21
    # the n-best decode calls are the full ones with n_best behind `scorer`
    full = list(nat.lib.ctcd_beam_decode_to_host.argtypes)
    assert list(nat.lib.ctcd_beam_decode_to_host_nbest.argtypes) == full[:14] + [ctypes.c_int] + full[14:]
    assert re.search(r"^#define CTCD_NBEST_BAD_RECORD 7$", header, re.M)


def test_new_unit_is_outside_the_kernel_list():
    from ctcdecode_amd import _build

    assert "nbest.hip" in _build.SOURCES and "nbest.h" in _build.HEADERS and "nbest.h" not in _build.KERNEL_HEADERS
    for name in ("decode_kernel.h", "decode_kernels.hip", "beam_core.h"):
        with open(os.path.join(ROOT, "ctcdecode_amd", "csrc", name)) as f:
            text = f.read()
        assert "nbest" not in text, name


def test_invalid_arguments_are_refused_without_a_device():
    """A fake non-NULL decoder pointer is never dereferenced: the argument checks come first."""
    nat = _native()
    lib = nat.lib
    buf = (ctypes.c_int32 * 64)()
    p = ctypes.addressof(buf)

    def expand(dec=p, hdr=p, ent=p, lab=p, n_labels=4, B=1, beam=4, T=4, n=1, tok=p, ts=p, status=None):
        return lib.ctcd_expand_compact_nbest(dec, hdr, ent, lab, n_labels, B, beam, T, n, tok, ts, status, None)

    assert expand(dec=None) == -1
    for n in (0, -1, 5, 1 << 20):
        assert expand(n=n) == -1, n
        assert b"n_best" in lib.ctcd_last_error()
    for kw in (dict(hdr=None), dict(ent=None), dict(lab=None), dict(tok=None), dict(ts=None), dict(B=-1), dict(beam=0, n=0), dict(T=-1), dict(n_labels=-1),
               dict(T=65537)):
        assert expand(**kw) == -1, kw
    assert expand(beam=4097) == -2  # the limit of ctcd_expand_compact
    assert expand(B=0) == 0 and expand(T=0) == 0  # nothing to do (no tensor is looked at)

    def decode(dec=p, probs=p, B=1, T=4, V=4, beam=4, top_n=40, blank=0, n=1, tok=p, ts=p, sc=p, ln=p):
        return lib.ctcd_beam_decode_nbest(dec, probs, None, B, T, V, beam, 4, 1.0, top_n, blank, 1, None, n, tok, ts, sc, ln, None, None)

    def to_host(dec=p, probs=p, B=1, T=4, V=4, beam=4, top_n=40, blank=0, n=1, tok=p, ts=p, sc=p, ln=p):
        return lib.ctcd_beam_decode_to_host_nbest(dec, probs, None, 0, B, T, V, beam, 4, 1.0, top_n, blank, 1, None, n, tok, ts, sc, ln, None, None)

    for fn in (decode, to_host):
        assert fn(dec=None) == -1
        for n in (0, -3, 5):
            assert fn(n=n) == -1, (fn, n)
            assert b"n_best" in lib.ctcd_last_error()
            with pytest.raises(ValueError, match="n_best"):
                nat.check(fn(n=n))
        for kw in (dict(probs=None), dict(tok=None), dict(ts=None), dict(sc=None), dict(ln=None), dict(B=-1), dict(T=-1), dict(V=0), dict(beam=0, n=0),
                   dict(top_n=0), dict(blank=4), dict(blank=-1)):
            assert fn(**kw) == -1, (fn, kw)
        assert fn(beam=16384, n=1) == -2  # the decode's own limit comes first, as in the full call


@pytest.mark.parametrize("bad", [0, -1, 17, 2.5, 1.0, "3", True, [1], float("nan")])
def test_keyword_validation_raises(bad):
    _native()
    import ctcdecode_amd

    with pytest.raises(ValueError, match="n_best"):
        ctcdecode_amd._n_best(bad, 16)


def test_keyword_on_every_route():
    """n_best=None on the five calls; on the drop-in ``decode`` it can only be given by keyword, behind the reference's parameters."""
    import inspect

    _native()
    import ctcdecode_amd

    dec = ctcdecode_amd.CTCBeamDecoder
    assert dec.decode.__kwdefaults__ == {"n_best": None} and dec.decode.__code__.co_varnames[:3] == ("self", "probs", "seq_lens")
    for fn in (dec.decode_device, dec.decode_padded, dec.expand_compact, ctcdecode_amd.DecodePipeline.submit):
        p = inspect.signature(fn).parameters
        assert "n_best" in p and p["n_best"].default is None, fn


def test_keyword_validation_accepts():
    _native()
    import numpy as np

    import ctcdecode_amd

    assert ctcdecode_amd._n_best(None, 16) is None
    assert [ctcdecode_amd._n_best(n, 16) for n in (1, 15, 16, np.int64(3))] == [1, 15, 16, 3]
