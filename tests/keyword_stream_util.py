"""Helpers of the keyword-stream tests (TEST INFRASTRUCTURE ONLY): what include/ctcdecode_amd.h "Keyword search of live streams" promises,
read off the one-shot restatement of tests/keyword_util.py, and the ctypes front-end of the host twin
(tests/native/keyword_stream_host.cpp)."""
import ctypes
import os
import subprocess

import numpy as np

import greedy_util as gu
import keyword_util as ku

HOST_SO = os.path.join(gu.ROOT, "oracle", "_build", "libctckws_host.so")
KEYS = ("scores", "starts", "ends", "end_scores", "end_starts", "chunk_scores", "chunk_starts", "chunk_ends")


def shifted(a, first):
    """Frame numbers of a stream that began at ``first``: a -1 stays -1."""
    a = np.asarray(a, np.int32)
    return np.where(a >= 0, a + np.int32(first), a).astype(np.int32)


def want_of(x, n, blank, mode, kws, first=0):
    """The one-shot result of one item's first n frames, as a stream reports it.  -> dict(scores, starts, ends [Q]; end_scores, end_starts [Q, n])."""
    rows = [ku.find_item(x, n, blank, mode, kw) for kw in kws]
    return dict(scores=np.asarray([r[0] for r in rows], np.float32), starts=shifted([r[1] for r in rows], first), ends=shifted([r[2] for r in rows], first),
                end_scores=np.stack([r[3][:n] for r in rows]), end_starts=np.stack([shifted(r[4][:n], first) for r in rows]))


def chunk_walk(want, lo, hi, first=0):
    """The header's `>=` walk from (-inf, -1, -1) over the traces of frames [lo, hi).  -> dict(chunk_scores, chunk_starts, chunk_ends [Q])."""
    Q = want["scores"].shape[0]
    out = dict(chunk_scores=np.full(Q, -np.inf, np.float32), chunk_starts=np.full(Q, -1, np.int32), chunk_ends=np.full(Q, -1, np.int32))
    for q in range(Q):
        for t in range(lo, hi):
            if want["end_scores"][q, t] >= out["chunk_scores"][q]:
                out["chunk_scores"][q], out["chunk_starts"][q], out["chunk_ends"][q] = want["end_scores"][q, t], want["end_starts"][q, t], t + first
        if not out["chunk_scores"][q] > -np.inf:
            out["chunk_starts"][q] = out["chunk_ends"][q] = -1
    return out


def check_call(got, want, lo, n, first, what):
    """One call that fed frames [lo, lo + n) of the item ``want`` describes up to lo + n: the traces of those frames, zeros behind them, the chunk's hit."""
    ku.assert_same(dict(end_scores=got["end_scores"][:, :n], end_starts=got["end_starts"][:, :n]),
                   dict(end_scores=want["end_scores"][:, lo:lo + n], end_starts=want["end_starts"][:, lo:lo + n]), what)
    assert not got["end_scores"][:, n:].any() and not got["end_starts"][:, n:].any(), what
    ku.assert_same(got, chunk_walk(want, lo, lo + n, first), what)


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_host():
    src = os.path.join(gu.NATIVE, "keyword_stream_host.cpp")
    csrc = os.path.join(gu.ROOT, "ctcdecode_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("keyword_stream.h", "keyword.h", "greedy.h", "align.h", "blank_skip.h", "exact_math_f64.h",
                                                     "exact_math_f64_tables.h", "exact_math.h")]
    if os.path.exists(HOST_SO) and all(os.path.getmtime(HOST_SO) >= os.path.getmtime(p) for p in deps):
        return HOST_SO
    os.makedirs(os.path.dirname(HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, HOST_SO)
    return HOST_SO


def host_lib():
    def load():
        lib = ctypes.CDLL(build_host())
        lib.ctckws_host_new.restype = ctypes.c_void_p
        lib.ctckws_host_new.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_longlong]
        lib.ctckws_host_free.argtypes = [ctypes.c_void_p]
        lib.ctckws_host_state_bytes.restype = ctypes.c_longlong
        for f in (lib.ctckws_host_frames, lib.ctckws_host_ended):
            f.argtypes = [ctypes.c_void_p]
        lib.ctckws_host_find.argtypes = [ctypes.c_void_p] * 2 + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2 + [ctypes.c_int] + [ctypes.c_void_p] * 9
        return lib
    return gu.cached("keyword stream lib", load)


class HostStream(object):
    """One stream of the twin: ``feed(stored [Tc, V], n, eos)`` -> (dict of KEYS, status [Q])."""

    def __init__(self, kws, first=0, Lk=None):
        self.kws, self.lens = ku.kw_tensors(kws, Lk)
        self.state = host_lib().ctckws_host_new(len(self.lens), self.kws.shape[1], first)
        assert self.state

    def __del__(self):
        if getattr(self, "state", None):
            host_lib().ctckws_host_free(self.state)

    def feed(self, stored, dtype, n, V, blank, mode, eos=False):
        stored = np.ascontiguousarray(stored)
        Tc, Q = stored.shape[0], len(self.lens)
        f32 = lambda shape: np.full(shape, -123.0, np.float32)  # noqa: E731
        i32 = lambda shape: np.full(shape, gu.SENTINEL, np.int32)  # noqa: E731
        outs = dict(scores=f32(Q), starts=i32(Q), ends=i32(Q), end_scores=f32((Q, Tc)), end_starts=i32((Q, Tc)), chunk_scores=f32(Q), chunk_starts=i32(Q),
                    chunk_ends=i32(Q))
        status = np.zeros(Q, np.int32)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        rc = host_lib().ctckws_host_find(self.state, p(stored), dtype, n, Tc, V, blank, mode, p(self.kws), p(self.lens), int(eos), *[p(outs[k]) for k in KEYS],
                                         p(status))
        assert rc == 0, "the twin refused its arguments"
        return outs, status

    frames = property(lambda self: host_lib().ctckws_host_frames(self.state))
    ended = property(lambda self: bool(host_lib().ctckws_host_ended(self.state)))
