"""Helpers of the stream-commit tests (TEST INFRASTRUCTURE ONLY): the host twin (tests/native/commit_host.cpp: the stream of
compact_util.HostStream with ctcdecode_amd/csrc/stream_commit.h run on its parked state), and the comparisons both test files hold
the code under test to -- a committed stream reports the oracle's rows with their first `committed` labels removed."""
import ctypes
import os

import compact_util as cu
import numpy as np
import oracle_util as ou
import peek_util as pu

ROOT = ou.ROOT
COMMIT_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctccommit_host.so")

_i32p = ctypes.POINTER(ctypes.c_int32)


def build_commit_host():
    import subprocess

    native = os.path.join(ROOT, "tests", "native")
    src = os.path.join(native, "commit_host.cpp")
    csrc = os.path.join(ROOT, "ctcdecode_amd", "csrc")
    deps = [src] + [os.path.join(native, f) for f in ("compact_host.cpp", "peek_host.cpp", "core_host.cpp")] + \
        [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if os.path.exists(COMMIT_HOST_SO) and all(os.path.getmtime(COMMIT_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return COMMIT_HOST_SO
    os.makedirs(os.path.dirname(COMMIT_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (COMMIT_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-DCTC_ASSUME_CHECKED", src, "-o", tmp, "-lpthread"], check=True)
    os.replace(tmp, COMMIT_HOST_SO)
    return COMMIT_HOST_SO


class HostStream(cu.HostStream):
    """One stream of the host twin: compact_util.HostStream's feed(), peek() and compact(), and commit().  The committed labels are
    kept HERE (the library under test does not keep them): ``tokens`` / ``timesteps``, ``committed_len``."""

    def __init__(self, *args, **kw):
        # (the library of the twin holds compact_host.cpp and peek_host.cpp as they are: the parent class binds the same names in it)
        saved = cu.build_compact_host
        cu.build_compact_host = build_commit_host
        try:
            cu.HostStream.__init__(self, *args, **kw)
        finally:
            cu.build_compact_host = saved
        self.lib.ctccommit_host_commit.argtypes = [ctypes.c_void_p, _i32p, _i32p, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        self.lib.ctccommit_host_node_thi.argtypes = [ctypes.c_void_p, ctypes.c_int]
        self.tokens = np.zeros((0,), np.int32)
        self.timesteps = np.zeros((0,), np.int32)
        self.live = 1

    committed_len = property(lambda self: int(self.tokens.shape[0]))

    def commit(self):
        """-> (tokens, timesteps) committed by this call (int32 arrays); ``live``: the nodes the stream keeps."""
        cap = max(1, self.frames)
        tok = np.full((cap,), -7, np.int32)
        ts = np.full((cap,), -7, np.int32)
        live = ctypes.c_int(0)
        m = self.lib.ctccommit_host_commit(self.c, ou._ptr(tok, _i32p), ou._ptr(ts, _i32p), cap, ctypes.byref(live))
        if m == -2:
            raise NotImplementedError("host stream: commit of a stream with a scorer")
        if m < 0:
            raise RuntimeError("host stream: commit returned %d" % m)
        self.live = int(live.value)
        self.tokens = np.concatenate([self.tokens, tok[:m]])
        self.timesteps = np.concatenate([self.timesteps, ts[:m]])
        return tok[:m].copy(), ts[:m].copy()

    def node_thi(self, i):
        return int(self.lib.ctccommit_host_node_thi(self.c, i))


def shifted(want, b, C):
    """The oracle's result dict reduced to item b (as item 0) with the first C labels of every row removed: what a stream that has
    committed C labels reports.  Scores, nres and row order are the oracle's."""
    n = int(want["nres"][b])
    lens = want["lens"][b:b + 1].copy()
    assert (lens[0, :n] >= C).all(), "an oracle row is shorter than the committed part"
    lens[0, :n] -= C
    tok = np.zeros_like(want["tokens"][b:b + 1])
    ts = np.zeros_like(want["timesteps"][b:b + 1])
    for p in range(n):
        r = int(lens[0, p])
        tok[0, p, :r] = want["tokens"][b, p, C:C + r]
        ts[0, p, :r] = want["timesteps"][b, p, C:C + r]
    return dict(tokens=tok, timesteps=ts, scores=want["scores"][b:b + 1].copy(), lens=lens, nres=want["nres"][b:b + 1].copy())


def assert_committed_prefix(want, b, tok, ts, what):
    """The committed labels are the first len(tok) positions of the oracle's row 0 -- and so of every row (pu.assert_starts_with)."""
    pu.assert_starts_with(want, b, np.asarray(tok), np.asarray(ts), what)


def assert_final(last, want, b, C, what):
    """last: a one-item result dict (any width) of a stream that committed C labels; want: the oracle's one-shot decode."""
    sh = shifted(want, b, C)
    n = int(sh["nres"][0])
    assert int(np.asarray(last["nres"]).reshape(-1)[0]) == n, "%s: n_results" % what
    assert np.array_equal(np.asarray(last["lens"]).reshape(1, -1)[:, :n], sh["lens"][:, :n]), "%s: lens differ" % what
    sa = np.ascontiguousarray(np.asarray(last["scores"]).reshape(1, -1)[:, :n], dtype=np.float32).view(np.uint32)
    assert np.array_equal(sa, np.ascontiguousarray(sh["scores"][:, :n]).view(np.uint32)), "%s: scores differ bitwise" % what
    for p in range(n):
        r = int(sh["lens"][0, p])
        assert np.array_equal(np.asarray(last["tokens"])[0, p, :r], sh["tokens"][0, p, :r]), "%s: tokens differ (row %d)" % (what, p)
        assert np.array_equal(np.asarray(last["timesteps"])[0, p, :r], sh["timesteps"][0, p, :r]), "%s: timesteps differ (row %d)" % (what, p)
        assert not np.asarray(last["tokens"])[0, p, r:].any() and not np.asarray(last["timesteps"])[0, p, r:].any(), "%s: row %d is not zero behind its end" % (what, p)
