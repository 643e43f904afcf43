"""Helpers of the stream-compaction tests (TEST INFRASTRUCTURE ONLY): the host twin (tests/native/compact_host.cpp: the stream of
peek_util.HostStream with ctcdecode_amd/csrc/stream_compact.h run on its parked state and the product's capacity bookkeeping), and
the live-set count both test files hold the code under test to -- computed from the oracle's result rows alone."""
import ctypes
import os

import numpy as np
import oracle_util as ou
import peek_util as pu

ROOT = ou.ROOT
COMPACT_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctccompact_host.so")

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)


def build_compact_host():
    import subprocess

    native = os.path.join(ROOT, "tests", "native")
    src = os.path.join(native, "compact_host.cpp")
    csrc = os.path.join(ROOT, "ctcdecode_amd", "csrc")
    deps = [src, os.path.join(native, "peek_host.cpp"), os.path.join(native, "core_host.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if os.path.exists(COMPACT_HOST_SO) and all(os.path.getmtime(COMPACT_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return COMPACT_HOST_SO
    os.makedirs(os.path.dirname(COMPACT_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (COMPACT_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-DCTC_ASSUME_CHECKED", src, "-o", tmp, "-lpthread"], check=True)
    os.replace(tmp, COMPACT_HOST_SO)
    return COMPACT_HOST_SO


class HostStream(pu.HostStream):
    """One stream of the host twin: peek_util.HostStream's feed() and peek(), the pool sized and grown as the product sizes and grows
    it (frames_hint; min_nodes > 0: the policy of ctcd_set_stream_compaction), and compact()."""

    def __init__(self, V, beam, frames_hint, cutoff_prob=1.0, cutoff_top_n=40, blank_id=0, lm=None, min_nodes=0):
        lib = ctypes.CDLL(build_compact_host())
        lib.ctccompact_host_create.restype = ctypes.c_void_p
        lib.ctccompact_host_create.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                               ctypes.c_char_p, ctypes.c_char_p, ctypes.c_longlong]
        lib.ctccompact_host_destroy.argtypes = [ctypes.c_void_p]
        lib.ctccompact_host_destroy.restype = None
        lib.ctccompact_host_inner.argtypes = [ctypes.c_void_p]
        lib.ctccompact_host_inner.restype = ctypes.c_void_p
        lib.ctccompact_host_prepare.argtypes = [ctypes.c_void_p, ctypes.c_int]
        for name in ("ctccompact_host_compact", "ctccompact_host_pool_count", "ctccompact_host_compactions", "ctccompact_host_parents_below"):
            getattr(lib, name).argtypes = [ctypes.c_void_p]
        for name in ("ctccompact_host_capacity", "ctccompact_host_bound"):
            getattr(lib, name).argtypes = [ctypes.c_void_p]
            getattr(lib, name).restype = ctypes.c_longlong
        lib.ctccompact_host_digest.argtypes = [ctypes.c_void_p]
        lib.ctccompact_host_digest.restype = ctypes.c_ulonglong
        lib.ctcpeek_host_feed.argtypes = [ctypes.c_void_p, _f32p, ctypes.c_int, ctypes.c_int, _i32p, _i32p, _f32p, _i32p, _i32p, ctypes.c_int]
        lib.ctcpeek_host_peek.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _i32p, _i32p, ctypes.c_int, _f32p, _i32p, _i32p, _i32p,
                                          ctypes.POINTER(ctypes.c_ulonglong)]
        self.lib = lib
        self.V, self.beam, self.frames = V, beam, 0
        if lm is not None:
            alpha, beta, path, labels = lm
            self.c = lib.ctccompact_host_create(V, beam, frames_hint, cutoff_prob, cutoff_top_n, blank_id, alpha, beta, os.fsencode(path), ou._pack(labels), min_nodes)
        else:
            self.c = lib.ctccompact_host_create(V, beam, frames_hint, cutoff_prob, cutoff_top_n, blank_id, 0.0, 0.0, None, None, min_nodes)
        if not self.c:
            raise RuntimeError("could not create the host stream")
        self.h = lib.ctccompact_host_inner(self.c)  # (what the inherited feed() and peek() hand to ctcpeek_host_*)

    def feed(self, rows, finish=False):
        n = np.asarray(rows).reshape(-1, self.V).shape[0]
        if self.lib.ctccompact_host_prepare(self.c, n) != 0:
            raise RuntimeError("host stream: the chunk cannot be prepared")
        return pu.HostStream.feed(self, rows, finish)

    def compact(self):
        """-> nodes the stream keeps (1 before any frame)."""
        m = self.lib.ctccompact_host_compact(self.c)
        if m < 0:
            raise RuntimeError("host stream: compact returned %d" % m)
        return m

    capacity = property(lambda self: int(self.lib.ctccompact_host_capacity(self.c)))
    bound = property(lambda self: int(self.lib.ctccompact_host_bound(self.c)))
    pool_count = property(lambda self: int(self.lib.ctccompact_host_pool_count(self.c)))
    compactions = property(lambda self: int(self.lib.ctccompact_host_compactions(self.c)))
    digest = property(lambda self: int(self.lib.ctccompact_host_digest(self.c)))

    def parents_below(self):
        return self.lib.ctccompact_host_parents_below(self.c) == 1

    def __del__(self):
        if getattr(self, "c", None):
            self.lib.ctccompact_host_destroy(self.c)
            self.c = None
        self.h = None  # (destroyed with it)


def oracle_live_count(res, b):
    """1 + the number of distinct non-empty prefixes of ALL result rows of item b: the root and every trie node some beam entry hangs
    below -- what a compaction must keep, counted on the oracle's output alone."""
    nodes = {}
    for p in range(int(res["nres"][b])):
        cur = 0
        for tok in res["tokens"][b, p, :int(res["lens"][b, p])].tolist():
            cur = nodes.setdefault((cur, tok), len(nodes) + 1)
    return 1 + len(nodes)


def blank_dominated_long(T=3000, V=29, seed=71):
    """The stream of the policy tests: blank-dominated rows, one item."""
    return ou.synth_logprobs(1, T, V, seed, blank_bias=4)
