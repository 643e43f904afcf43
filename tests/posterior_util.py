"""Helpers of the label-posterior tests (TEST INFRASTRUCTURE ONLY): the definition of include/ctcdecode_amd.h "Label posteriors"
restated in Python -- plain loops over frames and states with numpy.float32 scalars, expf / logf the box's own glibc through ctypes
(loglik_util's), written from the header's text and not from posterior.h -- a float64 numpy.logaddexp forward-backward for a tolerance
check, the cases the CPU and the GPU tests share (loglik_util's and three of its own), and the ctypes front-end of the host twin
(tests/native/posterior_host.cpp)."""
import ctypes
import os

import align_util as au
import loglik_util as lu
import numpy as np

ROOT = au.ROOT
NATIVE = au.NATIVE
POSTERIOR_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcposterior_host.so")
BAD_ROW = au.BAD_ROW
NEG_INF = lu.NEG_INF
F32 = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)

_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def e80(x):
    """x > 0 counts as 0; x < -80 gives 0.0f; otherwise glibc's expf(x)."""
    if x > 0:
        x = F32(0.0)
    if x < -80:
        return F32(0.0)
    return lu.expf(x)


def forward_backward(lp, n, y, blank):
    """One hypothesis that runs the recurrence (1 <= n, L <= n).  ``lp``: float32 [T, V].  -> (ll, a, b): a[t][s] and b[t][s] as lists
    of numpy.float32 (b is None if ll is -inf)."""
    L = len(y)
    S = 2 * L + 1
    z = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    a = [[NEG_INF] * S for _ in range(n)]
    a[0][0] = F32(lp[0, blank])
    if L >= 1:
        a[0][1] = F32(lp[0, z[1]])
    # (a state whose three predecessors are all -inf is lp + -inf = -inf: only the states from the first finite one of the frame before
    # to two beyond its last are computed, the others keep their -inf)
    def finite_range(v, lo, hi):
        f = [s for s in range(lo, hi) if v[s] != NEG_INF]
        return (f[0], f[-1] + 1) if f else (0, 0)

    lo, hi = finite_range(a[0], 0, S)
    for t in range(1, n):
        row, p, q = lp[t], a[t - 1], a[t]
        lo, hi = lo, min(S, hi + 2)
        for s in range(lo, hi):
            p1 = p[s - 1] if s >= 1 else NEG_INF
            p2 = p[s - 2] if s >= 3 and s % 2 == 1 and z[s] != z[s - 2] else NEG_INF
            q[s] = F32(F32(row[z[s]]) + lu.lse3(p[s], p1, p2))
        lo, hi = finite_range(q, lo, hi)
    ll = lu.lse3(a[n - 1][S - 1], a[n - 1][S - 2] if L >= 1 else NEG_INF, NEG_INF)
    if ll == NEG_INF:
        return ll, a, None
    b = [[NEG_INF] * S for _ in range(n)]
    b[n - 1][S - 1] = F32(lp[n - 1, blank])
    if L >= 1:
        b[n - 1][S - 2] = F32(lp[n - 1, z[S - 2]])
    lo, hi = finite_range(b[n - 1], 0, S)
    for t in range(n - 2, -1, -1):
        row, p, q = lp[t], b[t + 1], b[t]
        lo, hi = max(0, lo - 2), hi
        for s in range(lo, hi):
            p1 = p[s + 1] if s + 1 <= S - 1 else NEG_INF
            p2 = p[s + 2] if s % 2 == 1 and s + 2 <= S - 1 and z[s + 2] != z[s] else NEG_INF
            q[s] = F32(F32(row[z[s]]) + lu.lse3(p[s], p1, p2))
        lo, hi = finite_range(q, lo, hi)
    return ll, a, b


def posteriors(lp, n, y, blank, diag=None):
    """One valid hypothesis.  -> (peaks [L] int, occupancy [L], confidence [L], ll).  ``diag``: a dict whose counters "cells" (g formed
    from finite a, b), "clamped" (x > 0 formed) and "subnormal" (a non-zero product g * e80(lp) below FLT_MIN formed) are raised."""
    L = len(y)
    zero = ([0] * L, [F32(0.0)] * L, [F32(0.0)] * L)
    if n == 0:
        return zero + (F32(0.0) if L == 0 else NEG_INF,)
    if L > n:
        return zero + (NEG_INF,)
    with np.errstate(all="ignore"):
        ll, a, b = forward_backward(lp, n, y, blank)
        if ll == NEG_INF:
            return zero + (ll,)
        peaks, occs, confs = [], [], []
        for i in range(L):
            s, c = 2 * i + 1, int(y[i])
            occ, num, best, peak = F32(0.0), F32(0.0), None, 0
            for t in range(n - 1, -1, -1):
                if a[t][s] == NEG_INF or b[t][s] == NEG_INF:  # g = 0: both sums keep their bits, and 0 is the greatest only among zeros
                    if best is None or best == 0:
                        best, peak = F32(0.0), t
                    continue
                l = F32(lp[t, c])
                ab = F32(a[t][s] + b[t][s])
                if a[t][s] == NEG_INF or b[t][s] == NEG_INF or ab == NEG_INF:
                    g = F32(0.0)
                else:
                    x = F32(F32(ab - l) - ll)
                    g = e80(x)
                    if diag is not None:
                        diag["cells"] = diag.get("cells", 0) + 1
                        diag["clamped"] = diag.get("clamped", 0) + int(x > 0)
                prod = F32(g * e80(l))
                if diag is not None and 0 < float(prod) < FLT_MIN:
                    diag["subnormal"] = diag.get("subnormal", 0) + 1
                occ = F32(occ + g)
                num = F32(num + prod)
                if best is None or g >= best:  # (descending t: the smallest t among equals)
                    best, peak = g, t
            peaks.append(peak)
            occs.append(occ)
            confs.append(F32(num / occ) if occ != 0 else F32(0.0))
    return peaks, occs, confs, ll


def reference(lp, seq_lens, tokens, lens, blank):
    """The whole contract on a batch: ``lp`` float32 [B, T, V], ``seq_lens`` [B] or None, ``tokens`` [B, R, Ls], ``lens`` [B, R].
    -> dict(peaks int32 / occupancy / confidence float32 [B, R, Ls], loglik [B, R], status [B], valid [B, R] bool, diag)."""
    lp = np.ascontiguousarray(lp, np.float32)
    B, T, V = lp.shape
    R, Ls = tokens.shape[1], tokens.shape[2]
    out = dict(peaks=np.zeros((B, R, Ls), np.int32), occupancy=np.zeros((B, R, Ls), np.float32), confidence=np.zeros((B, R, Ls), np.float32),
               loglik=np.zeros((B, R), np.float32), status=np.zeros((B,), np.int32), valid=np.zeros((B, R), bool), diag={})
    for b in range(B):
        n = T if seq_lens is None else min(max(int(seq_lens[b]), 0), T)
        for r in range(R):
            L = int(lens[b, r])
            y = [int(c) for c in tokens[b, r, :L]] if 0 <= L <= Ls else None
            if y is None or any(c < 0 or c >= V or c == blank for c in y):
                out["status"][b] = BAD_ROW  # outputs 0
                continue
            pk, oc, cf, ll = posteriors(lp[b], n, y, blank, out["diag"])
            out["peaks"][b, r, :L], out["occupancy"][b, r, :L], out["confidence"][b, r, :L], out["loglik"][b, r] = pk, oc, cf, ll
            out["valid"][b, r] = True
    return out


def posteriors64(lp, n, y, blank):
    """The same quantities in float64 with numpy.logaddexp (a tolerance check, not a definition): -> (g [n, L], occupancy [L],
    confidence [L], ll); g is all 0 for a row without alignments."""
    L = len(y)
    S = 2 * L + 1
    if n == 0 or L > n:
        return np.zeros((n, L)), np.zeros(L), np.zeros(L), (0.0 if n == 0 and L == 0 else -np.inf)
    if L == 0:
        return np.zeros((n, 0)), np.zeros(0), np.zeros(0), float(np.asarray(lp[:n, blank], np.float64).sum())
    z =np.asarray([blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)])
    skip = np.zeros(S, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    skip_up = np.zeros(S, bool)
    skip_up[:-2] = skip[2:]
    lp = np.asarray(lp, np.float64)
    ninf = -np.inf
    with np.errstate(all="ignore"):
        a = np.full((n, S), ninf)
        a[0, :min(S, 2)] = lp[0, z[:2]]
        for t in range(1, n):
            p = a[t - 1]
            p1 = np.concatenate(([ninf], p[:-1]))
            p2 = np.where(skip, np.concatenate(([ninf, ninf], p[:-2])), ninf)
            a[t] = lp[t, z] + np.logaddexp(np.logaddexp(p, p1), p2)
        ll = np.logaddexp(a[n - 1, S - 1], a[n - 1, S - 2]) if L >= 1 else a[n - 1, S - 1]
        if not np.isfinite(ll):
            return np.zeros((n, L)), np.zeros(L), np.zeros(L), float(ll)
        b = np.full((n, S), ninf)
        b[n - 1, max(S - 2, 0):] = lp[n - 1, z[max(S - 2, 0):]]
        for t in range(n - 2, -1, -1):
            p = b[t + 1]
            p1 = np.concatenate((p[1:], [ninf]))
            p2 = np.where(skip_up, np.concatenate((p[2:], [ninf, ninf])), ninf)
            b[t] = lp[t, z] + np.logaddexp(np.logaddexp(p, p1), p2)
        lab = lp[:n][:, z[1::2]]
        x = a[:, 1::2] + b[:, 1::2] - lab - ll
        x = np.where(np.isnan(x), ninf, x)
        g = np.where(x < -80, 0.0, np.exp(np.minimum(x, 0.0)))
        e = np.where(lab < -80, 0.0, np.exp(np.minimum(lab, 0.0)))
        occ = g.sum(0)
        conf = np.where(occ > 0, (g * e).sum(0) / np.where(occ > 0, occ, 1.0), 0.0)
    return g, occ, conf, float(ll)


KEYS = ("peaks", "occupancy", "confidence", "loglik")


def assert_same(got, want, what=""):
    """Bit for bit: the float outputs as uint32, the peaks and the status exactly.  ``got``: dict with peaks / occupancy / confidence /
    loglik (/ status)."""
    for k in KEYS:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype)
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert bad.size == 0, "%s: %s differs at %s: got %r, want %r" % (what, k, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    if "status" in got:
        assert np.asarray(got["status"]).tolist() == want["status"].tolist(), "%s: status %s, want %s" % (what, got["status"], want["status"])


# ---- cases -------------------------------------------------------------------------------------------------------------------------
NEW_CASES = ["dyadic_single_path", "clamped", "subnormal"]
CASES = lu.CASES + NEW_CASES


def make_case(name):
    """-> dict(lp float32 [B, T, V], seq_lens int32 [B] or None, tokens, lens, blank).  Deterministic per name."""
    if name not in NEW_CASES:
        return lu.make_case(name)
    rng = np.random.default_rng(au.hash_name(name))
    blank, seq = 0, None
    if name == "dyadic_single_path":
        # L == n without adjacent repeats: one alignment; every lp a multiple of 0.25, so every sum is exact.  Items of 6, 5 and 1 frames.
        T, V = 6, 5
        lp = (-0.25 * rng.integers(0, 17, (3, T, V))).astype(np.float32)
        seq = np.asarray([6, 5, 1], np.int32)
        rows = [[au.cycle(6, V), au.cycle(6, V, first=2), [4, 1, 4, 2, 4, 3]], [au.cycle(5, V), au.cycle(5, V, first=3), [2, 1, 2, 1, 2]], [[1], [3], [4]]]
        tok, lens = au.pack_rows(rows, R=3, Ls=T)
    elif name == "clamped":
        # rows with few alignments (L only just below n): a cell that nearly every alignment passes has a + b - lp within rounding of
        # ll, and rounding lifts the difference above 0 in some of them
        T, V = 45, 6
        lp = au.log_softmax_rows(rng, 2, T, V, scale=1.0)
        seq = np.asarray([45, 41], np.int32)
        rows = [[au.cycle(int(n) - d, V, first=d) for d in (1, 2, 3, 5)] + au.random_rows(rng, 1, 2, 30, V, repeat=0.1)[0] for n in seq]
        tok, lens = au.pack_rows(rows, R=6, Ls=T)
    elif name == "subnormal":
        # frame 0 all but rules label 1 out (lp = -55) where the blank is merely unlikely (-15): the label's posterior there is about
        # 2 e^-40, and its product with e80(-55) about 2 e^-95 -- below FLT_MIN (e^-87.3), above the least subnormal (e^-103.3)
        T, V = 4, 3
        lp = np.full((2, T, V), np.log(1.0 / 3.0), np.float32)
        lp[:, 0, 0], lp[:, 0, 1], lp[:, 0, 2] = -15.0, -55.0, -56.5
        lp[1, 1:] = au.log_softmax_rows(rng, 1, T - 1, V)[0]
        seq = np.asarray([2, 4], np.int32)
        rows = [[[1], [2], [1, 2], []]] * 2
        tok, lens = au.pack_rows(rows, R=4, Ls=T)
    return dict(lp=np.ascontiguousarray(lp, np.float32), seq_lens=seq, tokens=tok, lens=lens, blank=blank)


_CACHE = {}


def case(name):
    """The case and its reference (computed once per process, shared among the tests that need it, and left unchanged)."""
    if name not in _CACHE:
        c = make_case(name)
        _CACHE[name] = (c, reference(c["lp"], c["seq_lens"], c["tokens"], c["lens"], c["blank"]))
    return _CACHE[name]


def release():
    """Drops the cached cases: a test module that is done with them leaves the process as it found it."""
    _CACHE.clear()


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_posterior_host():
    import subprocess

    src = os.path.join(NATIVE, "posterior_host.cpp")
    csrc = os.path.join(ROOT, "ctcdecode_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("posterior.h", "loglik.h", "align.h", "blank_skip.h", "exact_math_f64.h", "exact_math_f64_tables.h", "exact_math.h")]
    if os.path.exists(POSTERIOR_HOST_SO) and all(os.path.getmtime(POSTERIOR_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return POSTERIOR_HOST_SO
    os.makedirs(os.path.dirname(POSTERIOR_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (POSTERIOR_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, POSTERIOR_HOST_SO)
    return POSTERIOR_HOST_SO


def _lib():
    def make():
        lib = ctypes.CDLL(build_posterior_host())
        lib.ctcpost_host_posteriors.argtypes = [ctypes.c_void_p, ctypes.c_int, _i32p] + [ctypes.c_int] * 5 + [_i32p, _i32p, ctypes.c_int, ctypes.c_int, _i32p, _f32p, _f32p,
                                                                                                         _f32p, _i32p]
        lib.ctcpost_host_e80.argtypes = [ctypes.c_float]
        lib.ctcpost_host_e80.restype = ctypes.c_float
        lib.ctcpost_host_g.argtypes = [ctypes.c_float] * 4
        lib.ctcpost_host_g.restype = ctypes.c_float
        lib.ctcpost_host_slot_bytes.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.ctcpost_host_slot_bytes.restype = ctypes.c_ulonglong
        lib.ctcpost_host_wave_floats.argtypes = [ctypes.c_int]
        lib.ctcpost_host_wave_floats.restype = ctypes.c_ulonglong
        lib.ctcpost_host_grid.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_ulonglong]
        lib.ctcpost_host_grid.restype = ctypes.c_longlong
        lib.ctcpost_host_default_scratch.restype = ctypes.c_longlong
        return lib
    return au.cached("posterior host lib", make)


def host_posteriors(rows, seq_lens, tokens, lens, blank, log_input=1, dtype=0):
    """The twin over pre-filled outputs.  ``rows``: [B, T, V] float32 (dtype 0) or uint16 bit patterns (1: f16, 2: bf16)."""
    rows = np.ascontiguousarray(rows)
    B, T, V = rows.shape
    tokens, lens = np.ascontiguousarray(tokens, np.int32), np.ascontiguousarray(lens, np.int32)
    R, Ls = tokens.shape[1], tokens.shape[2]
    pk = np.full((B, R, Ls), 0x5A5A5A5A, np.int32)
    oc, cf = (np.full((B, R, Ls), np.float32(-123.0), np.float32) for _ in range(2))
    ll = np.full((B, R), np.float32(-123.0), np.float32)
    status = np.zeros((B,), np.int32)
    sl = None if seq_lens is None else np.ascontiguousarray(seq_lens, np.int32)
    rc = _lib().ctcpost_host_posteriors(rows.ctypes.data, dtype, None if sl is None else sl.ctypes.data_as(_i32p), B, T, V, blank, log_input,
                                        tokens.ctypes.data_as(_i32p), lens.ctypes.data_as(_i32p), R, Ls, pk.ctypes.data_as(_i32p), oc.ctypes.data_as(_f32p),
                                        cf.ctypes.data_as(_f32p), ll.ctypes.data_as(_f32p), status.ctypes.data_as(_i32p))
    assert rc >= 0, "the twin refused its arguments"
    return dict(peaks=pk, occupancy=oc, confidence=cf, loglik=ll, status=status, invalid_rows=rc)


def host_e80(x):
    return F32(_lib().ctcpost_host_e80(float(x)))


def host_g(a, b, lp, ll):
    return F32(_lib().ctcpost_host_g(float(a), float(b), float(lp), float(ll)))


def host_slot_bytes(T, Ls):
    return int(_lib().ctcpost_host_slot_bytes(int(T), int(Ls)))


def host_wave_floats(T):
    return int(_lib().ctcpost_host_wave_floats(int(T)))


def host_grid(rows, budget, slot_bytes):
    return int(_lib().ctcpost_host_grid(int(rows), int(budget), int(slot_bytes)))


def host_default_scratch():
    return int(_lib().ctcpost_host_default_scratch())
