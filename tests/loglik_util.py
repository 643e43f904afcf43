"""Helpers of the CTC log-likelihood tests (TEST INFRASTRUCTURE ONLY): the definition of include/ctcdecode_amd.h "CTC log-likelihood"
restated in Python -- a plain double loop over frames and states with numpy.float32 scalars, expf / logf the box's own glibc through
ctypes, written from the header's text and not from loglik.h -- a float64 numpy.logaddexp restatement for a tolerance check, the cases
the CPU and the GPU tests share (align_util's and four of its own), and the ctypes front-end of the host twin
(tests/native/loglik_host.cpp)."""
import ctypes
import os

import align_util as au
import numpy as np

ROOT = au.ROOT
NATIVE = au.NATIVE
LOGLIK_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcloglik_host.so")
BAD_ROW = au.BAD_ROW
NEG_INF = np.float32(-np.inf)
F32 = np.float32

_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)

# the pin of test_device_math_bit_exact_vs_host_libm: this box's glibc, float in, float out
_libm = ctypes.CDLL("libm.so.6")
_libm.expf.argtypes = [ctypes.c_float]
_libm.expf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
_libm.logf.restype = ctypes.c_float


def expf(x):
    return F32(_libm.expf(float(x)))


def logf(x):
    return F32(_libm.logf(float(x)))


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def lse3(v0, v1, v2):
    """logf((expf(v0 - m) + expf(v1 - m)) + expf(v2 - m)) + m, every operation one float32 operation; -inf if the maximum is -inf."""
    m = max(v0, v1, v2)
    if m == NEG_INF:
        return NEG_INF
    e0, e1, e2 = (F32(0.0) if v == NEG_INF else expf(F32(v - m)) for v in (v0, v1, v2))  # (expf(-inf) = 0)
    return F32(logf(F32(F32(e0 + e1) + e2)) + m)


def forward(lp, n, y, blank):
    """One hypothesis.  ``lp``: float32 [T, V] log-probabilities, ``n`` frames of it count, ``y``: the labels.  -> float32."""
    L = len(y)
    S = 2 * L + 1
    if n == 0:
        return F32(0.0) if L == 0 else NEG_INF
    if L > n:
        return NEG_INF
    z = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    a = [NEG_INF] * S
    a[0] = F32(lp[0, blank])
    if L >= 1:
        a[1] = F32(lp[0, z[1]])
    with np.errstate(all="ignore"):
        for t in range(1, n):
            row = lp[t]
            na = [NEG_INF] * S
            for s in range(S):
                p1 = a[s - 1] if s >= 1 else NEG_INF
                p2 = a[s - 2] if s >= 3 and s % 2 == 1 and z[s] != z[s - 2] else NEG_INF
                na[s] = F32(F32(row[z[s]]) + lse3(a[s], p1, p2))  # one float32 addition
            a = na
        return lse3(a[S - 1], a[S - 2] if L >= 1 else NEG_INF, NEG_INF)


def reference(lp, seq_lens, tokens, lens, blank):
    """The whole contract on a batch: ``lp`` float32 [B, T, V], ``seq_lens`` [B] or None, ``tokens`` [B, R, Ls], ``lens`` [B, R].
    -> dict(loglik [B, R] float32, status [B] int32, valid [B, R] bool)."""
    lp = np.ascontiguousarray(lp, np.float32)
    B, T, V = lp.shape
    R, Ls = tokens.shape[1], tokens.shape[2]
    out = dict(loglik=np.zeros((B, R), np.float32), status=np.zeros((B,), np.int32), valid=np.zeros((B, R), bool))
    for b in range(B):
        n = T if seq_lens is None else min(max(int(seq_lens[b]), 0), T)
        for r in range(R):
            L = int(lens[b, r])
            y = [int(c) for c in tokens[b, r, :L]] if 0 <= L <= Ls else None
            if y is None or any(c < 0 or c >= V or c == blank for c in y):
                out["status"][b] = BAD_ROW  # output 0
                continue
            out["loglik"][b, r] = forward(lp[b], n, y, blank)
            out["valid"][b, r] = True
    return out


def forward64(lp, n, y, blank):
    """The same recurrence in float64 with numpy.logaddexp (a tolerance check, not a definition).  -> (ll, A): A = the largest finite
    |a| of the recurrence."""
    L = len(y)
    S = 2 * L + 1
    if n == 0:
        return (0.0 if L == 0 else -np.inf), 0.0
    if L > n:
        return -np.inf, 0.0
    z = np.asarray([blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)])
    skip = np.zeros(S, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    lp = np.asarray(lp, np.float64)
    a = np.full(S, -np.inf)
    a[:min(S, 2)] = lp[0, z[:2]]
    big = np.abs(a[np.isfinite(a)]).max(initial=0.0)
    with np.errstate(all="ignore"):
        for t in range(1, n):
            p1 = np.concatenate(([-np.inf], a[:-1]))
            p2 = np.where(skip, np.concatenate(([-np.inf, -np.inf], a[:-2])), -np.inf)
            a = lp[t, z] + np.logaddexp(np.logaddexp(a, p1), p2)
            big = max(big, np.abs(a[np.isfinite(a)]).max(initial=0.0))
        ll = np.logaddexp(a[S - 1], a[S - 2]) if L >= 1 else a[S - 1]
    return float(ll), float(big)


def assert_same(got, want, what=""):
    """Bit for bit, as uint32.  ``got``: float32 [B, R] or a dict with loglik (/ status)."""
    g = got["loglik"] if isinstance(got, dict) else got
    g, w = np.ascontiguousarray(g, np.float32), np.ascontiguousarray(want["loglik"], np.float32)
    assert g.shape == w.shape, what
    bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
    assert bad.size == 0, "%s: log-likelihoods differ at %s: got %r, want %r" % (what, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])
    if isinstance(got, dict) and "status" in got:
        assert np.asarray(got["status"]).tolist() == want["status"].tolist(), "%s: status %s, want %s" % (what, got["status"], want["status"])


def single_path_rows(c):
    """(b, r, n) of the rows with exactly one alignment that reaches the end: L == 0, or L == n without adjacent repeats (n >= 1)."""
    B, T, _ = c["lp"].shape
    rows = []
    for b in range(B):
        n = T if c["seq_lens"] is None else min(max(int(c["seq_lens"][b]), 0), T)
        for r in range(c["tokens"].shape[1]):
            L = int(c["lens"][b, r])
            y = c["tokens"][b, r, :L]
            if n >= 1 and (L == 0 or (L == n and all(y[i] != y[i - 1] for i in range(1, L)))):
                rows.append((b, r, n))
    return rows


def path_sum(c, b, r, n):
    """The float32 sum, in frame order, of the lp along a single-path row's only alignment."""
    L = int(c["lens"][b, r])
    acc = None
    for t in range(n):
        v = F32(c["lp"][b, t, c["blank"] if L == 0 else int(c["tokens"][b, r, t])])
        acc = v if acc is None else F32(v + acc)
    return acc


# ---- cases -------------------------------------------------------------------------------------------------------------------------
NEW_CASES = ["zeros", "far_apart", "positive", "overflow"]
CASES = au.CASES + NEW_CASES


def make_case(name):
    """-> dict(lp float32 [B, T, V], seq_lens int32 [B] or None, tokens, lens, blank).  Deterministic per name."""
    if name not in NEW_CASES:
        return au.make_case(name)
    rng = np.random.default_rng(au.hash_name(name))
    blank, seq = 0, None
    if name == "zeros":
        # item 0: every log-probability -0.0 (a lone predecessor m = -0.0 yields +0 + m = +0.0: rows 0 and 4 have a single path);
        # item 1: every one +0.0; item 2: a mix of both zeros and two negative values
        T, V = 6, 8
        lp = np.zeros((3, T, V), np.float32)
        lp[0] = -0.0
        lp[2] = rng.choice(np.asarray([0.0, -0.0, -1.0, -0.25], np.float32), (T, V))
        rows = [[[], [1], [1, 2], [1, 1], au.cycle(6, V), [3, 3, 4]]] * 3
        tok, lens = au.pack_rows(rows, R=6, Ls=T)
    elif name == "far_apart":
        # frame 0 sets a[0][1] - a[0][0] to -87.5, -88.5 and -200 (items 0 .. 2) and to their negatives (items 3 .. 5): an expf term only
        # just survives, only just vanishes, vanishes; the other frames draw from values that keep such gaps coming
        T, V = 12, 5
        lp = rng.choice(np.asarray([-1.0, -44.0, -44.25, -88.5, -89.5, -201.0], np.float32), (6, T, V))
        for b, gap in enumerate((-87.5, -88.5, -200.0)):
            lp[b, 0, 0], lp[b, 0, 1:] = -1.0, -1.0 + gap
            lp[b + 3, 0, 0], lp[b + 3, 0, 1:] = -1.0 + gap, -1.0
        rows = [[[1], [2, 3], [1, 1], [], [4, 2, 1], [3, 4, 4, 1]]] * 6
        tok, lens = au.pack_rows(rows, R=6, Ls=T)
    elif name == "positive":
        # log_input == 1 takes the values as they are: unnormalised rows with positive entries
        T, V = 24, 8
        lp = (rng.standard_normal((2, T, V)) * 3.0).astype(np.float32)
        lp[1] += 5.0
        tok, lens = au.pack_rows(au.random_rows(rng, 2, 6, 10, V), R=6, Ls=T)
        seq = np.asarray([24, 17], np.int32)
    elif name == "overflow":
        # finite values near -3e38: item 0 has one such label (paths through it vanish, lp + a overflows to -inf), item 1 only such
        # values (every sum of two frames is -inf), item 2 such a blank (only rows that never need a blank stay finite)
        T, V = 8, 6
        lp = au.log_softmax_rows(rng, 3, T, V)
        lp[0, :, 2] = -3.0e38
        lp[1] = -2.0e38
        lp[2, :, 0] = -1.5e38
        rows = [[[1, 3], [2], [1, 2, 3], [], [4, 2, 2, 5], au.cycle(8, V)]] * 3
        tok, lens = au.pack_rows(rows, R=6, Ls=T)
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
def build_loglik_host():
    import subprocess

    src = os.path.join(NATIVE, "loglik_host.cpp")
    csrc = os.path.join(ROOT, "ctcdecode_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("loglik.h", "align.h", "blank_skip.h", "exact_math_f64.h", "exact_math_f64_tables.h", "exact_math.h")]
    if os.path.exists(LOGLIK_HOST_SO) and all(os.path.getmtime(LOGLIK_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return LOGLIK_HOST_SO
    os.makedirs(os.path.dirname(LOGLIK_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (LOGLIK_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, LOGLIK_HOST_SO)
    return LOGLIK_HOST_SO


def _lib():
    def make():
        lib = ctypes.CDLL(build_loglik_host())
        lib.ctcloglik_host_loglik.argtypes = [ctypes.c_void_p, ctypes.c_int, _i32p] + [ctypes.c_int] * 5 + [_i32p, _i32p, ctypes.c_int, ctypes.c_int, _f32p, _i32p]
        lib.ctcloglik_host_lse3.argtypes = [ctypes.c_float] * 3
        lib.ctcloglik_host_lse3.restype = ctypes.c_float
        lib.ctcloglik_host_units.argtypes = [ctypes.c_longlong, ctypes.c_int]
        lib.ctcloglik_host_units.restype = ctypes.c_longlong
        lib.ctcloglik_host_occupancy.argtypes = [ctypes.c_int]
        lib.ctcloglik_host_grid.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
        lib.ctcloglik_host_grid.restype = ctypes.c_longlong
        return lib
    return au.cached("loglik host lib", make)


def host_loglik(rows, seq_lens, tokens, lens, blank, log_input=1, dtype=0):
    """The twin over a pre-filled output.  ``rows``: [B, T, V] float32 (dtype 0) or uint16 bit patterns (1: f16, 2: bf16)."""
    rows = np.ascontiguousarray(rows)
    B, T, V = rows.shape
    tokens, lens = np.ascontiguousarray(tokens, np.int32), np.ascontiguousarray(lens, np.int32)
    R, Ls = tokens.shape[1], tokens.shape[2]
    out = np.full((B, R), np.float32(-123.0), np.float32)
    status = np.zeros((B,), np.int32)
    sl = None if seq_lens is None else np.ascontiguousarray(seq_lens, np.int32)
    rc = _lib().ctcloglik_host_loglik(rows.ctypes.data, dtype, None if sl is None else sl.ctypes.data_as(_i32p), B, T, V, blank, log_input,
                                      tokens.ctypes.data_as(_i32p), lens.ctypes.data_as(_i32p), R, Ls, out.ctypes.data_as(_f32p), status.ctypes.data_as(_i32p))
    assert rc >= 0, "the twin refused its arguments"
    return dict(loglik=out, status=status, invalid_rows=rc)


def host_lse3(v0, v1, v2):
    return F32(_lib().ctcloglik_host_lse3(float(v0), float(v1), float(v2)))


def host_units(rows, cls):
    return int(_lib().ctcloglik_host_units(int(rows), int(cls)))


def host_occupancy(cls):
    return int(_lib().ctcloglik_host_occupancy(int(cls)))


def host_grid(units, cap, cus, cls):
    return int(_lib().ctcloglik_host_grid(int(units), int(cap), int(cus), int(cls)))
