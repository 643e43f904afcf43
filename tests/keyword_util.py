"""Helpers of the keyword-search tests (TEST INFRASTRUCTURE ONLY): the definition of include/ctcdecode_amd.h "Keyword search" restated in
numpy float32 scalars, one operation at a time -- written from the header's text and not from keyword.h -- the case table the CPU and
the GPU tests share, and the ctypes front-end of the host twin (tests/native/keyword_host.cpp)."""
import ctypes
import math
import os
import subprocess

import numpy as np

import greedy_util as gu

HOST_SO = os.path.join(gu.ROOT, "oracle", "_build", "libctckw_host.so")
F32, NEG_INF = np.float32, np.float32(-np.inf)
F = 32  # the kernel's chunk of frames (keyword.h kKwChunk; test_keyword_host.py holds it against the twin's)


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def _lp(v, mode):
    return F32(v) if mode == 1 else F32(math.log(float(v) + gu.FLT_MIN))


def find_item(x, n, blank, mode, kw):
    """One keyword (a list of labels) against one item, ``x`` float32 [T, V].  -> (score, start, end, end_scores [T], end_starts [T])."""
    T, S = x.shape[0], 2 * len(kw) - 1
    z = [kw[s // 2] if s % 2 == 0 else blank for s in range(S)]
    d, best = [(NEG_INF, -1)] * S, (NEG_INF, -1, -1)
    tv, ts = np.zeros(T, np.float32), np.zeros(T, np.int32)
    with np.errstate(all="ignore"):
        for t in range(n):
            m = _lp(x[t, int(np.argmax(x[t]))], mode)
            nd = []
            for s in range(S):
                lp = _lp(x[t, z[s]], mode)
                r = NEG_INF if lp == NEG_INF else F32(lp - m)
                cands = [d[s]] + ([d[s - 1]] if s >= 1 else []) + ([d[s - 2]] if s >= 2 and s % 2 == 0 and z[s] != z[s - 2] else [])
                if s == 0:
                    cands.append((F32(0.0), t))
                b = cands[0]
                for c in cands[1:]:
                    if c[0] > b[0]:
                        b = c
                nd.append((F32(r + b[0]), b[1]))
            d = nd
            if d[-1][0] >= best[0]:
                best = (d[-1][0], d[-1][1], t)
            tv[t], ts[t] = d[-1]
    return (best if best[0] > NEG_INF else (best[0], -1, -1)) + (tv, ts)


def reference(c):
    """The whole contract on a case.  -> dict(scores, starts, ends [B, Q]; end_scores, end_starts [B, Q, T])."""
    x, (B, T, _), Q = c["x"], c["x"].shape, len(c["kws"])
    out = dict(scores=np.zeros((B, Q), np.float32), starts=np.zeros((B, Q), np.int32), ends=np.zeros((B, Q), np.int32),
               end_scores=np.zeros((B, Q, T), np.float32), end_starts=np.zeros((B, Q, T), np.int32))
    for b in range(B):
        n = T if c["seq_lens"] is None else min(max(int(c["seq_lens"][b]), 0), T)
        for q, kw in enumerate(c["kws"]):
            out["scores"][b, q], out["starts"][b, q], out["ends"][b, q], out["end_scores"][b, q], out["end_starts"][b, q] = find_item(x[b], n, c["blank"], c["mode"], kw)
    return out


def assert_same(got, want, what=""):
    for k, w in want.items():
        g = np.asarray(got[k]).reshape(w.shape)
        bad = np.argwhere((gu.bits(g) != gu.bits(w)) if w.dtype == np.float32 else (g != w))
        assert bad.size == 0, "%s: %s differs at %s: got %r, want %r" % (what, k, bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def kw_tensors(kws, Lk=None):
    Lk = Lk or max(len(k) for k in kws)
    a = np.zeros((len(kws), Lk), np.int32)
    for q, k in enumerate(kws):
        a[q, :len(k)] = k
    return a, np.asarray([len(k) for k in kws], np.int32)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
def _keyword(rng, L, V, blank):
    """L labels, none the blank, no two neighbours equal."""
    k = []
    while len(k) < L:
        c = int(rng.integers(0, V))
        if c != blank and (not k or c != k[-1]):
            k.append(c)
    return k


def case(name, dtype=0, mode=1, V=29, T=33, B=2, L=(3, 5), kws=None, seq_lens=None, paths=None, edit=None, width=None):
    """Random rows (or rows whose frame labels are ``paths``) and keywords of the lengths ``L``.  width: the lane group the call must take."""
    rng = np.random.default_rng(gu.hash_name("keyword " + name))
    blank = (0, V - 1)[len(name) % 2]
    raw = gu.path_rows(rng, paths, V, mode) if paths else gu.random_rows(rng, B, T, V, mode)
    if edit:
        edit(raw)
    stored, x = gu.as_dtype(raw, dtype)
    kws = kws or [_keyword(rng, l, V, blank) for l in L]
    Lk = max(len(k) for k in kws)
    return dict(name=name, stored=stored, x=x, seq_lens=None if seq_lens is None else np.asarray(seq_lens, np.int32), blank=blank, mode=mode, dtype=dtype,
                kws=kws, kernel=(dtype, mode == 0, V <= 128, width or (8 if Lk <= 8 else 16 if Lk <= 16 else 32 if Lk <= 32 else 64)))


def _neg_inf_rows(raw):
    raw[0, 3:6] = -np.inf  # frames of all -inf
    raw[:, :, 7] = -np.inf  # a label ruled out in every frame


_PATH = [1, 1, 0, 2, 2, 0, 0, 3, 4, 4, 0, 2, 5, 5]  # blank 0 ("window" has an even length): transcript 1 2 3 4 2 5, from frame 0 to the last
CASES = (
    # keyword lengths on both sides of every lane-group width (T >= 2L - 1 frames let a keyword with repeats fit too)
    [case("L%d" % L, dtype=i % 3, mode=i % 2, T=max(33, 2 * L + 3), B=1, L=(L, max(1, L - 2))) for i, L in enumerate((1, 8, 9, 16, 17, 32, 33, 64))]
    # every instantiation: element type x probabilities / log-probabilities x staged / gathered
    + [case("inst %d %d %d" % (dt, mode, V), dtype=dt, mode=mode, V=V, T=35) for dt in gu.DTYPES for mode in (0, 1) for V in (29, 130)]
    # T around the chunk on both routes; V on both sides of the staging threshold, and a long row
    + [case("T%d V%d" % (T, V), V=V, T=T) for V in (29, 130) for T in (F - 1, F, F + 1, 2 * F + 1)]
    + [case("V%d" % V, V=V, T=34, mode=V % 2) for V in (128, 129, 1025)]
    + [case("repeat", kws=[[5, 5, 7], [9, 9], [4, 6, 6, 6]]),
       case("longer than n", T=12, B=3, L=(6, 2), seq_lens=[4, 12, 5]),
       case("ragged", T=2 * F + 2, B=4, L=(1, 2, 4), seq_lens=[0, 1, 2 * F + 2, F + 1]),
       case("window", V=6, paths=[_PATH, _PATH[::-1]], kws=[[1, 2], [2, 5], [1, 2, 3, 4, 2, 5], [5, 2], [2, 1], [4]]),
       case("neg inf", V=12, T=20, kws=[[3, 5], [7], [2, 7, 4], [10]], edit=_neg_inf_rows)]
)
# (item, keyword, start, end) the restatement must give: a best window that starts at frame 0, one that ends at frame n - 1
WINDOWS = {"window": [(0, 0, 0, 4), (0, 1, 11, 13), (0, 2, 0, 13), (1, 3, 0, 2), (1, 4, 9, 13), (0, 5, 8, 9)]}


def reference_of(c):
    return gu.cached(("keyword", c["name"]), lambda: reference(c))


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_host():
    src = os.path.join(gu.NATIVE, "keyword_host.cpp")
    csrc = os.path.join(gu.ROOT, "ctcdecode_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("keyword.h", "greedy.h", "align.h", "blank_skip.h", "exact_math_f64.h", "exact_math_f64_tables.h", "exact_math.h")]
    if os.path.exists(HOST_SO) and all(os.path.getmtime(HOST_SO) >= os.path.getmtime(p) for p in deps):
        return HOST_SO
    os.makedirs(os.path.dirname(HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, HOST_SO)
    return HOST_SO


def host_lib():
    return gu.cached("keyword lib", lambda: ctypes.CDLL(build_host()))


def host_find(c, Lk=None):
    """The twin on a case, over output buffers of sentinel words.  -> (dict like reference's, status [Q])."""
    stored = np.ascontiguousarray(c["stored"])
    (B, T, V), (kws, lens) = stored.shape, kw_tensors(c["kws"], Lk)
    Q = len(lens)
    outs = dict(scores=np.full((B, Q), -123.0, np.float32), starts=np.full((B, Q), gu.SENTINEL, np.int32), ends=np.full((B, Q), gu.SENTINEL, np.int32),
                end_scores=np.full((B, Q, T), -123.0, np.float32), end_starts=np.full((B, Q, T), gu.SENTINEL, np.int32))
    status, sl = np.zeros(Q, np.int32), c["seq_lens"]
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
    rc = host_lib().ctckw_host_find(p(stored), c["dtype"], p(sl), B, T, V, c["blank"], c["mode"], p(kws), p(lens), Q, kws.shape[1],
                                    *[p(outs[k]) for k in ("scores", "starts", "ends", "end_scores", "end_starts")], p(status))
    assert rc == 0, "the twin refused its arguments"
    return outs, status
