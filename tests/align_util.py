"""Helpers of the forced-alignment tests (TEST INFRASTRUCTURE ONLY): the definition of include/ctcdecode_amd.h "Forced alignment"
restated in numpy float32 -- a plain double loop over frames and states, written from the header's text and not from align.h -- the
cases the CPU and the GPU tests share, and the ctypes front-end of the host twin (tests/native/align_host.cpp)."""
import ctypes
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
ALIGN_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcalign_host.so")
BAD_ROW = 8  # include/ctcdecode_amd.h CTCD_ALIGN_BAD_ROW
FLT_MIN = float(np.finfo(np.float32).tiny)
NEG_INF = np.float32(-np.inf)

_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def viterbi(lp, n, y, blank):
    """One hypothesis.  ``lp``: float32 [T, V] log-probabilities, ``n`` frames of it count, ``y``: the labels.  -> (score float32,
    start list, end list, aligned bool, ties): ``ties`` = the cells of the traced path (the end state included) at which two allowed
    predecessors share the greatest value -- more than zero means that another path has the same score, and the tie rules alone
    decided the spans."""
    L = len(y)
    S = 2 * L + 1
    if n == 0:
        return (np.float32(0.0) if L == 0 else NEG_INF), [0] * L, [0] * L, L == 0, 0
    z = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(S)]
    d = [NEG_INF] * S
    d[0] = np.float32(lp[0, blank])
    if L >= 1:
        d[1] = np.float32(lp[0, z[1]])
    bp = np.zeros((n, S), np.int8)
    tie = np.zeros((n, S), bool)
    for t in range(1, n):
        row = lp[t]
        nd = [NEG_INF] * S
        for s in range(S):
            best, arg, tied = d[s], 0, False  # stay: the largest state index comes first, and only a greater value replaces it
            if s >= 1:
                if d[s - 1] > best:
                    best, arg, tied = d[s - 1], 1, False
                elif d[s - 1] == best:
                    tied = True
            if s >= 3 and s % 2 == 1 and z[s] != z[s - 2]:
                if d[s - 2] > best:
                    best, arg, tied = d[s - 2], 2, False
                elif d[s - 2] == best:
                    tied = True
            nd[s] = np.float32(row[z[s]]) + best  # one float32 addition
            bp[t, s] = arg
            tie[t, s] = tied and best > NEG_INF
        d = nd
    e, ties = S - 1, 0
    if L >= 1:
        if d[S - 2] > d[S - 1]:
            e = S - 2
        elif d[S - 2] == d[S - 1] and d[e] > NEG_INF:
            ties += 1
    score = np.float32(d[e])
    if not score > NEG_INF:
        return NEG_INF, [0] * L, [0] * L, False, 0
    start, end = [0] * L, [0] * L
    seen = [False] * L
    s = e
    for t in range(n - 1, -1, -1):
        if s % 2 == 1:
            i = s // 2
            if not seen[i]:
                seen[i], end[i] = True, t
            start[i] = t
        if t > 0:
            ties += int(tie[t, s])
            s -= int(bp[t, s])
    assert all(seen), "a finite score whose path misses a label"
    return score, start, end, True, ties


def reference(lp, seq_lens, tokens, lens, blank):
    """The whole contract on a batch: ``lp`` float32 [B, T, V], ``seq_lens`` [B] or None, ``tokens`` [B, R, Ls], ``lens`` [B, R].
    -> dict(start, end [B, R, Ls] int32, scores [B, R] float32, status [B] int32, ties [B, R] int)."""
    lp = np.ascontiguousarray(lp, np.float32)
    B, T, V = lp.shape
    R, Ls = tokens.shape[1], tokens.shape[2]
    out = dict(start=np.zeros((B, R, Ls), np.int32), end=np.zeros((B, R, Ls), np.int32), scores=np.zeros((B, R), np.float32),
               status=np.zeros((B,), np.int32), ties=np.zeros((B, R), np.int64), aligned=np.zeros((B, R), bool))
    for b in range(B):
        n = T if seq_lens is None else min(max(int(seq_lens[b]), 0), T)
        for r in range(R):
            L = int(lens[b, r])
            y = [int(c) for c in tokens[b, r, :L]] if 0 <= L <= Ls else None
            if y is None or any(c < 0 or c >= V or c == blank for c in y):
                out["status"][b] = BAD_ROW  # outputs zero, score 0
                continue
            sc, st, en, ok, ties = viterbi(lp[b], n, y, blank)
            out["scores"][b, r] = sc
            out["start"][b, r, :L] = st
            out["end"][b, r, :L] = en
            out["ties"][b, r] = ties
            out["aligned"][b, r] = ok
    return out


def prob_to_lp(p):
    """log_input == 0, per element: float32(math.log(float64(p) + FLT_MIN))."""
    p = np.asarray(p, np.float32)
    flat = [np.float32(math.log(float(v) + FLT_MIN)) for v in p.reshape(-1)]
    return np.asarray(flat, np.float32).reshape(p.shape)


def assert_same(got, want, what=""):
    """Bit for bit: scores as uint32, spans and status exactly.  ``got``: dict with start / end / scores (/ status)."""
    assert got["scores"].shape == want["scores"].shape and got["start"].shape == want["start"].shape, what
    gs, ws = np.ascontiguousarray(got["scores"], np.float32).view(np.uint32), np.ascontiguousarray(want["scores"], np.float32).view(np.uint32)
    bad = np.argwhere(gs != ws)
    assert bad.size == 0, "%s: scores differ at %s: got %r, want %r" % (what, bad[:4].tolist(), got["scores"][tuple(bad[0])], want["scores"][tuple(bad[0])])
    for k in ("start", "end"):
        bad = np.argwhere(np.asarray(got[k]) != want[k])
        assert bad.size == 0, "%s: %s differs at %s: got %s, want %s" % (what, k, bad[:4].tolist(), np.asarray(got[k])[tuple(bad[0])], want[k][tuple(bad[0])])
    if "status" in got:
        assert np.asarray(got["status"]).tolist() == want["status"].tolist(), "%s: status %s, want %s" % (what, got["status"], want["status"])


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def log_softmax_rows(rng, B, T, V, scale=2.0):
    x = rng.standard_normal((B, T, V)) * scale
    x = x - np.log(np.exp(x).sum(-1, keepdims=True))
    return x.astype(np.float32)


def pack_rows(rows, R=None, Ls=None, fill=0):
    """rows: per item a list of label lists -> (tokens [B, R, Ls] int32, lens [B, R] int32); rows beyond an item's list have length 0."""
    B = len(rows)
    R = R or max(len(r) for r in rows)
    Ls = Ls if Ls is not None else max([len(y) for r in rows for y in r] + [1])
    tok = np.full((B, R, Ls), fill, np.int32)
    lens = np.zeros((B, R), np.int32)
    for b, item in enumerate(rows):
        for r, y in enumerate(item):
            tok[b, r, :len(y)] = y
            lens[b, r] = len(y)
    return tok, lens


def cycle(L, V, blank=0, first=0):
    """L labels without a repeat next to each other (no blank needs to fit between them)."""
    labs = [c for c in range(V) if c != blank]
    return [labs[(first + i) % len(labs)] for i in range(L)]


def random_rows(rng, B, R, Lmax, V, blank=0, repeat=0.3):
    rows = []
    labs = [c for c in range(V) if c != blank]
    for b in range(B):
        item = []
        for r in range(R):
            L = int(rng.integers(0, Lmax + 1))
            y = []
            for i in range(L):
                y.append(y[-1] if y and rng.random() < repeat else labs[int(rng.integers(0, len(labs)))])
            item.append(y)
        rows.append(item)
    return rows


def make_case(name):
    """-> dict(lp float32 [B, T, V], seq_lens int32 [B] or None, tokens, lens, blank).  Deterministic per name."""
    rng = np.random.default_rng(abs(hash_name(name)))
    blank, seq = 0, None
    if name == "edges":
        # L = 0 at n = 0 and 1; L = 1 at n = 1; L > n; "a a" at n = 3; L = n distinct / with one repeat; rows of length 0; ragged n with a 0
        T, V = 6, 8
        seq = np.asarray([0, 1, 3, 6, 9], np.int32)  # (9: clamped to T)
        rows = [[[], [1], [2, 3]], [[], [4], [1, 2]], [[1, 1], [1, 2, 3], [1, 1, 2], [], [5]], [[1, 2, 3, 4, 5, 6], [1, 2, 2, 4, 5, 6], [7, 7, 7], [3]],
                [[2, 2, 2], [1, 2, 3, 4, 5, 7], [6]]]
        tok, lens = pack_rows(rows, R=6, Ls=T)
        lp = log_softmax_rows(rng, 5, T, V)
    elif name == "one_frame":
        T, V = 1, 5
        tok, lens = pack_rows([[[], [2], [1, 2]], [[4], [], [3, 3]]], R=3, Ls=3)
        lp = log_softmax_rows(rng, 2, T, V)
    elif name == "wave_edge":
        # S = 63 and 65: item 0's rows all fit a wave (side by side, one per wave); item 1 has a row of 65 states (the workgroup runs its rows)
        T, V = 37, 8
        rows = [[cycle(31, V), cycle(30, V, first=2), [1, 1, 2], []], [cycle(32, V), cycle(31, V, first=1), [5], []]]
        tok, lens = pack_rows(rows, R=4, Ls=T)
        lp = log_softmax_rows(rng, 2, T, V)
        seq = np.asarray([37, 36], np.int32)
    elif name == "workgroup_edge":
        # S = 255, 257, 259 around the workgroup's 256 lanes (1 state per lane | 4); T only just >= L, V = 4
        T, V = 130, 4
        rows = [[cycle(127, V), cycle(128, V), cycle(129, V, first=1), cycle(64, V)]]
        tok, lens = pack_rows(rows, R=4, Ls=T)
        lp = log_softmax_rows(rng, 1, T, V, scale=1.0)
    elif name == "many_per_lane":
        # S = 1023 (4 states per lane) and 1025 (16); T only just >= L and no multiple of 16, V = 4
        T, V = 514, 4
        rows = [[cycle(512, V), cycle(511, V, first=2), [1, 2, 3], []]]
        tok, lens = pack_rows(rows, R=4, Ls=T)
        lp = log_softmax_rows(rng, 1, T, V, scale=1.0)
    elif name == "ties_half":
        # log-probabilities quantised to multiples of 0.5: sums are exact and equal sums are common
        T, V = 21, 5
        lp = (-0.5 * rng.integers(0, 4, (3, T, V))).astype(np.float32)
        tok, lens = pack_rows(random_rows(rng, 3, 8, 9, V), R=8, Ls=T)
        seq = np.asarray([21, 20, 13], np.int32)
    elif name == "ties_constant":
        # every frame the same row, every label the same value: every path of a hypothesis has the same score
        T, V = 19, 5
        lp = np.full((2, T, V), -1.25, np.float32)
        lp[1] = np.asarray([-0.5, -1.0, -1.0, -2.0, -0.5], np.float32)  # (frame-constant, not label-constant)
        tok, lens = pack_rows(random_rows(rng, 2, 8, 7, V), R=8, Ls=T)
    elif name == "neg_inf":
        # label 2 impossible over frames 3 .. 9 of item 0; frame 5 of item 1 impossible altogether (not aligned)
        T, V = 18, 6
        lp = log_softmax_rows(rng, 2, T, V)
        lp[0, 3:10, 2] = -np.inf
        lp[1, 5, :] = -np.inf
        rows = [[[1, 2, 3], [2, 2], [2], [], [4, 2, 2, 5]], [[1, 2, 3], [], [4]]]
        tok, lens = pack_rows(rows, R=5, Ls=T)
    elif name == "blank_last":
        T, V, blank = 23, 7, 6
        lp = log_softmax_rows(rng, 3, T, V)
        tok, lens = pack_rows(random_rows(rng, 3, 5, 10, V, blank=blank), R=5, Ls=T)
        seq = np.asarray([23, 11, 0], np.int32)
    elif name == "blank_mid":
        T, V, blank = 17, 5, 2
        lp = log_softmax_rows(rng, 2, T, V)
        tok, lens = pack_rows(random_rows(rng, 2, 6, 8, V, blank=blank), R=6, Ls=12)  # (L_stride below T)
    elif name == "forty_rows":
        # more hypotheses than scratch slots: 40 rows = 10 groups of four, rows of both kinds (a wave | the workgroup)
        T, V = 45, 6
        lp = log_softmax_rows(rng, 4, T, V)
        tok, lens = pack_rows(random_rows(rng, 4, 10, 40, V, repeat=0.1), R=10, Ls=T)
        seq = np.asarray([45, 44, 30, 45], np.int32)
    elif name == "mixed_group":
        # six rows, R = 3: the first group of four straddles the items and is long (S = 259: four states per lane; S = 7; S = 201: one
        # state per lane; 64 labels in item 1's 40 frames: no path inside a long group), the last group is partial and long (S = 79; S = 1)
        T, V = 130, 4
        rows = [[cycle(129, V, first=1), [1, 2, 3], cycle(100, V)], [cycle(64, V), cycle(39, V), []]]
        tok, lens = pack_rows(rows, R=3, Ls=T)
        lp = log_softmax_rows(rng, 2, T, V, scale=1.0)
        seq = np.asarray([130, 40], np.int32)
    else:
        raise KeyError(name)
    return dict(lp=np.ascontiguousarray(lp, np.float32), seq_lens=seq, tokens=tok, lens=lens, blank=blank)


CASES = ["edges", "one_frame", "wave_edge", "workgroup_edge", "many_per_lane", "ties_half", "ties_constant", "neg_inf", "blank_last", "blank_mid", "forty_rows",
         "mixed_group"]


def hash_name(name):
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


_CACHE = {}


def cached(key, make):
    """A reference computed once, shared among the tests that need it, and left unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case(name):
    """The case and its reference (computed once per process)."""
    def make():
        c = make_case(name)
        return c, reference(c["lp"], c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    return cached(("case", name), make)


def to_bf16_bits(x):
    """float32 -> the bfloat16 below it in magnitude (truncation: the tests need values that bf16 holds, not a rounding rule)."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_bits_to_f32(u):
    return (u.astype(np.uint32) << 16).view(np.float32)


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_align_host():
    import subprocess

    src = os.path.join(NATIVE, "align_host.cpp")
    csrc = os.path.join(ROOT, "ctcdecode_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("align.h", "blank_skip.h", "exact_math_f64.h", "exact_math_f64_tables.h", "exact_math.h")]
    if os.path.exists(ALIGN_HOST_SO) and all(os.path.getmtime(ALIGN_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return ALIGN_HOST_SO
    os.makedirs(os.path.dirname(ALIGN_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (ALIGN_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, ALIGN_HOST_SO)
    return ALIGN_HOST_SO


def _lib():
    lib = ctypes.CDLL(build_align_host())
    lib.ctcalign_host_align.argtypes = [ctypes.c_void_p, ctypes.c_int, _i32p] + [ctypes.c_int] * 5 + [_i32p, _i32p, ctypes.c_int, ctypes.c_int, _i32p, _i32p, _f32p, _i32p]
    lib.ctcalign_host_slot_bytes.restype = ctypes.c_longlong
    lib.ctcalign_host_grid.restype = ctypes.c_longlong
    lib.ctcalign_host_grid.argtypes = [ctypes.c_longlong, ctypes.c_longlong, ctypes.c_int, ctypes.c_int]
    lib.ctcalign_host_default_scratch.restype = ctypes.c_longlong
    return lib


def host_align(rows, seq_lens, tokens, lens, blank, log_input=1, dtype=0, fill=0x5A5A5A5A):
    """The twin over output buffers of ``fill`` words.  ``rows``: [B, T, V] float32 (dtype 0) or uint16 bit patterns (1: f16, 2: bf16)."""
    rows = np.ascontiguousarray(rows)
    B, T, V = rows.shape
    tokens, lens = np.ascontiguousarray(tokens, np.int32), np.ascontiguousarray(lens, np.int32)
    R, Ls = tokens.shape[1], tokens.shape[2]
    st = np.full((B, R, Ls), fill, np.int32)
    en = np.full((B, R, Ls), fill, np.int32)
    sc = np.full((B, R), np.float32(-123.0), np.float32)
    status = np.zeros((B,), np.int32)
    sl = None if seq_lens is None else np.ascontiguousarray(seq_lens, np.int32)
    rc = _lib().ctcalign_host_align(rows.ctypes.data, dtype, None if sl is None else sl.ctypes.data_as(_i32p), B, T, V, blank, log_input,
                                    tokens.ctypes.data_as(_i32p), lens.ctypes.data_as(_i32p), R, Ls, st.ctypes.data_as(_i32p), en.ctypes.data_as(_i32p),
                                    sc.ctypes.data_as(_f32p), status.ctypes.data_as(_i32p))
    assert rc >= 0, "the twin refused its arguments"
    return dict(start=st, end=en, scores=sc, status=status, invalid_rows=rc)


def host_slot_bytes(T, Ls):
    return int(_lib().ctcalign_host_slot_bytes(int(T), int(Ls)))


def host_grid(rows, budget, T, Ls):
    return int(_lib().ctcalign_host_grid(int(rows), int(budget), int(T), int(Ls)))


def host_npl(S):
    return int(_lib().ctcalign_host_npl(int(S)))


def host_row_words(S):
    return int(_lib().ctcalign_host_row_words(int(S)))


def host_max_labels():
    return int(_lib().ctcalign_host_max_labels())


def host_default_scratch():
    return int(_lib().ctcalign_host_default_scratch())
