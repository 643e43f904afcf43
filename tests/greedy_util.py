"""Helpers of the greedy-decode tests (TEST INFRASTRUCTURE ONLY): the definition of include/ctcdecode_amd.h "Greedy decode" restated in
numpy float32 / Python -- a plain loop over an item's frames, written from the header's text and not from greedy.h; expf / logf are the
box's own glibc through ctypes, as in tests/loglik_util.py -- the cases the CPU and the GPU tests share, and the ctypes front-end of
the host twin (tests/native/greedy_host.cpp)."""
import ctypes
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
GREEDY_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcgreedy_host.so")
F32 = np.float32
FLT_MIN = float(np.finfo(np.float32).tiny)
NEG_INF = np.float32(-np.inf)
SENTINEL = 0x5A5A5A5A
MODES = (0, 1, 2)   # include/ctcdecode_amd.h log_input: probabilities, log-probabilities, raw logits
DTYPES = (0, 1, 2)  # CTCD_DTYPE_F32 / F16 / BF16

_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)
_libm = ctypes.CDLL("libm.so.6")
_libm.expf.argtypes = [ctypes.c_float]
_libm.expf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
_libm.logf.restype = ctypes.c_float


# ---- the definition ----------------------------------------------------------------------------------------------------------------
def frame_label(row):
    """The index of the greatest value: an ordered, strict `>` walked from c = 0 (numpy.argmax: the first of the greatest; -0.0 == +0.0)."""
    return int(np.argmax(row))


_XOR = [np.arange(64) ^ (1 << k) for k in range(6)]


def log_softmax_at(row, c):
    """The value ctcd_log_softmax writes for label c of the frame ``row`` (float32 [V]): (x - m) - logf(s), m the maximum (a zero one
    taken as +0), s the float32 sum of expf(x_j - m) over 64 chains j mod 64 in increasing j, then the butterfly l ^ 1, ^ 2, .. ^ 32;
    expf below -88 is 0; -inf for m = -inf."""
    m = F32(np.max(row)) + F32(0.0)
    if not m > NEG_INF:
        return NEG_INF
    d = (row - m).astype(np.float32)
    terms = np.zeros(((len(row) + 63) // 64) * 64, np.float32)
    terms[:len(row)] = [0.0 if v < -88.0 else _libm.expf(float(v)) for v in d]
    p = np.zeros(64, np.float32)
    for chunk in terms.reshape(-1, 64):  # chain l: its terms in increasing j
        p = p + chunk
    for x in _XOR:
        p = p + p[x]
    return F32(F32(row[c] - m) - F32(_libm.logf(float(p[0]))))


def winner_lp(row, c, mode):
    if mode == 1:
        return F32(row[c])
    if mode == 0:
        return F32(math.log(float(row[c]) + FLT_MIN))
    return log_softmax_at(row, c)


def greedy_item(x, n, blank, mode):
    """One item.  ``x``: float32 [T, V], ``n`` frames of it count.  -> (tokens, starts, ends, label_scores, score, labels c*(t), lps)."""
    labs = [frame_label(x[t]) for t in range(n)]
    lps = [winner_lp(x[t], labs[t], mode) for t in range(n)]
    tokens, starts, ends, lsc = [], [], [], []
    for t in range(n):
        c = labs[t]
        if c == blank:
            continue
        if t == 0 or c != labs[t - 1]:
            tokens.append(c)
            starts.append(t)
            ends.append(t)
            lsc.append(lps[t])
        else:  # frame t goes on with the run: the greatest lp, the earlier frame's among equals
            ends[-1] = t
            if lps[t] > lsc[-1]:
                lsc[-1] = lps[t]
    score = F32(0.0)
    for t in range(n):
        score = lps[t] if t == 0 else F32(score + lps[t])  # one float32 addition per frame, in frame order
    return tokens, starts, ends, lsc, score, labs, lps


def reference(x, seq_lens, blank, mode):
    """The whole contract on a batch: ``x`` float32 [B, T, V] (half rows: their float copies).  -> dict(tokens, starts, ends int32
    [B, T], label_scores float32 [B, T], scores float32 [B], lens int32 [B], labels: per item the list c*(t))."""
    x = np.ascontiguousarray(x, np.float32)
    B, T, V = x.shape
    out = dict(tokens=np.zeros((B, T), np.int32), starts=np.zeros((B, T), np.int32), ends=np.zeros((B, T), np.int32),
               label_scores=np.zeros((B, T), np.float32), scores=np.zeros((B,), np.float32), lens=np.zeros((B,), np.int32), labels=[], lps=[])
    for b in range(B):
        n = T if seq_lens is None else min(max(int(seq_lens[b]), 0), T)
        tok, st, en, ls, sc, labs, lps = greedy_item(x[b], n, blank, mode)
        L = len(tok)
        out["tokens"][b, :L], out["starts"][b, :L], out["ends"][b, :L], out["label_scores"][b, :L] = tok, st, en, ls
        out["scores"][b], out["lens"][b] = sc, L
        out["labels"].append(labs)
        out["lps"].append(lps)
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits1(v):
    return int(np.float32(v).view(np.uint32))


def assert_same(got, want, what=""):
    """Bit for bit: floats as uint32, integers exactly.  ``got``: dict with tokens / starts / scores / lens (/ ends / label_scores)."""
    for k in ("lens", "tokens", "starts", "ends"):
        if k in got and got[k] is not None:
            g = np.asarray(got[k]).reshape(want[k].shape)
            bad = np.argwhere(g != want[k])
            assert bad.size == 0, "%s: %s differs at %s: got %s, want %s" % (what, k, bad[:4].tolist(), g[tuple(bad[0])], want[k][tuple(bad[0])])
    for k in ("scores", "label_scores"):
        if k in got and got[k] is not None:
            g = np.asarray(got[k]).reshape(want[k].shape)
            bad = np.argwhere(bits(g) != bits(want[k]))
            assert bad.size == 0, "%s: %s differs at %s: got %r, want %r" % (what, k, bad[:4].tolist(), g[tuple(bad[0])], want[k][tuple(bad[0])])


# ---- element types -------------------------------------------------------------------------------------------------------------------
def to_bf16_bits(x):
    """float32 -> the bfloat16 nearest to it (ties to even; infinities stay)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(u):
    return (u.astype(np.uint32) << 16).view(np.float32)


def as_dtype(x, dtype):
    """-> (what the twin reads: float32 or uint16 bit patterns, the float32 copy of it)."""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == 0:
        return x, x
    if dtype == 1:
        with np.errstate(over="ignore"):
            h = x.astype(np.float16)
        return h.view(np.uint16), h.astype(np.float32)
    u = to_bf16_bits(x)
    return u, bf16_bits_to_f32(u)


def to_torch(torch, stored, dtype, device="cuda"):
    """The stored rows of as_dtype as a tensor of the element type on the device."""
    if dtype == 0:
        return torch.from_numpy(stored).to(device)
    t = torch.from_numpy(stored.view(np.int16)).to(device)
    return t.view(torch.float16 if dtype == 1 else torch.bfloat16)


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
def hash_name(name):
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def random_rows(rng, B, T, V, mode, scale=2.0):
    """Rows of the kind the mode expects: probabilities, log-probabilities or logits."""
    z = rng.standard_normal((B, T, V)) * scale
    if mode == 2:
        return z.astype(np.float32)
    z = z - z.max(-1, keepdims=True)
    lp = z - np.log(np.exp(z).sum(-1, keepdims=True))
    return (np.exp(lp) if mode == 0 else lp).astype(np.float32)


def path_rows(rng, paths, V, mode):
    """Rows whose frame labels are ``paths`` (per item a list of labels): the winner clearly above the rest, its value random."""
    B, T = len(paths), max(len(p) for p in paths)
    if mode == 0:
        x = (rng.random((B, T, V)) * 0.01).astype(np.float32)
        win = lambda: 0.5 + 0.4 * rng.random()  # noqa: E731
    else:
        x = (-6.0 - rng.random((B, T, V))).astype(np.float32)
        win = lambda: -0.05 - rng.random()  # noqa: E731
    for b, p in enumerate(paths):
        for t, c in enumerate(p):
            x[b, t, c] = win()
    return x


V_LIST = (1, 2, 29, 63, 64, 65, 255, 256, 257, 260, 264, 1023, 1024, 1025, 1028, 2056, 4098, 4104, 10000, 10248)
T_LIST = (1, 63, 64, 65, 1023, 1024, 1025, 2049)


def shape_case(V, mode, dtype, T=None, B=2):
    """Random rows of V labels in the given mode and element type.  -> dict(stored, x, seq_lens, blank, mode, dtype)."""
    rng = np.random.default_rng(hash_name("shape %d %d %d %s" % (V, mode, dtype, T)))
    T = T if T is not None else (8 if V >= 10000 else (5 if V > 1000 else 9))
    stored, x = as_dtype(random_rows(rng, B, T, V, mode, scale=1.0 if V > 64 else 2.0), dtype)
    blank = (0, V // 2, V - 1)[(V + mode) % 3]
    return dict(stored=stored, x=x, seq_lens=None, blank=blank, mode=mode, dtype=dtype)


def _case(raw, mode, dtype, blank, seq_lens=None):
    stored, x = as_dtype(raw, dtype)
    return dict(stored=stored, x=x, seq_lens=None if seq_lens is None else np.asarray(seq_lens, np.int32), blank=blank, mode=mode, dtype=dtype)


TIE_PATTERNS = {29: [(3, 17), (0, 28), (5, 6, 7), (28, 1)], 65: [(1, 64), (0, 64), (63, 64), (10, 20, 30)], 301: [(3, 67), (0, 300), (70, 200, 299), (130, 65)],
                4096: [(5, 6), (7, 8), (3, 259), (70, 300, 900), (0, 4095), (1030, 5), (2051, 2040, 9), (4095, 4094), (2048 + 16, 17)],
                10000: [(9999, 4, 5000), (2563, 2564), (1024, 9)]}


def tie_case(V, mode, dtype):
    """One frame per pattern of TIE_PATTERNS[V]: two or three equal maxima in different lanes, waves and vector words -- the smallest
    index must win; then -0.0 against +0.0 both ways round, and a frame without a finite value (-inf; probabilities: zeros).  The blank
    is the last label, so that label 0 is emitted."""
    rng = np.random.default_rng(hash_name("ties %d %d %d" % (V, mode, dtype)))
    pats = TIE_PATTERNS[V]
    T = len(pats) + 3
    top = 0.5 if mode == 0 else 0.0
    raw = (rng.random((1, T, V)) * 0.01 if mode == 0 else -2.0 - rng.random((1, T, V))).astype(np.float32)
    for t, pat in enumerate(pats):
        raw[0, t, list(pat)] = top
    a, b = V // 3, V - 2
    t = len(pats)
    if mode == 0:  # a frame of zeros of both signs: label 0
        raw[0, t] = 0.0
        raw[0, t, 0] = -0.0
        raw[0, t + 1] = -0.0
        raw[0, t + 1, b] = 0.0
        raw[0, t + 2] = 0.0
    else:
        raw[0, t, a], raw[0, t, b] = -0.0, 0.0
        raw[0, t + 1, a], raw[0, t + 1, b] = 0.0, -0.0
        raw[0, t + 2] = -np.inf
    return _case(raw, mode, dtype, V - 1)


def coarse_case(V, mode, dtype, B=2, T=6):
    """Rows of rounded random values (every element type holds them exactly): most frames have several equal maxima."""
    rng = np.random.default_rng(hash_name("coarse %d %d %d" % (V, mode, dtype)))
    z = rng.standard_normal((B, T, V))
    raw = np.minimum(np.round(np.abs(z) * 2), 4) / 8 if mode == 0 else -np.round(np.abs(z) * 3)
    return _case(raw.astype(np.float32), mode, dtype, min(1, V - 1))


def tied_frames(c):
    """How many frames of the case have more than one greatest value."""
    x = c["x"]
    return int(((x == x.max(-1, keepdims=True)).sum(-1) > 1).sum()), x.shape[0] * x.shape[1]


def emission_case(blank, mode, dtype):
    """V = 6, T = 12: all frames blank (L = 0); no blank and no repeat (L = T, no tail to zero); "a a _ a" (two labels) inside a longer
    row; "a a a ..." (one label)."""
    rng = np.random.default_rng(hash_name("emission %d %d %d" % (blank, mode, dtype)))
    V, T = 6, 12
    nb = [c for c in range(V) if c != blank]
    a, c = nb[1], nb[3]
    paths = [[blank] * T, [nb[t % len(nb)] for t in range(T)], [a, a, blank, a, blank, blank, c, c, c, a, a, blank], [a] * T]
    return _case(path_rows(rng, paths, V, mode), mode, dtype, blank), paths


def long_run_case(mode):
    """T = 1200, V = 4, blank 0: runs that end at frame 63 and start at 64, that end at 1023 and start at 1024, a run over frames
    1000 .. 1100 and one over 5 .. 1195, between frames of random labels.  Log-probabilities: -0.0 and +0.0 in one run, on both sides of
    frame 1024, both ways round."""
    rng = np.random.default_rng(hash_name("long runs %d" % mode))
    V, T = 4, 1200
    paths = [list(rng.integers(0, V, T)) for _ in range(3)]
    paths[0][56:60], paths[0][60:64], paths[0][64:71], paths[0][71] = [0] * 4, [1] * 4, [2] * 7, 0
    paths[0][999], paths[0][1000:1101], paths[0][1101] = 0, [3] * 101, 1
    paths[1][1009], paths[1][1010:1024], paths[1][1024:1041], paths[1][1041] = 0, [1] * 14, [2] * 17, 0
    paths[2][4], paths[2][5:1196], paths[2][1196] = 0, [3] * 1191, 0
    raw = path_rows(rng, [[int(v) for v in p] for p in paths], V, mode)
    if mode == 1:
        raw[0, 1010, 3], raw[0, 1050, 3] = 0.0, -0.0
        raw[2, 500, 3], raw[2, 1100, 3] = -0.0, 0.0
    return _case(raw, mode, 0, 0, seq_lens=[1200, 1200, 1199])


def score_case(kind, V, dtype):
    """neg_inf (log-probabilities, logits): a frame of -inf mid-row, after which the score stays -inf.  dominant (logits): one logit far
    above the rest (lp = +0.0 or -0.0), and differences around -88, where expf becomes 0.  prob_exact (probabilities): exact 0 and 1."""
    rng = np.random.default_rng(hash_name("score %s %d %d" % (kind, V, dtype)))
    w = V // 2
    if kind.startswith("neg_inf"):
        mode = 1 if kind.endswith("log") else 2
        raw = random_rows(rng, 2, 10, V, mode)
        raw[0, 4] = -np.inf
        raw[1, 0] = -np.inf
        raw[1, 6, : V // 2] = -np.inf  # (half of a frame: its winner is finite)
    elif kind == "dominant":
        mode = 2
        raw = np.full((1, 8, V), -200.0, np.float32)
        raw[0, 0, w] = 50.0
        raw[0, 1], raw[0, 1, w] = -100.0, -0.0
        raw[0, 2], raw[0, 2, w] = -100.0, 0.0
        for t, d in ((3, -87.9), (4, -88.1), (5, -89.0), (6, -87.0)):
            raw[0, t], raw[0, t, w] = 3.0 + d, 3.0
        raw[0, 7] = rng.standard_normal(V) * 30  # (a few terms count, most are below -88)
    else:
        mode = 0
        raw = np.zeros((1, 5, V), np.float32)
        raw[0, 0, w] = 1.0
        raw[0, 2] = 1.0
        raw[0, 3, V - 1], raw[0, 3, 0] = 1.0, 0.5
        raw[0, 4] = random_rows(rng, 1, 1, V, 0)[0, 0]
    return _case(raw, mode, dtype, 0)


_CACHE = {}


def cached(key, make):
    """A reference computed once, shared among the tests that need it, and left unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case_reference(c):
    return reference(c["x"], c["seq_lens"], c["blank"], c["mode"])


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_greedy_host():
    src = os.path.join(NATIVE, "greedy_host.cpp")
    csrc = os.path.join(ROOT, "ctcdecode_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("greedy.h", "align.h", "blank_skip.h", "exact_math_f64.h", "exact_math_f64_tables.h", "exact_math.h")]
    if os.path.exists(GREEDY_HOST_SO) and all(os.path.getmtime(GREEDY_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return GREEDY_HOST_SO
    os.makedirs(os.path.dirname(GREEDY_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (GREEDY_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, GREEDY_HOST_SO)
    return GREEDY_HOST_SO


def _lib():
    def make():
        lib = ctypes.CDLL(build_greedy_host())
        lib.ctcgreedy_host_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, _i32p] + [ctypes.c_int] * 5 + [_i32p, _i32p, _i32p, _f32p, _f32p, _i32p]
        lib.ctcgreedy_host_combine.argtypes = [ctypes.c_float, ctypes.c_int, ctypes.c_float, ctypes.c_int]
        lib.ctcgreedy_host_vec_rows.argtypes = [ctypes.c_ulonglong, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        lib.ctcgreedy_host_scratch_bytes.argtypes = [ctypes.c_longlong, ctypes.c_longlong]
        lib.ctcgreedy_host_scratch_bytes.restype = ctypes.c_longlong
        return lib
    return cached("lib", make)


def host_decode(stored, dtype, seq_lens, blank, mode, details=True):
    """The twin over output buffers of sentinel words.  ``stored``: [B, T, V] float32 (dtype 0) or uint16 bit patterns (1: f16, 2: bf16)."""
    stored = np.ascontiguousarray(stored)
    B, T, V = stored.shape
    tok, st, en = (np.full((B, T), SENTINEL, np.int32) for _ in range(3))
    ls = np.full((B, T), SENTINEL, np.int32).view(np.float32)
    sc = np.full((B,), np.float32(-123.0), np.float32)
    lens = np.full((B,), SENTINEL, np.int32)
    sl = None if seq_lens is None else np.ascontiguousarray(seq_lens, np.int32)
    rc = _lib().ctcgreedy_host_decode(stored.ctypes.data, dtype, None if sl is None else sl.ctypes.data_as(_i32p), B, T, V, blank, mode, tok.ctypes.data_as(_i32p),
                                      st.ctypes.data_as(_i32p), en.ctypes.data_as(_i32p) if details else None, ls.ctypes.data_as(_f32p) if details else None,
                                      sc.ctypes.data_as(_f32p), lens.ctypes.data_as(_i32p))
    assert rc == 0, "the twin refused its arguments"
    return dict(tokens=tok, starts=st, ends=en if details else None, label_scores=ls if details else None, scores=sc, lens=lens)


def host_combine(va, ca, vb, cb):
    return int(_lib().ctcgreedy_host_combine(float(va), int(ca), float(vb), int(cb)))


def host_lanes_per_frame(V):
    return int(_lib().ctcgreedy_host_lanes_per_frame(int(V)))


def host_vec_rows(base, V, dtype, mode):
    return bool(_lib().ctcgreedy_host_vec_rows(int(base), int(V), int(dtype), int(mode)))


def host_logits_f4(V):
    return int(_lib().ctcgreedy_host_logits_f4(int(V)))


def host_scratch_bytes(B, T):
    return int(_lib().ctcgreedy_host_scratch_bytes(int(B), int(T)))
