"""Helpers of the edit-distance tests (TEST INFRASTRUCTURE ONLY): the definition of include/ctcdecode_amd.h "Edit distance" restated in
numpy -- a two-row dynamic programme over plain sequences, written from the header's text and not from editdist.h (no lanes, no strips,
no classes) -- the cases the CPU and the GPU tests share, and the ctypes front-end of the host twin (tests/native/editdist_host.cpp)."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NATIVE = os.path.join(ROOT, "tests", "native")
EDIT_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcedit_host.so")
SENTINEL = 0x5A5A5A5A
GARBAGE = -0x12345678  # what stands at and beyond a row's length: a token no case uses
BAD_ROW = 8            # CTCD_ALIGN_BAD_ROW
MAX_STRIP = 2048
CLASSES = (1, 2, 4, 8, 16, 32)  # what the header promises: columns per lane; the twin reports what the build compiles
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

_i32p = ctypes.POINTER(ctypes.c_int32)


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def lev(a, b):
    """Unit-cost Levenshtein distance of two int32 sequences.  Two rows: ``prev`` is the row of the distances between a[:i-1] and every
    prefix of b, ``cur`` the row for a[:i].  cur[j] = min(prev[j] + 1, cur[j-1] + 1, prev[j-1] + (a[i-1] != b[j-1])).  The dependence
    on cur[j-1] is resolved exactly by a running minimum: cur[j] = min over k <= j of (t[k] + j - k), t the minimum of the other two
    terms (t[0] = i)."""
    a = np.asarray(a, np.int32).ravel()
    b = np.asarray(b, np.int32).ravel()
    if len(a) > len(b):
        a, b = b, a  # (symmetric; the loop runs over the shorter one)
    if len(a) == 0:
        return int(len(b))
    idx = np.arange(len(b) + 1, dtype=np.int64)
    prev = idx.copy()
    for i in range(1, len(a) + 1):
        t = np.empty(len(b) + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != a[i - 1]))
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev[-1])


def lev_plain(a, b):
    """The same definition cell by cell, in Python integers (small cases: it checks the vectorised form above)."""
    a, b = [int(v) for v in a], [int(v) for v in b]
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[-1]


def reference(x, x_lens, y=None, y_lens=None):
    """The whole contract.  x int32 [B, R, L], x_lens [B, R]; y [B, Q, Lq], y_lens [B, Q], or None: pairwise.  -> (out int32 [B, R, Q],
    status int32 [B]).  An item with a length outside its bounds has status 8 and zero outputs."""
    x = np.asarray(x, np.int32)
    x_lens = np.asarray(x_lens, np.int64)
    B, R, L = x.shape
    pairwise = y is None
    if pairwise:
        y, y_lens = x, x_lens
    y = np.asarray(y, np.int32)
    y_lens = np.asarray(y_lens, np.int64)
    Q, Lq = y.shape[1], y.shape[2]
    out = np.zeros((B, R, Q), np.int32)
    status = np.zeros((B,), np.int32)
    for b in range(B):
        if (x_lens[b] < 0).any() or (x_lens[b] > L).any() or (y_lens[b] < 0).any() or (y_lens[b] > Lq).any():
            status[b] = BAD_ROW
            continue
        for i in range(R):
            for j in range(Q):
                if pairwise and j <= i:
                    out[b, i, j] = out[b, j, i]  # (lev is symmetric and lev(a, a) = 0: the triangle once)
                    continue
                out[b, i, j] = lev(x[b, i, :x_lens[b, i]], y[b, j, :y_lens[b, j]])
    return out, status


_CACHE = {}


def cached(key, make):
    """A reference computed once, shared among the tests that need it, and left unchanged."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def hash_name(name):
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def klass(n):
    """The class the header assigns a strip of n >= 1 tokens: the least power of two C with 64 C >= n."""
    c = 1
    while 64 * c < n:
        c *= 2
    return c


def strip_lengths(C):
    """The strip lengths of class C's grid: around one lane's columns, around the last lane, the class's last length -- and the first
    length of the next class (which that class runs)."""
    ns = {0, 1, C - 1, C, C + 1, 63 * C, 64 * C - 1, 64 * C}
    if 64 * C + 1 <= MAX_STRIP:
        ns.add(64 * C + 1)
    return sorted(n for n in ns if n >= 0)


def streamed_lengths(n):
    return sorted({n, n + 1, n + 62, n + 63, n + 64, n + 65, 3 * n})


def pack_rows(rows, width=None):
    """Rows of different lengths -> (int32 [len(rows), width] with GARBAGE at and beyond each length, lens int32)."""
    width = max([len(r) for r in rows] + [0]) if width is None else width
    t = np.full((len(rows), width), GARBAGE, np.int32)
    for k, r in enumerate(rows):
        t[k, :len(r)] = r
    return t, np.asarray([len(r) for r in rows], np.int32)


def related_rows(rng, n, m, alphabet):
    """A strip of n and a streamed row of m tokens that share material: the longer one is the shorter one with tokens inserted, then a
    tenth of its positions redrawn -- distances well below max(n, m), and every kind of edit on the best path."""
    a = rng.integers(0, alphabet, n).astype(np.int32)
    pos = np.sort(rng.choice(m, n, replace=False)) if n else np.zeros(0, np.int64)
    b = rng.integers(0, alphabet, m).astype(np.int32)
    b[pos] = a
    flip = rng.random(m) < 0.1
    b[flip] = rng.integers(0, alphabet, int(flip.sum()))
    return a, b


def grid_case(C, swap):
    """One launch for class C: every (n, m) of the grid as an item of its own (R = Q = 1).  swap = False: x holds the strips, y the
    streamed rows; True: the other way round.  -> dict(x, x_lens, y, y_lens) with [B, 1, L] tensors, and the list of (n, m)."""
    rng = np.random.default_rng(hash_name("grid %d" % C))
    pairs = [(n, m) for n in strip_lengths(C) for m in streamed_lengths(n)]
    rows = [related_rows(rng, n, m, 4) for n, m in pairs]
    s, s_lens = pack_rows([r[0] for r in rows])
    t, t_lens = pack_rows([r[1] for r in rows])
    s, t = s[:, None, :], t[:, None, :]
    s_lens, t_lens = s_lens[:, None], t_lens[:, None]
    c = dict(x=t, x_lens=t_lens, y=s, y_lens=s_lens) if swap else dict(x=s, x_lens=s_lens, y=t, y_lens=t_lens)
    c["pairs"] = pairs
    return c


def closed_form_cases(C):
    """(name, a, b, distance) whose distance needs no second implementation, on strips of class C."""
    rng = np.random.default_rng(hash_name("closed %d" % C))
    n = 64 * C - (1 if C > 1 else 0)
    m = n + 70
    a = rng.integers(0, 4, n).astype(np.int32)
    long = rng.integers(0, 4, m).astype(np.int32)
    out = [("equal", a, a.copy(), 0),
           ("disjoint", a, (long + 10).astype(np.int32), m),
           ("prefix", long[:n].copy(), long, m - n),
           ("suffix", long[m - n:].copy(), long, m - n)]
    cols = sorted({c for l in range(1, 64) for c in (l * C, l * C + 1) if 1 <= c <= n} | {n})  # 1-based: both sides of all 63 lane boundaries
    for c in cols:
        b = a.copy()
        b[c - 1] = 7
        out.append(("substitution at column %d" % c, a, b, 1))
    d = np.arange(n, dtype=np.int32)  # distinct tokens: one deletion and one insertion, nothing cheaper
    if n >= 2:
        out.append(("rotation", d, np.roll(d, -1), 2))
    return out


def token_value_case():
    """Rows over {INT32_MIN, -1, 0, 2^31 - 1}: equality of values, not of differences that overflow."""
    rng = np.random.default_rng(hash_name("token values"))
    vals = np.asarray([I32_MIN, -1, 0, I32_MAX], np.int64)
    rows_x = [vals[rng.integers(0, 4, n)].astype(np.int32) for n in (1, 2, 7, 64, 65, 130)]
    rows_y = [vals[rng.integers(0, 4, n)].astype(np.int32) for n in (1, 3, 64, 200)]
    rows_x.append(np.asarray([I32_MIN], np.int32))
    rows_y.append(np.asarray([I32_MAX], np.int32))  # (their difference is -1 mod 2^32; their distance is 1)
    rows_x.append(np.asarray([0, -1, I32_MIN], np.int32))
    rows_y.append(np.asarray([0, -1, I32_MIN], np.int32))
    x, xl = pack_rows(rows_x)
    y, yl = pack_rows(rows_y)
    return dict(x=x[None], x_lens=xl[None], y=y[None], y_lens=yl[None])


MIXED_X_LENS = (0, 1, 5, 63, 64, 65, 100, 128, 129, 200, 256, 257, 300, 511, 512, 513, 700, 1000, 1024, 1025, 1500, 2047, 2048, 0)
MIXED_Y_LENS = (0, 40, 400, 2048, 3000)


def mixed_case():
    """B = 3, R = 40, Q = 5: pairs of every class and empty rows in one launch, 600 pairs.  (150 workgroups: at the default grid every
    wave takes one pair; the GPU tests also run it at a grid capped to one and two workgroups.)  The rows of an item derive from one
    base row, as the rows of a beam do."""
    rng = np.random.default_rng(hash_name("mixed"))
    B, R, Q, L, Lq = 3, 40, 5, 2048, 3000
    x = np.full((B, R, L), GARBAGE, np.int32)
    y = np.full((B, Q, Lq), GARBAGE, np.int32)
    xl = np.zeros((B, R), np.int32)
    yl = np.zeros((B, Q), np.int32)
    for b in range(B):
        base = rng.integers(0, 6, Lq).astype(np.int32)
        for i in range(R):
            n = MIXED_X_LENS[(i + 7 * b) % len(MIXED_X_LENS)]
            row = base[:n].copy()
            flip = rng.random(n) < 0.05
            row[flip] = rng.integers(0, 6, int(flip.sum()))
            x[b, i, :n], xl[b, i] = row, n
        for j in range(Q):
            n = MIXED_Y_LENS[(j + b) % Q]
            row = base[Lq - n:].copy() if (j + b) % 2 else base[:n].copy()
            y[b, j, :n], yl[b, j] = row, n
    return dict(x=x, x_lens=xl, y=y, y_lens=yl)


def with_bad_length(c, name, b, bad, side="x"):
    """A copy of the case ``c`` (cached under ``name``) whose item b has one length out of bounds.  -> (case, (out, status) from the case's
    own reference: item b zeroed and its status raised, every other item as it was)."""
    want, status = (a.copy() for a in cached(("ref", name), lambda: case_reference(c)))
    d = dict(c)
    key = "x_lens" if side == "x" else "y_lens"
    d[key] = c[key].copy()
    d[key][b, d[key].shape[1] // 2] = bad
    want[b] = 0
    status[b] = BAD_ROW
    return d, (want, status)


def many_short_case(B=5, R=64, L=24):
    """Pairwise, B x R (R - 1) / 2 = 10080 pairs of short rows: several times the waves of the default grid, so every wave comes round
    the persistent loop again and moves from item to item."""
    rng = np.random.default_rng(hash_name("many short"))
    x = np.full((B, R, L), GARBAGE, np.int32)
    xl = rng.integers(0, L + 1, (B, R)).astype(np.int32)
    for b in range(B):
        base = rng.integers(0, 3, L).astype(np.int32)
        for i in range(R):
            row = base[:xl[b, i]].copy()
            flip = rng.random(len(row)) < 0.3
            row[flip] = rng.integers(0, 3, int(flip.sum()))
            x[b, i, :len(row)] = row
    return dict(x=x, x_lens=xl, y=None, y_lens=None)


def pairwise_case(R, B=2, L=150):
    """Rows of a beam: edits of one base row per item, lengths 0 .. L, an empty row among them (R >= 3)."""
    rng = np.random.default_rng(hash_name("pairwise %d" % R))
    x = np.full((B, R, L), GARBAGE, np.int32)
    xl = np.zeros((B, R), np.int32)
    for b in range(B):
        base = rng.integers(0, 5, L).astype(np.int32)
        for i in range(R):
            n = 0 if (R >= 3 and i == 2) else int(rng.integers(1, L + 1))
            row = base[:n].copy()
            flip = rng.random(n) < 0.1
            row[flip] = rng.integers(0, 5, int(flip.sum()))
            x[b, i, :n], xl[b, i] = row, n
    return dict(x=x, x_lens=xl, y=None, y_lens=None)


def limit_case():
    """L = Lq = 2048: all 0 against all 1 (2048), and one random pair."""
    rng = np.random.default_rng(hash_name("limit"))
    x = np.stack([np.zeros(2048, np.int32), rng.integers(0, 4, 2048).astype(np.int32)])[None]
    y = np.stack([np.ones(2048, np.int32), rng.integers(0, 4, 2048).astype(np.int32)])[None]
    lens = np.full((1, 2), 2048, np.int32)
    return dict(x=x, x_lens=lens, y=y, y_lens=lens.copy())


def gpu_strip_lengths():
    """The strip length of every pair the GPU test file launches in its grid, mixed, pairwise and limit cases (the shorter row of each
    non-empty pair): the CPU suite checks that they reach every class the build compiles."""
    ns = []
    for C in CLASSES:
        ns += [min(n, m) for n, m in grid_case(C, False)["pairs"]]
    c = mixed_case()
    for b in range(c["x"].shape[0]):
        ns += [min(int(a), int(q)) for a in c["x_lens"][b] for q in c["y_lens"][b]]
    for R in (1, 2, 7, 40):
        c = pairwise_case(R)
        for b in range(c["x"].shape[0]):
            ns += [min(int(c["x_lens"][b, i]), int(c["x_lens"][b, j])) for i in range(R) for j in range(i + 1, R)]
    ns.append(2048)
    return [n for n in ns if n > 0]


def case_reference(c):
    return reference(c["x"], c["x_lens"], c["y"], c["y_lens"])


# ---- the host twin -------------------------------------------------------------------------------------------------------------------
def build_edit_host():
    src = os.path.join(NATIVE, "editdist_host.cpp")
    deps = [src, os.path.join(ROOT, "ctcdecode_amd", "csrc", "editdist.h")]
    if os.path.exists(EDIT_HOST_SO) and all(os.path.getmtime(EDIT_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return EDIT_HOST_SO
    os.makedirs(os.path.dirname(EDIT_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (EDIT_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", tmp], check=True)
    os.replace(tmp, EDIT_HOST_SO)
    return EDIT_HOST_SO


def _lib():
    def make():
        lib = ctypes.CDLL(build_edit_host())
        lib.ctcedit_host_distance.argtypes = [_i32p, _i32p] + [ctypes.c_int] * 3 + [_i32p, _i32p] + [ctypes.c_int] * 2 + [_i32p, _i32p, ctypes.POINTER(ctypes.c_longlong)]
        lib.ctcedit_host_pair.argtypes = [_i32p, ctypes.c_int, _i32p, ctypes.c_int]
        lib.ctcedit_host_pair_of.argtypes = [ctypes.c_longlong, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p]
        lib.ctcedit_host_pairs_per_item.argtypes = [ctypes.c_int] * 3
        lib.ctcedit_host_pairs_per_item.restype = ctypes.c_longlong
        lib.ctcedit_host_result_at.argtypes = [ctypes.c_int] * 3 + [_i32p]
        lib.ctcedit_host_cell.argtypes = [ctypes.c_int] * 3 + [ctypes.c_int32] * 2
        lib.ctcedit_host_num_classes.argtypes = [_i32p]
        return lib
    return cached("lib", make)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def host_distance(x, x_lens, y=None, y_lens=None):
    """The twin over an output of sentinel words.  -> (rc, out [B, R, Q], status [B], pairs)."""
    x = np.ascontiguousarray(x, np.int32)
    xl = np.ascontiguousarray(x_lens, np.int32)
    B, R, L = x.shape
    y = None if y is None else np.ascontiguousarray(y, np.int32)
    yl = None if y_lens is None else np.ascontiguousarray(y_lens, np.int32)
    Q, Lq = (R, L) if y is None else (y.shape[1], y.shape[2])
    out = np.full((B, R, Q), SENTINEL, np.int32)
    status = np.zeros((max(B, 1),), np.int32)
    pairs = ctypes.c_longlong(-1)
    rc = _lib().ctcedit_host_distance(_ptr(x), _ptr(xl), B, R, L, _ptr(y), _ptr(yl), Q, Lq, _ptr(out), _ptr(status), ctypes.byref(pairs))
    return rc, out, status[:B], int(pairs.value)


def host_pair(a, b):
    a = np.ascontiguousarray(a, np.int32)
    b = np.ascontiguousarray(b, np.int32)
    return int(_lib().ctcedit_host_pair(_ptr(a), len(a), _ptr(b), len(b)))


def host_class(n):
    return int(_lib().ctcedit_host_class(int(n)))


def host_classes():
    buf = np.zeros(16, np.int32)
    k = _lib().ctcedit_host_num_classes(_ptr(buf))
    return tuple(int(v) for v in buf[:k])


def host_pair_of(w, R, Q, pairwise):
    buf = np.zeros(3, np.int32)
    _lib().ctcedit_host_pair_of(int(w), int(R), int(Q), 1 if pairwise else 0, _ptr(buf))
    return tuple(int(v) for v in buf)


def host_pairs_per_item(R, Q, pairwise):
    return int(_lib().ctcedit_host_pairs_per_item(int(R), int(Q), 1 if pairwise else 0))


def host_result_at(m, n, C):
    buf = np.zeros(3, np.int32)
    _lib().ctcedit_host_result_at(int(m), int(n), int(C), _ptr(buf))
    return tuple(int(v) for v in buf)


def host_cell(up, left, diag, a, b):
    return int(_lib().ctcedit_host_cell(int(up), int(left), int(diag), int(a), int(b)))


# ---- minimum Bayes risk ----------------------------------------------------------------------------------------------------------------
def mbr_reference(D, log_weights):
    """float64: w = softmax(log_weights[b]); risk[b, i] = sum_j w[b, j] D[b, i, j]; rows of -inf weight have risk +inf; index: the
    smallest i of least risk, -1 for an item without a finite weight."""
    D = np.asarray(D, np.float64)
    lw = np.asarray(log_weights, np.float64)
    B, R = lw.shape
    risk = np.full((B, R), np.inf)
    index = np.full((B,), -1, np.int64)
    for b in range(B):
        live = np.isfinite(lw[b])
        if not live.any():
            continue
        e = np.where(live, np.exp(lw[b] - lw[b][live].max()), 0.0)
        w = e / e.sum()
        r = (D[b] * w[None, :]).sum(1)
        risk[b] = np.where(live, r, np.inf)
        index[b] = int(np.argmin(risk[b]))
    return index, risk
