"""Helpers of the edit-operation tests (TEST INFRASTRUCTURE ONLY): the definition of include/ctcdecode_amd.h "Edit operations" restated
from the header's text and not from editops.h -- no lanes, no strips, no classes, no packed int32: the key (D, S) is a tuple in the
cell-by-cell form and the enumeration, and D * 2^32 + S in int64 in the vectorised form, which keeps the whole key matrix and walks back
over it -- the cases the CPU and the GPU tests share (the rows are those of tests/editdist_util.py), and the ctypes front-end of the
host twin (tests/native/editops_host.cpp)."""
import ctypes
import os
import subprocess

import editdist_util as eu
import numpy as np

OPS_HOST_SO = os.path.join(eu.ROOT, "oracle", "_build", "libctceditops_host.so")
MAX_DIM = 262144
E = 1 << 32  # one edit in the int64 key: (1, 0); a substitution is E + 1: (1, 1)

_i32p = ctypes.POINTER(ctypes.c_int32)


# ---- the definition ------------------------------------------------------------------------------------------------------------------
def key_matrix(x, y):
    """K[i][j] = D * 2^32 + S of x[:i] against y[:j], int64 [lx + 1, ly + 1].  Row i from row i - 1: t[j] is the least of the pair's and
    the x-only candidate, and the y-only step, which adds (1, 0) per position, is resolved exactly by a running minimum, as in
    editdist_util.lev."""
    x = np.asarray(x, np.int32).ravel()
    y = np.asarray(y, np.int32).ravel()
    idx = np.arange(len(y) + 1, dtype=np.int64) * E
    K = np.empty((len(x) + 1, len(y) + 1), np.int64)
    K[0] = idx
    for i in range(1, len(x) + 1):
        prev = K[i - 1]
        t = np.empty(len(y) + 1, np.int64)
        t[0] = i * E
        t[1:] = np.minimum(prev[1:] + E, prev[:-1] + np.where(y != x[i - 1], E + 1, 0))
        K[i] = np.minimum.accumulate(t - idx) + idx
    return K


def key_of(x, y):
    """(D, S) alone, two rows at a time (long rows)."""
    x = np.asarray(x, np.int32).ravel()
    y = np.asarray(y, np.int32).ravel()
    swap = len(x) > len(y)  # (the key is symmetric under exchanging the rows; the loop runs over the shorter one)
    if swap:
        x, y = y, x
    idx = np.arange(len(y) + 1, dtype=np.int64) * E
    prev = idx.copy()
    for i in range(1, len(x) + 1):
        t = np.empty(len(y) + 1, np.int64)
        t[0] = i * E
        t[1:] = np.minimum(prev[1:] + E, prev[:-1] + np.where(y != x[i - 1], E + 1, 0))
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev[-1] >> 32), int(prev[-1] & (E - 1))


def counts_from_key(D, S, lx, ly):
    """(H, S, Del, I) from the optimal key and the lengths."""
    ins, dele = (D - S + lx - ly) // 2, (D - S - lx + ly) // 2
    assert 2 * ins == D - S + lx - ly and 2 * dele == D - S - lx + ly
    return lx - S - ins, S, dele, ins


def walk_back(K, x, y):
    """The canonical alignment over a whole int64 key matrix: the header's three rules from (lx, ly) down to (0, 0).  -> (x_to_y, y_to_x)
    as lists, -1 for a token without a partner."""
    i, j = len(x), len(y)
    x_to_y, y_to_x = [-1] * i, [-1] * j
    while i > 0 or j > 0:
        if i > 0 and j > 0 and K[i - 1][j - 1] + (E + 1 if x[i - 1] != y[j - 1] else 0) == K[i][j]:
            x_to_y[i - 1], y_to_x[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif i > 0 and K[i - 1][j] + E == K[i][j]:
            i -= 1
        else:
            assert j > 0 and K[i][j - 1] + E == K[i][j]
            j -= 1
    return x_to_y, y_to_x


def align_ref(x, y):
    """-> ((D, S), (H, S, Del, I), x_to_y, y_to_x) of two plain sequences."""
    x = np.asarray(x, np.int32).ravel()
    y = np.asarray(y, np.int32).ravel()
    K = key_matrix(x, y)
    D, S = int(K[-1, -1] >> 32), int(K[-1, -1] & (E - 1))
    x_to_y, y_to_x = walk_back(K, x, y)
    return (D, S), counts_from_key(D, S, len(x), len(y)), x_to_y, y_to_x


def align_plain(x, y):
    """The same cell by cell with tuples (small cases: it checks the vectorised form above).  -> as align_ref."""
    x, y = [int(v) for v in x], [int(v) for v in y]
    add = lambda k, d, s: (k[0] + d, k[1] + s)  # noqa: E731
    K = [[(j, 0) for j in range(len(y) + 1)]] + [[(i, 0)] + [None] * len(y) for i in range(1, len(x) + 1)]
    for i in range(1, len(x) + 1):
        for j in range(1, len(y) + 1):
            ne = x[i - 1] != y[j - 1]
            K[i][j] = min(add(K[i - 1][j - 1], int(ne), int(ne)), add(K[i - 1][j], 1, 0), add(K[i][j - 1], 1, 0))
    i, j = len(x), len(y)
    x_to_y, y_to_x = [-1] * i, [-1] * j
    while i > 0 or j > 0:
        ne = i > 0 and j > 0 and x[i - 1] != y[j - 1]
        if i > 0 and j > 0 and add(K[i - 1][j - 1], int(ne), int(ne)) == K[i][j]:
            x_to_y[i - 1], y_to_x[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif i > 0 and add(K[i - 1][j], 1, 0) == K[i][j]:
            i -= 1
        else:
            j -= 1
    D, S = K[len(x)][len(y)]
    return (D, S), counts_from_key(D, S, len(x), len(y)), x_to_y, y_to_x


def enumerate_alignments(x, y):
    """Every alignment of two tiny rows, by recursion over the three kinds of step.  -> the list of ((D, S), x_to_y, y_to_x)."""
    x, y = [int(v) for v in x], [int(v) for v in y]
    out = []

    def go(i, j, D, S, xm, ym):
        if i == len(x) and j == len(y):
            out.append(((D, S), tuple(xm), tuple(ym)))
            return
        if i < len(x) and j < len(y):
            ne = int(x[i] != y[j])
            go(i + 1, j + 1, D + ne, S + ne, xm + [j], ym + [i])
        if i < len(x):
            go(i + 1, j, D + 1, S, xm + [-1], ym)
        if j < len(y):
            go(i, j + 1, D + 1, S, xm, ym + [-1])

    go(0, 0, 0, 0, [], [])
    return out


def canonical_of_enumeration(x, y):
    """The header's definition with no dynamic programme at all: best[i][j], the least key over the enumerated alignments of x[:i] and
    y[:j], then the walk's three rules on those.  -> as align_ref, and the set of S over the alignments of least D."""
    x, y = [int(v) for v in x], [int(v) for v in y]
    best = [[min(k for k, _, _ in enumerate_alignments(x[:i], y[:j])) for j in range(len(y) + 1)] for i in range(len(x) + 1)]
    whole = enumerate_alignments(x, y)
    D = min(k[0] for k, _, _ in whole)
    subs = {k[1] for k, _, _ in whole if k[0] == D}
    i, j = len(x), len(y)
    x_to_y, y_to_x = [-1] * i, [-1] * j
    while i > 0 or j > 0:
        ne = int(i > 0 and j > 0 and x[i - 1] != y[j - 1])
        if i > 0 and j > 0 and (best[i - 1][j - 1][0] + ne, best[i - 1][j - 1][1] + ne) == best[i][j]:
            x_to_y[i - 1], y_to_x[j - 1] = j - 1, i - 1
            i, j = i - 1, j - 1
        elif i > 0 and (best[i - 1][j][0] + 1, best[i - 1][j][1]) == best[i][j]:
            i -= 1
        else:
            j -= 1
    key = best[len(x)][len(y)]
    return key, counts_from_key(key[0], key[1], len(x), len(y)), x_to_y, y_to_x, subs


def reference(x, x_lens, y=None, y_lens=None, maps=False):
    """The whole contract.  x int32 [B, R, L], x_lens [B, R]; y [B, Q, Lq], y_lens [B, Q], or None: pairwise (counts only).
    -> (counts int32 [B, R, Q, 4], status int32 [B]) and, with maps, (x_to_y [B, R, Q, L], y_to_x [B, R, Q, Lq]) in front of status.
    An item with a length outside its bounds has status 8, zero counts and maps of -1."""
    x = np.asarray(x, np.int32)
    x_lens = np.asarray(x_lens, np.int64)
    B, R, L = x.shape
    pairwise = y is None
    assert not (pairwise and maps)
    if pairwise:
        y, y_lens = x, x_lens
    y = np.asarray(y, np.int32)
    y_lens = np.asarray(y_lens, np.int64)
    Q, Lq = y.shape[1], y.shape[2]
    counts = np.zeros((B, R, Q, 4), np.int32)
    x_to_y = np.full((B, R, Q, L), -1, np.int32) if maps else None
    y_to_x = np.full((B, R, Q, Lq), -1, np.int32) if maps else None
    status = np.zeros((B,), np.int32)
    for b in range(B):
        if (x_lens[b] < 0).any() or (x_lens[b] > L).any() or (y_lens[b] < 0).any() or (y_lens[b] > Lq).any():
            status[b] = eu.BAD_ROW
            continue
        for i in range(R):
            for j in range(Q):
                lx, ly = int(x_lens[b, i]), int(y_lens[b, j])
                if pairwise and j < i:
                    H, S, dele, ins = counts[b, j, i]
                    counts[b, i, j] = (H, S, ins, dele)  # (computed once per pair: the exchange is the header's statement)
                    continue
                if pairwise and j == i:
                    counts[b, i, j] = (lx, 0, 0, 0)
                    continue
                if maps:
                    _, c, xm, ym = align_ref(x[b, i, :lx], y[b, j, :ly])
                    x_to_y[b, i, j, :lx], y_to_x[b, i, j, :ly] = xm, ym
                else:
                    c = counts_from_key(*key_of(x[b, i, :lx], y[b, j, :ly]), lx, ly)
                counts[b, i, j] = c
    return (counts, x_to_y, y_to_x, status) if maps else (counts, status)


def case_reference(c, maps=False):
    return reference(c["x"], c["x_lens"], c["y"], c["y_lens"], maps)


def counts_from_maps(x_to_y, y_to_x, x, y, lx, ly):
    """(H, S, Del, I) recomputed from a pair's two maps and its rows."""
    paired = [p for p in range(lx) if x_to_y[p] >= 0]
    H = sum(1 for p in paired if x[p] == y[x_to_y[p]])
    return H, len(paired) - H, ly - sum(1 for q in range(ly) if y_to_x[q] >= 0), lx - len(paired)


def check_maps(x_to_y, y_to_x, lx, ly):
    """The properties every pair of maps has: inverse on paired positions, strictly increasing partners, -1 at and beyond the lengths."""
    xm, ym = np.asarray(x_to_y), np.asarray(y_to_x)
    assert (xm[lx:] == -1).all() and (ym[ly:] == -1).all()
    px = np.nonzero(xm[:lx] >= 0)[0]
    py = np.nonzero(ym[:ly] >= 0)[0]
    assert (xm[px] < ly).all() and (ym[py] < lx).all()
    assert (ym[xm[px]] == px).all() and (xm[ym[py]] == py).all() and len(px) == len(py)
    assert (np.diff(xm[px]) > 0).all() and (np.diff(ym[py]) > 0).all()


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def map_strip_lengths(C):
    return sorted({1, C, C + 1, 63 * C + 1, 64 * C - 1, 64 * C})


def map_streamed_lengths(n):
    return [n, n + 1, n + 63, n + 64, n + 65]


def map_grid_case(C, swap):
    """One launch for class C's map grid: every (n, m) as an item of its own (R = Q = 1).  swap = False: x holds the strips (x-only steps
    run along the strip); True: y does.  Rows over two symbols share material, so that ties between the three steps are everywhere."""
    rng = np.random.default_rng(eu.hash_name("map grid %d" % C))
    pairs = [(n, m) for n in map_strip_lengths(C) for m in map_streamed_lengths(n)]
    rows = [eu.related_rows(rng, n, m, 2 if k % 2 else 4) for k, (n, m) in enumerate(pairs)]
    s, s_lens = eu.pack_rows([r[0] for r in rows])
    t, t_lens = eu.pack_rows([r[1] for r in rows])
    s, t = s[:, None, :], t[:, None, :]
    s_lens, t_lens = s_lens[:, None], t_lens[:, None]
    c = dict(x=t, x_lens=t_lens, y=s, y_lens=s_lens) if swap else dict(x=s, x_lens=s_lens, y=t, y_lens=t_lens)
    c["pairs"] = pairs
    return c


def tie_cases(C):
    """(name, x, y, counts (H, S, Del, I), x_to_y, y_to_x) whose answers follow from the header's text alone, on rows long enough to be
    strips of class C.  [a, b] against [b, a] has two alignments of distance 2 without a substitution -- keep a or keep b -- and one with
    two substitutions: the walk, coming from the end, takes the pair x[0] = a with y[1] = a (rule 2 before rule 3 at (2, 2)).  The tie
    sits in front of a common run P of k >= 1 distinct tokens, which pair off as hits and keep anything behind them from standing
    against anything in front of them; a tail of distinct tokens behind P on one side makes that side the longer row, the streamed
    one: its tokens have no partner, and the other side has none left to substitute them with."""
    n = 64 * C - 2 if C > 1 else 40
    k = n - 2
    pad = np.arange(100, 100 + n, dtype=np.int32)  # distinct tokens, none of them 1 or 2
    ab, ba = np.asarray([1, 2], np.int32), np.asarray([2, 1], np.int32)
    out = [("ab/ba", ab, ba, (1, 0, 1, 1), [1, -1], [-1, 0]), ("ba/ab", ba, ab, (1, 0, 1, 1), [1, -1], [-1, 0])]
    for extra_x, extra_y in ((0, 0), (0, 70), (70, 0)):
        x = np.concatenate([ab, pad[:k], np.arange(1000, 1000 + extra_x)]).astype(np.int32)
        y = np.concatenate([ba, pad[:k], np.arange(2000, 2000 + extra_y)]).astype(np.int32)
        xm = [1, -1] + list(range(2, k + 2)) + [-1] * extra_x
        ym = [-1, 0] + list(range(2, k + 2)) + [-1] * extra_y
        out.append(("tie before a run of %d, tails %d / %d" % (k, extra_x, extra_y), x, y, (k + 1, 0, 1 + extra_y, 1 + extra_x), xm, ym))
    a = pad.copy()
    out.append(("equal", a, a.copy(), (n, 0, 0, 0), list(range(n)), list(range(n))))
    out.append(("disjoint", a, (pad + 5000).astype(np.int32), (0, n, 0, 0), list(range(n)), list(range(n))))  # (equal lengths: any gap costs two)
    long = np.arange(100, 170 + n, dtype=np.int32)
    m = len(long)
    out.append(("prefix", long[:n].copy(), long, (n, 0, m - n, 0), list(range(n)), list(range(n)) + [-1] * (m - n)))
    out.append(("suffix as x", long[m - n:].copy(), long, (n, 0, m - n, 0), list(range(m - n, m)), [-1] * (m - n) + list(range(n))))
    out.append(("suffix as y", long, long[m - n:].copy(), (n, 0, 0, m - n), [-1] * (m - n) + list(range(n)), list(range(m - n, m))))
    # a rotation of n >= 3 distinct tokens, y = x[1:] + x[:1]: x[0] is inserted and y[n - 1] deleted; pairing those two would cost 2 (n - 1)
    out.append(("rotation", a, np.roll(a, -1), (n - 1, 0, 1, 1), [-1] + list(range(n - 1)), list(range(1, n)) + [-1]))
    return out


def slot_reuse_cases():
    """Two calls' worth of pairs for one slot: a long pair of class 16 followed by a short one of class 1, and the reverse (B = 2, one
    pair per item: with one slot the second pair finds what the first left)."""
    rng = np.random.default_rng(eu.hash_name("slot reuse"))
    long_a, long_b = eu.related_rows(rng, 700, 900, 2)
    short_a, short_b = eu.related_rows(rng, 9, 30, 2)
    out = []
    for order in ((0, 1), (1, 0)):
        xs, ys = [(long_a, short_a)[k] for k in order], [(long_b, short_b)[k] for k in order]
        x, xl = eu.pack_rows(xs)
        y, yl = eu.pack_rows(ys)
        out.append(dict(x=x[:, None], x_lens=xl[:, None], y=y[:, None], y_lens=yl[:, None]))
    return out


def limit_case(longest=MAX_DIM):
    """max(L, Lq) = 262144 against a strip of 3 tokens none of which occurs in the long row: D = 262144, S = 3 -- the greatest key."""
    x = np.asarray([[[7, 8, 9]]], np.int32)
    y = np.zeros((1, 1, longest), np.int32)
    return dict(x=x, x_lens=np.asarray([[3]], np.int32), y=y, y_lens=np.asarray([[longest]], np.int32))


# ---- the host twin -------------------------------------------------------------------------------------------------------------------
def build_ops_host():
    src = os.path.join(eu.NATIVE, "editops_host.cpp")
    deps = [src] + [os.path.join(eu.ROOT, "ctcdecode_amd", "csrc", h) for h in ("editdist.h", "editops.h")]
    if os.path.exists(OPS_HOST_SO) and all(os.path.getmtime(OPS_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return OPS_HOST_SO
    os.makedirs(os.path.dirname(OPS_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (OPS_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", tmp], check=True)
    os.replace(tmp, OPS_HOST_SO)
    return OPS_HOST_SO


def _lib():
    def make():
        lib = ctypes.CDLL(build_ops_host())
        ll = ctypes.c_longlong
        lib.ctcedit_host_counts.argtypes = [_i32p, _i32p] + [ctypes.c_int] * 3 + [_i32p, _i32p] + [ctypes.c_int] * 2 + [_i32p, _i32p, ctypes.POINTER(ll)]
        lib.ctcedit_host_align.argtypes = [_i32p, _i32p] + [ctypes.c_int] * 3 + [_i32p, _i32p] + [ctypes.c_int] * 2 + [_i32p] * 4 + [ll, ctypes.c_int, ctypes.POINTER(ll)]
        lib.ctcedit_host_slot_bytes.argtypes = [ctypes.c_int] * 2
        lib.ctcedit_host_slot_bytes.restype = ll
        lib.ctcedit_host_key_cell.argtypes = [ctypes.c_int] * 3 + [ctypes.c_int32] * 2
        lib.ctcedit_host_key_cell_dir.argtypes = [ctypes.c_int] * 3 + [ctypes.c_int32] * 2 + [ctypes.c_int, _i32p]
        lib.ctcedit_host_key.argtypes = [_i32p, ctypes.c_int, _i32p, ctypes.c_int]
        lib.ctcedit_host_counts_of.argtypes = [ctypes.c_int] * 3 + [_i32p]
        return lib
    return eu.cached("ops lib", make)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def _tensors(x, x_lens, y, y_lens):
    x = np.ascontiguousarray(x, np.int32)
    xl = np.ascontiguousarray(x_lens, np.int32)
    y = None if y is None else np.ascontiguousarray(y, np.int32)
    yl = None if y_lens is None else np.ascontiguousarray(y_lens, np.int32)
    B, R, L = x.shape
    Q, Lq = (R, L) if y is None else (y.shape[1], y.shape[2])
    return x, xl, y, yl, B, R, L, Q, Lq


def host_counts(x, x_lens, y=None, y_lens=None):
    """The twin over an output of sentinel words.  -> (rc, counts [B, R, Q, 4], status [B], pairs)."""
    x, xl, y, yl, B, R, L, Q, Lq = _tensors(x, x_lens, y, y_lens)
    out = np.full((B, R, Q, 4), eu.SENTINEL, np.int32)
    status = np.zeros((max(B, 1),), np.int32)
    pairs = ctypes.c_longlong(-1)
    one = np.zeros(1, np.int32)  # (a general-mode y of no elements still needs an address)
    rc = _lib().ctcedit_host_counts(_ptr(x), _ptr(xl), B, R, L, None if y is None else _ptr(y if y.size else one), _ptr(yl), Q, Lq, _ptr(out), _ptr(status),
                                    ctypes.byref(pairs))
    return rc, out, status[:B], int(pairs.value)


def host_align(x, x_lens, y, y_lens, budget=0, fill=0xA5):
    """The twin over outputs of sentinel words.  -> (rc, x_to_y, y_to_x, counts, status, slot bytes)."""
    x, xl, y, yl, B, R, L, Q, Lq = _tensors(x, x_lens, y, y_lens)
    xm = np.full((B, R, Q, L), eu.SENTINEL, np.int32)
    ym = np.full((B, R, Q, Lq), eu.SENTINEL, np.int32)
    counts = np.full((B, R, Q, 4), eu.SENTINEL, np.int32)
    status = np.zeros((max(B, 1),), np.int32)
    sb = ctypes.c_longlong(-1)
    one = np.zeros(1, np.int32)
    rc = _lib().ctcedit_host_align(_ptr(x), _ptr(xl), B, R, L, None if y is None else _ptr(y if y.size else one), _ptr(yl), Q, Lq, _ptr(xm), _ptr(ym), _ptr(counts),
                                   _ptr(status), int(budget), int(fill), ctypes.byref(sb))
    return rc, xm, ym, counts, status[:B], int(sb.value)


def host_pair_align(a, b, **kw):
    """One pair of plain sequences through the twin's align.  -> (counts tuple, x_to_y list, y_to_x list)."""
    a, b = np.asarray(a, np.int32).ravel(), np.asarray(b, np.int32).ravel()
    rc, xm, ym, counts, _, _ = host_align(a[None, None], [[len(a)]], b[None, None], [[len(b)]], **kw)
    assert rc == 0
    return tuple(int(v) for v in counts[0, 0, 0]), xm[0, 0, 0].tolist(), ym[0, 0, 0].tolist()


def host_slot_bytes(L, Lq):
    return int(_lib().ctcedit_host_slot_bytes(int(L), int(Lq)))


def host_key_cell(up, left, diag, a, b):
    return int(_lib().ctcedit_host_key_cell(int(up), int(left), int(diag), int(a), int(b)))


def host_key_cell_dir(up, left, diag, a, b, x_strip):
    d = np.zeros(1, np.int32)
    v = int(_lib().ctcedit_host_key_cell_dir(int(up), int(left), int(diag), int(a), int(b), 1 if x_strip else 0, _ptr(d)))
    return v, int(d[0])


def host_key(a, b):
    a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
    k = int(_lib().ctcedit_host_key(_ptr(a), len(a), _ptr(b), len(b)))
    return k >> 12, k & 4095
