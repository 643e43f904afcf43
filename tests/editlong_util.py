"""What the long-pair tests share (ctcd_set_edit_long; ctcdecode_amd/csrc/editlong.h): the references, the cases and the host twin.
Distances come from ``editdist_util.lev``.  Counts come from ``key_ref`` below: the header's recurrence over K = D * 2^32 + S in two
int64 rows (editops_util's reference keeps the whole matrix, half a gigabyte at 8193 x 8193)."""
import ctypes
import os
import subprocess

import editdist_util as eu
import numpy as np

STRIPS = (2049, 4095, 4096, 4097, 6145)  # one column in tile 2 | .. | the first hand-off through the slot (W = 2) | round two's second tile
# streamed rows against the longest strip, disjoint alphabets (D = m, S = n whatever the path): at two waves tile 2 follows tile 0 on
# wave 0 while tile 1 still reads tile 0's ring -- its last row m at index 1 (12545 = 1 mod 256), or at index 65 with m = 1 mod 64
DISJOINT = (12545, 12609)
LONG_HOST_SO = os.path.join(eu.ROOT, "oracle", "_build", "libctcedit_long_host.so")
_E = 1 << 32


def streamed(n):  # the block edge and the two-block lag
    return (n, n + 1, n + 63, n + 64, n + 129, 2 * n + 5)


def key_ref(a, b):
    """(D, S) of "Edit operations": K[i][j] = min(K[i-1][j-1] + (a != b ? (1,1) : (0,0)), K[i-1][j] + (1,0), K[i][j-1] + (1,0)) over
    K = D * 2^32 + S, row by row; the dependence on K[i][j-1] is a running minimum, as in ``editdist_util.lev``."""
    a, b = np.asarray(a, np.int32).ravel(), np.asarray(b, np.int32).ravel()
    if len(a) > len(b):
        a, b = b, a  # (the key matrix is its own transpose)
    idx = np.arange(len(b) + 1, dtype=np.int64) * _E
    prev = idx.copy()
    for i in range(1, len(a) + 1):
        t = np.empty(len(b) + 1, np.int64)
        t[0] = i * _E
        t[1:] = np.minimum(prev[1:] + _E, prev[:-1] + np.where(b != a[i - 1], _E + 1, 0))
        prev = np.minimum.accumulate(t - idx) + idx
    return int(prev[-1] >> 32), int(prev[-1] & (_E - 1))


def counts_ref(x, y):  # -> (H, S, Del, I) of hypothesis x against reference y
    D, S = key_ref(x, y)
    ins, dele = (D - S + len(x) - len(y)) // 2, (D - S - len(x) + len(y)) // 2
    return (len(x) - S - ins, S, dele, ins)


def strip_case(n):
    """One item per streamed length of ``streamed(n)``, alternately over 2 and 4 symbols, the strips in x.  In closed form: for the
    longest strip the DISJOINT items; for 4097 equal rows, the first token dropped, and one substitution in the last column of tile 0
    and in the first of tile 1, on either side.  -> dict(x, x_lens, y, y_lens) of [B, 1, L] tensors, dist [B], counts [B, 4]."""
    def make():
        rng = np.random.default_rng(eu.hash_name("long %d" % n))
        rows = [eu.related_rows(rng, n, m, 2 if k % 2 else 4) for k, m in enumerate(streamed(n))]
        rows = [(a, b, eu.lev(a, b), counts_ref(a, b)) for a, b in rows]
        for m in DISJOINT if n == STRIPS[-1] else ():
            rows.append((rng.integers(0, 2, n).astype(np.int32), rng.integers(2, 4, m).astype(np.int32), m, (0, n, m - n, 0)))
        if n == 4097:
            base = (np.arange(n) * 7 % 5).astype(np.int32)
            rows += [(base, base, 0, (n, 0, 0, 0)), (base[1:], base, 1, (n - 1, 0, 1, 0))]
            for pos in (eu.MAX_STRIP - 1, eu.MAX_STRIP):
                y = base.copy()
                y[pos] = 9
                rows += [(base, y, 1, (n - 1, 1, 0, 0)), (y, base, 1, (n - 1, 1, 0, 0))]
        (x, xl), (y, yl) = eu.pack_rows([r[0] for r in rows]), eu.pack_rows([r[1] for r in rows])
        return dict(x=x[:, None], x_lens=xl[:, None], y=y[:, None], y_lens=yl[:, None], dist=np.asarray([r[2] for r in rows], np.int32),
                    counts=np.asarray([r[3] for r in rows], np.int32))
    return eu.cached(("long strip", n), make)


MIXED_ROWS, MIXED_REFS = (0, 1, 300, 2048, 2049, 5000), (0, 2048, 2049, 5200)


def mixed_case():
    """B = 3; rows of MIXED_ROWS against references of MIXED_REFS; item 1 has a bad length.  The references cover the valid items."""
    rng = np.random.default_rng(eu.hash_name("long mixed"))
    src = rng.integers(0, 4, (3, 6000)).astype(np.int32)
    noisy = lambda s, lens, width: eu.pack_rows([np.where(rng.random(k) < 0.15, rng.integers(0, 4, k), s[:k]).astype(np.int32) for k in lens], width)  # noqa: E731
    xs, ys = [noisy(s, MIXED_ROWS, 5000) for s in src], [noisy(s, MIXED_REFS, 5200) for s in src]
    c = dict(x=np.stack([v[0] for v in xs]), x_lens=np.stack([v[1] for v in xs]), y=np.stack([v[0] for v in ys]), y_lens=np.stack([v[1] for v in ys]))
    c["x_lens"][1, 2] = 5001
    dist, counts = np.zeros((3, 6, 4), np.int32), np.zeros((3, 6, 4, 4), np.int32)
    for b, (i, lx), (j, ly) in ((b, r, q) for b in (0, 2) for r in enumerate(MIXED_ROWS) for q in enumerate(MIXED_REFS)):
        counts[b, i, j] = counts_ref(c["x"][b, i, :lx], c["y"][b, j, :ly])
        dist[b, i, j] = eu.lev(c["x"][b, i, :lx], c["y"][b, j, :ly])
    return dict(c, dist=dist, counts=counts, long_pairs=2 * sum(min(lx, ly) > eu.MAX_STRIP for lx in MIXED_ROWS for ly in MIXED_REFS))


# ---- the host twin -------------------------------------------------------------------------------------------------------------------
def _lib():
    def make():
        src = os.path.join(eu.NATIVE, "editlong_host.cpp")
        deps = [src] + [os.path.join(eu.ROOT, "ctcdecode_amd", "csrc", h) for h in ("editdist.h", "editops.h", "editlong.h")]
        if not (os.path.exists(LONG_HOST_SO) and all(os.path.getmtime(LONG_HOST_SO) >= os.path.getmtime(p) for p in deps)):
            os.makedirs(os.path.dirname(LONG_HOST_SO), exist_ok=True)
            tmp = "%s.%d.tmp" % (LONG_HOST_SO, os.getpid())
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", tmp], check=True)
            os.replace(tmp, LONG_HOST_SO)
        return ctypes.CDLL(LONG_HOST_SO)
    return eu.cached("long lib", make)


def host_pair(x, y, W, counts):
    x, y = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(y, np.int32)
    out = np.full(4, eu.SENTINEL, np.int32)
    _lib().ctcedit_long_host_pair(eu._ptr(x), len(x), eu._ptr(y), len(y), W, int(counts), eu._ptr(out))
    return tuple(int(v) for v in out) if counts else int(out[0])


def host_sched(g, w, m, n, W, q=0):
    """-> the ten words of ctcedit_long_host_sched (tests/native/editlong_host.cpp)."""
    out = np.zeros(10, np.int32)
    _lib().ctcedit_long_host_sched(g, w, m, n, W, q, eu._ptr(out))
    return [int(v) for v in out]
