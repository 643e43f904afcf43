"""The CTC prefix scores on the CPU: prefix.h's routines run sequentially (host twin, tests/native/prefix_host.cpp) against the numpy
restatement of the header (tests/prefix_util.py) and the log-likelihood's lattice, bit for bit; the restatement against all paths."""
import ctypes
import itertools
import os
import subprocess

import align_util as au
import loglik_util as lu
import numpy as np
import prefix_util as pu
import pytest

# n on both sides of the scores kernel's chunk (32) and the advance kernel's tile (16), and 0, 1, 2; frame 16 all -inf
CASE = dict(T=33, V=6, seq_lens=[33, 0, 1, 2, 15, 16, 17, 31, 32], R=1, seed=3, inf_frames=[16])
Y = [2, 2, 3, 1]  # the labels a prefix grows by: a repeat among them, and more of them than the short items have frames


def _twin():
    so, src = os.path.join(au.ROOT, "oracle", "_build", "libctcprefix_host.so"), os.path.join(au.NATIVE, "prefix_host.cpp")
    os.makedirs(os.path.dirname(so), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.ctcprefix_host_eos.restype = ctypes.c_float
    return lambda name, *a: getattr(lib, "ctcprefix_host_" + name)(*[x.ctypes.data_as(ctypes.c_void_p) if isinstance(x, np.ndarray) else int(x) for x in a])


@pytest.mark.parametrize("prob", [0, 1])
def test_twin_restatement_and_lattice_agree(prob):
    """Every item of the case, a prefix grown label by label: the twin's cols, scores of all labels and eos == the restatement's; the
    restated cols == a[t][S-2], a[t][S-1] of loglik_util.forward's recurrence and eos == loglik_util.forward -- prefixes longer than
    n and a whole frame of -inf included.  prob: the twin reads probabilities, the restatement their float32(log(p + FLT_MIN))."""
    c, twin = pu.make_case(**CASE), au.cached("prefix twin", _twin)
    rows = np.exp(c["lp"].astype(np.float64)).astype(np.float32) if prob else c["lp"]
    lp, (T, V), cands = (au.prob_to_lp(rows) if prob else rows), rows.shape[1:], np.arange(1, rows.shape[2], dtype=np.int32)
    for b, n in enumerate(c["seq_lens"]):
        got, want, one = np.full((T, 2), np.nan, np.float32), pu.r_init(lp[b], n), dict(seq_lens=np.asarray([n]))
        twin("init", rows[b], prob, n, V, got)
        for L in range(len(Y) + 1):
            last, sc = (Y[L - 1] if L else -1), np.zeros(V - 1, np.float32)
            twin("scores", rows[b], prob, n, V, got, L, last, cands, V - 1, sc)
            pu.same_bits(got[None, None], want[None, None], "twin: cols of %s" % Y[:L], one)
            pu.same_bits(sc, pu.r_scores(lp[b], n, want, L, last, cands), "twin: scores after %s" % Y[:L])
            pu.same_bits(want[None, None], pu.lattice_cols(lp[b], n, Y[:L])[None, None], "lattice: cols of %s" % Y[:L], one)
            eos = [np.float32(twin("eos", n, got, L)), pu.r_eos(n, want, L), lu.forward(lp[b], n, Y[:L], 0)]
            assert len({e.view(np.uint32).item() for e in eos}) == 1, (b, L, eos)
            if L < len(Y):
                nxt = np.full((T, 2), np.nan, np.float32)
                twin("advance", rows[b], prob, n, V, got, L, last, Y[L], nxt)
                got, want = nxt, pu.r_advance(lp[b], n, want, L, last, Y[L])


# The restatement's largest deviation from the float64 brute force on these inputs, measured: 8.05e-7 (T 6, V 3; values of magnitude
# up to about 12, whose float32 ulp is 9.5e-7); the bound is 4 x that, for other libm roundings.
BRUTE_TOL = 3.3e-6


@pytest.mark.parametrize("T,V,seed", [(6, 3, 0), (5, 3, 1), (4, 2, 2), (1, 3, 3)])
def test_restatement_against_all_paths(T, V, seed):
    """float64, every one of the V^T paths: psi(g.c) = log of the summed probability of the paths whose collapse starts with g.c,
    eos(g) = of those whose collapse is g, and exp(psi(g)) = exp(eos(g)) + sum_c exp(psi(g.c))."""
    lp = au.log_softmax_rows(np.random.default_rng(seed), 1, T, V)[0]
    mass = {}
    for path in itertools.product(range(V), repeat=T):
        y = tuple(k for k, _ in itertools.groupby(path) if k != 0)
        mass[y] = mass.get(y, 0.0) + float(np.exp(sum(float(lp[t, s]) for t, s in enumerate(path))))
    todo, labels = [((), pu.r_init(lp, T), 0.0)], np.arange(1, V)
    while todo:
        g, cols, psi_g = todo.pop()
        last = g[-1] if g else -1
        psi = pu.r_scores(lp, T, cols, len(g), last, labels)
        got = [float(pu.r_eos(T, cols, len(g)))] + [float(v) for v in psi]
        want = [mass.get(g, 0.0)] + [sum(p for y, p in mass.items() if y[:len(g) + 1] == g + (int(k),)) for k in labels]
        for a, w in zip(got, want):
            assert (w == 0.0 and a == -np.inf) or abs(a - np.log(w)) <= BRUTE_TOL, (g, a, w)
        lhs, rhs = np.exp(psi_g), np.exp(np.asarray(got)).sum()  # (every term within a factor exp(+-BRUTE_TOL))
        assert abs(lhs - rhs) <= BRUTE_TOL * (lhs + rhs), g
        if len(g) < 3:
            todo += [(g + (int(k),), pu.r_advance(lp, T, cols, len(g), last, int(k)), float(v)) for k, v in zip(labels, psi)]
