"""Keyword search on the CPU (include/ctcdecode_amd.h "Keyword search"): the host twin of keyword.h against the numpy restatement, bit for
bit, on the case table the GPU test runs; the restatement against a float64 brute force over every window; the greedy property."""
import numpy as np
import pytest

import greedy_util as gu
import keyword_util as ku


@pytest.mark.parametrize("c", ku.CASES, ids=lambda c: c["name"])
def test_twin_equals_restatement(c):
    want = ku.reference_of(c)
    got, status = ku.host_find(c)
    ku.assert_same(got, want, c["name"])
    assert not status.any()
    for b, q, s, e in ku.WINDOWS.get(c["name"], []):
        assert (want["starts"][b, q], want["ends"][b, q]) == (s, e), (b, q)


def test_twin_shapes_and_invalid_keywords():
    lib = ku.host_lib()
    assert lib.ctckw_host_chunk() == ku.F
    assert [lib.ctckw_host_lane_group(L) for L in (0, 1, 8, 9, 16, 17, 32, 33, 64)] == [8, 8, 8, 16, 16, 32, 32, 64, 64]
    assert [lib.ctckw_host_staged(V) for V in (1, 128, 129)] == [1, 1, 0]
    c = dict(ku.case("invalid", V=9, T=6), kws=[[3], [8], [9], [3, -1], []])  # blank 8 (an odd name): a blank label, a label >= V, a negative one, no label
    got, status = ku.host_find(c, Lk=2)
    assert status.tolist() == [0, 8, 8, 8, 8]
    assert (got["scores"][:, 1:] == 0).all() and (got["starts"][:, 1:] == -1).all() and (got["ends"][:, 1:] == -1).all() and (got["end_scores"][:, 1:] == 0).all()


def _brute(rel, z):
    """float64, every window [ts, te]: enter state 0 at ts, be in the last state at te.  -> (values [n, n], greatest |partial sum|)."""
    n, S = rel.shape[0], len(z)
    val, big = np.full((n, n), -np.inf), 0.0
    for ts in range(n):
        d = [-np.inf] * S
        for t in range(ts, n):
            pred = lambda s: [d[s]] + ([d[s - 1]] if s else []) + ([d[s - 2]] if s >= 2 and s % 2 == 0 and z[s] != z[s - 2] else [])  # noqa: E731
            d = [rel[t, z[s]] + ((0.0 if s == 0 else -np.inf) if t == ts else max(pred(s))) for s in range(S)]
            big = max([big] + [abs(v) for v in d if np.isfinite(v)])
            val[ts, t] = d[-1]
    return val, big


@pytest.mark.parametrize("seed,T,kw", [(1, 12, [1, 2, 3]), (2, 12, [2, 2]), (3, 9, [4]), (14, 11, [3, 1, 3]), (5, 7, [1, 1, 2]), (6, 12, [2, 4])])
def test_definition_against_float64_brute_force(seed, T, kw):
    x = gu.random_rows(np.random.default_rng(seed), 1, T, 5, 1)[0]  # V = 5, blank 0
    score, start, end, _, _ = ku.find_item(x, T, 0, 1, kw)
    rel = x.astype(np.float64) - x.astype(np.float64).max(-1, keepdims=True)
    val, big = _brute(rel, [kw[s // 2] if s % 2 == 0 else 0 for s in range(2 * len(kw) - 1)])
    bound = 2 * T * 2.0 ** -23 * big  # one subtraction and one addition per cell, along a path of at most n cells
    ts, te = np.unravel_index(np.argmax(val), val.shape)
    others = val.copy()
    others[ts, te] = -np.inf
    print("score %r brute %r bound %g margin %g" % (score, val[ts, te], bound, val[ts, te] - others.max()))
    assert val[ts, te] - others.max() > bound, "the seed leaves the best window no margin"
    assert abs(float(score) - val[ts, te]) <= bound
    assert (start, end) == (ts, te)


@pytest.mark.parametrize("mode", (0, 1))
def test_greedy_runs_score_zero(mode):
    path = [1, 1, 0, 2, 3, 3, 0, 0, 4, 5, 5, 6, 0, 7, 7]  # the transcript 1 .. 7: no label recurs
    x = gu.path_rows(np.random.default_rng(7 + mode), [path], 8, mode)[0]
    tok, st, en = gu.greedy_item(x, len(path), 0, mode)[:3]
    assert tok == [1, 2, 3, 4, 5, 6, 7]
    for i in range(len(tok)):
        for j in range(i, min(i + 4, len(tok))):
            score, start, end, _, _ = ku.find_item(x, len(path), 0, mode, tok[i:j + 1])
            assert (gu.bits1(score), start, end) == (0, st[i], en[j]), (i, j)
