"""The edit distance's host code (ctcdecode_amd/csrc/editdist.h) against the numpy restatement of the header's definition
(tests/editdist_util.py), exactly, on the CPU: the twin tests/native/editdist_host.cpp runs the routines the kernel compiles with 64
simulated lanes.  Strip lengths around every class's lane and wave boundaries, streamed lengths around the 64-token blocks, both
roles, closed forms, token values at the ends of int32, random small cases, the limit, the routines one by one, and the stand-alone
sanitizer driver on the same cases."""
import os
import struct
import subprocess

import editdist_util as eu
import numpy as np
import pytest


def _check(c, what):
    want, want_status = eu.cached(("ref", what), lambda: eu.case_reference(c))
    rc, out, status, pairs = eu.host_distance(c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0, what
    bad = np.argwhere(out != want)
    assert bad.size == 0, "%s: differs at %s: got %s, want %s" % (what, bad[:4].tolist(), out[tuple(bad[0])], want[tuple(bad[0])])
    assert (status == want_status).all(), what
    B, R, Q = want.shape
    assert pairs == (B * R * (R - 1) // 2 if c["y"] is None else B * R * Q), what
    return want


def test_the_restatement_agrees_with_its_cell_by_cell_form():
    rng = np.random.default_rng(3)
    for _ in range(300):
        a, b = rng.integers(0, 3, int(rng.integers(0, 14))), rng.integers(0, 3, int(rng.integers(0, 14)))
        assert eu.lev(a, b) == eu.lev_plain(a, b)
    assert eu.lev([1, 2, 3], []) == 3 and eu.lev([], []) == 0 and eu.lev([1, 2, 3], [2, 3, 4]) == 2


@pytest.mark.parametrize("swap", (False, True), ids=("x_is_strip", "y_is_strip"))
@pytest.mark.parametrize("C", eu.CLASSES)
def test_twin_equals_the_restatement_over_the_length_grid(C, swap):
    c = eu.grid_case(C, swap)
    want = _check(c, "grid %d %s" % (C, swap))
    # the grid is what it says: every strip length of the class with every streamed length, the distances not all trivial
    assert {n for n, _ in c["pairs"]} == set(eu.strip_lengths(C))
    assert {eu.klass(n) for n, _ in c["pairs"] if n} >= {C}
    assert all(want[k, 0, 0] >= m - n for k, (n, m) in enumerate(c["pairs"]))
    assert any(m - n < want[k, 0, 0] < m for k, (n, m) in enumerate(c["pairs"]) if n)


@pytest.mark.parametrize("C", eu.CLASSES)
def test_closed_forms(C):
    for name, a, b, d in eu.closed_form_cases(C):
        assert eu.host_pair(a, b) == d, "class %d %s" % (C, name)
        assert eu.host_pair(b, a) == d, "class %d %s, swapped" % (C, name)
        if len(a) <= 300:
            assert eu.lev(a, b) == d, "class %d %s: the restatement" % (C, name)


def test_token_values_are_compared_as_values():
    c = eu.token_value_case()
    _check(c, "token values")
    assert eu.host_pair([eu.I32_MIN], [eu.I32_MAX]) == 1 and eu.host_pair([eu.I32_MIN, -1], [eu.I32_MIN, -1]) == 0
    assert eu.host_pair([0], [-1]) == 1 and eu.host_pair([eu.I32_MAX], [eu.I32_MAX]) == 0
    assert eu.host_cell(5, 5, 5, eu.I32_MIN, eu.I32_MAX) == 6 and eu.host_cell(5, 5, 5, -1, -1) == 5
    assert eu.host_cell(2, 9, 9, 1, 1) == 3 and eu.host_cell(9, 2, 9, 1, 1) == 3 and eu.host_cell(9, 9, 2, 1, 2) == 3


@pytest.mark.parametrize("alphabet", (2, 4))
def test_random_small_cases(alphabet):
    rng = np.random.default_rng(11 + alphabet)
    for k in range(200):
        a = rng.integers(0, alphabet, int(rng.integers(0, 80))).astype(np.int32)
        b = rng.integers(0, alphabet, int(rng.integers(0, 200))).astype(np.int32)
        want = eu.lev(a, b)
        assert eu.host_pair(a, b) == want and eu.host_pair(b, a) == want, (k, len(a), len(b))


def test_the_limit():
    c = eu.limit_case()
    want = _check(c, "limit")
    assert want[0, 0, 0] == 2048 and 0 < want[0, 1, 1] < 2048
    x = np.zeros((1, 1, 2049), np.int32)
    rc, _, _, _ = eu.host_distance(x, [[2049]], x, [[2049]])
    assert rc == -2
    rc, out, _, _ = eu.host_distance(np.zeros((1, 1, 5000), np.int32), [[5000]], np.ones((1, 1, 8), np.int32), [[8]])
    assert rc == 0 and out[0, 0, 0] == 5000


def _check_against(c, want, what):
    rc, out, status, _ = eu.host_distance(c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0 and (out == want[0]).all() and (status == want[1]).all(), what


def test_a_launch_mixing_every_class_and_empty_rows():
    """The 600 pairs of tests/test_gpu_editdist.py's mixed launch, and the same launch with a bad length in the middle item."""
    c = eu.mixed_case()
    _check(c, "mixed")
    for side, bad in (("x", 2049), ("y", -1)):
        d, want = eu.with_bad_length(c, "mixed", 1, bad, side)
        assert want[1].tolist() == [0, eu.BAD_ROW, 0] and (want[0][0] != 0).any() and (want[0][2] != 0).any()
        _check_against(d, want, "mixed, bad %s length" % side)


def test_many_short_pairs_with_a_bad_item_between_good_ones():
    c = eu.many_short_case()
    _check(c, "many short")
    d, want = eu.with_bad_length(c, "many short", 2, 25)
    assert (want[0][1] != 0).any() and (want[0][3] != 0).any()
    _check_against(d, want, "many short, bad item")


def test_pairwise_mode():
    c = eu.pairwise_case(7)
    want = _check(c, "pairwise 7")
    assert (want == want.transpose(0, 2, 1)).all() and (np.diagonal(want, axis1=1, axis2=2) == 0).all()
    rc, out, _, pairs = eu.host_distance(c["x"], c["x_lens"], c["x"].copy(), c["x_lens"].copy())
    assert rc == 0 and (out == want).all() and pairs == 2 * 7 * 7
    for R in (1, 2):
        _check(eu.pairwise_case(R), "pairwise %d" % R)


def test_bad_lengths_zero_the_item_and_raise_its_status():
    c = eu.pairwise_case(7, B=3, L=40)
    for bad in (-1, 41):
        xl = c["x_lens"].copy()
        xl[1, 3] = bad
        want, want_status = eu.reference(c["x"], xl)
        assert want_status.tolist() == [0, eu.BAD_ROW, 0] and (want[1] == 0).all()
        rc, out, status, _ = eu.host_distance(c["x"], xl)
        assert rc == 0 and (out == want).all() and (status == want_status).all()
        y, yl = c["x"][:, :2].copy(), c["x_lens"][:, :2].copy()
        yl[2, 1] = bad
        want, want_status = eu.reference(c["x"], c["x_lens"], y, yl)
        rc, out, status, _ = eu.host_distance(c["x"], c["x_lens"], y, yl)
        assert rc == 0 and (out == want).all() and status.tolist() == [0, 0, eu.BAD_ROW]


def test_degenerate_shapes():
    z = np.zeros
    for shape_x, shape_y in (((0, 3, 4), (0, 2, 4)), ((2, 0, 4), (2, 2, 4)), ((2, 3, 4), (2, 0, 4))):
        rc, out, _, pairs = eu.host_distance(z(shape_x, np.int32), z(shape_x[:2], np.int32), z(shape_y, np.int32), z(shape_y[:2], np.int32))
        assert rc == 0 and pairs == 0 and (out == eu.SENTINEL).all()
    yl = np.asarray([[3, 0], [1, 4]], np.int32)
    rc, out, _, _ = eu.host_distance(z((2, 3, 0), np.int32), z((2, 3), np.int32), np.ones((2, 2, 4), np.int32), yl)
    assert rc == 0 and (out == yl[:, None, :]).all()  # L == 0: the other side's lengths


def test_class_function_covers_exactly_its_declared_classes():
    assert eu.host_classes() == eu.CLASSES
    got = {}
    for n in range(1, eu.MAX_STRIP + 1):
        c = eu.host_class(n)
        assert c == eu.klass(n) and 64 * c >= n and (c == 1 or 64 * (c // 2) < n)
        got.setdefault(c, []).append(n)
    assert tuple(sorted(got)) == eu.host_classes()
    assert [got[c][0] for c in eu.CLASSES] == [1, 65, 129, 257, 513, 1025] and got[32][-1] == 2048


@pytest.mark.parametrize("R", (1, 2, 3, 40))
def test_pair_enumeration_is_a_bijection_onto_the_upper_triangle(R):
    per = eu.host_pairs_per_item(R, R, True)
    assert per == R * (R - 1) // 2
    B = 3
    seen = [eu.host_pair_of(w, R, R, True) for w in range(B * per)]
    assert seen == [(b, i, j) for b in range(B) for i in range(R) for j in range(i + 1, R)]
    Q = 5
    assert eu.host_pairs_per_item(R, Q, False) == R * Q
    assert [eu.host_pair_of(w, R, Q, False) for w in range(B * R * Q)] == [(b, i, j) for b in range(B) for i in range(R) for j in range(Q)]


def test_pair_enumeration_of_a_large_triangle():
    R = 46341  # R (R - 1) / 2 > 2^30: the estimate's rounding is settled by the integer steps
    per = eu.host_pairs_per_item(R, R, True)
    off = lambda i: i * (2 * R - i - 1) // 2  # noqa: E731
    for i in (0, 1, 2, R // 2, R - 3, R - 2):
        for k, j in ((off(i), i + 1), (off(i + 1) - 1, R - 1)):
            assert eu.host_pair_of(5 * per + k, R, R, True) == (5, i, j)


def test_result_lane_arithmetic():
    for C in eu.CLASSES:
        for n in (1, C, C + 1, 63 * C + 1, 64 * C):
            for m in (n, n + 100):
                lane, col, steps = eu.host_result_at(m, n, C)
                assert lane * C + col + 1 == n and 0 <= col < C and 0 <= lane < 64
                assert steps == m + lane  # lane l computes row r at step r + l - 1: row m of the result's lane is the last step


def test_gpu_cases_reach_every_compiled_class():
    hit = {eu.host_class(n) for n in eu.gpu_strip_lengths()}
    assert hit == set(eu.host_classes()), sorted(set(eu.host_classes()) - hit)


def _write_case(path, c):
    want, status = eu.case_reference(c)
    x = np.ascontiguousarray(c["x"], np.int32)
    B, R, L = x.shape
    pairwise = c["y"] is None
    Q, Lq = (R, L) if pairwise else c["y"].shape[1:]
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", B, R, L, Q, Lq, 1 if pairwise else 0))
        f.write(x.tobytes())
        f.write(np.ascontiguousarray(c["x_lens"], np.int32).tobytes())
        if not pairwise:
            f.write(np.ascontiguousarray(c["y"], np.int32).tobytes())
            f.write(np.ascontiguousarray(c["y_lens"], np.int32).tobytes())
        f.write(np.ascontiguousarray(want, np.int32).tobytes())
        f.write(np.ascontiguousarray(status, np.int32).tobytes())


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/editdist_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own: the grids of three
    classes in both roles, the token values, pairwise mode and a bad length against the restatement's outputs, and the exactly-sized
    pairs the driver makes itself."""
    bad = eu.pairwise_case(7, B=2, L=40)
    bad["x_lens"] = bad["x_lens"].copy()
    bad["x_lens"][1, 0] = 41
    cases = [eu.grid_case(1, False), eu.grid_case(2, True), eu.grid_case(8, False), eu.token_value_case(), eu.pairwise_case(7), eu.pairwise_case(1), bad]
    files = []
    for k, c in enumerate(cases):
        files.append(str(tmp_path / ("case%d.bin" % k)))
        _write_case(files[-1], c)
    exe = str(tmp_path / "editdist_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(eu.NATIVE, "editdist_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failures" in r.stdout
