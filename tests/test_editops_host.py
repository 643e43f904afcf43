"""The edit operations' host code (ctcdecode_amd/csrc/editops.h) against the restatement of the header's definition
(tests/editops_util.py), exactly, on the CPU: the twin tests/native/editops_host.cpp runs the routines the kernels compile with 64
simulated lanes and a back-pointer slot of exactly the size the entry point allocates per wave.  The restatement itself against the
enumeration of all alignments; counts and maps over every class's lane and wave boundaries in both roles; the tie rule in closed
forms; slot reuse; the limits; degenerate and invalid cases; and the stand-alone sanitizer driver on written case files."""
import os
import struct
import subprocess

import editdist_util as eu
import editops_util as ou
import numpy as np
import pytest


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def test_the_restatement_equals_the_enumeration_of_all_alignments():
    """500 random pairs over 2 and 4 symbols, lengths 0 .. 7: the least (D, S) over all alignments, the counts, and the canonical maps
    found by the walk's three rules on enumerated prefix optima, against the vectorised and the cell-by-cell restatement.  At least 5 %
    of the pairs have more than one S at the optimal D: the tie rule decides something."""
    rng = np.random.default_rng(20261021)
    ties = 0
    for k in range(500):
        alphabet = 2 if k % 2 else 4
        x, y = rng.integers(0, alphabet, int(rng.integers(0, 8))), rng.integers(0, alphabet, int(rng.integers(0, 8)))
        key, counts, xm, ym, subs = ou.canonical_of_enumeration(x, y)
        assert key[1] == min(subs) and key[0] == eu.lev_plain(x, y)
        assert ou.align_ref(x, y) == (key, counts, xm, ym), (x, y)
        assert ou.align_plain(x, y) == (key, counts, xm, ym), (x, y)
        assert ou.key_of(x, y) == key == ou.key_of(y, x)
        kt, ct, xt, yt = ou.align_ref(y, x)  # the transpose: the same key, Del and I exchanged (the maps need not be transposes)
        assert kt == key and ct == (counts[0], counts[1], counts[3], counts[2])
        assert ou.counts_from_maps(xm, ym, x, y, len(x), len(y)) == counts
        ties += len(subs) > 1
    print("pairs with more than one S at the optimal D: %d of 500" % ties)
    assert ties >= 25
    assert ou.align_ref([1, 2], [2, 1]) == ((2, 0), (1, 0, 1, 1), [1, -1], [-1, 0])  # the header's example


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
def _check_counts(c, what):
    want, want_status = eu.cached(("ops counts", what), lambda: ou.case_reference(c))
    rc, out, status, pairs = ou.host_counts(c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0, what
    bad = np.argwhere((out != want).any(-1))
    assert bad.size == 0, "%s: differs at %s: got %s, want %s" % (what, bad[:4].tolist(), out[tuple(bad[0])], want[tuple(bad[0])])
    assert (status == want_status).all(), what
    B, R, Q = want.shape[:3]
    assert pairs == (B * R * (R - 1) // 2 if c["y"] is None else B * R * Q), what
    return want


def _check_identities(c, counts):
    """H + S + I == lx, H + S + Del == ly, and S + Del + I == the distance twin's answer on the same tensors."""
    H, S, Del, I = (counts[..., k] for k in range(4))
    yl = c["x_lens"] if c["y"] is None else c["y_lens"]
    assert (H + S + I == np.asarray(c["x_lens"])[:, :, None]).all() and (H + S + Del == np.asarray(yl)[:, None, :]).all()
    rc, dist, _, _ = eu.host_distance(c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0 and (S + Del + I == dist).all()


@pytest.mark.parametrize("swap", (False, True), ids=("x_is_strip", "y_is_strip"))
@pytest.mark.parametrize("C", eu.CLASSES)
def test_twin_counts_equal_the_restatement_over_the_length_grid(C, swap):
    c = eu.grid_case(C, swap)
    want = _check_counts(c, "grid %d %s" % (C, swap))
    _check_identities(c, want)
    assert (want[:, 0, 0, 1] > 0).any() and (want[:, 0, 0, 2] > 0).any() and (want[:, 0, 0, 3] > 0).any()  # every kind of edit occurs


@pytest.mark.parametrize("alphabet", (2, 4))
def test_random_small_cases_in_both_argument_orders(alphabet):
    rng = np.random.default_rng(31 + alphabet)
    for k in range(150):
        a = rng.integers(0, alphabet, int(rng.integers(0, 80))).astype(np.int32)
        b = rng.integers(0, alphabet, int(rng.integers(0, 200))).astype(np.int32)
        key, counts, xm, ym = ou.align_ref(a, b)
        assert ou.host_key(a, b) == key == ou.host_key(b, a), (k, len(a), len(b))
        assert ou.host_pair_align(a, b) == (counts, xm, ym), (k, len(a), len(b))
        _, ct, xt, yt = ou.align_ref(b, a)
        assert ou.host_pair_align(b, a) == (ct, xt, yt), (k, len(a), len(b))
        assert sum(counts[1:]) == eu.host_pair(a, b)


def test_pairwise_counts_and_the_mixed_launch():
    for R in (1, 2, 7):
        c = eu.pairwise_case(R)
        want = _check_counts(c, "pairwise %d" % R)  # (R = 7 last: its tensors go through the general mode below)
        _check_identities(c, want)
        assert (want == want.transpose(0, 2, 1, 3)[..., [0, 1, 3, 2]]).all()
        assert (np.diagonal(want[..., 0], axis1=1, axis2=2) == c["x_lens"]).all() and (np.diagonal(want[..., 1:].sum(-1), axis1=1, axis2=2) == 0).all()
    rc, out, _, pairs = ou.host_counts(c["x"], c["x_lens"], c["x"].copy(), c["x_lens"].copy())  # the general mode on the same rows
    assert rc == 0 and pairs == 2 * 7 * 7 and (out == want).all()
    m = eu.mixed_case()
    _check_identities(m, _check_counts(m, "mixed"))


# ---- maps ------------------------------------------------------------------------------------------------------------------------------
def _check_maps_case(c, what):
    want = eu.cached(("ops maps", what), lambda: ou.case_reference(c, True))
    rc, xm, ym, counts, status, sb = ou.host_align(c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0 and sb == ou.host_slot_bytes(c["x"].shape[2], c["y"].shape[2]), what
    for got, ref, name in ((xm, want[1], "x_to_y"), (ym, want[2], "y_to_x"), (counts, want[0], "counts")):
        bad = np.argwhere(got != ref)
        assert bad.size == 0, "%s: %s differs at %s: got %s, want %s" % (what, name, bad[:4].tolist(), got[tuple(bad[0])], ref[tuple(bad[0])])
    assert (status == want[3]).all()
    return xm, ym, counts


@pytest.mark.parametrize("swap", (False, True), ids=("x_is_strip", "y_is_strip"))
@pytest.mark.parametrize("C", eu.CLASSES)
def test_twin_maps_equal_the_restatement_over_the_length_grid(C, swap):
    """Strips of 1, C, C + 1, 63 C + 1, 64 C - 1 and 64 C tokens against streamed rows of n, n + 1, n + 63, n + 64 and n + 65; and the
    properties every pair of maps has."""
    c = ou.map_grid_case(C, swap)
    assert {n for n, _ in c["pairs"]} == set(ou.map_strip_lengths(C)) and {eu.klass(n) for n, _ in c["pairs"]} >= {C}
    xm, ym, counts = _check_maps_case(c, "map grid %d %s" % (C, swap))
    dirs = set()
    for k in range(len(c["pairs"])):
        lx, ly = int(c["x_lens"][k, 0]), int(c["y_lens"][k, 0])
        ou.check_maps(xm[k, 0, 0], ym[k, 0, 0], lx, ly)
        assert ou.counts_from_maps(xm[k, 0, 0], ym[k, 0, 0], c["x"][k, 0], c["y"][k, 0], lx, ly) == tuple(counts[k, 0, 0])
        dirs |= {name for name, v in zip(("S", "Del", "I"), counts[k, 0, 0, 1:]) if v}
    assert {"S", "I" if swap else "Del"} <= dirs  # (the longer row's surplus has no partner; the other kind needs luck at these lengths)


@pytest.mark.parametrize("C", eu.CLASSES)
def test_closed_forms_with_ties(C):
    """The header's [a, b] / [b, a] example in both argument orders, alone and in front of a common run on rows that reach class C, with
    a tail on either side that makes that side the streamed row; equal and disjoint rows, a prefix, a suffix, a rotation."""
    for name, x, y, counts, xm, ym in ou.tie_cases(C):
        assert ou.host_pair_align(x, y) == (counts, xm, ym), "class %d %s" % (C, name)
        assert ou.host_key(x, y) == (sum(counts[1:]), counts[1]), "class %d %s" % (C, name)
        if len(x) <= 300:
            assert ou.align_ref(x, y)[1:] == (counts, xm, ym), "class %d %s: the restatement" % (C, name)
        if len(x) and len(y):
            assert eu.klass(min(len(x), len(y))) == (C if len(x) > 2 else 1), name


def test_the_cell_and_its_direction():
    E = 4096
    assert ou.host_key_cell(5 * E, 5 * E, 5 * E, 1, 2) == 6 * E and ou.host_key_cell(5 * E, 5 * E, 5 * E, 3, 3) == 5 * E
    assert ou.host_key_cell(9 * E, 9 * E, 2 * E + 7, 1, 2) == 3 * E + 8  # a substitution counts in both halves
    assert ou.host_key_cell(5 * E, 5 * E, 5 * E + 1, eu.I32_MIN, eu.I32_MAX) == 6 * E  # (6, 0) from a side before (6, 2) from the pair
    # all three candidates equal (6, 0): the pair wins in either role
    for x_strip in (False, True):
        assert ou.host_key_cell_dir(5 * E, 5 * E, 6 * E, 4, 4, x_strip) == (6 * E, 0)
    # the two one-sided steps tie and the pair loses: the x-only step wins -- along the strip (2) when x is the strip, else the stream (1)
    assert ou.host_key_cell_dir(5 * E, 5 * E, 5 * E + 1, 1, 2, True) == (6 * E, 2)
    assert ou.host_key_cell_dir(5 * E, 5 * E, 5 * E + 1, 1, 2, False) == (6 * E, 1)
    # only one attains the key
    assert ou.host_key_cell_dir(4 * E, 5 * E, 6 * E, 1, 2, True) == (5 * E, 1) and ou.host_key_cell_dir(5 * E, 4 * E, 6 * E, 1, 2, False) == (5 * E, 2)


# ---- the slot --------------------------------------------------------------------------------------------------------------------------
def test_slot_reuse():
    """A long pair of class 16 and a short one of class 1 through ONE slot, in both orders, over a slot preset to two different bytes:
    the outputs equal those of a fresh slot per pair.  Nothing depends on what the slot held."""
    for c in ou.slot_reuse_cases():
        assert sorted(eu.klass(int(min(a, b))) for a, b in zip(c["x_lens"][:, 0], c["y_lens"][:, 0])) == [1, 16]
        fresh = [ou.host_pair_align(c["x"][k, 0, :c["x_lens"][k, 0]], c["y"][k, 0, :c["y_lens"][k, 0]]) for k in range(2)]
        for fill in (0x00, 0xFF, 0xA5):
            rc, xm, ym, counts, _, sb = ou.host_align(c["x"], c["x_lens"], c["y"], c["y_lens"], fill=fill)
            assert rc == 0 and sb == 900 * 64 * 4
            for k in range(2):
                lx, ly = int(c["x_lens"][k, 0]), int(c["y_lens"][k, 0])
                assert (tuple(counts[k, 0, 0]), xm[k, 0, 0, :lx].tolist(), ym[k, 0, 0, :ly].tolist()) == fresh[k]
                ou.check_maps(xm[k, 0, 0], ym[k, 0, 0], lx, ly)
        want = ou.case_reference(c, True)
        assert (xm == want[1]).all() and (ym == want[2]).all() and (counts == want[0]).all()


def test_slot_size():
    assert ou.host_slot_bytes(1000, 1000) == 1000 * 64 * 4 and ou.host_slot_bytes(1024, 5000) == 5000 * 64 * 4
    assert ou.host_slot_bytes(1025, 1025) == 1025 * 64 * 8 and ou.host_slot_bytes(2048, 2048) == 2048 * 64 * 8 == 1 << 20
    assert ou.host_slot_bytes(3, ou.MAX_DIM) == ou.MAX_DIM * 64 * 4
    assert ou.host_slot_bytes(0, 100) == 0 and ou.host_slot_bytes(100, 0) == 0


# ---- limits ----------------------------------------------------------------------------------------------------------------------------
def test_the_limits():
    """max(L, Lq) = 262144 against a strip of 3 tokens that occur nowhere in it: D = 262144, S = 3, the greatest key.  One more position
    is refused.  Pairwise mode into align is refused.  A slot larger than the budget is refused."""
    c = ou.limit_case()
    for a, b in ((c, False), (c, True)):
        x, xl, y, yl = (a["y"], a["y_lens"], a["x"], a["x_lens"]) if b else (a["x"], a["x_lens"], a["y"], a["y_lens"])
        rc, out, _, _ = ou.host_counts(x, xl, y, yl)
        D = ou.MAX_DIM
        assert rc == 0 and out[0, 0, 0].tolist() == ([0, 3, 0, D - 3] if b else [0, 3, D - 3, 0])
        assert D * 4096 + 3 < 2 ** 31 and (D + 1) * 4096 + 4095 < 2 ** 31
    rc, xm, ym, counts, _, sb = ou.host_align(c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0 and sb == ou.MAX_DIM * 64 * 4 and counts[0, 0, 0].tolist() == [0, 3, ou.MAX_DIM - 3, 0]
    # the walk pairs from the end: the three substitutions stand against the last three tokens of the long row
    assert xm[0, 0, 0].tolist() == [ou.MAX_DIM - 3, ou.MAX_DIM - 2, ou.MAX_DIM - 1] and (ym[0, 0, 0, :-3] == -1).all() and ym[0, 0, 0, -3:].tolist() == [0, 1, 2]
    over = ou.limit_case(ou.MAX_DIM + 1)
    assert ou.host_counts(over["x"], over["x_lens"], over["y"], over["y_lens"])[0] == -2
    assert ou.host_counts(over["y"], over["y_lens"], over["x"], over["x_lens"])[0] == -2
    assert ou.host_align(over["x"], over["x_lens"], over["y"], over["y_lens"])[0] == -2
    wide = np.zeros((1, 1, 2049), np.int32)
    assert ou.host_counts(wide, [[2049]], wide, [[2049]])[0] == -2 and ou.host_counts(wide, [[2049]])[0] == -2
    p = eu.pairwise_case(7)
    assert ou.host_align(p["x"], p["x_lens"], None, None)[0] == -1  # no alignments in pairwise mode
    s = ou.slot_reuse_cases()[0]
    need = 900 * 64 * 4
    assert ou.host_align(s["x"], s["x_lens"], s["y"], s["y_lens"], budget=need - 1)[0] == -2
    assert ou.host_align(s["x"], s["x_lens"], s["y"], s["y_lens"], budget=need)[0] == 0


# ---- degenerate and invalid cases ------------------------------------------------------------------------------------------------------
def test_bad_lengths_zero_the_item_and_raise_its_status():
    c = eu.pairwise_case(7, B=3, L=40)
    for bad in (-1, 41):
        xl = c["x_lens"].copy()
        xl[1, 3] = bad
        want, want_status = ou.reference(c["x"], xl)
        assert want_status.tolist() == [0, eu.BAD_ROW, 0] and (want[1] == 0).all() and (want[0] != 0).any()
        rc, out, status, _ = ou.host_counts(c["x"], xl)
        assert rc == 0 and (out == want).all() and (status == want_status).all()
        y, yl = c["x"][:, :2].copy(), c["x_lens"][:, :2].copy()
        yl[2, 1] = bad
        want = ou.reference(c["x"], c["x_lens"], y, yl, True)
        rc, out, status, _ = ou.host_counts(c["x"], c["x_lens"], y, yl)
        assert rc == 0 and (out == want[0]).all() and status.tolist() == [0, 0, eu.BAD_ROW]
        rc, xm, ym, counts, status, _ = ou.host_align(c["x"], c["x_lens"], y, yl)
        assert rc == 0 and status.tolist() == [0, 0, eu.BAD_ROW]
        assert (xm == want[1]).all() and (ym == want[2]).all() and (counts == want[0]).all()
        assert (xm[2] == -1).all() and (ym[2] == -1).all() and (counts[2] == 0).all() and (xm[1] >= 0).any()
    one = c["x"][:, :1], c["x_lens"][:, :1].copy()  # pairwise items of one row: a diagonal only, and still validated
    one[1][2, 0] = 41
    rc, out, status, pairs = ou.host_counts(one[0], one[1])
    assert rc == 0 and pairs == 0 and status.tolist() == [0, 0, eu.BAD_ROW]
    assert out[:, 0, 0].tolist() == [[int(one[1][0, 0]), 0, 0, 0], [int(one[1][1, 0]), 0, 0, 0], [0, 0, 0, 0]]


def test_degenerate_shapes():
    z = np.zeros
    for shape_x, shape_y in (((0, 3, 4), (0, 2, 4)), ((2, 0, 4), (2, 2, 4)), ((2, 3, 4), (2, 0, 4))):
        args = z(shape_x, np.int32), z(shape_x[:2], np.int32), z(shape_y, np.int32), z(shape_y[:2], np.int32)
        rc, out, _, pairs = ou.host_counts(*args)
        assert rc == 0 and pairs == 0 and (out == eu.SENTINEL).all()
        rc, xm, ym, counts, _, sb = ou.host_align(*args)
        assert rc == 0 and sb == 0 and (xm == eu.SENTINEL).all() and (counts == eu.SENTINEL).all()
    yl = np.asarray([[3, 0], [1, 4]], np.int32)
    ones = np.ones((2, 2, 4), np.int32)
    # L == 0: every reference token is a deletion; Lq == 0: every hypothesis token an insertion; empty rows on either side of full tensors
    rc, xm, ym, counts, _, sb = ou.host_align(z((2, 3, 0), np.int32), z((2, 3), np.int32), ones, yl)
    assert rc == 0 and sb == 0 and xm.shape == (2, 3, 2, 0) and (ym == -1).all()
    assert (counts[..., 2] == yl[:, None, :]).all() and (counts[..., [0, 1, 3]] == 0).all()
    rc, xm, ym, counts, _, sb = ou.host_align(ones, yl, z((2, 3, 0), np.int32), z((2, 3), np.int32))
    assert rc == 0 and sb == 0 and ym.shape == (2, 2, 3, 0) and (xm == -1).all()
    assert (counts[..., 3] == yl[:, :, None]).all() and (counts[..., :3] == 0).all()
    rc, out, _, _ = ou.host_counts(z((2, 3, 0), np.int32), z((2, 3), np.int32), ones, yl)
    assert rc == 0 and (out == counts.transpose(0, 2, 1, 3)[..., [0, 1, 3, 2]]).all()
    rc, xm, ym, counts, _, _ = ou.host_align(ones, yl, ones[:, :1], z((2, 1), np.int32))  # empty references in a tensor with columns
    assert rc == 0 and (xm == -1).all() and (ym == -1).all() and (counts[..., 3] == yl[:, :, None]).all()
    assert ou.host_counts(z((2, 3, 0), np.int32), z((2, 3), np.int32))[1].tolist() == z((2, 3, 3, 4), np.int32).tolist()


# ---- the sanitizer driver --------------------------------------------------------------------------------------------------------------
def _write_case(path, c, mode):
    x = np.ascontiguousarray(c["x"], np.int32)
    B, R, L = x.shape
    pairwise = mode == 1
    Q, Lq = (R, L) if pairwise else c["y"].shape[1:]
    ref = ou.case_reference(c, mode == 2)
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", B, R, L, Q, Lq, mode))
        f.write(x.tobytes())
        f.write(np.ascontiguousarray(c["x_lens"], np.int32).tobytes())
        if not pairwise:
            f.write(np.ascontiguousarray(c["y"], np.int32).tobytes())
            f.write(np.ascontiguousarray(c["y_lens"], np.int32).tobytes())
        for a in ref:
            f.write(np.ascontiguousarray(a, np.int32).tobytes())


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/editops_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own: count grids of two
    classes, map grids of three classes in both roles, slot reuse, pairwise mode and a bad length against the restatement's outputs, and
    the exactly-sized pairs the driver makes itself."""
    bad = eu.pairwise_case(7, B=2, L=40)
    bad = dict(bad, x_lens=bad["x_lens"].copy(), y=bad["x"][:, :3].copy(), y_lens=bad["x_lens"][:, :3].copy())
    bad["x_lens"][1, 0] = 41
    cases = [(eu.grid_case(1, False), 0), (eu.grid_case(4, True), 0), (eu.pairwise_case(7), 1), (eu.pairwise_case(1), 1),
             (ou.map_grid_case(1, False), 2), (ou.map_grid_case(2, True), 2), (ou.map_grid_case(8, False), 2), (ou.slot_reuse_cases()[0], 2),
             (ou.slot_reuse_cases()[1], 2), (bad, 2), (bad, 0)]
    files = []
    for k, (c, mode) in enumerate(cases):
        files.append(str(tmp_path / ("case%d.bin" % k)))
        _write_case(files[-1], c, mode)
    exe = str(tmp_path / "editops_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(eu.NATIVE, "editops_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failures" in r.stdout
