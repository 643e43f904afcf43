"""The lattice matrix on the CPU (tests/lattice_matrix_util.py): the matrix case holds what it is built for -- values exact in every
element type, rows of all four kernel classes by the documented rule -- and on it, on the limit case (S = 4095), on the third-wave case
and on the wide vocabulary the host twins of align.h / loglik.h / posterior.h (tests/native/*_host.cpp) equal the restatements of the
header's definitions bit for bit, for all six (element type, input mode) pairs; the closed form the limit case is checked against equals
the three restatements at L = n = 300.  The references are those of tests/test_gpu_lattice_matrix.py, computed once per process."""
import align_util as au
import lattice_matrix_util as mu
import numpy as np
import posterior_util as pu
import pytest


@pytest.fixture(scope="module", autouse=True)
def _references_released_afterwards():
    """The cases and their references live for this module's tests only: the tests that run after it find the process as it was."""
    yield
    import gc

    mu.release()
    gc.collect()


def test_the_matrix_values_are_exact_in_every_element_type():
    c = mu.case("matrix")
    for dt in mu.DTYPES:
        assert mu.exact_in(c["lp"], dt) and mu.exact_in(c["p"], dt), dt
    assert (c["lp"] * 8 == np.round(c["lp"] * 8)).all() and c["lp"].min() == -6.0 and c["lp"].max() == 0.0
    assert (c["p"] * 256 == np.round(c["p"] * 256)).all() and 0.0 <= c["p"].min() and c["p"].max() < 1.0
    zeros = float((c["p"] == 0).mean())
    assert 0.002 <= zeros <= 0.012, "about 0.2 % of the entries were set to 0, besides those drawn as 0 / 256"
    assert tuple(c["lp"].shape) == (4, 518, 5) and tuple(c["tokens"].shape) == (4, 4, 518) and int(c["lens"].sum()) == 1718


def test_the_matrix_holds_every_class_in_one_launch():
    """The census, from the documented rule: each of the classes 0, 1, 4 and 16 owns at least one row that runs the recurrence; the
    sizes next to the thresholds are there; the all-short group lies inside one item and every row of it runs the recurrence."""
    c = mu.case("matrix")
    rows, groups = mu.census(c)
    R = c["tokens"].shape[1]
    for cls in (0, 1, 4, 16):
        assert len(rows[cls]) >= 1, "no row of class %d" % cls
    S = {cls: sorted(s for _, _, s in rows[cls]) for cls in rows}
    assert S[16] == [1027] and S[4] == [393, 401, 1021] and S[0] == [5, 57, 61, 63]
    assert 65 in S[1] and min(S[1]) <= 64 and max(S[1]) <= 256, "class 1: S = 65, and a short row inside a long group"
    assert sum(len(v) for v in rows.values()) == 16, "all 16 rows run the recurrence"
    assert [short for _, short, _ in groups] == [False, False, False, True]
    g0, _, states = groups[0]
    assert {mu_cls(s) for s in states} == {16, 4, 1}, "group 0: a class-16 row, a class-4 row and rows of one state per lane"
    for g0, short, states in groups:
        if short:
            assert g0 // R == (g0 + 3) // R and all(s is not None for s in states) and len(states) == 4
    # the shape allows every class: launch_classes goes by 2 * min(L_stride, T) + 1
    assert 2 * min(c["tokens"].shape[2], c["lp"].shape[1]) + 1 > 1024
    # and the half-type and probability tests of test_gpu_align / _loglik / _posterior stay within class 0: this file's reason to be
    for name in ("blank_last", "ties_half"):
        o = au.make_case(name)
        assert 2 * min(o["tokens"].shape[2], o["lp"].shape[1]) + 1 <= 64, name


def mu_cls(S):
    return 1 if S <= 256 else (4 if S <= 1024 else 16)


@pytest.mark.parametrize("mode", mu.MODES)
@pytest.mark.parametrize("dtype", mu.DTYPES)
@pytest.mark.parametrize("feature", mu.FEATURES)
def test_twin_equals_the_restatement_on_the_matrix(feature, dtype, mode):
    c = mu.case("matrix")
    want = mu.want("matrix", feature, mode)
    got = mu.host(feature, c, c["lp"] if mode == "log" else c["p"], dtype, mode)
    mu.ASSERT_SAME[feature](got, want, "matrix %s %s %s" % (feature, dtype, mode))
    print("reference times (s):", {k: round(v, 2) for k, v in mu.TIMES.items()})


def test_the_single_path_identity_at_300():
    """What the limit case is checked against, against all three restatements at a size they run in about a second."""
    c = mu.single_path_case(300)
    exp = mu.single_path_expected(c)
    for dt in mu.DTYPES:
        assert mu.exact_in(c["lp"], dt), dt
    for feature in mu.FEATURES:
        want = mu.REFERENCE[feature](c["lp"], c["seq_lens"], c["tokens"], c["lens"], c["blank"])
        mu.ASSERT_SAME[feature](exp[feature], want, "single path, " + feature)
    assert (exp["posteriors"]["occupancy"].view(np.uint32) == 0x3F800000).all() and (exp["align"]["start"][0, 1] == np.arange(300)).all()
    assert np.isfinite(exp["loglik"]["loglik"]).all() and (exp["loglik"]["loglik"] < 0).all()


@pytest.mark.parametrize("dtype", mu.DTYPES)
def test_twins_at_the_limit(dtype):
    """max_states: L = n = 2047, S = 4095, the most the entry points accept; the twins against the closed form."""
    c = mu.case("max_states")
    assert c["lp"].shape == (1, 2047, 4) and c["lens"].tolist() == [[2047, 2047]] and mu.exact_in(c["lp"], dtype)
    assert au.host_npl(4095) == 16 and pu.host_slot_bytes(2047, 2047) == 2047 * 4095 * 4 + (-(2047 * 4095 * 4) % 256)
    exp = mu.max_states_expected()
    for feature in mu.FEATURES:
        mu.ASSERT_SAME[feature](mu.host(feature, c, c["lp"], dtype), exp[feature], "max_states %s %s" % (feature, dtype))


def test_twins_on_the_third_wave():
    """third_wave: S = 2061, states 2048 .. 2060 lie in the workgroup's third wave (lane 128 at 16 states per lane), and the row has
    many alignments: its log-likelihood exceeds its best path's score."""
    c = mu.case("third_wave")
    L, n = int(c["lens"][0, 0]), c["lp"].shape[1]
    assert 2 * L + 1 == 2061 and n == 1040 and (2 * L) // 16 == 128
    want = {f: mu.want("third_wave", f) for f in mu.FEATURES}
    print("reference times (s):", {k: round(v, 2) for k, v in mu.TIMES.items() if k[0] == "third_wave"})
    ll, sc = want["loglik"]["loglik"][0, 0], want["align"]["scores"][0, 0]
    assert np.isfinite(sc) and ll > sc + 1.0, "many alignments"
    assert (want["posteriors"]["occupancy"][0, 0, :L] > 0).all() and want["posteriors"]["peaks"][0, 0, L - 1] >= L - 1
    for feature in mu.FEATURES:
        mu.ASSERT_SAME[feature](mu.host(feature, c, c["lp"]), want[feature], "third_wave " + feature)


@pytest.mark.parametrize("variant", ["log", "prob", "float16", "bfloat16"])
def test_twins_on_the_wide_vocabulary(variant):
    """big_vocab: V = 70001, labels on both sides of 2^8 and 2^16, blank 69999.  The half variants are checked against the restatement
    on the half copy widened back, as the half tests of the three features do."""
    c = mu.case("big_vocab")
    assert c["lp"].shape == (2, 12, 70001) and c["blank"] == 69999 and set(mu.used_columns(c)) == set(mu.BIG_VOCAB_LABELS) | {69999}
    for feature in mu.FEATURES:
        if variant in ("log", "prob"):
            want = mu.want("big_vocab", feature, variant)
            got = mu.host(feature, c, c["lp"] if variant == "log" else c["p"], "float32", variant)
        else:
            h = mu.widen(mu.half_bits(c["lp"], variant), variant)
            want = mu.reference_on("big_vocab", feature, variant, h)
            got = mu.host(feature, c, c["lp"], variant)
        finite = want["scores"] if feature == "align" else want["loglik"]
        assert np.isfinite(finite).sum() >= 8 and np.isfinite(finite[0, 0]), "rows with alignments, the one of all eight labels among them"
        mu.ASSERT_SAME[feature](got, want, "big_vocab %s %s" % (feature, variant))
