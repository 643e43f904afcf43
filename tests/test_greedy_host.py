"""Greedy decode on the CPU: the routines of ctcdecode_amd/csrc/greedy.h run sequentially (host twin, tests/native/greedy_host.cpp)
against the numpy / Python restatement of the header's definition (tests/greedy_util.py), bit for bit -- scores and label scores as
uint32, labels and frames exactly -- over the shapes the GPU tests use, the three element types and the three input modes, and a few
hundred random small cases; the rule that combines two partial winners; the shape arithmetic that picks a kernel; the stand-alone
sanitizer driver on the same cases."""
import os
import struct
import subprocess

import greedy_util as gu
import numpy as np
import pytest


def _check(c, what):
    want = gu.cached(("ref", what), lambda: gu.case_reference(c))
    got = gu.host_decode(c["stored"], c["dtype"], c["seq_lens"], c["blank"], c["mode"])
    for k in ("tokens", "starts", "ends", "lens"):
        assert not (got[k] == gu.SENTINEL).any(), "%s: a position of %s was not written" % (what, k)
    assert not (got["label_scores"].view(np.int32) == gu.SENTINEL).any(), "%s: a position of label_scores was not written" % what
    gu.assert_same(got, want, what)
    return want


@pytest.mark.parametrize("V", gu.V_LIST)
def test_twin_equals_the_restatement_over_the_label_counts(V):
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            _check(gu.shape_case(V, mode, dtype), "V %d mode %d dtype %d" % (V, mode, dtype))


@pytest.mark.parametrize("T", gu.T_LIST)
def test_twin_equals_the_restatement_over_the_frame_counts(T):
    for mode in gu.MODES:
        c = gu.shape_case(3, mode, 0, T=T)
        want = _check(c, "T %d mode %d" % (T, mode))
        assert want["lens"].max() > 0 or T == 1


def test_seq_lens_are_clamped():
    for mode in gu.MODES:
        c = gu.shape_case(5, mode, 0, T=12, B=6)
        c["seq_lens"] = np.asarray([0, 1, 7, 12, 40, -3], np.int32)
        want = _check(c, "seq_lens mode %d" % mode)
        assert want["lens"][0] == 0 and want["lens"][5] == 0 and want["scores"][0] == 0 and want["scores"][5] == 0
        full = gu.reference(c["x"], None, c["blank"], mode)
        assert np.array_equal(want["tokens"][3:5], full["tokens"][3:5]), "a length above T counts as T"
        assert want["starts"][2, : want["lens"][2]].max(initial=0) < 7


@pytest.mark.parametrize("V", sorted(gu.TIE_PATTERNS))
def test_among_equal_maxima_the_smallest_index_wins(V):
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            c = gu.tie_case(V, mode, dtype)
            want = _check(c, "ties V %d mode %d dtype %d" % (V, mode, dtype))
            labs, pats = want["labels"][0], gu.TIE_PATTERNS[V]
            assert labs[: len(pats)] == [min(p) for p in pats]
            if mode == 0:
                assert labs[len(pats):] == [0, 0, 0]
            else:
                assert labs[len(pats):] == [V // 3, V // 3, 0] and np.isneginf(want["scores"][0]), "-0.0 == +0.0; a frame of -inf gives label 0"
                assert want["tokens"][0, want["lens"][0] - 1] == 0, "label 0 is emitted where the blank is another label"


@pytest.mark.parametrize("V", [29, 1024, 10000])
def test_rounded_rows_tie_in_most_frames(V):
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            c = gu.coarse_case(V, mode, dtype, B=1 if V > 5000 else 2, T=4 if V > 5000 else 6)
            tied, frames = gu.tied_frames(c)
            assert V < 100 or tied * 2 > frames, (tied, frames)
            _check(c, "coarse V %d mode %d dtype %d" % (V, mode, dtype))


@pytest.mark.parametrize("blank", [0, 3, 5])
def test_emission(blank):
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            c, paths = gu.emission_case(blank, mode, dtype)
            want = _check(c, "emission blank %d mode %d dtype %d" % (blank, mode, dtype))
            assert want["labels"] == paths
            a = paths[3][0]
            assert want["lens"].tolist() == [0, 12, 4, 1], "all blank; no blank and no repeat; a a _ a _ _ c c c a a _; a a a ..."
            assert want["tokens"][2, :2].tolist() == [a, a] and want["starts"][2, :2].tolist() == [0, 3] and want["ends"][2, :2].tolist() == [1, 3]
            assert want["starts"][3, 0] == 0 and want["ends"][3, 0] == 11


@pytest.mark.parametrize("mode", gu.MODES)
def test_runs_across_the_chunk_boundaries(mode):
    c = gu.long_run_case(mode)
    want = _check(c, "long runs mode %d" % mode)
    spans = [set(zip(want["starts"][b, : want["lens"][b]].tolist(), want["ends"][b, : want["lens"][b]].tolist())) for b in range(3)]
    assert {(60, 63), (64, 70), (1000, 1100)} <= spans[0] and {(1010, 1023), (1024, 1040)} <= spans[1] and (5, 1195) in spans[2]
    if mode == 1:  # the earlier zero of the run
        i0 = want["starts"][0].tolist().index(1000)
        i2 = want["starts"][2].tolist().index(5)
        assert gu.bits1(want["label_scores"][0, i0]) == 0 and gu.bits1(want["label_scores"][2, i2]) == 0x80000000


@pytest.mark.parametrize("kind", ["neg_inf_log", "neg_inf_logits", "dominant", "prob_exact"])
def test_scores_at_the_edges_of_float32(kind):
    for V in (29, 1024):
        for dtype in gu.DTYPES:
            c = gu.score_case(kind, V, dtype)
            want = _check(c, "score %s V %d dtype %d" % (kind, V, dtype))
            if kind.startswith("neg_inf"):
                assert np.isneginf(want["scores"]).all() and np.isfinite(want["lps"][1][6])
            elif kind == "dominant":
                assert [gu.bits1(v) for v in want["lps"][0][:3]] == [0, 0x80000000, 0], "+0.0 - +0.0, -0.0 - +0.0, +0.0 - +0.0"
                assert [gu.bits1(v) for v in want["lps"][0][3:7]] == [0] * 4 and want["lps"][0][7] < 0, "terms near and below expf(-88) leave the sum at 1"
            else:
                assert gu.bits1(want["lps"][0][0]) == 0 and want["labels"][0][:4] == [V // 2, 0, 0, V - 1]


def test_random_small_cases():
    rng = np.random.default_rng(7)
    for i in range(300):
        B, T, V = int(rng.integers(1, 4)), int(rng.integers(0, 20)), int(rng.integers(1, 9))
        mode, dtype = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        raw = gu.random_rows(rng, B, T, V, mode, scale=3.0)
        if i % 3 == 0:  # coarse values: ties
            raw = np.round(raw * 2) / 2 if mode else np.round(raw * 4) / 4
        c = gu._case(raw.astype(np.float32), mode, dtype, int(rng.integers(0, V)), seq_lens=rng.integers(-2, T + 3, B) if i % 2 else None)
        want = gu.case_reference(c)
        got = gu.host_decode(c["stored"], dtype, c["seq_lens"], c["blank"], mode, details=bool(i % 5))
        gu.assert_same(got, want, "random %d" % i)


def test_combining_partial_winners():
    """The greater value, else the smaller index, whichever way round; "none yet" loses to everything; -0.0 == +0.0."""
    none = 0x7FFFFFFF
    for (va, ca, vb, cb, want) in ((1.0, 5, 2.0, 3, 3), (1.0, 5, 2.0, 9, 9), (1.0, 5, 1.0, 3, 3), (-0.0, 7, 0.0, 2, 2), (0.0, 7, -0.0, 9, 7),
                                   (-np.inf, none, -np.inf, 4, 4), (-np.inf, none, -np.inf, none, none), (-np.inf, 3, -np.inf, 4, 3)):
        assert gu.host_combine(va, ca, vb, cb) == want and gu.host_combine(vb, cb, va, ca) == want, (va, ca, vb, cb)


def test_shape_arithmetic():
    assert [gu.host_lanes_per_frame(v) for v in (1, 2, 3, 29, 32, 33, 63, 64, 65, 10000)] == [1, 2, 4, 32, 32, 64, 64, 64, 64, 64]
    assert [gu.host_logits_f4(v) for v in (260, 1024, 1028, 2048, 2052, 4096, 4100, 10240, 10244, 16384)] == [1, 1, 2, 2, 4, 4, 10, 10, 16, 16]
    for mode in gu.MODES:
        assert not gu.host_vec_rows(0, 256, 0, mode) and gu.host_vec_rows(0, 260, 0, mode) and not gu.host_vec_rows(0, 4098, 0, mode)
        assert not gu.host_vec_rows(4, 1024, 0, mode) and not gu.host_vec_rows(2, 1024, 1, mode), "a base one element off the boundary"
    assert gu.host_vec_rows(0, 16384, 0, 2) and not gu.host_vec_rows(0, 16388, 0, 2) and gu.host_vec_rows(0, 16388, 0, 1)
    assert gu.host_vec_rows(8, 260, 2, 2) and not gu.host_vec_rows(8, 264, 2, 1) and gu.host_vec_rows(16, 264, 2, 1) and not gu.host_vec_rows(16, 260, 2, 1)
    assert gu.host_scratch_bytes(1, 1) == 256 and gu.host_scratch_bytes(256, 1000) == 256 * 1000 * 8


def _write_case(path, c, want):
    B, T, V = c["x"].shape
    with open(path, "wb") as f:
        f.write(struct.pack("<7i", B, T, V, c["blank"], c["mode"], c["dtype"], 0 if c["seq_lens"] is None else 1))
        f.write(np.ascontiguousarray(c["stored"]).tobytes())
        if c["seq_lens"] is not None:
            f.write(np.ascontiguousarray(c["seq_lens"], np.int32).tobytes())
        for k, dt in (("tokens", np.int32), ("starts", np.int32), ("ends", np.int32), ("label_scores", np.float32), ("scores", np.float32), ("lens", np.int32)):
            f.write(np.ascontiguousarray(want[k], dt).tobytes())


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/greedy_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own: cases of every mode
    and element type against the restatement's outputs, and the rows the driver makes itself."""
    cases = [gu.shape_case(29, 1, 0), gu.shape_case(65, 2, 1), gu.shape_case(257, 0, 2), gu.tie_case(301, 2, 2), gu.tie_case(65, 0, 1), gu.long_run_case(1),
             gu.emission_case(3, 2, 0)[0], gu.score_case("dominant", 29, 0), gu.score_case("neg_inf_log", 29, 1)]
    seq = gu.shape_case(5, 1, 0, T=12, B=6)
    seq["seq_lens"] = np.asarray([0, 1, 7, 12, 40, -3], np.int32)
    files = []
    for i, c in enumerate(cases + [seq]):
        files.append(str(tmp_path / ("case%02d.bin" % i)))
        _write_case(files[-1], c, gu.case_reference(c))
    exe = str(tmp_path / "greedy_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(gu.NATIVE, "greedy_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failures" in r.stdout
