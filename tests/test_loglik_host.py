"""The CTC log-likelihood on the CPU: the routines of ctcdecode_amd/csrc/loglik.h run sequentially (host twin,
tests/native/loglik_host.cpp) against the Python restatement of the header's definition (tests/loglik_util.py), bit for bit as uint32;
the restatement against a float64 recurrence; single-path rows against the plain sum of their log-probabilities; the input modes; the
grid arithmetic; the stand-alone sanitizer driver on the same cases."""
import os
import struct
import subprocess

import align_util as au
import loglik_util as lu
import numpy as np
import pytest


@pytest.mark.parametrize("name", lu.CASES)
def test_twin_equals_the_restatement(name):
    c, want = lu.case(name)
    got = lu.host_loglik(c["lp"], c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    assert got["invalid_rows"] == 0 and want["valid"].all()
    lu.assert_same(got, want, name)


@pytest.mark.parametrize("name", lu.CASES)
def test_restatement_within_the_float32_bound_of_float64(name):
    """|ll32 - ll64| <= n * 2^-23 * (A + 3) on every finite row, A the largest finite |a| of the float64 recurrence: per frame a cell
    gains at most about one ulp of its value from the two additions and one ulp of at most log 3 from logf; the factor 2 is the margin.
    (Rows of the overflow case whose float32 value overflowed to -inf are not finite rows.)"""
    c, want = lu.case(name)
    B, T, _ = c["lp"].shape
    finite, worst = 0, 0.0
    for b in range(B):
        n = T if c["seq_lens"] is None else min(max(int(c["seq_lens"][b]), 0), T)
        for r in range(c["tokens"].shape[1]):
            ll32 = want["loglik"][b, r]
            L = int(c["lens"][b, r])
            ll64, A = lu.forward64(c["lp"][b], n, c["tokens"][b, r, :L], c["blank"])
            if not np.isfinite(ll32):
                assert np.isneginf(ll32) and (np.isneginf(ll64) or A > 1e38), (name, b, r, ll32, ll64)
                continue
            finite += 1
            bound = n * 2.0 ** -23 * (A + 3.0)
            assert abs(float(ll32) - ll64) <= bound, (name, b, r, float(ll32), ll64, bound)
            worst = max(worst, abs(float(ll32) - ll64) / bound if bound else 0.0)
    print("%s: %d finite rows, worst |ll32 - ll64| / bound = %.4f" % (name, finite, worst))
    assert finite >= 1, "the check passed on nothing"


def test_the_new_cases_cover_what_they_are_named_for():
    c, want = lu.case("zeros")
    ll = want["loglik"]
    assert np.signbit(c["lp"][0]).all() and not np.signbit(c["lp"][1]).any()
    for r in (0, 4):  # single-path rows of -0.0 values: logf(1) + m = +0 + -0.0 = +0.0, where the plain sum is -0.0
        assert ll[0, r] == 0 and not np.signbit(ll[0, r]) and np.signbit(lu.path_sum(c, 0, r, 6)), r
    assert ll[1, 1] == lu.logf(np.float32(6.0)) or ll[1, 1] > 1.0, "six alignments of one label over zeros"
    assert np.isneginf(ll[:, 3]).sum() == 0 and np.isfinite(ll).all()
    c, want = lu.case("far_apart")
    gaps = [float(c["lp"][b, 0, 1] - c["lp"][b, 0, 0]) for b in range(6)]
    assert gaps == [-87.5, -88.5, -200.0, 87.5, 88.5, 200.0]
    assert lu.expf(np.float32(-87.5)) > 0 and lu.lse3(np.float32(-1.0), np.float32(-88.5), lu.NEG_INF) == np.float32(-1.0)
    assert np.isfinite(want["loglik"]).all()
    c, want = lu.case("positive")
    assert (c["lp"] > 0).mean() > 0.3 and (want["loglik"] > 0).any() and np.isfinite(want["loglik"]).all()
    c, want = lu.case("overflow")
    ll = want["loglik"]
    assert np.isfinite(c["lp"]).all() and np.isneginf(ll[1]).all() and ll[0, 0] > -100, "item 1: every sum of two frames overflows"
    assert np.isfinite(ll[0, 1]) and ll[0, 1] < -1e38 and np.isneginf(ll[0, 4]), "item 0: one frame on label 2 is finite, two overflow"
    assert np.isfinite(ll[2, 5]) and np.isneginf(ll[2, 3]), "item 2: the row that needs no blank is finite, the empty row overflows"


def test_lse3_of_the_twin_equals_the_restatement():
    rng = np.random.default_rng(11)
    vals = [lu.NEG_INF] + [np.float32(v) for v in (-0.0, 0.0, -1.0, -87.5, -88.0, -88.5, -103.9, -104.5, -200.0, -3e38, 4.0)]
    trips = [(a, b, c) for a in vals for b in vals for c in vals]
    trips += [tuple(np.float32(v) for v in -rng.random(3) * rng.choice([1.0, 10.0, 100.0])) for _ in range(2000)]
    with np.errstate(all="ignore"):
        for t in trips:
            g, w = lu.host_lse3(*t), lu.lse3(*t)
            assert g.view(np.uint32) == w.view(np.uint32), (t, g, w)


def test_single_path_rows_are_the_sum_of_their_log_probabilities():
    """L == 0, and L == n without adjacent repeats: one alignment, and every cell on it has one finite predecessor m, so the cell is
    lp + (+0 + m) and the likelihood's bits are those of the float32 sum in frame order (no running value of these cases is -0.0)."""
    seen = 0
    for name in ("edges", "one_frame", "workgroup_edge", "neg_inf", "blank_last", "far_apart", "positive"):
        c, want = lu.case(name)
        for b, r, n in lu.single_path_rows(c):
            s = lu.path_sum(c, b, r, n)
            assert want["loglik"][b, r].view(np.uint32) == s.view(np.uint32), (name, b, r, want["loglik"][b, r], s)
            seen += 1
    assert seen >= 12, seen


def test_probability_mode_equals_math_log_per_element():
    c, _ = lu.case("ties_half")
    rng = np.random.default_rng(5)
    p = rng.random(c["lp"].shape).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    p[0, 3, 1] = 0.0  # log(FLT_MIN): finite
    p[1, 2, :] = 0.0
    want = lu.reference(au.prob_to_lp(p), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    lu.assert_same(lu.host_loglik(p, c["seq_lens"], c["tokens"], c["lens"], c["blank"], log_input=0), want, "probabilities")
    assert np.isfinite(want["loglik"]).sum() >= 20


def test_half_rows_are_read_as_their_float_copies():
    c, _ = lu.case("blank_last")
    h = c["lp"].astype(np.float16)
    want = lu.reference(h.astype(np.float32), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    lu.assert_same(lu.host_loglik(h.view(np.uint16), c["seq_lens"], c["tokens"], c["lens"], c["blank"], dtype=1), want, "f16")
    bits = au.to_bf16_bits(c["lp"])
    want = lu.reference(au.bf16_bits_to_f32(bits), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    lu.assert_same(lu.host_loglik(bits, c["seq_lens"], c["tokens"], c["lens"], c["blank"], dtype=2), want, "bf16")


def test_invalid_rows_raise_their_item_alone():
    c, want = lu.case("blank_mid")
    V, blank = c["lp"].shape[2], c["blank"]
    r0 = int(np.argmax(c["lens"][0] > 1))
    for what, edit in (("label = V", lambda t, l: t.__setitem__((0, r0, 1), V)), ("label = blank", lambda t, l: t.__setitem__((0, r0, 0), blank)),
                       ("label < 0", lambda t, l: t.__setitem__((0, r0, 0), -7)), ("length < 0", lambda t, l: l.__setitem__((0, r0), -1)),
                       ("length > L_stride", lambda t, l: l.__setitem__((0, r0), t.shape[2] + 1))):
        tok, lens = c["tokens"].copy(), c["lens"].copy()
        edit(tok, lens)
        got = lu.host_loglik(c["lp"], c["seq_lens"], tok, lens, blank)
        ref = lu.reference(c["lp"], c["seq_lens"], tok, lens, blank)
        assert got["invalid_rows"] == 1 and got["status"].tolist() == [lu.BAD_ROW, 0], what
        assert got["loglik"][0, r0] == 0 and not ref["valid"][0, r0], what
        lu.assert_same(got, ref, what)
        keep = np.ones(c["lens"].shape, bool)
        keep[0, r0] = False
        assert np.array_equal(got["loglik"][keep].view(np.uint32), want["loglik"][keep].view(np.uint32)), what


def test_grid_arithmetic():
    """Units: groups of four rows (class 0) or rows; the grid: min(units, cap), the default cap = compute units x the workgroups the
    class's registers allow on one; at least one."""
    assert [lu.host_units(n, 0) for n in (1, 4, 5, 40, 41)] == [1, 1, 2, 10, 11] and [lu.host_units(n, c) for n in (1, 40) for c in (1, 4, 16)] == [1] * 3 + [40] * 3
    occ = {c: lu.host_occupancy(c) for c in (0, 1, 4, 16)}
    assert all(1 <= v <= 8 for v in occ.values()) and occ[16] <= occ[4] <= occ[1]
    for c in (0, 1, 4, 16):
        assert lu.host_grid(10 ** 6, 0, 256, c) == 256 * occ[c] and lu.host_grid(10 ** 6, 0, 1, c) == occ[c]
        assert lu.host_grid(10, 0, 256, c) == 10 and lu.host_grid(10, 3, 256, c) == 3 and lu.host_grid(10, 1, 256, c) == 1 and lu.host_grid(2, 3, 256, c) == 2
        assert lu.host_grid(1, 0, 0, c) == 1 and lu.host_grid(0, 0, 256, c) == 1, "never an empty grid"
    assert lu.host_grid(25600, 0, 256, 1) == 256 * occ[1]


def _write_case(path, c, want, log_input=1):
    B, T, V = c["lp"].shape
    R, Ls = c["tokens"].shape[1:]
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", B, T, V, R, Ls, c["blank"], log_input, 0, 0 if c["seq_lens"] is None else 1))
        f.write(np.ascontiguousarray(c["lp"], np.float32).tobytes())
        if c["seq_lens"] is not None:
            f.write(np.ascontiguousarray(c["seq_lens"], np.int32).tobytes())
        for a, dt in ((c["tokens"], np.int32), (c["lens"], np.int32), (want["loglik"], np.float32), (want["status"], np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/loglik_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own: the cases above against
    the restatement's outputs, one of them with out-of-range labels and lengths, and the rows the driver makes itself."""
    files = []
    for name in lu.CASES:
        c, want = lu.case(name)
        files.append(str(tmp_path / (name + ".bin")))
        _write_case(files[-1], c, want)
    c, _ = lu.case("blank_mid")
    tok, lens = c["tokens"].copy(), c["lens"].copy()
    tok[0, 0, 0], tok[1, 1, 0], lens[0, 2], lens[1, 3] = c["lp"].shape[2], c["blank"], -3, tok.shape[2] + 5
    lens[0, 0], lens[1, 1] = max(lens[0, 0], 1), max(lens[1, 1], 1)
    bad = dict(c, tokens=tok, lens=lens)
    want = lu.reference(bad["lp"], bad["seq_lens"], tok, lens, bad["blank"])
    assert want["status"].tolist() == [lu.BAD_ROW, lu.BAD_ROW]
    files.append(str(tmp_path / "invalid.bin"))
    _write_case(files[-1], bad, want)
    exe = str(tmp_path / "loglik_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(lu.NATIVE, "loglik_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failures" in r.stdout
