"""The label posteriors on the CPU: the routines of ctcdecode_amd/csrc/posterior.h run sequentially (host twin,
tests/native/posterior_host.cpp) against the Python restatement of the header's definition (tests/posterior_util.py), bit for bit as
uint32; the restatement against a float64 forward-backward; what the three new cases are named for; the input modes and dtypes; the
slot and grid arithmetic; the stand-alone sanitizer driver on the same cases."""
import os
import struct
import subprocess

import align_util as au
import loglik_util as lu
import numpy as np
import posterior_util as pu
import pytest

# The twin runs a row state by state, whatever its size: the sweeps over dtypes and modes leave out the one case whose restatement
# takes seconds (T 514, S 1025), which the float32 test covers.
SWEEP = [n for n in pu.CASES if n != "many_per_lane"]


@pytest.mark.parametrize("name", pu.CASES)
def test_twin_equals_the_restatement(name):
    c, want = pu.case(name)
    got = pu.host_posteriors(c["lp"], c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    assert got["invalid_rows"] == 0 and want["valid"].all()
    for k in pu.KEYS:  # a pre-filled output is written everywhere
        assert not (got[k] == (0x5A5A5A5A if k == "peaks" else np.float32(-123.0))).any(), k
    pu.assert_same(got, want, name)


@pytest.mark.parametrize("name", pu.CASES)
def test_loglik_is_the_log_likelihood(name):
    """The fourth output against loglik_util's restatement of "CTC log-likelihood", computed on its own."""
    c, want = pu.case(name)
    ref = lu.case(name)[1] if name in lu.CASES else lu.reference(c["lp"], c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    lu.assert_same(want["loglik"], ref, name)
    assert want["status"].tolist() == ref["status"].tolist()


# What the float32 restatement was seen to differ by from the float64 one on these cases (the largest over all of them; many_per_lane
# sets each: 514 frames of sums near -700), and what is allowed: four times that.
#   occupancy   2.065e-2 frames          -> 8.26e-2      (the cases of at most 45 frames: 6.2e-4)
#   confidence  4.99e-5                  -> 2.0e-4       (the cases of at most 45 frames: 3.1e-6)
#   peaks       g64[float64's peak] - g64[float32's peak]: 2.66e-4 -> 1.07e-3
SEEN = dict(occupancy=2.065e-2, confidence=4.99e-5, peak_gap=2.66e-4)
ALLOWED = {k: 4.0 * v for k, v in SEEN.items()}


@pytest.mark.parametrize("name", pu.CASES)
def test_restatement_agrees_with_float64(name):
    """A sanity check of the definition, not a definition: occupancy and confidence against a float64 numpy.logaddexp forward-backward,
    and the float32 peak a (near-)maximum of the float64 posterior.  Rows that touch the overflow case's values near -3e38 are left out:
    their float32 sums overflow to -inf where float64's do not."""
    c, want = pu.case(name)
    B, T, _ = c["lp"].shape
    seen = dict(occupancy=0.0, confidence=0.0, peak_gap=0.0)
    rows = 0
    for b in range(B):
        n = T if c["seq_lens"] is None else min(max(int(c["seq_lens"][b]), 0), T)
        for r in range(c["tokens"].shape[1]):
            L = int(c["lens"][b, r])
            y = c["tokens"][b, r, :L]
            if L == 0 or (np.isfinite(c["lp"][b, :n]) & (c["lp"][b, :n] < -1e37)).any():
                continue
            g, occ, conf, ll = pu.posteriors64(c["lp"][b], n, y, c["blank"])
            assert np.isfinite(ll) == bool(np.isfinite(want["loglik"][b, r])), (name, b, r)
            if not np.isfinite(ll):
                assert not want["occupancy"][b, r].any() and not want["confidence"][b, r].any() and not want["peaks"][b, r].any()
                continue
            rows += 1
            seen["occupancy"] = max(seen["occupancy"], float(np.abs(want["occupancy"][b, r, :L] - occ).max()))
            seen["confidence"] = max(seen["confidence"], float(np.abs(want["confidence"][b, r, :L] - conf).max()))
            seen["peak_gap"] = max(seen["peak_gap"], float((g.max(0) - g[want["peaks"][b, r, :L], np.arange(L)]).max()))
            conf32 = want["confidence"][b, r, :L]
            assert ((conf32 >= 0) & (conf32 <= 1)).all(), (name, b, r)
    print("%s: %d rows, largest differences %s, allowed %s" % (name, rows, seen, ALLOWED))
    for k in seen:
        assert seen[k] <= ALLOWED[k], (name, k, seen[k], ALLOWED[k])
    if name not in ("one_frame", "overflow"):
        assert rows >= 1, "the check passed on nothing"


def test_the_new_cases_cover_what_they_are_named_for():
    c, want = pu.case("dyadic_single_path")
    B, T, _ = c["lp"].shape
    assert (c["lp"] * 4 == np.round(c["lp"] * 4)).all()
    for b in range(B):
        n = int(c["seq_lens"][b])
        for r in range(c["tokens"].shape[1]):
            L = int(c["lens"][b, r])
            y = c["tokens"][b, r, :L]
            assert L == n and all(y[i] != y[i - 1] for i in range(1, L)), "one alignment"
            assert want["occupancy"][b, r, :L].view(np.uint32).tolist() == [0x3F800000] * L, "occupancy == 1.0f"
            assert want["peaks"][b, r, :L].tolist() == list(range(L))
            for i in range(L):
                assert want["confidence"][b, r, i].view(np.uint32) == lu.expf(c["lp"][b, i, y[i]]).view(np.uint32), (b, r, i)
            assert want["loglik"][b, r].view(np.uint32) == lu.path_sum(c, b, r, n).view(np.uint32)
    for name in ("clamped", "forty_rows", "far_apart"):
        assert pu.case(name)[1]["diag"]["clamped"] >= 1, name + ": the restatement forms x > 0 at least once"
    c, want = pu.case("subnormal")
    assert want["diag"].get("subnormal", 0) >= 1, "the restatement forms a subnormal product"
    g0 = pu.posteriors64(c["lp"][0], 2, [1], 0)[0][0, 0]
    assert np.exp(-41.0) < g0 < np.exp(-38.0) and c["lp"][0, 0, 1] == -55.0, "g near e^-40 meets e80(lp) near e^-55"
    assert np.isfinite(want["loglik"]).sum() >= 6 and (want["confidence"][:, 0, 0] > 0.1).all()


def test_e80_and_g_of_the_twin_equal_the_restatement():
    rng = np.random.default_rng(12)
    xs = [np.float32(v) for v in (-np.inf, -0.0, 0.0, 1e-7, 5.0, -80.0, np.nextafter(np.float32(-80), np.float32(-81)), np.nextafter(np.float32(-80), np.float32(0)),
                                  -87.0, -3e38, -40.0, -55.0)]
    xs += [np.float32(v) for v in -rng.random(2000) * rng.choice([1.0, 10.0, 100.0], 2000)]
    for x in xs:
        assert pu.host_e80(x).view(np.uint32) == pu.e80(x).view(np.uint32), x
    assert pu.e80(np.float32(3.0)) == 1 and pu.e80(np.float32(-80.0)) > 0 and pu.e80(np.float32(-80.001)) == 0
    assert pu.host_g(-np.inf, -1.0, -1.0, -2.0) == 0 and pu.host_g(-1.0, -np.inf, -1.0, -2.0) == 0 and pu.host_g(-3e38, -3e38, -1.0, -2.0) == 0
    with np.errstate(all="ignore"):
        for _ in range(500):
            a, b, lp, ll = (np.float32(v) for v in -rng.random(4) * 50)
            want = pu.e80(np.float32(np.float32(np.float32(a + b) - lp) - ll))
            assert pu.host_g(a, b, lp, ll).view(np.uint32) == want.view(np.uint32)


@pytest.mark.parametrize("name", SWEEP)
def test_half_rows_are_read_as_their_float_copies(name):
    c, _ = pu.case(name)
    with np.errstate(over="ignore"):  # (the overflow case's values become -inf)
        h = c["lp"].astype(np.float16)
    want = pu.reference(h.astype(np.float32), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    pu.assert_same(pu.host_posteriors(h.view(np.uint16), c["seq_lens"], c["tokens"], c["lens"], c["blank"], dtype=1), want, "f16")
    bits = au.to_bf16_bits(c["lp"])
    want = pu.reference(au.bf16_bits_to_f32(bits), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    pu.assert_same(pu.host_posteriors(bits, c["seq_lens"], c["tokens"], c["lens"], c["blank"], dtype=2), want, "bf16")


@pytest.mark.parametrize("name", SWEEP)
def test_probability_mode_equals_math_log_per_element(name):
    """log_input == 0 on probabilities drawn for the case's shape and labels, two of them 0 (log(FLT_MIN): finite); raw logits reach
    the twin as the log-softmax rows, which is the log-probability mode of every other test."""
    c, _ = pu.case(name)
    rng = np.random.default_rng(5)
    p = rng.random(c["lp"].shape).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    p[0, 0, 1] = 0.0
    p[-1, -1, :] = 0.0
    want = pu.reference(au.prob_to_lp(p), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    pu.assert_same(pu.host_posteriors(p, c["seq_lens"], c["tokens"], c["lens"], c["blank"], log_input=0), want, "probabilities")


def test_invalid_rows_raise_their_item_alone():
    c, want = pu.case("blank_mid")
    V, blank = c["lp"].shape[2], c["blank"]
    r0 = int(np.argmax(c["lens"][0] > 1))
    for what, edit in (("label = V", lambda t, l: t.__setitem__((0, r0, 1), V)), ("label = blank", lambda t, l: t.__setitem__((0, r0, 0), blank)),
                       ("label < 0", lambda t, l: t.__setitem__((0, r0, 0), -7)), ("length < 0", lambda t, l: l.__setitem__((0, r0), -1)),
                       ("length > L_stride", lambda t, l: l.__setitem__((0, r0), t.shape[2] + 1))):
        tok, lens = c["tokens"].copy(), c["lens"].copy()
        edit(tok, lens)
        got = pu.host_posteriors(c["lp"], c["seq_lens"], tok, lens, blank)
        ref = pu.reference(c["lp"], c["seq_lens"], tok, lens, blank)
        assert got["invalid_rows"] == 1 and got["status"].tolist() == [pu.BAD_ROW, 0], what
        assert not ref["valid"][0, r0] and all(not got[k][0, r0].any() for k in pu.KEYS), what
        pu.assert_same(got, ref, what)
        keep = np.ones(c["lens"].shape, bool)
        keep[0, r0] = False
        for k in pu.KEYS:
            assert np.array_equal(got[k][keep].view(np.uint32), want[k][keep].view(np.uint32)), (what, k)


def test_slot_and_grid_arithmetic():
    """A slot: T x (2 min(L_stride, T) + 1) floats, or T x 4 x 64 for four one-wave rows, whichever is larger, rounded up to 256 bytes;
    the grid: min(rows, budget / slot), at least one; the default budget pays for 256 slots at T = L_stride = 1000."""
    def slot(T, Ls):
        S = 2 * min(Ls, T) + 1
        return (T * max(S, 256) * 4 + 255) // 256 * 256

    for T, Ls in ((0, 0), (1, 1), (1, 0), (37, 37), (45, 45), (130, 130), (130, 12), (12, 130), (514, 514), (1000, 1000), (2047, 2047), (5000, 2047), (127, 500), (128, 128)):
        assert pu.host_slot_bytes(T, Ls) == slot(T, Ls), (T, Ls)
        assert pu.host_slot_bytes(T, Ls) % 256 == 0 and pu.host_slot_bytes(T, Ls) >= 4 * 4 * pu.host_wave_floats(T) >= 4 * 4 * 63 * T
    assert pu.host_wave_floats(37) == 37 * 64
    default = pu.host_default_scratch()
    assert default == 2 << 30
    s1000 = pu.host_slot_bytes(1000, 1000)
    assert 8.0e6 <= s1000 <= 8.01e6 and pu.host_grid(10 ** 6, 0, s1000) >= 256, "one workgroup per compute unit at T = L_stride = 1000"
    assert pu.host_grid(10 ** 6, 0, s1000) == default // s1000 and pu.host_grid(100, 0, s1000) == 100
    s = pu.host_slot_bytes(45, 45)
    assert pu.host_grid(40, 3 * s, s) == 3 and pu.host_grid(40, 3 * s + s - 1, s) == 3 and pu.host_grid(40, s, s) == 1 and pu.host_grid(40, 1, s) == 1
    assert pu.host_grid(2, 3 * s, s) == 2 and pu.host_grid(0, 0, s) == 1 and pu.host_grid(5, 0, 0) == 5
    big = pu.host_slot_bytes(5000, 2047)
    assert big == 5000 * 4095 * 4 + (-(5000 * 4095 * 4) % 256) and pu.host_grid(10 ** 4, 0, big) == default // big >= 1


def _write_case(path, c, want, log_input=1):
    B, T, V = c["lp"].shape
    R, Ls = c["tokens"].shape[1:]
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", B, T, V, R, Ls, c["blank"], log_input, 0, 0 if c["seq_lens"] is None else 1))
        f.write(np.ascontiguousarray(c["lp"], np.float32).tobytes())
        if c["seq_lens"] is not None:
            f.write(np.ascontiguousarray(c["seq_lens"], np.int32).tobytes())
        for a, dt in ((c["tokens"], np.int32), (c["lens"], np.int32), (want["peaks"], np.int32), (want["occupancy"], np.float32), (want["confidence"], np.float32),
                      (want["loglik"], np.float32), (want["status"], np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/posterior_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own: the cases above
    against the restatement's outputs, one of them with out-of-range labels and lengths, and the rows the driver makes itself."""
    files = []
    for name in pu.CASES:
        c, want = pu.case(name)
        files.append(str(tmp_path / (name + ".bin")))
        _write_case(files[-1], c, want)
    c, _ = pu.case("blank_mid")
    tok, lens = c["tokens"].copy(), c["lens"].copy()
    tok[0, 0, 0], tok[1, 1, 0], lens[0, 2], lens[1, 3] = c["lp"].shape[2], c["blank"], -3, tok.shape[2] + 5
    lens[0, 0], lens[1, 1] = max(lens[0, 0], 1), max(lens[1, 1], 1)
    bad = dict(c, tokens=tok, lens=lens)
    want = pu.reference(bad["lp"], bad["seq_lens"], tok, lens, bad["blank"])
    assert want["status"].tolist() == [pu.BAD_ROW, pu.BAD_ROW]
    files.append(str(tmp_path / "invalid.bin"))
    _write_case(files[-1], bad, want)
    exe = str(tmp_path / "posterior_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(pu.NATIVE, "posterior_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failures" in r.stdout
