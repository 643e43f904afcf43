"""Pins the CPU restatement (oracle/ctc_oracle.cpp) to the reference.

(a) the reference's own golden strings (tests/test_decode.py:31-32 of the reference),
(b) the survey's known-answer table,
(c) the committed fixtures produced by the real reference build (tests/golden, tests/golden/make_golden.py),
(d) live differential runs against oracle/_ref where it is built, else against its stored results (tests/golden/live).
"""
import os

import numpy as np
import pytest

import golden_util as gu
import oracle_util as ou

VOCAB = ["'", " ", "a", "b", "c", "d", "_"]


def _string(r, b, p):
    return "".join(VOCAB[x] for x in r["tokens"][b, p, : r["lens"][b, p]])


def test_reference_golden_strings():
    args, _ = gu.load("ref_fixtures_prob")
    r = ou.decode(which="restated", **args)
    assert _string(r, 0, 0) == "acdc"  # tests/test_decode.py:32, test_beam_search_decoder_1
    assert _string(r, 1, 0) == "b'a"   # test_beam_search_decoder_2
    args, _ = gu.load("ref_fixtures_log")  # test_beam_search_decoder_batch_log
    r = ou.decode(which="restated", **args)
    assert (_string(r, 0, 0), _string(r, 1, 0)) == ("acdc", "b'a")


def test_survey_known_answers():
    args, _ = gu.load("ref_fixtures_prob")
    r = ou.decode(which="restated", **args)
    want = [(0, 0, 6.480284, "acdc", [0, 1, 4, 5]), (0, 1, 6.483004, "acd ", [0, 1, 4, 5]), (0, 2, 6.521161, "acda", [0, 1, 4, 5]),
            (1, 0, 4.989980, "b'a", [0, 2, 4]), (1, 1, 5.298550, "b'da", [0, 2, 3, 4]), (1, 2, 5.337018, "b' a", [0, 2, 3, 4])]
    for b, p, sc, s, ts in want:
        assert _string(r, b, p) == s
        assert abs(float(r["scores"][b, p]) - sc) < 1e-5
        assert r["timesteps"][b, p, : len(ts)].tolist() == ts
    assert r["nres"].tolist() == [20, 20]


@pytest.mark.parametrize("name", gu.names())
def test_restatement_matches_committed_reference_fixtures(name):
    args, want = gu.load(name)
    got = ou.decode(which="restated", **args)
    ou.assert_same(got, want, name)


@pytest.mark.skipif(not ou.have_reference(), reason="oracle/_ref not built (needs the reference checkout)")
@pytest.mark.parametrize("name", gu.names())
def test_fixtures_reproduce_from_live_reference(name):
    args, want = gu.load(name)
    got = ou.decode(which="reference", **args)
    ou.assert_same(got, want, name)


CASES = [
    dict(B=3, T=90, V=29, K=10, seed=11),
    dict(B=2, T=250, V=29, K=64, seed=12),
    dict(B=2, T=200, V=29, K=50, seed=13, quant=0.5),
    dict(B=2, T=150, V=5, K=30, seed=14, quant=1.0, blank_id=2),
    dict(B=2, T=150, V=29, K=20, seed=15, blank_bias=5.0),
    dict(B=2, T=60, V=200, K=16, seed=16, top_n=12),
    dict(B=1, T=500, V=29, K=100, seed=17),
    # vocabulary pruning as implemented (decoder_utils.cpp:10-45): the cumulative cut really triggers below ln 2
    dict(B=2, T=120, V=29, K=24, seed=18, top_n=40, cutoff_prob=0.5),
    dict(B=2, T=120, V=29, K=24, seed=19, top_n=10, cutoff_prob=0.6),
    dict(B=2, T=100, V=40, K=16, seed=20, top_n=6, prob_input=True),
    dict(B=2, T=100, V=40, K=16, seed=21, top_n=40, cutoff_prob=0.55, prob_input=True),
    dict(B=2, T=60, V=1000, K=20, seed=22, top_n=40, cutoff_prob=0.99),
    dict(B=2, T=80, V=64, K=20, seed=23, top_n=8, quant=0.5),            # equal values at the cut: std::sort's order decides
    dict(B=2, T=80, V=29, K=20, seed=24, top_n=40, cutoff_prob=0.6, quant=0.25),
    dict(B=2, T=50, V=64, K=8, seed=25, top_n=1),
]


def case_id(c):
    return "B%(B)d_T%(T)d_V%(V)d_K%(K)d_s%(seed)d" % c


def case_inputs(c):
    blank = c.get("blank_id", 0)
    lp = ou.synth_logprobs(c["B"], c["T"], c["V"], c["seed"], quant=c.get("quant"), blank_bias=c.get("blank_bias", 0.0), blank_id=blank)
    x = np.exp(lp) if c.get("prob_input") else lp
    kw = dict(beam=c["K"], cutoff_top_n=c.get("top_n", 40), cutoff_prob=c.get("cutoff_prob", 1.0), blank_id=blank, log_input=not c.get("prob_input"))
    return x, kw


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_live_differential(c):
    """The live reference where oracle/_ref is built, else its stored results (tests/golden/live)."""
    x, kw = case_inputs(c)
    ou.assert_same(ou.decode(x, which="restated", **kw), gu.reference_result("oracle_" + case_id(c), x, **kw))


def test_prob_and_log_input_agree_on_labels():
    lp = ou.synth_logprobs(2, 50, 29, 21)
    a = ou.decode(lp, beam=8, log_input=True)
    b = ou.decode(np.exp(lp), beam=8, log_input=False)
    assert np.array_equal(a["tokens"][:, 0], b["tokens"][:, 0])


def test_kernel_matrix_overflow_frames_are_not_inf_frames():
    """The degenerate utterance of every scorer-free case of tests/test_gpu_kernel_matrix.py exercises the overflow: with its two
    -3e38 frames written as -inf instead, the oracle's result for that utterance changes."""
    import kernel_matrix_util as km

    for c in km.CASES:
        if c["lm"]:
            continue
        d = km.degenerate_item(c)
        args = dict(beam=c["K"], cutoff_prob=c["cutoff_prob"], cutoff_top_n=c["top_n"], blank_id=c["blank"], which="restated")
        lp, sl = km.inputs(c)
        r = ou.decode(lp, sl, **args)
        lp_inf, _ = km.inputs(c, overflow_as_inf=True)
        assert not np.array_equal(lp, lp_inf)
        q = ou.decode(lp_inf, sl, **args)
        same = all(np.array_equal(r[k][d], q[k][d]) for k in ("tokens", "timesteps", "lens")) and np.array_equal(
            r["scores"][d].view(np.uint32), q["scores"][d].view(np.uint32))
        assert not same, km.case_id(c)



# ---- the vocabulary prune alone, frame by frame (decoder_utils.cpp:10-45 get_pruned_log_probs): the restatement's prune_vocab and
# the host twin's prune_row against the reference's own function, bit for bit -- the yardstick of tests/test_gpu_prepass_matrix.py
PRUNE_CPS = (1.0, 0.99, 0.6, 0.3, 0.0, -0.0, -0.5, 1.5, float("nan"), 5e-324)
PRUNE_DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "live", "pruned_rows.json")


def _prune_rows_for(V, log_input, seed):
    """Rows of every kind the prune must get right: random, ties inside and across the cut (a 0.5 grid), peaky (the cumulative cut
    stops early), every third label -inf / 0, a frame of -inf / all 0, probabilities near FLT_MIN, rows that do not sum to 1."""
    rng = np.random.default_rng(seed)
    rows = []
    for kind in range(9):
        z = rng.standard_normal(V) * 2.0
        if kind == 2:
            z[rng.integers(0, V)] += 9.0
        lp = z - z.max() - np.log(np.exp(z - z.max()).sum())
        if kind == 1:
            lp = np.round(lp * 2) / 2
        elif kind == 3:
            lp = np.round(lp)  # (coarser: long runs of equal values)
        elif kind == 4:
            lp[::3] = -np.inf
        elif kind == 5:
            lp[:] = -np.inf
        elif kind == 6:
            lp = np.log(rng.random(V) * 3.0)  # (sums to about 1.5 V)
        elif kind == 7:
            lp = np.log(rng.random(V) * 1e-3)  # (sums to well below 1: the cut runs to cutoff_top_n)
        elif kind == 8:
            lp = np.log(rng.random(V) * 4 * np.finfo(np.float32).tiny)  # (probabilities near FLT_MIN, subnormal included)
            lp[rng.integers(0, V)] = np.log(0.5)
        rows.append(lp)
    x = np.array(rows)
    x = (np.exp(x) if not log_input else x).astype(np.float32)
    return x


def _near_cut_rows(base_cp, log_input, V=70, seed=3):
    """Rows whose first partial sum log(1 + p0) lands on cutoff_prob: three rows sharing p0 = expm1(base_cp) (as float32), tails of
    different sizes; -> (rows, [the double the reference's log_sum_exp(0, log p0) gives, and its two neighbours])."""
    rng = np.random.default_rng(seed)
    p0 = np.float32(np.expm1(base_cp))
    rows = np.stack([rng.random(V) * s for s in (1e-9, 1e-4, 1e-2)]).astype(np.float32)
    rows[:, 5] = p0
    rows = (np.log(rows) if log_input else rows).astype(np.float32)
    x0 = np.float64(rows[0, 5]) if log_input else np.log(np.float64(rows[0, 5]))  # (the reference's log p0, from the float32 it reads)
    c = np.log(np.exp(0.0) + np.exp(x0))  # (decoder_utils.h:47-54 with xmax = 0)
    cps = [float(np.nextafter(c, -np.inf)), float(c), float(np.nextafter(c, np.inf))]
    return rows, cps


def _prune_cases():
    out = []
    for li in (1, 0):
        for V in (29, 70):
            x = _prune_rows_for(V, li, 40 + V + li)
            for cp in PRUNE_CPS:
                for top_n in (1, 40, 64, 65, V, V + 7):
                    out.append(("V%d_li%d_cp%r_n%d" % (V, li, cp, top_n), x, cp, top_n, li))
        for base in (0.6, 0.3):
            x, cps = _near_cut_rows(base, li)
            for k, cp in enumerate(cps):
                for top_n in (1, 3, 40):
                    out.append(("near%r_%d_li%d_n%d" % (base, k, li, top_n), x, cp, top_n, li))
    return out


def _digest(*arrays):
    import hashlib

    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(repr((a.shape, a.dtype.str)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _prune_digests():
    """case name -> [input digest, output digest] of the reference's get_pruned_log_probs (tests/golden/make_golden_pruned.py)."""
    import json

    with open(PRUNE_DIGESTS) as f:
        return json.load(f)


def test_pruned_rows_restatement_and_host_twin_equal_the_reference():
    """Count, labels in std::sort order, float values: oracle/ctc_oracle.cpp's prune_vocab and the host core's prune_row equal the
    reference's get_pruned_log_probs bit for bit -- over cutoff_prob 1, 0.99, 0.6, 0.3, +-0, negative, above 1, NaN and subnormal,
    cutoff_top_n 1 / 40 / 64 / 65 / >= V, log and probability rows, and rows whose first partial sum sits on cutoff_prob.  The
    reference is oracle/_ref where it is built with the per-frame entry, else its recorded digests (tests/golden/live/pruned_rows.json)."""
    stored = _prune_digests()
    cases = _prune_cases()
    assert set(stored) == {c[0] for c in cases}
    n_host = 0
    for name, x, cp, top_n, li in cases:
        got = ou.pruned_rows(x, cp, top_n, li, which="restated")
        assert stored[name][0] == _digest(x, np.float64(cp), np.int32(top_n), np.int32(li)), name + ": the recorded digest is of other inputs"
        if ou.have_reference_prune():
            want = ou.pruned_rows(x, cp, top_n, li, which="reference")
            ou.assert_same_pruned(got, want, name)
            assert stored[name][1] == _digest(*want), name + ": the live reference disagrees with its recorded digest"
        assert _digest(*got) == stored[name][1], name
        if li and (0.0 <= cp < 1.0 or top_n < x.shape[-1]):  # (the host twin prunes the log-probability rows of pruned configurations)
            ou.assert_same_pruned(ou.pruned_rows(x, cp, top_n, li, which="host"), got, name + " host twin")
            n_host += 1
    assert n_host > 100


def test_pruned_rows_edge_semantics():
    """What the comparison above pins, spelled out: a negative or NaN cutoff_prob makes no cumulative cut (log of it is NaN); 0 and
    -0 keep one candidate (log 0 = -inf < 0, and every partial sum is >= 0); cutoff_top_n >= V with no cut keeps all V in label order."""
    x = _prune_rows_for(70, 1, 5)
    for cp in (-0.5, float("nan"), 1.5):
        cnt, lab, _ = ou.pruned_rows(x, cp, 40, True)
        assert np.all(cnt == 40)
        cnt, lab, _ = ou.pruned_rows(x, cp, 70, True)
        assert np.all(cnt == 70) and np.array_equal(lab, np.tile(np.arange(70), (len(x), 1)))
    for cp in (0.0, -0.0):
        cnt, _, _ = ou.pruned_rows(x, cp, 40, True)
        assert np.all(cnt == 1)
    cnt, _, _ = ou.pruned_rows(x, 5e-324, 40, True)  # (a subnormal cut: a frame of -inf never reaches it, cum stays log 1 = 0)
    assert cnt[5] == 40 and np.all(np.delete(cnt, 5) == 1)
