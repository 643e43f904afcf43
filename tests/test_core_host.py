"""The GPU decoder's per-utterance core (ctcdecode_amd/csrc/beam_core.h) compiled for the host with a sequential
execution policy, against the oracle and the committed reference fixtures.  This validates the ALGORITHM the HIP kernel
runs (DFS-ordered beam + LCP array, Euler-tour candidate slots, exact tie replay) without a GPU; the -m gpu tests then
check the same source running as a workgroup."""
import numpy as np
import pytest

import degenerate_util as du
import golden_util as gu
import oracle_util as ou
import rank_epoch_util as reu


@pytest.mark.parametrize("name", [n for n in gu.names() if "prob" not in n])
def test_core_matches_reference_fixtures(name):
    args, want = gu.load(name)
    assert args.pop("log_input")
    ou.assert_same(ou.decode_core_host(**args), want, name)


def test_core_randomized_against_oracle():
    rng = np.random.default_rng(7)
    stats = np.zeros(5, np.int64)
    for it in range(120):
        V = int(rng.choice([3, 5, 9, 29, 29, 64]))
        K = int(rng.choice([1, 2, 5, 16, 50, 100, 128]))
        T = int(rng.integers(1, 200))
        quant = [None, None, 0.5, 1.0, 0.25, 2.0][int(rng.integers(0, 6))]
        bias = float(rng.choice([0, 0, 3, 6, -2]))
        blank = int(rng.integers(0, V))
        top_n = int(rng.choice([40, 40, 40, max(1, V // 2), 3]))
        lp = ou.synth_logprobs(2, T, V, 5000 + it, quant=quant, blank_bias=bias, blank_id=blank)
        sl = rng.integers(0, T + 5, size=2).astype(np.int32) if it % 4 == 0 else None
        kw = dict(beam=K, blank_id=blank, cutoff_top_n=top_n)
        a = ou.decode(lp, sl, which="restated", want_stats=True, **kw)
        ou.assert_same(a, ou.decode_core_host(lp, sl, **kw), "case %d V=%d K=%d T=%d q=%s" % (it, V, K, T, quant))
        stats += a["stats"].sum(0)
    # the sweep must actually exercise the hard paths: tie splits at the K boundary, revived dead-interior nodes
    assert stats[1] > 100 and stats[2] > 1000, stats


def test_core_north_star_shape():
    lp = ou.synth_logprobs(2, 1000, 29, 5)
    ou.assert_same(ou.decode(lp, beam=100), ou.decode_core_host(lp, beam=100))


def _edge_cases():
    yield "only_blank", ou.synth_logprobs(2, 20, 1, 1), dict(beam=5)
    yield "two_labels_k1", ou.synth_logprobs(2, 30, 2, 2), dict(beam=1, blank_id=1)
    yield "one_frame", ou.synth_logprobs(3, 1, 29, 3), dict(beam=100)
    lp = ou.synth_logprobs(2, 60, 9, 4)
    lp[:, ::3, 2] = -np.inf
    lp[:, 5, :] = -np.inf
    yield "minus_inf_inputs", lp, dict(beam=12)
    lp = ou.synth_logprobs(2, 40, 9, 5)
    lp[:, :, 0] = 0.0
    yield "certain_blank", lp, dict(beam=12)
    lp = np.full((2, 50, 6), np.float32(-1.7917595), np.float32)
    yield "all_equal_maximal_ties", lp, dict(beam=20)
    yield "coarse_quantised", ou.synth_logprobs(1, 300, 4, 7, quant=4.0), dict(beam=64, blank_id=3)
    lp = ou.synth_logprobs(2, 40, 9, 8)
    lp[0, 10:20, :] = -3.0e38
    yield "near_minus_flt_max", lp, dict(beam=12)
    # zeros of both signs (scores that are -0.0 / +0.0 compare equal), positive "log-probabilities", a denormal
    lp = np.zeros((2, 30, 5), np.float32)
    lp[:, :, 1] = -0.0
    lp[:, ::2, 2] = 0.25
    lp[:, 1::3, 3] = -1e-40
    lp[1, :, 0] = -0.0
    yield "signed_zeros_and_positive_values", lp, dict(beam=16)
    # every log-probability -0.0: sums of a prefix score and a log-probability are then never -0 (the score is not), which
    # is what lets the child-scoring loop skip the zero canonicalisation of its keys (beam_core.h ord_f32_raw)
    yield "all_negative_zero", np.full((2, 25, 7), np.float32(-0.0), np.float32), dict(beam=24)


EDGE = list(_edge_cases())


@pytest.mark.parametrize("name,lp,kw", EDGE, ids=[e[0] for e in EDGE])
def test_core_edge_cases(name, lp, kw):
    ou.assert_same(ou.decode(lp, which="restated", **kw), ou.decode_core_host(lp, **kw), name)


@pytest.mark.parametrize("name,lp,kw", EDGE, ids=[e[0] for e in EDGE])
def test_oracle_edge_cases_against_live_reference(name, lp, kw):
    """The live reference where oracle/_ref is built, else its stored results (tests/golden/live)."""
    ou.assert_same(ou.decode(lp, which="restated", **kw), gu.reference_result("core_edge_" + name, lp, **kw), name)


def _degenerate_sweep(n, seed, reference_every=0, prune=False, chunked=False):
    rng = np.random.default_rng(seed)
    kinds = set()
    for it in range(n):
        meta, lp = du.make_case(rng)
        kw = dict(beam=meta["K"], blank_id=meta["blank"])
        sl = None
        if prune:
            kw.update(cutoff_top_n=int(rng.choice([40, max(1, meta["V"] // 2), 3, 1])), cutoff_prob=float(rng.choice([1.0, 1.0, 0.9, 0.5])))
            sl = rng.integers(0, meta["T"] + 3, size=2).astype(np.int32) if it % 3 == 0 else None
        want = ou.decode(lp, sl, which="restated", **kw)
        if chunked:
            bounds = sorted(set(int(v) for v in rng.integers(0, meta["T"] + 1, size=int(rng.integers(0, 6)))))
            got = ou.decode_core_host_chunked(lp, bounds, **kw)
        else:
            got = ou.decode_core_host(lp, sl, **kw)
        ou.assert_same(want, got, "degenerate case %d %s %s" % (it, meta, kw))
        if reference_every and it % reference_every == 0 and ou.have_reference():
            ou.assert_same(want, ou.decode(lp, sl, which="reference", **kw), "oracle vs live reference, case %d %s" % (it, meta))
        kinds.add(meta["kind"])
    assert len(kinds) == len(du.KINDS)


def test_core_degenerate_inputs_follow_the_reference_argument_order():
    """Whole frames of -inf, sums that overflow, -inf tail padding without seq_lens: log_sum_exp(-FLT_MAX, -inf) depends
    on the order of its arguments (decoder_utils.h:47-54), i.e. on the permutation std::nth_element left in `prefixes`
    (ctc_beam_search_decoder.cpp:87-142,150-154).  Round 2 always added the repeat contribution first and differed from
    the reference on 20-90 % of such inputs; danger mode (beam_core.h enter_danger) replays the order."""
    _degenerate_sweep(300, 101, reference_every=3)


def test_core_degenerate_inputs_pruned_and_ragged():
    _degenerate_sweep(150, 102, reference_every=5, prune=True)


def test_core_degenerate_inputs_streamed():
    """Danger mode is part of the parked stream state: any chunking of a degenerate utterance equals the one-shot result."""
    _degenerate_sweep(150, 103, chunked=True)


@pytest.mark.parametrize("level", ["1", "2"])
def test_core_degenerate_inputs_hbm_scratch_layouts(monkeypatch, level):
    monkeypatch.setenv("CTC_HOST_BIG", level)
    _degenerate_sweep(60, 104 + int(level))


@pytest.mark.parametrize("level", ["1", "2"])
def test_core_hbm_scratch_layout(monkeypatch, level):
    """The wide-beam workspace layouts: level 1 keeps the rare-path per-slot arrays outside the workgroup's LDS, level 2
    (beam_width ~1000) also the slot keys and the rarely read per-entry arrays."""
    monkeypatch.setenv("CTC_HOST_BIG", level)
    for seed, kw in [(44, dict(quant=0.5)), (45, dict(blank_bias=3.0)), (46, {})]:
        lp = ou.synth_logprobs(2, 150, 29, seed, **kw)
        ou.assert_same(ou.decode(lp, beam=64), ou.decode_core_host(lp, beam=64))
    lp = ou.synth_logprobs(1, 40, 29, 47)
    ou.assert_same(ou.decode(lp, beam=1000), ou.decode_core_host(lp, beam=1000), "beam 1000")


def test_core_rank_table_tags_wrap():
    """The pruned default's compile-time class tags the rank table's entries with the frame (mod 1024) instead of taking a frame's candidates
    out of the table again; the table is wiped when the tags repeat: utterances longer than 1024 frames, against the oracle."""
    for seed, (V, top_n, K, T) in enumerate([(300, 20, 30, 2100), (64, 40, 50, 1100)]):
        lp = ou.synth_logprobs(1, T, V, 4400 + seed)
        want = ou.decode(lp, beam=K, cutoff_top_n=top_n)
        got = ou.decode_core_host(lp, None, beam=K, cutoff_top_n=top_n)
        ou.assert_same(got, want, "rank-table tags V=%d T=%d" % (V, T))


# ---- the rank table of the pruned default's compile-time class across frame 1023 mod 1024 (beam_core.h kRankEpoch; the inputs:
# rank_epoch_util.py).  The shapes are the class's (decode_impl of tests/native/core_host.cpp runs decode_utterance<false, 2> for them);
# CTC_HOST_NO_CLASS2=1 runs the run-time layout instead, which takes every frame's candidates out of its table.


def _class2_and_runtime_layout_match_oracle(monkeypatch, lp, what, beam=reu.K, cutoff_top_n=reu.TOP_N, **kw):
    kw.update(beam=beam, cutoff_top_n=cutoff_top_n)
    want = ou.decode(lp, **kw)
    ou.assert_same(ou.decode_core_host(lp, **kw), want, what + " (class 2)")
    with monkeypatch.context() as m:
        m.setenv("CTC_HOST_NO_CLASS2", "1")
        ou.assert_same(ou.decode_core_host(lp, **kw), want, what + " (run-time layout)")
    return want


def test_core_rank_epoch_unwritten_entry_is_not_rank_63(monkeypatch):
    """Regression: the blank is never a candidate and at frame 1023 drops below nineteen labels at -3.0 -- its never-written entry
    (0xFFFF) read as frame 1023's rank 63 (a log-probability past the 20 candidates, one non-blank candidate too few)."""
    lp = reu.prune_blank(ou.synth_logprobs(2, 1100, reu.V, 501), reu.TOP_N)
    lp[:, 1023, :20] = -3.0
    lp[:, 1023, 0] = -3.5
    _class2_and_runtime_layout_match_oracle(monkeypatch, lp, "seed 501, T=1100")


@pytest.mark.parametrize("T", [1023, 1024, 1025, 2047, 2048, 2049, 3100])
@pytest.mark.parametrize("kind", reu.KINDS)
def test_core_rank_epoch_wraps(monkeypatch, kind, T):
    _class2_and_runtime_layout_match_oracle(monkeypatch, reu.epoch_case(kind, T), "%s T=%d" % (kind, T))


def test_core_rank_epoch_randomized():
    """Bounded sweep over the class (beam <= 112, cutoff_top_n <= 40, V up to 1000) past frame 1023, the blank biased out of the
    candidates in many frames."""
    rng = np.random.default_rng(2024)
    for it in range(8):
        V = int(rng.choice([64, 300, 1000]))
        K = int(rng.choice([8, 30, 64, 112]))
        top_n = int(rng.choice([5, 20, 40]))
        T = int(rng.integers(1000, 2201))
        lp = ou.synth_logprobs(1, T, V, 9100 + it, blank_bias=float(rng.choice([-2.0, -3.0, -5.0])))
        if it % 2:
            reu.strong_wrap_frames(lp, top_n, it)
        kw = dict(beam=K, cutoff_top_n=top_n)
        ou.assert_same(ou.decode_core_host(lp, **kw), ou.decode(lp, **kw), "case %d V=%d K=%d top_n=%d T=%d" % (it, V, K, top_n, T))


@pytest.mark.parametrize("kind,K,top_n", [("blank_pruned_at_wraps", 100, 40), ("stale_tag", reu.K, reu.TOP_N)])
def test_core_rank_epoch_streamed(monkeypatch, kind, K, top_n):
    """Pruned streams of the class: load_state wipes the rank table at every chunk start, so a chunk that starts at frame 1023 or 2047
    looks up every label that is not one of its first frame's candidates in a wiped table; one-frame chunks across the wraps.  Every
    chunking equals the one-shot oracle, in the class and in the run-time layout."""
    T = 2100
    lp = reu.epoch_case(kind, T, top_n=top_n)
    kw = dict(beam=K, cutoff_top_n=top_n)
    want = ou.decode(lp, **kw)
    chunkings = [[1023], [1024], [2047], [1023, 2047], list(range(1020, 1028)) + list(range(2044, 2052)), [500, 1023, 1024, 1025, 2047, 2048]]
    for bounds in chunkings:
        ou.assert_same(ou.decode_core_host_chunked_pruned(lp, bounds, **kw), want, "%s chunks %s" % (kind, bounds))
    with monkeypatch.context() as m:
        m.setenv("CTC_HOST_NO_CLASS2", "1")
        ou.assert_same(ou.decode_core_host_chunked_pruned(lp, chunkings[-1], **kw), want, "%s run-time layout, chunks %s" % (kind, chunkings[-1]))


def test_core_streaming_equals_one_shot():
    """The stream state (beam parked between chunks) on the host build: arbitrary chunkings, empty chunks included."""
    rng = np.random.default_rng(3)
    for it in range(40):
        V = int(rng.choice([3, 9, 29]))
        K = int(rng.choice([2, 16, 50, 100]))
        T = int(rng.integers(2, 150))
        quant = [None, 0.5, 1.0][int(rng.integers(0, 3))]
        lp = ou.synth_logprobs(2, T, V, 900 + it, quant=quant, blank_bias=float(rng.choice([0, 3])))
        bounds = sorted(set(int(x) for x in rng.integers(0, T + 1, size=int(rng.integers(0, 6)))))
        ou.assert_same(ou.decode(lp, beam=K), ou.decode_core_host_chunked(lp, bounds, beam=K), "chunks %s" % bounds)


def _stream_matrix_host_cases():
    import stream_matrix_util as sm

    by_kernel = dict((e["kernel"], e) for e in sm.STREAM_CASES if not e["production"])
    return [(by_kernel[k], x, y) for k, x, y in sm.HOST_HAND_OVERS]


@pytest.mark.parametrize("e,x,y", _stream_matrix_host_cases(), ids=["%s-%d-%d" % ("k%d%d%d%d_%d_lm%d_occ%d" % e["kernel"], x, y) for e, x, y in _stream_matrix_host_cases()])
def test_core_stream_hand_over_between_instantiations(e, x, y):
    """The streamed kernel matrix's inputs and chunk bounds (tests/stream_matrix_util.py: ragged, ties, the overflow frames split by a
    boundary, an empty chunk, a boundary behind the -inf frame) on the host twin: every chunk by instantiation x, every chunk by y,
    and the stream handed from one to the other at the T // 2 bound, in both directions -- each equal to the oracle's one-shot
    decode of the ragged batch.  (CTC_ASSUME_CHECKED build: a bound the parked state breaks for the next instantiation fails here.)"""
    import kernel_matrix_util as km
    import stream_matrix_util as sm

    c = e["case"]
    lp, sl = km.inputs(c)
    kw = sm.oracle_args(c)
    want = ou.decode(lp, sl, which="restated", **kw)
    if ou.have_reference():
        ou.assert_same(ou.decode(lp, sl, which="reference", **kw), want, "the two oracles")
    b = sm.bounds(e)
    n, m = len(b) - 1, sm.mid_index(e)
    for inst in ([x] * n, [y] * n, [x] * m + [y] * (n - m), [y] * m + [x] * (n - m)):
        got = ou.decode_core_host_chunked_mixed(lp, b, inst, seq_lens=sl, **kw)
        ou.assert_same(got, want, "%s bounds %s instantiations %s" % (sm.entry_id(e), b, inst))


def test_core_time_steps_beyond_16_bits():
    """A pool node packs its label and the low 16 bits of its time step into one word (12-byte nodes); launches that can pass
    frame 65535 keep the high bits in a side array.  One-shot and streamed across the boundary."""
    T = 66500
    lp = ou.synth_logprobs(1, T, 3, 17, blank_bias=2.5)  # blank-dominated: the label sequences stay short, their time steps span all of T
    want = ou.decode(lp, beam=4)
    assert int(want["timesteps"][0, 0, : want["lens"][0, 0]].max()) > 65536
    ou.assert_same(want, ou.decode_core_host(lp, beam=4), "T > 65536")
    ou.assert_same(want, ou.decode_core_host_chunked(lp, [100, 65000, 65536, 65537, 66000], beam=4), "T > 65536, streamed")


def test_core_helpers():
    """ord_f32 (score -> sortable key), the shift forms of the divisions, log2 helpers, info-word packing."""
    import ctypes

    lib = ctypes.CDLL(ou.build_core_host())
    lib.ctccore_check_helpers.restype = ctypes.c_longlong
    lib.ctccore_check_helpers.argtypes = [ctypes.c_ulonglong, ctypes.c_longlong]
    assert lib.ctccore_check_helpers(12345, 2_000_000) == 0


def test_compact_results_expand_to_the_padded_tensors():
    """Compact delivery (beam_core.h OutRefs::c_*, compact_results.h): every entry hands over only the labels it does not
    share with its DFS predecessor; expanded, the result must be the padded tensors exactly -- zeros included."""
    for seed, (B, T, V, K, kw) in enumerate([(3, 200, 29, 50, {}), (2, 150, 9, 100, dict(quant=0.5)), (4, 60, 29, 16, dict(ragged=True)),
                                             (2, 2, 3, 50, dict(blank_id=1)), (2, 300, 29, 100, dict(blank_bias=4.0))]):
        blank = kw.get("blank_id", 0)
        lp = ou.synth_logprobs(B, T, V, 300 + seed, quant=kw.get("quant"), blank_bias=kw.get("blank_bias", 0.0), blank_id=blank)
        sl = np.array([T, 0, 1, T // 2][:B], np.int32) if kw.get("ragged") else None
        want = ou.decode(lp, sl, beam=K, blank_id=blank)
        got = ou.decode_core_host_compact(lp, sl, beam=K, blank_id=blank)
        ou.assert_same(got, want, "compact case %d" % seed)
        assert np.array_equal(got["tokens"], want["tokens"]) and np.array_equal(got["timesteps"], want["timesteps"])  # the zero fill too
        assert got["labels_used"] <= int(want["lens"].sum())
        if T >= 150 and not kw.get("blank_bias"):
            assert got["labels_used"] * 2 < int(want["lens"].sum()), "the beam's sequences overlap: far fewer labels travel than rows hold"


def test_log_softmax_host_twin_is_a_log_softmax():
    """The host twin of the logits pre-pass (exact definition in include/ctcdecode_amd.h) against float64 arithmetic."""
    rng = np.random.default_rng(11)
    for V in (1, 2, 29, 64, 65, 130, 1000):
        x = (rng.standard_normal((7, V)) * 4).astype(np.float32)
        x[1, :] -= 200.0
        if V > 2:
            x[2, 1] = -np.inf
            x[3, :] = -np.inf
        y = ou.log_softmax_rows(x)
        with np.errstate(invalid="ignore", divide="ignore"):
            x64 = x.astype(np.float64)
            m = x64.max(-1, keepdims=True)
            want = x64 - m - np.log(np.exp(x64 - m).sum(-1, keepdims=True))
        ok = np.isfinite(want)
        assert np.allclose(y[ok], want[ok], rtol=0, atol=2e-6 * (1 + np.log(V)))
        assert np.all(np.isneginf(y[~ok]))


def test_core_negative_cutoff_prob_makes_no_cumulative_cut():
    """A negative or NaN cutoff_prob: log(cutoff_prob) is NaN, so the reference makes no cumulative cut (decoder_utils.cpp:16,21) and
    keeps cutoff_top_n candidates per frame -- the decode equals the one with cutoff_prob 1.0, and the oracle's."""
    lp = ou.synth_logprobs(2, 60, 50, 31)
    kw = dict(beam=10, cutoff_top_n=12)
    plain = ou.decode_core_host(lp, cutoff_prob=1.0, **kw)
    for cp in (-0.5, float("nan")):
        got = ou.decode_core_host(lp, cutoff_prob=cp, **kw)
        ou.assert_same(got, ou.decode(lp, cutoff_prob=cp, which="reference" if ou.have_reference() else "restated", **kw), "cp %r" % cp)
        ou.assert_same(got, plain, "cp %r vs 1.0" % cp)
    # (and a real cut below ln 2 does change it: the comparison above is not vacuous)
    cut = ou.decode_core_host(lp, cutoff_prob=0.3, **kw)
    assert not all(np.array_equal(cut[k], plain[k]) for k in ("tokens", "lens", "scores"))
