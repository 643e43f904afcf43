"""-m gpu tests of the batched scorer hook (ctcd_scorer_create_callback_batch: CallbackScorer.batched / from_c_batch, KenlmScorer) and
of the device filter of repeated misses (beam_core.h lmq_first): the built-in ARPA tables behind the batched hook must give the reference
fixtures and the built-in path bit for bit, every distinct window asked once, in far fewer calls than windows."""
import ctypes
import os
import sys

import numpy as np
import pytest

import fake_kenlm
import golden_util as gu
import oracle_util as ou
from test_lm import LABELS29, TEST_ARPA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


class _Builtin(object):
    """A built-in scorer of the library (ctcd_scorer_create over an ARPA file): ``batch(windows)`` is a batched Python callback over
    ctcd_scorer_cond_log10 that records every window and call; ``fn_batch`` / ``handle`` put ctcd_scorer_cond_log10_batch behind the
    hook natively."""

    def __init__(self, labels, lm_path, device=0):
        from ctcdecode_amd import _native as n

        self.n = n
        arr = (ctypes.c_char_p * len(labels))(*[x.encode("utf-8") for x in labels])
        self.handle = ctypes.c_void_p()
        n.check(n.lib.ctcd_scorer_create(ctypes.byref(self.handle), 0.0, 0.0, lm_path.encode(), arr, len(labels), device))
        self.order = int(n.lib.ctcd_scorer_max_order(self.handle))
        self.vocabulary = fake_kenlm.arpa_words(lm_path)
        self.fn_batch = ctypes.cast(n.lib.ctcd_scorer_cond_log10_batch, ctypes.c_void_p).value
        self.cond_log10 = fake_kenlm.library_backend(n.lib, self.handle)
        self.asked, self.calls = [], 0

    def batch(self, windows):
        self.calls += 1
        self.asked.extend(windows)
        return [self.cond_log10(w) for w in windows]

    def close(self):
        self.n.lib.ctcd_scorer_destroy(self.handle)


def _with_nres(got, want):
    got = dict(got)
    got["nres"] = want["nres"]
    return got


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _same(got, want, what=""):
    for g, w in zip(got, want):
        assert np.array_equal(np.asarray(g).view(np.uint32), np.asarray(w).view(np.uint32)), what


def _scorer(kind, inner, labels, alpha, beta):
    import ctcdecode_amd

    if kind == "python":
        return ctcdecode_amd.CallbackScorer.batched(inner.batch, inner.vocabulary, inner.order, labels, alpha=alpha, beta=beta, device="cuda:0")
    return ctcdecode_amd.CallbackScorer.from_c_batch(inner.fn_batch, inner.handle.value, inner.vocabulary, inner.order, labels, alpha=alpha, beta=beta,
                                                     device="cuda:0")


@pytest.mark.parametrize("kind", ["python", "native"])
@pytest.mark.parametrize("name", gu.lm_names())
def test_batched_hook_reference_fixtures(torch_mod, name, kind):
    """Every committed LM fixture (pruned, ragged seq_lens included) through the batched hook: decode(), decode_device() and the compact
    results equal the reference's outputs bit for bit, with the scorer waiting on the GPU and with a launch per round of misses.  Each
    distinct window is asked once, in fewer calls than windows; a warm decode asks nothing."""
    import ctcdecode_amd

    args, lm, want = gu.load_lm(name)
    x = torch_mod.from_numpy(np.ascontiguousarray(args["probs"]))
    sl = torch_mod.from_numpy(args["seq_lens"]) if args.get("seq_lens") is not None else None
    T = x.shape[1]
    for wait in (True, False):
        inner = _Builtin(lm["labels"], lm["lm_path"])
        try:
            sc = _scorer(kind, inner, lm["labels"], lm["alpha"], lm["beta"])
            dec = ctcdecode_amd.CTCBeamDecoder(lm["labels"], scorer=sc, cutoff_top_n=args["cutoff_top_n"], cutoff_prob=args.get("cutoff_prob", 1.0),
                                               beam_width=args["beam"], blank_id=args["blank_id"], log_probs_input=bool(args["log_input"]), device="cuda:0")
            dec.set_scorer_wait(wait)
            out, scs, ts, ln = dec.decode(x, sl)
            ou.assert_same(_with_nres(dict(tokens=out.numpy(), timesteps=ts.numpy(), scores=scs.numpy(), lens=ln.numpy()), want), want, name)
            calls, batches = sc.callback_calls(), sc.callback_batches()
            assert calls > 0 and 0 < batches <= calls
            if kind == "python":
                assert len(inner.asked) == calls and len(set(inner.asked)) == calls and inner.calls == batches
                assert all(len(w) == inner.order for w in inner.asked)
            queued, distinct, _ = dec.last_scorer_pairs()
            assert distinct == calls and queued >= distinct
            got2 = _np(dec.decode_device(x, sl))  # warm: nothing is asked
            assert sc.callback_calls() == calls and sc.callback_batches() == batches
            ou.assert_same(_with_nres(dict(tokens=got2[0], scores=got2[1], timesteps=got2[2], lens=got2[3]), want), want, name + " warm")
            # compact results from a cold cache: a fresh scorer
            sc2 = _scorer(kind, inner, lm["labels"], lm["alpha"], lm["beta"])
            dec2 = ctcdecode_amd.CTCBeamDecoder(lm["labels"], scorer=sc2, cutoff_top_n=args["cutoff_top_n"], cutoff_prob=args.get("cutoff_prob", 1.0),
                                                beam_width=args["beam"], blank_id=args["blank_id"], log_probs_input=bool(args["log_input"]), device="cuda:0")
            dec2.set_scorer_wait(wait)
            hdr, ent, labs, csc, cln = dec2.decode_compact(x, sl)
            cout, cts = dec2.expand_compact(hdr, ent, labs, T)
            _same(_np((cout, csc, cts, cln)), (out.numpy(), scs.numpy(), ts.numpy(), ln.numpy()), (name, "compact", wait))
            assert sc2.callback_calls() == calls
        finally:
            inner.close()


@pytest.mark.parametrize("kind", ["python", "native"])
def test_batched_hook_batch_pruning_and_streaming(torch_mod, kind):
    """A batch whose utterances park at different frames, ragged, with and without vocabulary pruning, waiting on and off: equal to the
    built-in scorer; far fewer calls than windows on a cold cache; then the batched hook behind OnlineCTCBeamDecoder (chunks that split
    parked frames) equals one-shot."""
    import ctcdecode_amd

    B, T, V, K = 24, 120, 29, 32
    lp = ou.synth_logprobs(B, T, V, 4243, blank_bias=1.0)
    lp[:, :, LABELS29.index(" ")] += np.float32(1.5)
    lp = ou.log_softmax_rows(lp)
    sl = np.random.default_rng(7).integers(0, T + 1, size=B).astype(np.int32)
    x, xs = torch_mod.from_numpy(lp), torch_mod.from_numpy(sl)
    inner = _Builtin(LABELS29, TEST_ARPA)
    try:
        for topn, cp in ((V, 1.0), (12, 0.999)):
            ref = ctcdecode_amd.CTCBeamDecoder(LABELS29, model_path=TEST_ARPA, alpha=0.7, beta=0.9, beam_width=K, cutoff_top_n=topn, cutoff_prob=cp,
                                               log_probs_input=True)
            want = _np(ref.decode(x, xs))
            for wait in (True, False):
                sc = _scorer(kind, inner, LABELS29, 0.7, 0.9)
                dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, scorer=sc, beam_width=K, cutoff_top_n=topn, cutoff_prob=cp, log_probs_input=True)
                dec.set_scorer_wait(wait)
                _same(_np(dec.decode(x, xs)), want, (topn, cp, wait))
                assert sc.callback_calls() > 100 and sc.callback_batches() < sc.callback_calls(), (sc.callback_calls(), sc.callback_batches())
        sc = _scorer(kind, inner, LABELS29, 0.7, 0.9)
        ref = ctcdecode_amd.CTCBeamDecoder(LABELS29, model_path=TEST_ARPA, alpha=0.7, beta=0.9, beam_width=K, log_probs_input=True)
        want = _np(ref.decode(x[:6]))
        dec = ctcdecode_amd.OnlineCTCBeamDecoder(LABELS29, scorer=sc, beam_width=K, log_probs_input=True)
        states = [ctcdecode_amd.DecoderState(dec) for _ in range(6)]
        bounds = [0, 7, 7, 40, T]
        for i in range(len(bounds) - 1):
            out, scs, ts, ln = dec.decode(x[:6, bounds[i]:bounds[i + 1]], states, [i == len(bounds) - 2] * 6)
        assert np.array_equal(scs.numpy().view(np.uint32), want[1].view(np.uint32)) and np.array_equal(ln.numpy(), want[3])
        L = out.shape[2]
        assert np.array_equal(out.numpy(), want[0][:, : out.shape[1], :L]) and np.array_equal(ts.numpy(), want[2][:, : out.shape[1], :L])
        assert sc.callback_calls() > 0
        if kind == "native":
            with pytest.raises(NotImplementedError, match="no helper threads"):
                sc.set_callback_threads(4)  # (a batched callback takes no helper threads: CTCD_EUNSUPPORTED)
        else:
            with pytest.raises(ValueError):
                sc.set_callback_threads(4)
    finally:
        inner.close()


def test_kenlm_scorer_over_fake_module(torch_mod, monkeypatch):
    """KenlmScorer -- now on the batched hook -- over the fake `kenlm` module (tests/fake_kenlm.py, backed by ctcd_scorer_cond_log10 of
    test.arpa's built-in tables) equals model_path=test.arpa bit for bit; the fake itself answers every window the decode asked exactly
    as ctcd_scorer_cond_log10 does."""
    import ctcdecode_amd

    inner = _Builtin(LABELS29, TEST_ARPA)
    try:
        asked = []

        def recording(words):
            asked.append(tuple(words))
            return inner.cond_log10(words)

        monkeypatch.setitem(sys.modules, "kenlm", fake_kenlm.module(recording, inner.vocabulary, inner.order))
        lp = ou.synth_logprobs(4, 80, 29, 31, blank_bias=1.0)
        x = torch_mod.from_numpy(lp)
        ref = ctcdecode_amd.CTCBeamDecoder(LABELS29, model_path=TEST_ARPA, alpha=0.5, beta=1.0, beam_width=50, log_probs_input=True)
        want = _np(ref.decode(x))
        sc = ctcdecode_amd.KenlmScorer(TEST_ARPA, inner.vocabulary, LABELS29, alpha=0.5, beta=1.0)
        dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, scorer=sc, beam_width=50, log_probs_input=True)
        _same(_np(dec.decode(x)), want, "KenlmScorer")
        assert sc.callback_calls() > 0 and sc.callback_batches() < sc.callback_calls()
        kenlm = sys.modules["kenlm"]
        model = kenlm.Model(TEST_ARPA)
        full = sorted({w for w in asked if len(w) == inner.order})
        assert 0 < len(full) <= sc.callback_calls()  # (windows with an unknown word are answered before BaseScore)
        for w in full:  # (the fake against the library's tables, window by window)
            assert ctcdecode_amd.KenlmScorer.cond_log10(kenlm, model, w) == inner.cond_log10(w), w
    finally:
        inner.close()


def test_batched_hook_errors(torch_mod):
    """An exception, a result of the wrong length, NaN or +-inf from the batched callback fails the decode with a clear error; the
    decoder -- and the scorer, once its callback behaves -- stay usable."""
    import ctcdecode_amd

    lp = ou.synth_logprobs(3, 40, 29, 12, blank_bias=1.0)
    lp[:, :, LABELS29.index(" ")] += np.float32(1.5)
    x = torch_mod.from_numpy(ou.log_softmax_rows(lp))
    ref = ctcdecode_amd.CTCBeamDecoder(LABELS29, model_path=TEST_ARPA, alpha=0.5, beta=1.0, beam_width=16, log_probs_input=True)
    want = _np(ref.decode(x))
    inner = _Builtin(LABELS29, TEST_ARPA)

    class Boom(Exception):
        pass

    mode = {"m": None}

    def flaky(windows):
        m = mode["m"]
        if m == "raise":
            raise Boom("model offline")
        r = inner.batch(windows)
        if m == "short":
            return r[:-1]
        if m in ("nan", "inf", "-inf"):
            return [float(m)] * len(r)
        return r

    try:
        for wait in (True, False):
            sc = ctcdecode_amd.CallbackScorer.batched(flaky, inner.vocabulary, inner.order, LABELS29, alpha=0.5, beta=1.0)
            dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, scorer=sc, beam_width=16, log_probs_input=True)
            dec.set_scorer_wait(wait)
            for m, exc, match in (("raise", Boom, "offline"), ("short", ValueError, "answers for"), ("nan", Exception, "NaN"), ("inf", Exception, "infinite"),
                                  ("-inf", Exception, "infinite")):
                mode["m"] = m
                with pytest.raises(exc, match=match):
                    dec.decode(x)
            mode["m"] = None
            _same(_np(dec.decode(x)), want, ("after the errors", wait))
    finally:
        inner.close()


def test_miss_filter_at_configs4_shape(torch_mod):
    """configs[4]'s shape -- 128 x 1500 frames of transcript-like rows, beam 100, test.arpa -- behind the batched hook with the device
    filter of repeated misses on and off: identical outputs (and the built-in path's), the same windows asked, and fewer queued pairs
    per distinct window with the filter on."""
    import bench
    import ctcdecode_amd

    labels = ["_", "'", " "] + [chr(ord("a") + i) for i in range(26)]
    voc = [w for w in bench.arpa_unigrams(TEST_ARPA) if w not in ("<s>", "</s>", "<unk>")]
    x = bench.synth_transcript_rows(torch_mod, 128, 1500, labels, voc, 7).to("cuda:0")
    ref = ctcdecode_amd.CTCBeamDecoder(labels, model_path=TEST_ARPA, alpha=0.5, beta=1.0, cutoff_top_n=29, beam_width=100, log_probs_input=True)
    want = ref.decode_device(x, None)
    inner = _Builtin(labels, TEST_ARPA)
    try:
        stats = {}
        for on in (False, True):
            sc = _scorer("native", inner, labels, 0.5, 1.0)
            dec = ctcdecode_amd.CTCBeamDecoder(labels, scorer=sc, cutoff_top_n=29, beam_width=100, log_probs_input=True)
            dec.set_scorer_filter(on)
            got = dec.decode_device(x, None)
            for g, w in zip(got, want):
                assert torch_mod.equal(g, w), on
            stats[on] = dec.last_scorer_pairs()
            assert stats[on][1] == sc.callback_calls() > 1000 and sc.callback_batches() * 2 < sc.callback_calls()
            del dec, sc
        (q0, d0, r0), (q1, d1, r1) = stats[False], stats[True]
        assert d0 == d1
        assert q1 / d1 < q0 / d0, stats
        assert r1 <= r0, stats
    finally:
        inner.close()
