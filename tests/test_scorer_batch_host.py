"""CPU tests of the batched scorer hook's surroundings: the fake `kenlm` module KenlmScorer is tested with (tests/fake_kenlm.py),
the per-utterance filter of repeated misses in the host build of the core (beam_core.h lmq_first), and the new C ABI symbols."""
import os
import re

import numpy as np

import fake_kenlm
import golden_util as gu
import oracle_util as ou
from test_lm import KENLM_KATS, LABELS29, TEST_ARPA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["ctcd_scorer_create_callback_batch", "ctcd_scorer_cond_log10_batch", "ctcd_scorer_callback_batches", "ctcd_last_scorer_pairs",
               "ctcd_set_scorer_filter"]


def _fixture_windows(lm, want, order):
    """Every window of the words of a fixture decode's results (each beam's transcript, "<s>"-padded as make_ngram pads it), with "</s>"."""
    labels = lm["labels"]
    out = set()
    for b in range(want["tokens"].shape[0]):
        for k in range(int(want["nres"][b])):
            text = "".join(labels[t] for t in want["tokens"][b, k, : want["lens"][b, k]])
            words = ["<s>"] * (order - 1) + text.split() + ["</s>"]
            for i in range(order - 1, len(words)):
                out.add(tuple(words[i - order + 1: i + 1]))
    return sorted(out)


def test_fake_kenlm_matches_product_tables():
    """KenlmScorer's window logic (KenlmScorer.cond_log10) over the fake module answers as the product's own tables do: every window
    of the results of the test.arpa fixtures, and kenlm's published windows.  On the CPU the fake rests on the restated scorer; its
    converted double is turned back into the float32 log10 exactly (fake_kenlm.restated_backend)."""
    import ctcdecode_amd

    names = [n for n in gu.lm_names() if os.path.basename(gu.load_lm(n)[1]["lm_path"]) == "test.arpa"]
    assert names
    sc = ou.Scorer(0.0, 0.0, TEST_ARPA, LABELS29, "restated")
    order = sc.max_order()
    kenlm = fake_kenlm.module(fake_kenlm.restated_backend(sc), fake_kenlm.arpa_words(TEST_ARPA), order)
    model = kenlm.Model(TEST_ARPA)
    assert model.order == 5 and "looking" in model and "this_is_not_found" not in model
    windows = set()
    for n in names:
        args, lm, want = gu.load_lm(n)
        windows.update(_fixture_windows(lm, want, order))
    windows.update(tuple(w[-order:]) for w, _ in KENLM_KATS)
    assert len(windows) > 20
    oov = 0
    for w in sorted(windows):
        got = ctcdecode_amd.KenlmScorer.cond_log10(kenlm, model, w)
        ref, _ = ou.core_host_lm_cond(TEST_ARPA, LABELS29, list(w))
        if ref == -1000.0:
            assert got is None, w
            oov += 1
        else:
            assert got is not None and np.float32(got) == np.float32(ref * fake_kenlm.NUM_FLT_LOGE), (w, got, ref)
            # (the reference's conversion of that float32 gives the product's double back bit for bit)
            assert float(np.float32(got)) / fake_kenlm.NUM_FLT_LOGE == ref, w
    assert oov > 0
    # the state carries at most order - 1 words, as kenlm's does
    st, out = kenlm.State(), kenlm.State()
    model.NullContextWrite(st)
    for w in ["<s>", "looking", "on", "a", "little", "more"]:
        model.BaseScore(st, w, out)
        st, out = out, st
    assert st.words == ("looking", "on", "a", "little", "more")[-(order - 1):]


def test_host_core_with_miss_filter_matches_fixtures():
    """The host build of the core behind the hook runs the per-utterance filter of repeated misses (beam_core.h lmq_first: the host
    driver sets LmView::cb = 1, filter on): outputs equal the committed LM fixtures and the built-in path over a random sweep."""
    for name in gu.lm_names():
        args, lm, want = gu.load_lm(name)
        if args["cutoff_top_n"] < args["probs"].shape[2]:
            continue  # (the hook's host driver takes unpruned rows)
        got = ou.decode_core_host_lm_cb(args["probs"], lm["alpha"], lm["beta"], lm["lm_path"], lm["labels"], seq_lens=args["seq_lens"],
                                        beam=args["beam"], blank_id=args["blank_id"], log_input=args["log_input"])
        ou.assert_same(got, want, name)
    rng = np.random.default_rng(1234)
    labels = ["_", "'", " "] + [chr(ord("a") + i) for i in range(26)]
    for it in range(12):
        arpa = os.path.join(gu.DATA_DIR, ["test.arpa", "chars.arpa", "abcd_words.arpa"][it % 3])
        labs = labels if it % 3 != 2 else ["_", " ", "a", "b", "c", "d"]
        T, K = int(rng.integers(1, 70)), int(rng.choice([1, 8, 40]))
        lp = ou.synth_logprobs(2, T, len(labs), int(rng.integers(0, 1 << 30)), blank_bias=float(rng.choice([0.0, 2.0])))
        alpha, beta = float(rng.choice([0.5, 1.3])), float(rng.choice([0.0, 1.0]))
        a = ou.decode_core_host_lm(lp, alpha, beta, arpa, labs, beam=K, cutoff_top_n=len(labs), threads=1)
        b = ou.decode_core_host_lm_cb(lp, alpha, beta, arpa, labs, beam=K)
        ou.assert_same(b, a, "it %d" % it)


def test_batched_hook_symbols_are_declared_and_exported():
    import ctypes

    import __graft_entry__ as g

    g.build()
    from ctcdecode_amd import _build, _native

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ctcdecode_amd.h")).read(), flags=re.S)
    assert "ctcd_cond_log10_batch_fn" in text
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _native.SYMBOLS, name
        assert hasattr(lib, name), name
        assert hasattr(_native.lib, name), name
