"""-m gpu: every scorer instantiation of the decode kernel, driven through the select's tie and replay paths.

The kernel matrix's own inputs leave the degenerate frames out for scorer cases, and the scorer breaks most of the coarse item's ties:
the scorer kernels -- the wide-beam ones among them, whose per-entry scorer state lives in HBM scratch and whose replay derives its
info words from the layout -- ran the device's crowded-bucket rounds, single-value exit, big-tie resolution, mid-utterance
nth_element replay and danger mode a handful of times, or never.  select_path_inputs (tests/select_path_util.py) reach all of them in
every scorer class; test_select_paths.py certifies that on the host twin, whose select is a sequential stand-in for the device's
wave-parallel routines.  Here each of the 26 kernels decodes those inputs: the hook must report the case's kernel and layout, and the
four outputs must equal the oracle's (restated scorer) bit for bit -- in one launch, and again fed chunk by chunk through
OnlineCTCBeamDecoder with a compaction behind every chunk, so that the replay's order, the danger flag, the overflowed scores and the
scorer's per-entry state are parked and loaded at the boundaries select_path_bounds chooses (test_stream_matrix_plan.py holds what
they must give).  Callback cases run the built-in tables behind the callback, in both set_scorer_wait forms.  commit() is refused
for scorer streams and stays out."""
import numpy as np
import pytest

import kernel_matrix_util as km
import oracle_util as ou
import select_path_util as sp
import stream_matrix_util as sm
from test_gpu_decode import _with_nres
from test_gpu_kernel_matrix import _decoder, _run
from test_gpu_stream_matrix import _callback_scorers, _feed, _result
from test_gpu_stream_matrix import _decoder as _stream_decoder

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def wide99(tmp_path_factory):
    from test_lm import make_wide_label_lm

    return make_wide_label_lm(tmp_path_factory.mktemp("select_paths_lm"))


_WANT = {}


def _setup(wide99, monkeypatch, c):
    """-> (lm spec, lp, sl, the oracle's one-shot decode of select_path_inputs: computed once per case, shared, left unchanged)."""
    if c["general"]:  # (read when the decoder is created)
        monkeypatch.setenv("CTCD_GENERAL_LM_KERNEL", "1")
    lm = km.lm_spec(c, *wide99)
    assert len(lm[1]) == c["V"]
    key = km.case_id(c)
    if key not in _WANT:
        lp, sl = sp.select_path_inputs(c, lm[1])
        want = ou.decode(lp, sl, scorer=ou.Scorer(lm[2], lm[3], lm[0], lm[1], "restated"), **sm.oracle_args(c))
        for a in [lp, sl] + list(want.values()):
            a.setflags(write=False)
        _WANT[key] = (lp, sl, want)
    return (lm,) + _WANT[key]


@pytest.mark.parametrize("c", sp.scorer_cases(), ids=km.case_id)
def test_select_paths_in_one_launch(torch_mod, wide99, monkeypatch, c):
    lm, lp, sl, want = _setup(wide99, monkeypatch, c)
    labels = lm[1]
    what = "%s on select_path_inputs" % km.case_id(c)
    lp, sl = np.array(lp), np.array(sl)  # (torch.from_numpy wants writable arrays)
    if not c["callback"]:
        got = _run(torch_mod, _decoder(c, labels, lm), c, lp, sl)
        ou.assert_same(_with_nres(got, want), want, what)
        return
    import ctcdecode_amd
    from test_gpu_lm import _BuiltinBehindCallback

    inner = _BuiltinBehindCallback(dict(labels=labels, lm_path=lm[0]))
    try:
        for wait in (True, False):
            sc = ctcdecode_amd.CallbackScorer(inner, inner.vocabulary, inner.order, labels, alpha=lm[2], beta=lm[3], device="cuda:0")
            dec = _decoder(c, labels, lm, callback_scorer=sc)
            dec.set_scorer_wait(wait)
            got = _run(torch_mod, dec, c, lp, sl)
            ou.assert_same(_with_nres(got, want), want, what + " wait=%s" % wait)
            assert sc.callback_calls() > 0
    finally:
        inner.close()


@pytest.mark.parametrize("e", sp.stream_entries(), ids=sm.entry_id)
def test_select_paths_behind_a_parked_state(torch_mod, wide99, monkeypatch, e):
    """The entry's select_path_inputs fed over select_path_bounds, all streams compacted behind every chunk that held a frame: every
    such chunk launches the entry's kernel, and the streams end bit for bit like the oracle's one-shot decode."""
    import ctcdecode_amd

    c = e["case"]
    lm, lp, sl, want = _setup(wide99, monkeypatch, c)
    labels = lm[1]
    B, T, K = c["B"], c["T"], c["K"]
    bounds = sp.select_path_bounds(e)
    x = torch_mod.from_numpy(np.array(lp)).to("cuda:0")
    sl = np.array(sl)
    inner, scorers = _callback_scorers(c, labels, lm)
    try:
        for scorer, wait in scorers:
            dec = _stream_decoder(c, labels, lm, callback_scorer=scorer)
            if wait is not None:
                dec.set_scorer_wait(wait)
            states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
            compacted = []

            def before(i):
                if i > 0 and bounds[i] > bounds[i - 1]:
                    live = dec.compact(states)
                    assert len(live) == B and min(live) >= 1
                    compacted.append(bounds[i])
                return None

            out, _ = _feed(torch_mod, dec, states, x, sl, bounds, [e["kernel"]] * (len(bounds) - 1), before=before)
            assert compacted == sorted(set(bounds[1:-1])), compacted
            got = _result(out, K, T)
            ou.assert_same(_with_nres(got, want), want, "%s bounds %s wait=%s" % (sm.entry_id(e), bounds, wait))
            if scorer is not None:
                assert scorer.callback_calls() > 0
    finally:
        if inner is not None:
            inner.close()
