"""-m gpu: every instantiation of the decode kernel a stream can launch, fed a parked state.  One entry per stream-reachable item of
CTC_KERNEL_LIST (tests/stream_matrix_util.py; test_stream_matrix_plan.py proves the table covers them), and one more per OCC2 key
that reaches it through the batch size alone.  The chunks (a one-frame chunk, a boundary between the two overflow frames, an empty
chunk, boundaries behind tie frames and behind the -inf frame) must each launch exactly the expected kernel, and the stream must
end bit for bit like the oracle's one-shot decode of the ragged batch; ctc_stream_peek_kernel and the ctc_stream_compact_* kernels
must read what that instantiation's save_state parked; and a stream handed from one kernel to another between two chunks -- as
serving does when the batch size crosses the CU count or the shape statistic flips the subtree search -- must decode the same.

Commit behind every scorer-free instantiation: the ctc_stream_commit_* kernels re-root what that instantiation parked, and its
load_state continues the re-rooted block -- over inputs on which a commit hands out labels at several boundaries (commit_inputs: the
matrix's items and one whose confidence fades; test_stream_matrix_plan.py proves that they do), across every scorer-free hand-over,
and, behind four keys the long commit tests never reach, at depths past an express level."""
import numpy as np
import pytest

import commit_util as mu
import compact_util as cu
import kernel_matrix_util as km
import oracle_util as ou
import peek_util as pu
import stream_matrix_util as sm
from test_gpu_decode import _with_nres
from test_gpu_stream_commit import _walk_device as _commit_walk
from test_gpu_stream_compact import _final, _walk_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def wide99(tmp_path_factory):
    from test_lm import make_wide_label_lm

    return make_wide_label_lm(tmp_path_factory.mktemp("stream_matrix_lm"))


def _cu_count(torch):
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _configure(c):
    from ctcdecode_amd import _native

    return lambda dec: sm.configure(dec, c, _native.lib, _native.check)


def _decoder(c, labels, lm, callback_scorer=None):
    import ctcdecode_amd

    kw = dict(cutoff_top_n=c["top_n"], cutoff_prob=c["cutoff_prob"], beam_width=c["K"], blank_id=c["blank"], log_probs_input=True,
              device="cuda:0")
    if callback_scorer is not None:
        dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, scorer=callback_scorer, **kw)
    elif lm is not None:
        dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, model_path=lm[0], alpha=lm[2], beta=lm[3], **kw)
    else:
        dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, **kw)
    _configure(c)(dec)
    assert dec.last_kernel() is None and dec.last_layout() == -1
    return dec


def _result(out, K, T, items=None):
    tok, sc, ts, ln = out
    items = list(range(tok.shape[0])) if items is None else items
    got = dict(tokens=np.zeros((len(items), K, T), np.int32), timesteps=np.zeros((len(items), K, T), np.int32), scores=sc.numpy()[items],
               lens=ln.numpy()[items])
    got["tokens"][:, :tok.shape[1], :tok.shape[2]] = tok.numpy()[items]
    got["timesteps"][:, :ts.shape[1], :ts.shape[2]] = ts.numpy()[items]
    return got


def _feed(torch, dec, states, x, sl, bounds, kernels, before=None, items=None):
    """Feed the chunks of `bounds` to the streams `items` (default: all) of the batch x [B, T, V] with lengths sl; every stream ends
    at the last chunk.  kernels[i]: what last_kernel() must report after chunk i, if it held a frame.  before(i): called in front of
    chunk i; may return the items to feed from there on.  -> (the last call's results, the items it fed)."""
    items = list(range(x.shape[0])) if items is None else items
    out = None
    n = len(bounds) - 1
    for i in range(n):
        if before is not None:
            items = before(i) or items
        lo, hi = bounds[i], bounds[i + 1]
        lens = sm.chunk_lens(sl[items], lo, hi)
        out = dec.decode(x[items, lo:hi], [states[b] for b in items], [i == n - 1] * len(items), seq_lens=torch.from_numpy(lens))
        if hi > lo:
            assert dec.last_kernel() == tuple(kernels[i]), "chunk %d [%d, %d) launched %s, expected %s" % (i, lo, hi, dec.last_kernel(), tuple(kernels[i]))
            assert dec.last_layout() == km.expected_layout(tuple(kernels[i]))
    return out, items


def _setup(torch, wide99, monkeypatch, c):
    """-> (labels, lm spec or None, lp, sl, the oracle's one-shot results of the ragged batch: the restatement's and, without a
    scorer and where it was built, the compiled reference's)."""
    if c["general"]:  # (read when the decoder is created)
        monkeypatch.setenv("CTCD_GENERAL_LM_KERNEL", "1")
    lm = km.lm_spec(c, *wide99) if c["lm"] else None
    labels = lm[1] if lm else [str(i) for i in range(c["V"])]
    assert len(labels) == c["V"]
    lp, sl = km.inputs(c, labels)
    args = sm.oracle_args(c)
    if lm is None:
        wants = [ou.decode(lp, sl, which="restated", **args)]
        if ou.have_reference():
            wants.append(ou.decode(lp, sl, which="reference", **args))
    else:
        wants = [ou.decode(lp, sl, scorer=ou.Scorer(lm[2], lm[3], lm[0], labels, "restated"), **args)]
    return labels, lm, lp, sl, wants


def _callback_scorers(c, labels, lm):
    """The decoders' scorers of a case: [None] or, for a callback case, one CallbackScorer per set_scorer_wait form (the built-in
    tables behind the callback).  -> (inner or None, [(scorer, wait)])."""
    if not c["callback"]:
        return None, [(None, None)]
    import ctcdecode_amd
    from test_gpu_lm import _BuiltinBehindCallback

    inner = _BuiltinBehindCallback(dict(labels=labels, lm_path=lm[0]))
    mk = lambda: ctcdecode_amd.CallbackScorer(inner, inner.vocabulary, inner.order, labels, alpha=lm[2], beta=lm[3], device="cuda:0")  # noqa: E731
    return inner, [(mk(), True), (mk(), False)]


@pytest.mark.parametrize("e", sm.STREAM_CASES, ids=sm.entry_id)
def test_streamed_instantiation(torch_mod, wide99, monkeypatch, e):
    """The entry's ragged batch fed over its bounds: every chunk that holds a frame launches the entry's kernel, and the streams end
    bit for bit like the oracle's one-shot decode and like the same decoder class fed in one call.  Callback cases: both
    set_scorer_wait forms."""
    import ctcdecode_amd

    c = sm.sized_case(e, _cu_count(torch_mod))
    labels, lm, lp, sl, wants = _setup(torch_mod, wide99, monkeypatch, c)
    B, T, K = c["B"], c["T"], c["K"]
    bounds = sm.bounds(e)
    what = "%s bounds %s" % (sm.entry_id(e), bounds)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    inner, scorers = _callback_scorers(c, labels, lm)
    try:
        for scorer, wait in scorers:
            dec = _decoder(c, labels, lm, callback_scorer=scorer)
            if wait is not None:
                dec.set_scorer_wait(wait)
            states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
            out, _ = _feed(torch_mod, dec, states, x, sl, bounds, [e["kernel"]] * (len(bounds) - 1))
            got = _result(out, K, T)
            for want in wants:
                ou.assert_same(_with_nres(got, want), want, "%s wait=%s" % (what, wait))
            # the same decoder class in one call
            one = _decoder(c, labels, lm, callback_scorer=scorer)
            if wait is not None:
                one.set_scorer_wait(wait)
            out1, _ = _feed(torch_mod, one, [ctcdecode_amd.DecoderState(one) for _ in range(B)], x, sl, [0, T], [e["kernel"]])
            ou.assert_same(_with_nres(_result(out1, K, T), wants[0]), wants[0], "%s wait=%s: one call" % (what, wait))
            if scorer is not None:
                assert scorer.callback_calls() > 0
    finally:
        if inner is not None:
            inner.close()


@pytest.mark.parametrize("e", [e for e in sm.STREAM_CASES if not e["production"]], ids=sm.entry_id)
def test_peek_and_compact_behind_every_instantiation(torch_mod, wide99, monkeypatch, e):
    """The walk of test_gpu_stream_compact.py over the entry's ragged batch and bounds: peeks (n_best in {1, K}, since in {0, stable})
    at every boundary against the oracle's decode of the frames so far, a compaction of all streams at every second boundary (kept
    nodes = the oracle's live set; later peeks and the end unchanged).  Callback-scorer streams cannot be peeked; they compact.
    (Every key once: the serving-route entries of the OCC2 keys park through the same kernels as their switch-forced twins, and a walk
    over their CU count + 8 streams costs a minute of oracle decodes.)"""
    c = e["case"]
    labels, lm, lp, sl, _ = _setup(torch_mod, wide99, monkeypatch, c)
    kw = sm.oracle_args(c)
    inner, scorers = _callback_scorers(c, labels, lm)
    try:
        _walk_device(torch_mod, lp, kw, 2, labels=labels, lm=(lm[2], lm[3], lm[0]) if lm else None,
                     scorer=ou.Scorer(lm[2], lm[3], lm[0], labels, "restated") if lm else None, which="restated" if lm else None, late=0,
                     peeks=not c["callback"], bounds=sm.bounds(e), seq_lens=sl, configure=_configure(c), kernel=e["kernel"],
                     layout=km.expected_layout(e["kernel"]), decoder_scorer=scorers[0][0], check=bool(c["callback"]))
    finally:
        if inner is not None:
            inner.close()


@pytest.mark.parametrize("e", [e for e in sm.STREAM_CASES if not e["production"] and not e["case"]["lm"]], ids=sm.entry_id)
def test_commit_behind_every_instantiation(torch_mod, e):
    """The walk of test_gpu_stream_commit.py over commit_inputs (the entry's ragged batch and the fading item) at commit_bounds:
    every chunk that holds a frame launches the entry's kernel and layout; all streams are committed twice after every chunk but the
    last -- count, labels, absolute time steps and kept nodes per stream against the oracle at that stream's age, the second call
    hands out nothing; peeks (n_best in {1, K}) after every call against the oracle's rows shifted by the committed length; at the
    end committed ++ reported row == the one-shot decode for every row of every stream, against both oracles."""
    c = e["case"]
    lp, sl = sm.commit_inputs(c)
    done = _commit_walk(torch_mod, lp, dict(beam=c["K"], cutoff_top_n=c["top_n"]), 1, bounds=sm.commit_bounds(e), seq_lens=sl, configure=_configure(c),
                        kernel=e["kernel"], layout=km.expected_layout(e["kernel"]), blank_id=c["blank"], cutoff_prob=c["cutoff_prob"])
    assert done[sm.fading_index(c)] >= 2, done


@pytest.mark.parametrize("d", sm.DEEP_WALKS, ids=sm.deep_walk_id)
def test_commit_deep_walk_behind_an_instantiation(torch_mod, d):
    """Two fading items of 128 frames behind the key's kernel, committed every 16 frames: a stream ends with a committed length that
    is no multiple of 32 and more than an express level's labels uncommitted (test_stream_matrix_plan.py proves it on the oracle),
    so the kernel's load_state, its later chunks and finish() follow express pointers laid out in re-rooted coordinates."""
    c, lp, bounds = sm.deep_inputs(d)
    done = _commit_walk(torch_mod, lp, dict(beam=c["K"], cutoff_top_n=c["top_n"]), 1, bounds=bounds, configure=_configure(c), kernel=d["kernel"],
                        layout=km.expected_layout(d["kernel"]), blank_id=c["blank"], cutoff_prob=c["cutoff_prob"])
    assert any(n % 32 != 0 for n in done) and min(done) > 0, done


@pytest.mark.parametrize("direction", ["x_then_y", "y_then_x"])
@pytest.mark.parametrize("h", sm.HAND_OVERS, ids=sm.hand_over_id)
def test_stream_hand_over_between_kernels(torch_mod, wide99, monkeypatch, h, direction):
    """One stream, one kernel for the chunks up to the T // 2 bound and another behind it (stream_matrix_util.HAND_OVERS), both ways:
    last_kernel() on both sides, the end against the oracle's one-shot decode.  `few`: only three of the CU count + 8 streams are fed
    on that side, so that the batch does not outnumber the CUs (the others wait, or join with their first frame)."""
    import ctcdecode_amd

    ncu = _cu_count(torch_mod)
    c = dict(h["case"], B=h["case"]["B"] or ncu + sm.PRODUCTION_EXTRA)
    labels, lm, lp, sl, wants = _setup(torch_mod, wide99, monkeypatch, c)
    B, T, K = c["B"], c["T"], c["K"]
    bounds = sm.plain_bounds(T)
    m = bounds.index(T // 2)
    sides = [(h["x"], h["kernel_x"]), (h["y"], h["kernel_y"])]
    if direction == "y_then_x":
        sides.reverse()
    n = len(bounds) - 1
    kernels = [sides[0][1]] * m + [sides[1][1]] * (n - m)
    # the streams that are handed over: without a scorer the tie item and the degenerate item are among them
    few = [0, 1, 2] if c["lm"] or B == 3 else [0, 2, km.degenerate_item(c)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec = _decoder(dict(c, **{k: v for k, v in sides[0][0].items() if k != "few"}), labels, lm)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]

    def items_of(side):
        return few if side.get("few") else list(range(B))

    def before(i):
        if i != m:
            return None
        _configure(dict(c, **{k: v for k, v in sides[1][0].items() if k != "few"}))(dec)
        return items_of(sides[1][0])

    # (all streams first, then three: the others are dropped where they stand.  Three first: the others join behind the bound, with
    #  frame T // 2 of their item as their stream's first frame; only the three streams cross the hand-over and are compared)
    out, fed = _feed(torch_mod, dec, states, x, sl, bounds, kernels, before=before, items=items_of(sides[0][0]))
    src = few if "few" in h["x"] else list(range(B))
    got = _result(out, K, T, items=[fed.index(b) for b in src])
    for want in wants:
        w = dict((k, v[src]) for k, v in want.items())
        ou.assert_same(_with_nres(got, w), w, "%s %s: %s -> %s at frame %d" % (h["name"], direction, sides[0][1], sides[1][1], T // 2))


@pytest.mark.parametrize("direction", ["x_then_y", "y_then_x"])
@pytest.mark.parametrize("h", [h for h in sm.HAND_OVERS if not h["case"]["lm"]], ids=sm.hand_over_id)
def test_commit_in_front_of_a_hand_over(torch_mod, h, direction):
    """A re-rooted state across a hand-over: commit_inputs fed as in test_stream_hand_over_between_kernels, and every stream that
    crosses is committed at the T // 2 bound, directly before the switch (count, labels, time steps, kept nodes against the oracle at
    the stream's age; the fading item commits labels there).  last_kernel() on both sides; the end: committed ++ reported row ==
    the one-shot decode, against both oracles."""
    import ctcdecode_amd

    ncu = _cu_count(torch_mod)
    c = dict(h["case"], B=h["case"]["B"] or ncu + sm.PRODUCTION_EXTRA)
    lp, sl = sm.commit_inputs(c)
    fade = sm.fading_index(c)
    B, T, K = c["B"] + 1, c["T"], c["K"]
    args = sm.oracle_args(c)
    oracles = ["restated"] + (["reference"] if ou.have_reference() else [])
    bounds = sm.hand_over_commit_bounds(h)
    mid = sm.hand_over_commit_mid(h)
    m = bounds.index(mid)
    sides = [(h["x"], h["kernel_x"]), (h["y"], h["kernel_y"])]
    if direction == "y_then_x":
        sides.reverse()
    n = len(bounds) - 1
    kernels = [sides[0][1]] * m + [sides[1][1]] * (n - m)
    few = sm.hand_over_few(c)
    src = few if "few" in h["x"] else list(range(B))  # the streams that cross the hand-over
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec = _decoder(dict(c, **{k: v for k, v in sides[0][0].items() if k != "few"}), [str(i) for i in range(c["V"])], None)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    committed = {}

    def items_of(side):
        return few if side.get("few") else list(range(B))

    def before(i):
        if i != m:
            return None
        got = dec.commit([states[b] for b in src])
        for j, b in enumerate(src):
            F = min(int(sl[b]), mid)
            what = "%s %s: commit of stream %d at frame %d" % (h["name"], direction, b, F)
            want = pu.oracle_prefix(lp[b:b + 1], F, oracles[-1], **args)
            k = max(0, pu.common_prefix_len(want, 0) - 1)
            g_tok, g_ts = got[j][0].numpy(), got[j][1].numpy()
            assert len(g_tok) == k == len(g_ts), "%s: %d labels committed, want %d" % (what, len(g_tok), k)
            assert np.array_equal(g_tok, want["tokens"][0, 0, :k]) and np.array_equal(g_ts, want["timesteps"][0, 0, :k]), what
            assert states[b].committed_len == k and states[b].pool_nodes == cu.oracle_live_count(want, 0) - k, "%s: nodes kept" % what
            committed[b] = (g_tok, g_ts)
        assert len(committed[fade][0]) > 0, "the commit in front of the hand-over handed the fading item nothing"
        _configure(dict(c, **{k: v for k, v in sides[1][0].items() if k != "few"}))(dec)
        return items_of(sides[1][0])

    out, fed = _feed(torch_mod, dec, states, x, sl, bounds, kernels, before=before, items=items_of(sides[0][0]))
    assert sorted(committed) == sorted(src)
    for b in src:
        F = int(sl[b])
        for oracle in oracles:
            what = "%s %s: %s -> %s at frame %d, stream %d (%s oracle)" % (h["name"], direction, sides[0][1], sides[1][1], mid, b, oracle)
            want = pu.oracle_prefix(lp[b:b + 1], F, oracle, **args)
            mu.assert_committed_prefix(want, 0, committed[b][0], committed[b][1], what + ": committed")
            mu.assert_final(_final(out, fed.index(b), K, F, want), want, 0, len(committed[b][0]), what)


def test_stream_hand_over_through_the_automatic_subtree_switch(torch_mod):
    """PROF 0 <-> 3 as serving gets it: the shape statistic of a checked chunk chooses the next chunk's build.  Blank-dominated rows
    (the first chunk runs the plain build and reports chains, the second runs the subtree search), then random rows (bushy beams:
    back to the plain build).  Both switches must happen, and the stream must end like the oracle's one-shot decode."""
    import ctcdecode_amd

    a = sm.AUTO_SUBTREE
    V, K, B, bounds = a["V"], a["K"], a["B"], a["bounds"]
    T, nb = bounds[-1], a["blank_frames"]
    lp = np.concatenate([ou.synth_logprobs(B, nb, V, a["seed"], blank_bias=a["blank_bias"]), ou.synth_logprobs(B, T - nb, V, a["seed"] + 1)], axis=1)
    want = ou.decode(lp, beam=K, which="restated")
    dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, cutoff_top_n=V, blank_id=0, log_probs_input=True, device="cuda:0")
    dec.set_threads(a["threads"])
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    ran = []
    out = None
    for i in range(len(bounds) - 1):
        out = dec.decode(x[:, bounds[i]:bounds[i + 1]], states, [i == len(bounds) - 2] * B)  # (checked: the statistic is read)
        ran.append(dec.last_kernel())
    print("kernels per chunk:", ran)
    assert all(k[1:] == (0, 1, 0, 1024, 0, 0) for k in ran), ran
    profs = [k[0] for k in ran]
    assert profs[0] == 0 and profs[1] == 3, "the chains of the first chunk did not switch the subtree search on: %s" % profs
    assert profs[-1] == 0, "the bushy beams of the random rows did not switch it off again: %s" % profs
    ou.assert_same(_with_nres(_result(out, K, T), want), want, "automatic subtree switch %s" % profs)
