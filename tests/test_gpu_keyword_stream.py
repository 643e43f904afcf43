"""Keyword search of live streams on the device (include/ctcdecode_amd.h "Keyword search of live streams"): ``KeywordState`` and
``OnlineCTCBeamDecoder.find_keywords``, fed chunk by chunk, against the one-shot restatement of tests/keyword_util.py on the concatenation, bit for bit."""
import numpy as np
import pytest
import torch

import greedy_util as gu
import keyword_stream_util as su
import keyword_util as ku

pytestmark = pytest.mark.gpu


def _decoder(V, blank, mode=1, cls="OnlineCTCBeamDecoder", **kw):
    import ctcdecode_amd
    return getattr(ctcdecode_amd, cls)([str(i) for i in range(V)], blank_id=blank, log_probs_input=mode == 1, device="cuda:0", **kw)


def _states(dec, lists, first=0):
    import ctcdecode_amd
    return [ctcdecode_amd.KeywordState(dec, *map(torch.from_numpy, ku.kw_tensors(kws)), first_frame=first) for kws in lists]


def _play(dec, c, plan, lists=None, first=0, states=None, pos=None, probs=None):
    """Feeds the streams (one per item of the case) the calls of ``plan`` -- (Tc, per-stream lengths or None) -- each stream from where it
    stands, and checks every call against the one-shot result of the stream's item.  -> (states, positions)."""
    B, T, _ = c["x"].shape
    lists = lists or [c["kws"]] * B
    states, pos = states or _states(dec, lists, first), pos or [0] * B
    rows = gu.to_torch(torch, c["stored"], c["dtype"]) if probs is None else probs
    want = [gu.cached(("keyword stream", c["name"], b, first, str(lists[b])), lambda: su.want_of(c["x"][b], T, c["blank"], c["mode"], lists[b], first)) for b in range(B)]
    for Tc, lens in plan:
        chunk = torch.zeros((B, Tc, rows.shape[2]), dtype=rows.dtype, device="cuda")
        for b in range(B):
            chunk[b, :min(Tc, T - pos[b])] = rows[b, pos[b]:pos[b] + Tc]
        outs = dec.find_keywords(chunk, states, [False] * B, None if lens is None else torch.tensor(lens, dtype=torch.int32), details=True)
        assert len(outs) == 8 and all(o.is_cuda for o in outs)
        for b in range(B):
            n = Tc if lens is None else lens[b]
            got = dict(zip(su.KEYS, (o[b].cpu().numpy() for o in outs)))
            su.check_call(got, want[b], pos[b], n, first, "stream %d at frame %d" % (b, pos[b]))
            pos[b] += n
            if pos[b] == T:
                ku.assert_same(got, {k: want[b][k] for k in su.KEYS[:3]}, "stream %d against the one-shot result" % b)
    return states, pos


@pytest.mark.parametrize("dt,mode,V", [(dt, mode, V) for dt in gu.DTYPES for mode in (0, 1) for V in (128, 129)])
def test_every_instantiation(dt, mode, V):
    c = ku.case("stream inst %d %d %d" % (dt, mode, V), dtype=dt, mode=mode, V=V, T=70)
    dec = _decoder(V, c["blank"], mode)
    assert dec.last_keyword_kernel() is None
    _play(dec, c, [(33, None), (1, None), (36, None)])
    assert dec.last_keyword_kernel() == (dt, mode == 0, V <= 128, 8)


@pytest.mark.parametrize("V", (29, 130))
@pytest.mark.parametrize("cuts", ([31, 0, 32, 7], [32, 33, 5], [33, 1, 1, 35], [64, 6]), ids=lambda c: "cut%d" % c[0])
def test_chunk_lengths_around_the_stage(cuts, V):
    c = ku.case("stream cuts V%d" % V, V=V, T=70, L=(2, 5, 1))
    _play(_decoder(V, c["blank"]), c, [(n, None) for n in cuts])


@pytest.mark.parametrize("L", (8, 9, 16, 17, 32, 33, 64))
def test_lane_group_edges(L):
    c = ku.case("stream L%d" % L, dtype=L % 3, mode=L % 2, T=70, B=1, L=(L, max(1, L - 2)))
    dec = _decoder(29, c["blank"], c["mode"])
    _play(dec, c, [(33, None), (37, None)], first=1000)
    assert dec.last_keyword_kernel()[3] == c["kernel"][3]


def test_keyword_count_across_waves_and_workgroups():
    rng = np.random.default_rng(5)
    c = ku.case("stream Q edge", T=40, B=1, kws=[ku._keyword(rng, 1 + q % 8, 28, 0) for q in range(33)])  # 33 keywords (labels 1 .. 27) on 8 lanes each: two workgroups
    _play(_decoder(29, c["blank"]), c, [(17, None), (23, None)])


def test_lists_differ_per_stream_and_lengths_are_ragged():
    c, rng = ku.case("stream ragged", T=40, B=3), np.random.default_rng(9)
    lists = [[ku._keyword(rng, L, 29, c["blank"]) for L in Ls] for Ls in ((3, 8), (1, 8), (8, 2))]  # (one shape of list, [2, 8]; other keywords)
    dec = _decoder(29, c["blank"])
    states, pos = _play(dec, c, [(20, [20, 0, 7]), (33, [5, 33, 0]), (15, [15, 7, 15]), (18, [0, 0, 18])], lists=lists)
    assert pos == [40, 40, 40] and [s.info()["frames"] for s in states] == pos


def _ties(raw):
    """The frames the fused winner must settle as the argmax pass does (V = 29, log-probabilities): the greatest value twice, in columns of
    different lanes and of one lane of the 8; +0.0 and -0.0 the two greatest, in either order; a frame of -inf."""
    for t, (a, b) in ((2, (3, 12)), (5, (4, 20)), (34, (27, 2))):
        raw[:, t, b] = raw[:, t, a] = raw[:, t].max(-1) + 0.25
    raw[:, 7], raw[:, 36] = np.minimum(raw[:, 7], -0.5), np.minimum(raw[:, 36], -0.5)
    raw[:, 7, 6], raw[:, 7, 9], raw[:, 36, 6], raw[:, 36, 9] = 0.0, -0.0, -0.0, 0.0
    raw[:, 9] = raw[:, 40] = -np.inf


def test_the_fused_winner_has_the_argmax_pass_bits():
    c = ku.case("stream ties", T=45, kws=[[3, 6], [12, 9], [6], [9, 4], [20, 27, 2]], edit=_ties)
    dec, rows = _decoder(29, c["blank"]), torch.from_numpy(c["stored"]).cuda()
    states, _ = _play(dec, c, [(33, None), (12, None)])
    outs = dec.find_keywords(rows[:, :0], states, [True, True])  # (an empty call that ends the streams returns the running result)
    assert all(s.ended and s.info()["ended"] for s in states)
    k, lens = ku.kw_tensors(c["kws"])
    one = _decoder(29, c["blank"], cls="CTCBeamDecoder").find_keywords(rows, None, torch.from_numpy(k).cuda(), torch.from_numpy(lens))
    ku.assert_same(dict(zip(su.KEYS, (o.cpu().numpy() for o in outs))), dict(zip(su.KEYS[:3], (o.cpu().numpy() for o in one))), "against the one-shot call")


def test_logits_equal_log_softmax_rows():
    c = ku.case("stream logits", T=40)
    logits = torch.from_numpy(gu.random_rows(np.random.default_rng(3), 2, 40, 29, 2)).cuda()
    rows = _decoder(29, c["blank"], 0, cls="CTCBeamDecoder", logits_input=True).log_softmax(logits)
    c = dict(c, stored=rows.cpu().numpy(), x=rows.cpu().numpy())
    _play(_decoder(29, c["blank"], 0, logits_input=True), c, [(33, None), (7, None)], probs=logits)


def test_reset_reuse_and_refusals_leave_the_streams_intact():
    import ctcdecode_amd
    c = ku.case("stream refusals", T=40)
    dec, rows = _decoder(29, c["blank"]), torch.from_numpy(c["stored"]).cuda()
    states, pos = _play(dec, c, [(25, None)], first=3)
    other = _states(dec, [[[1, 2, 3]]])[0]  # another shape of list
    late = ctcdecode_amd.KeywordState(dec, *map(torch.from_numpy, ku.kw_tensors(c["kws"])), first_frame=2 ** 31 - 1)
    for sts, exc in (([states[0], states[0]], ValueError), ([states[0], other], ValueError), ([states[0], late], NotImplementedError)):
        with pytest.raises(exc):
            dec.find_keywords(rows[:, :1], sts, [False, False])
    _play(dec, c, [(15, None)], first=3, states=states, pos=pos)  # (what was refused fed nothing)
    dec.find_keywords(rows[:, :0], states, [True, True])
    with pytest.raises(ValueError):
        dec.find_keywords(rows[:, :1], states, [False, False])
    for s in states:
        s.reset(7)
    _play(dec, c, [(40, None)], first=7, states=states)


@pytest.mark.parametrize("mode", (0, 1))
def test_a_greedy_label_run_across_a_cut_scores_zero_at_greedy_frames(mode):
    import ctcdecode_amd
    path = [1, 1, 0, 2, 3, 3, 0, 0, 4, 5, 5, 6, 0, 7, 7]  # cut at 4 and 10: inside the runs of 3 and of 5
    x = torch.from_numpy(gu.path_rows(np.random.default_rng(7 + mode), [path], 8, mode)).cuda()
    dec, tok, st, en = _decoder(8, 0, mode), [], [], []
    greedy = [ctcdecode_amd.GreedyState(dec, 100)]
    for lo, hi in ((0, 4), (4, 10), (10, 15)):
        o = [t.cpu() for t in dec.greedy_decode_device(x[:, lo:hi], greedy, [hi == 15], details=True)]
        tok, st, en = tok + o[0][0, 0, :int(o[3])].tolist(), st + o[2][0, 0, :int(o[3])].tolist(), en + o[4][0, 0, :int(o[6])].tolist()
    assert tok == [1, 2, 3, 4, 5, 6, 7]
    runs = [(i, j) for i in range(7) for j in range(i, min(i + 4, 7))]
    states = _states(dec, [[tok[i:j + 1] for i, j in runs]], first=100)
    for lo, hi in ((0, 4), (4, 10), (10, 15)):
        scores, starts, ends = (o.cpu().numpy() for o in dec.find_keywords(x[:, lo:hi], states, [False]))
    assert (scores.view(np.uint32) == 0).all()
    assert starts[0].tolist() == [st[i] for i, _ in runs] and ends[0].tolist() == [en[j] for _, j in runs]
