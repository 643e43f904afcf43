"""-m gpu: OnlineCTCBeamDecoder.compact on the device -- the ctc_stream_compact_* kernels on the parked states of live streams.  What
a compaction keeps is counted against the trie the oracle's own result rows span; every peek and every final result must equal the
oracle's one-shot decode bit for bit however often and wherever the streams were compacted (streams of different ages and a stream
without frames in one call, check=False chunks queued in front of it; a stream compacted on both sides of frame 65535, where the
time steps' high parts travel through the gather and store kernels); the policy bounds a long stream's memory; a block shrinks
exactly when the rule says so."""
import ctypes
import os

import compact_util as cu
import numpy as np
import oracle_util as ou
import peek_util as pu
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _state(dec, frames_hint=0):
    """A DecoderState whose block is sized for frames_hint frames (the class itself always asks for the default, 1024)."""
    import ctcdecode_amd
    from ctcdecode_amd import _native

    if not frames_hint:
        return ctcdecode_amd.DecoderState(dec)
    st = ctcdecode_amd.DecoderState.__new__(ctcdecode_amd.DecoderState)
    st._decoder = dec
    h = ctypes.c_void_p()
    sc = getattr(dec, "_scorer", None)
    _native.check(_native.lib.ctcd_stream_create_lm(dec._handle, ctypes.byref(h), dec._num_labels, dec._beam_width, int(frames_hint),
                                                    sc.handle if sc is not None else None))
    st.state = h
    return st


def _capacity(st):
    from ctcdecode_amd import _native

    return int(_native.lib.ctcd_stream_pool_capacity(st.state))


def _final(out, b, K, F, want):
    tok, sc, ts, ln = out
    got = dict(tokens=np.zeros((1, K, F), np.int32), timesteps=np.zeros((1, K, F), np.int32), scores=sc[b:b + 1].numpy(), lens=ln[b:b + 1].numpy(),
               nres=want["nres"])
    w = min(F, tok.shape[2])
    got["tokens"][0, :tok.shape[1], :w] = tok[b, :, :w].numpy()
    got["timesteps"][0, :ts.shape[1], :w] = ts[b, :, :w].numpy()
    return got


def _peek_view(res, b):
    tok, sc, ts, ln, stable = res
    lens, scores = ln[b].numpy(), sc[b].numpy()
    nres = tok.shape[1]
    while nres > 0 and lens[nres - 1] == 0 and scores[nres - 1] == 0:  # (rows beyond a stream's own n_results are zero)
        nres -= 1
    return dict(tokens=tok[b].numpy(), timesteps=ts[b].numpy(), scores=scores, lens=lens, nres=max(nres, 1), stable=int(stable[b]))


def _walk_device(torch_mod, lp, kw, every, chunk=10, labels=None, lm=None, scorer=None, which=None, late=2, frames_hint=0, peeks=True,
                 bounds=None, seq_lens=None, configure=None, kernel=None, layout=None, decoder_scorer=None, check=False):
    """B streams, the last one `late` chunks younger than the others, and one more that is never fed.  Chunks go in with check=False;
    after every `every`-th call ALL streams are compacted together, twice: kept nodes and pool bound against the oracle's live set at
    each stream's own age.  Peeks (n_best in {1, K}, since in {0, stable}) after every call; every stream's end against the one-shot.

    bounds: the chunk boundaries (default: every `chunk` frames; an empty chunk is fed as one); seq_lens: per-item lengths of a ragged
    batch (every chunk then carries its own seq_lens).  configure(dec): sets the new decoder's switches; kernel / layout: what
    last_kernel() / last_layout() must report after every chunk that held a frame.  decoder_scorer: a CallbackScorer for the decoder
    (`scorer` stays the oracle's); kw may also hold blank_id and cutoff_prob, for the decoder and the oracle alike."""
    import ctcdecode_amd

    which = which or pu.which_oracle()
    B, T, V = lp.shape
    K = kw["beam"]
    labels = labels or [str(i) for i in range(V)]
    dkw = dict(beam_width=K, cutoff_top_n=kw.get("cutoff_top_n", 40), cutoff_prob=kw.get("cutoff_prob", 1.0), blank_id=kw.get("blank_id", 0),
               log_probs_input=True, device="cuda:0")
    if decoder_scorer is not None:
        dkw.update(scorer=decoder_scorer)
    elif lm is not None:
        dkw.update(model_path=lm[2], alpha=lm[0], beta=lm[1])
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, **dkw)
    if configure is not None:
        configure(dec)
    states = [_state(dec, frames_hint) for _ in range(B)]
    idle = _state(dec, frames_hint)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    cache = {}

    def want_at(b, F):
        if (b, F) not in cache:
            cache[(b, F)] = pu.oracle_prefix(lp[b:b + 1], F, which, scorer=scorer, **kw)
        return cache[(b, F)]

    if bounds is None:
        assert (T // chunk) * chunk == T
        bounds = list(range(0, T + 1, chunk))
    assert bounds[0] == 0 and bounds[-1] == T
    item_len = [T] * B if seq_lens is None else [int(v) for v in seq_lens]
    frames = [0] * B  # frames a stream has decoded
    pos = [0] * B     # rows of its item that have been handed over (past a short item's end too)
    steps = len(bounds) - 1
    assert steps > late
    compacted = 0
    out = None
    for c in range(steps):
        n = bounds[c + 1] - bounds[c]
        idx = [b for b in range(B) if b < B - 1 or c >= late]
        rows = torch_mod.stack([x[b, pos[b]:pos[b] + n] for b in idx])
        lens = [max(0, min(item_len[b] - pos[b], n)) for b in idx]
        end = c == steps - 1
        out = dec.decode(rows, [states[b] for b in idx], [end] * len(idx), seq_lens=None if seq_lens is None else torch_mod.tensor(lens, dtype=torch_mod.int32),
                         check=check)
        if n > 0 and kernel is not None:
            assert dec.last_kernel() == tuple(kernel), "chunk %d launched %s, expected %s" % (c, dec.last_kernel(), tuple(kernel))
        if n > 0 and layout is not None:
            assert dec.last_layout() == layout
        for i, b in enumerate(idx):
            pos[b] += n
            frames[b] += lens[i]
        if end:
            break
        if c % every == every - 1:
            sizes = [s.nbytes for s in states]
            live = dec.compact(states + [idle])
            assert live[B] == 1 and idle.pool_nodes == 1, "a stream without frames keeps the root alone"
            for b in range(B):
                want_live = cu.oracle_live_count(want_at(b, frames[b]), 0)
                assert live[b] == want_live, "step %d stream %d F=%d: %d nodes kept, the oracle's rows span %d" % (c, b, frames[b], live[b], want_live)
                if frames[b] > 0:
                    assert states[b].pool_nodes == want_live
                assert states[b].nbytes <= sizes[b]
            sizes = [s.nbytes for s in states]
            assert dec.compact(states + [idle]) == live and [s.nbytes for s in states] == sizes, "a second compaction changed something"
            compacted += 1
        if peeks:
            for nb in sorted({1, K}):
                for use_stable in (False, True):
                    since = [pu.common_prefix_len(want_at(b, frames[b]), 0) if use_stable else 0 for b in idx]
                    res = dec.peek([states[b] for b in idx], n_best=nb, since=since)
                    for i, b in enumerate(idx):
                        pu.assert_peek_equals(_peek_view(res, i), want_at(b, frames[b]), 0, nb, since[i],
                                              "step %d stream %d F=%d n_best=%d since=%d" % (c, b, frames[b], nb, since[i]))
    assert compacted > 0
    for i, b in enumerate(range(B)):
        want = want_at(b, frames[b])
        ou.assert_same(_final(out, i, K, frames[b], want), want, "stream %d: the final result after the compactions" % b)


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("case", pu.five_classes() + [pu.pruned_class()], ids=lambda c: c["name"])
def test_compact_device_changes_nothing_and_keeps_the_oracles_trie(torch_mod, case, every):
    _walk_device(torch_mod, case["lp"], case["kw"], every)


def test_compact_device_small_blocks_grow_between_compactions(torch_mod):
    """frames_hint = 4: the blocks double between the compactions (the grow path copies a compacted pool)."""
    case = pu.five_classes()[0]
    _walk_device(torch_mod, case["lp"], case["kw"], 3, frames_hint=4)


def test_compact_device_with_the_built_in_scorer(torch_mod):
    c = pu.LM_PEEK_CASES[0]
    lp, kw = pu.lm_case_inputs(c)
    path = os.path.join(pu.DATA, c["arpa"])
    which = pu.which_oracle()
    sc = ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which)
    _walk_device(torch_mod, lp, kw, 1, labels=c["labels"], lm=(c["alpha"], c["beta"], path), scorer=sc, which=which)


def test_compact_device_wide_beam(torch_mod):
    """Beam 500 over 29 labels: the parked state the wide-beam layout writes."""
    _walk_device(torch_mod, ou.synth_logprobs(3, 80, 29, 68, quant=0.25), dict(beam=500), 1, chunk=20, late=1)


def test_compact_device_callback_scorer_stream(torch_mod):
    """Streams behind a callback scorer (the built-in tables behind the callback), compacted after every chunk: the kept nodes against
    the oracle's live set, the end against the one-shot decode with the built-in scorer.  (Such streams cannot be peeked.)"""
    import ctcdecode_amd
    from test_gpu_lm import _BuiltinBehindCallback

    c = pu.LM_PEEK_CASES[0]
    lp, kw = pu.lm_case_inputs(c)
    lp = lp[:2]
    path = os.path.join(pu.DATA, c["arpa"])
    which = pu.which_oracle()
    osc = ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which)
    K, T = kw["beam"], lp.shape[1]
    inner = _BuiltinBehindCallback(dict(labels=c["labels"], lm_path=path))
    try:
        cs = ctcdecode_amd.CallbackScorer(inner, inner.vocabulary, inner.order, c["labels"], alpha=c["alpha"], beta=c["beta"], device="cuda:0")
        dec = ctcdecode_amd.OnlineCTCBeamDecoder(c["labels"], beam_width=K, cutoff_top_n=kw["cutoff_top_n"], blank_id=0, log_probs_input=True, device="cuda:0",
                                                 scorer=cs)
        states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
        x = torch_mod.from_numpy(lp).to("cuda:0")
        out = None
        for lo in range(0, T, 20):
            end = lo + 20 >= T
            out = dec.decode(x[:, lo:lo + 20], states, [end, end])
            if not end:
                live = dec.compact(states)
                want = pu.oracle_prefix(lp, lo + 20, which, scorer=osc, **kw)
                assert live == [cu.oracle_live_count(want, b) for b in range(2)], (lo, live)
        want = pu.oracle_prefix(lp, T, which, scorer=osc, **kw)
        for b in range(2):
            one = dict((k, v[b:b + 1]) for k, v in want.items())
            ou.assert_same(_final(out, b, K, T, one), one, "callback-scorer stream %d after the compactions" % b)
    finally:
        inner.close()


def test_compact_device_64_streams_at_random_boundaries(torch_mod):
    """64 streams in one decoder; after every chunk (queued with check=False) a random subset is compacted in one call."""
    import ctcdecode_amd

    which = pu.which_oracle()
    B, T, V, K, chunk = 64, 120, 29, 20, 10
    lp = np.concatenate([ou.synth_logprobs(B // 2, T, V, 72), ou.synth_logprobs(B // 2, T, V, 73, blank_bias=4)])
    dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    rng = np.random.default_rng(74)
    events = 0
    out = None
    for lo in range(0, T, chunk):
        end = lo + chunk == T
        out = dec.decode(x[:, lo:lo + chunk], states, [end] * B, check=False)
        if end:
            break
        pick = [b for b in range(B) if rng.random() < 0.4]
        if not pick:
            continue
        live = dec.compact([states[b] for b in pick])
        want = pu.oracle_prefix(lp, lo + chunk, which, beam=K)
        assert live == [cu.oracle_live_count(want, b) for b in pick], "F=%d" % (lo + chunk)
        assert [states[b].pool_nodes for b in pick] == live
        events += len(pick)
    assert events > B
    want = ou.decode(lp, which=which, beam=K)
    for b in range(B):
        one = dict((k, v[b:b + 1]) for k, v in want.items())
        ou.assert_same(_final(out, b, K, T, one), one, "stream %d of 64" % b)


def test_compact_device_block_shrinks_when_the_rule_says_so(torch_mod):
    """frames_hint = 50 at beam 10.  A compaction at 100 frames (capacity 100 frames: the need, max(501, 2 * live), is more than a
    quarter of it) leaves ctcd_stream_bytes as it is; at 1000 frames the block holds 1600 frames' nodes and the stream moves to one of
    max(501, 2 * live) nodes; a compaction directly after changes nothing again.  The stream ends with the oracle's result."""
    import ctcdecode_amd

    which = pu.which_oracle()
    T, V, K, chunk, hint = 1500, 29, 10, 100, 50
    lp = cu.blank_dominated_long(T, V)
    dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    st = _state(dec, hint)
    assert _capacity(st) == hint * K + 1
    x = torch_mod.from_numpy(lp).to("cuda:0")
    out = None
    for lo in range(0, T, chunk):
        end = lo + chunk == T
        out = dec.decode(x[:, lo:lo + chunk], [st], [end], check=False)
        F = lo + chunk
        if F == 100:
            before, cap = st.nbytes, _capacity(st)
            assert cap == 100 * K + 1
            live = dec.compact([st])[0]
            assert 4 * max(hint * K + 1, 2 * live) > cap, "the inputs do not exercise the rule"
            assert st.nbytes == before and _capacity(st) == cap
        if F == 1000:
            before, cap = st.nbytes, _capacity(st)
            assert cap == 1600 * K + 1
            live = dec.compact([st])[0]
            assert live == cu.oracle_live_count(pu.oracle_prefix(lp, F, which, beam=K), 0)
            need = max(hint * K + 1, 2 * live)
            assert 4 * need <= cap, "the inputs do not exercise the rule"
            assert need <= _capacity(st) < need + K and st.nbytes < before // 4, (need, _capacity(st), st.nbytes, before)
            after = st.nbytes
            assert dec.compact([st])[0] == live and st.nbytes == after
    want = pu.oracle_prefix(lp, T, which, beam=K)
    ou.assert_same(_final(out, 0, K, T, want), want, "after the move to a smaller block")


def test_compact_device_timesteps_beyond_16_bits(torch_mod):
    """test_compact_host_timesteps_beyond_16_bits on the device, at the shape of test_time_steps_beyond_16_bits (3 labels, beam 4): a
    stream across frame 65535, chunks queued with check=False, compacted at frame 65000 and at frame 65600 -- the gather and store
    kernels carry the high parts of the kept nodes' time steps.  A second stream of the same rows is compacted at frame 65600 alone:
    its block has grown to 65536 frames and more, and the move to a smaller one takes nodes with high parts along (the first
    stream's block moves at frame 65000, before any node has one).  Kept nodes and a full peek against the oracle after each
    compaction, time steps past 65535 among them; the end against the one-shot decode."""
    import ctcdecode_amd

    which = pu.which_oracle()
    T, K = 65536 + 300, 4
    lp = ou.synth_logprobs(1, T, 3, 17, blank_bias=2.5)
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(["0", "1", "2"], beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    sts = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
    x = torch_mod.from_numpy(np.concatenate([lp, lp])).to("cuda:0")
    for lo, hi, who in ((0, 65000, [0]), (65000, 65600, [0, 1])):
        dec.decode(x[:, lo:hi], sts, [False, False], check=False)
        want = pu.oracle_prefix(lp, hi, which, beam=K)
        want_live = cu.oracle_live_count(want, 0)
        moves = who[-1:]  # the stream compacted for the first time: its block holds hi frames' nodes
        assert all(4 * 2 * want_live <= _capacity(sts[b]) for b in moves), "the inputs do not exercise the shrink rule"
        before = [sts[b].nbytes for b in who]
        live = dec.compact([sts[b] for b in who])
        assert live == [want_live] * len(who) and [sts[b].pool_nodes for b in who] == live, "F=%d: %s nodes kept, want %d" % (hi, live, want_live)
        assert all(sts[b].nbytes < n // 4 for b, n in zip(who, before) if b in moves), "F=%d: the block did not move to a smaller one" % hi
        assert dec.compact([sts[b] for b in who]) == live, "F=%d: a second compaction changed something" % hi
        res = dec.peek([sts[b] for b in who], n_best=K)
        for i in range(len(who)):
            pu.assert_peek_equals(_peek_view(res, i), want, 0, K, 0, "F=%d stream %d after the compaction" % (hi, who[i]))
        if hi > 65536:
            assert all(int(res[2][i].max()) > 65535 for i in range(len(who))), "no kept node's time step lies past frame 65535"
    out = dec.decode(x[:, 65600:], sts, [True, True], check=False)
    final = pu.oracle_prefix(lp, T, which, beam=K)
    for b in range(2):
        ou.assert_same(_final(out, b, K, T, final), final, "T > 65536 after the compactions (stream %d)" % b)
    assert int(out[2].max()) > 65535


def test_compact_device_policy_bounds_the_capacity(torch_mod):
    """The host test's stream on the device: 3000 blank-dominated frames in 100-frame chunks (check=False) from frames_hint = 200 at
    beam 10.  compact_pool_above=1: capacity <= max(initial, 2 * (L_max + 100 * beam)) nodes throughout; without it the capacity reaches
    3000 * beam.  Both end with the oracle's result."""
    import ctcdecode_amd

    which = pu.which_oracle()
    T, V, K, chunk, hint = 3000, 29, 10, 100, 200
    lp = cu.blank_dominated_long(T, V)
    want = pu.oracle_prefix(lp, T, which, beam=K)
    l_max = max(cu.oracle_live_count(pu.oracle_prefix(lp, F, which, beam=K), 0) for F in range(chunk, T, chunk))
    x = torch_mod.from_numpy(lp).to("cuda:0")
    peaks = {}
    for above in (1, None):
        dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0",
                                                 compact_pool_above=above)
        st = _state(dec, hint)
        initial = _capacity(st)
        assert initial == hint * K + 1
        peak, peak_bytes = initial, st.nbytes
        out = None
        for lo in range(0, T, chunk):
            out = dec.decode(x[:, lo:lo + chunk], [st], [lo + chunk == T], check=False)
            peak, peak_bytes = max(peak, _capacity(st)), max(peak_bytes, st.nbytes)
            assert st.pool_nodes <= _capacity(st)
        ou.assert_same(_final(out, 0, K, T, want), want, "compact_pool_above=%s: the final result" % above)
        peaks[above] = (initial, peak, peak_bytes)
    print("L_max %d; policy on: %s; off: %s" % (l_max, peaks[1], peaks[None]))
    assert peaks[1][1] <= max(peaks[1][0], 2 * (l_max + chunk * K)), (peaks[1], l_max)
    assert peaks[None][1] >= T * K and peaks[None][2] > 4 * peaks[1][2], peaks


def test_compact_refusals_leave_the_decoder_usable(torch_mod):
    import ctcdecode_amd
    from ctcdecode_amd import _native

    V, K, T = 29, 20, 40
    lp = ou.synth_logprobs(2, T, V, 69)
    labels = [str(i) for i in range(V)]
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    wide = ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=K + 5, blank_id=0, log_probs_input=True, device="cuda:0")
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec.decode(x[:, :20], states, [False, False], check=False)
    assert dec.compact([]) == []
    with pytest.raises(ValueError):
        dec.compact([states[0], ctcdecode_amd.DecoderState(wide)])  # (a state of another decoder: refused by the class)
    with pytest.raises(ValueError):
        dec.compact([states[0], states[0]])
    arr = (ctypes.c_void_p * 2)(states[0].state.value, ctcdecode_amd.DecoderState(wide).state.value)
    stream = torch_mod.cuda.current_stream().cuda_stream
    assert _native.lib.ctcd_stream_compact(dec._handle, arr, 2, None, stream) == -1  # CTCD_EINVAL: another beam width
    with pytest.raises(ValueError):
        ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=K, device="cuda:0", compact_pool_above=0)
    assert _native.lib.ctcd_set_stream_compaction(dec._handle, -1) == -1
    live = dec.compact(states)
    want20 = pu.oracle_prefix(lp, 20, pu.which_oracle(), beam=K)
    assert live == [cu.oracle_live_count(want20, b) for b in range(2)]
    out = dec.decode(x[:, 20:], states, [True, True])
    want = ou.decode(lp, which=pu.which_oracle(), beam=K)
    for b in range(2):
        one = dict((k, v[b:b + 1]) for k, v in want.items())
        ou.assert_same(_final(out, b, K, T, one), one, "after the refused compactions")
