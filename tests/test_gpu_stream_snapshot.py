"""-m gpu: OnlineCTCBeamDecoder.save / restore on the device -- the ctc_stream_export_kernel / ctc_stream_import_kernel pair around
the compaction.  A stream that is saved, dropped and restored (into the same decoder, a second one, one that launches another kernel,
one whose scorer was built separately) goes on bit-identically: every peek after the restore equals the peek before the save and the
oracle's decode of the frames fed so far, every end is the oracle's one-shot decode (with the committed labels removed, where the
stream had committed); the image has the format's size for the oracle's live trie, is canonical, and equals the host twin's image of
the same stream byte for byte; what must be refused is refused and leaves decoder and streams usable."""
import os

import commit_util as mu
import compact_util as cu
import numpy as np
import oracle_util as ou
import peek_util as pu
import pytest
import snapshot_util as su
from test_gpu_stream_compact import _capacity, _final, _peek_view, _state

pytestmark = pytest.mark.gpu

FIXED_1024 = (0, 0, 1, 0, 1024, 0, 0)
FIXED_RUNTIME_THREADS = (0, 0, 1, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _dec(labels, K, **kw):
    import ctcdecode_amd
    from ctcdecode_amd import _native

    labels = [str(i) for i in range(labels)] if isinstance(labels, int) else labels
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0", **kw)
    _native.check(_native.lib.ctcd_set_subtree_search(dec._handle, 0))
    _native.check(_native.lib.ctcd_set_cu_sharing(dec._handle, 0))
    return dec


def _peeks(dec, states, K):
    return [(nb, dec.peek(states, n_best=nb)) for nb in sorted({1, K})]


def _assert_peeks(dec, states, K, wants, before, what, committed=None):
    """The peeks now equal `before` (if given) and the oracle (wants[b]: the one-item decode of stream b's frames so far)."""
    now = _peeks(dec, states, K)
    for i, (nb, res) in enumerate(now):
        for b in range(len(states)):
            got = _peek_view(res, b)
            C = committed[b] if committed else 0
            pu.assert_peek_equals(got, mu.shifted(wants[b], 0, C), 0, nb, 0, "%s stream %d n_best=%d" % (what, b, nb))
            if before is not None:
                old = _peek_view(before[i][1], b)
                for k in ("tokens", "timesteps", "lens"):
                    assert np.array_equal(got[k], old[k]), "%s stream %d: the peek's %s changed over save / restore" % (what, b, k)
                assert np.array_equal(got["scores"].view(np.uint32), old["scores"].view(np.uint32)) and got["stable"] == old["stable"], what
    return now


def _assert_images(blobs, K, lm, wants, frames, what, committed=None):
    import ctcdecode_amd

    for b, blob in enumerate(blobs):
        assert blob.dtype == np.uint8 or str(blob.dtype) == "torch.uint8"
        assert not blob.is_cuda and blob.dim() == 1
        M = cu.oracle_live_count(wants[b], 0) - (committed[b] if committed else 0) if frames[b] > 0 else 1
        inf = ctcdecode_amd.snapshot_info(blob)
        assert (inf["nodes"], inf["frames"], inf["beam"], inf["scorer_kind"]) == (M, frames[b], K, 1 if lm else 0), (what, b, inf, M)
        assert blob.numel() == su.image_bytes(K, lm, M) == inf["bytes"], (what, b, blob.numel(), M)
    return [int(ctcdecode_amd.snapshot_info(blob)["nodes"]) for blob in blobs]


def _ends(out, K, T, want, what, committed=None):
    for b in range(out[0].shape[0]):
        one = su.one(want, b)
        if committed:
            mu.assert_final(_final(out, b, K, T, dict(nres=one["nres"])), want, b, committed[b], "%s stream %d" % (what, b))
        else:
            ou.assert_same(_final(out, b, K, T, one), one, "%s stream %d" % (what, b))


def _walk(torch_mod, lp, kw, chunk, save_after, labels=None, dec_kw=None, dec2_kw=None, scorer=None, hint=0):
    """B streams fed in chunks; after the chunks in save_after: peek, save, drop the states, restore into the OTHER decoder, peek.
    -> node counts of the images."""
    which = pu.which_oracle()
    B, T, V = lp.shape
    K = kw["beam"]
    okw = dict(kw)
    decs = [_dec(labels or V, K, cutoff_top_n=kw.get("cutoff_top_n", 40), **(dec_kw or {})),
            _dec(labels or V, K, cutoff_top_n=kw.get("cutoff_top_n", 40), **(dec2_kw or dec_kw or {}))]
    import ctcdecode_amd

    cur = 0
    states = [ctcdecode_amd.DecoderState(decs[0]) for _ in range(B)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    nodes = []
    out = None
    for c in range(T // chunk):
        end = c == T // chunk - 1
        out = decs[cur].decode(x[:, c * chunk:(c + 1) * chunk], states, [end] * B, check=False)
        F = (c + 1) * chunk
        if end or c + 1 not in save_after:
            continue
        wants = [pu.oracle_prefix(lp[b:b + 1], F, which, scorer=scorer, **okw) for b in range(B)]
        before = _assert_peeks(decs[cur], states, K, wants, None, "before the save at F=%d" % F)
        blobs = decs[cur].save(states)
        nodes += _assert_images(blobs, K, scorer is not None, wants, [F] * B, "F=%d" % F)
        again = decs[cur].save(states)
        assert all(torch_mod.equal(a, b) for a, b in zip(blobs, again)), "a second save gives other bytes"
        del states
        cur = 1 - cur
        states = decs[cur].restore([bytes(blobs[0].numpy().tobytes())] + list(blobs[1:]), frames_hint=hint)
        assert [s.frames for s in states] == [F] * B
        _assert_peeks(decs[cur], states, K, wants, before, "after the restore at F=%d" % F)
        third = decs[cur].save(states)
        assert all(torch_mod.equal(a, b) for a, b in zip(blobs, third)), "save -> restore -> save gives other bytes"
    _ends(out, K, T, pu.oracle_prefix(lp, T, which, scorer=scorer, **okw), "the end")
    return nodes


def test_save_restore_randn_into_a_second_decoder(torch_mod):
    lp = ou.synth_logprobs(3, 120, 29, 61)
    nodes = _walk(torch_mod, lp, dict(beam=20), 20, (2, 4))
    assert len(nodes) == 6 and all(m % 256 != 0 and m > 20 for m in nodes), nodes


def test_save_restore_beyond_the_express_levels(torch_mod):
    """peaky rows saved where row 0 is more than 64 labels long: the express words of depths 32 and 64 travel -- the peek from depth 0
    (in _walk) and the stream's end walk through them."""
    case = pu.five_classes()[4]
    lp, kw = case["lp"][:, :300], case["kw"]
    want = pu.oracle_prefix(lp, 200, pu.which_oracle(), **kw)
    assert all(int(want["lens"][b, 0]) > 64 for b in range(3)), want["lens"][:, 0]
    _walk(torch_mod, lp, kw, 100, (2,))


@pytest.mark.parametrize("shape", ["pruned", "beam500", "beam1"])
def test_save_restore_pruned_wide_and_single_beams(torch_mod, shape):
    if shape == "pruned":
        case = pu.pruned_class()
        _walk(torch_mod, case["lp"], case["kw"], 30, (1, 3))
    elif shape == "beam500":
        _walk(torch_mod, ou.synth_logprobs(2, 40, 29, 67), dict(beam=500), 10, (1, 3))
    else:
        _walk(torch_mod, ou.synth_logprobs(3, 120, 29, 61), dict(beam=1), 20, (2, 4), hint=4)


def test_one_call_with_streams_of_three_ages_a_fresh_one_and_a_one_frame_one(torch_mod):
    import ctcdecode_amd

    which = pu.which_oracle()
    lp = ou.synth_logprobs(5, 90, 29, 68)
    K, T = 20, 90
    dec, dec2 = _dec(29, K), _dec(29, K)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(5)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    ages = [60, 30, 10, 0, 1]
    for b, F in enumerate(ages):  # stream 3 is never fed
        for lo in range(0, F, 10):
            dec.decode(x[b:b + 1, lo:min(F, lo + 10)], [states[b]], [False], check=False)
    wants = [pu.oracle_prefix(lp[b:b + 1], F, which, beam=K) for b, F in enumerate(ages)]
    before = _assert_peeks(dec, states, K, wants, None, "before the save")
    blobs = dec.save(states)
    _assert_images(blobs, K, False, wants, ages, "five ages")
    assert blobs[3].numel() == su.image_bytes(K, False, 1)
    assert [s.frames for s in states] == ages
    new = dec2.restore(blobs)
    assert [s.frames for s in new] == ages and [s.pool_nodes for s in new] == [s.pool_nodes for s in states]
    _assert_peeks(dec2, new, K, wants, before, "after the restore")
    final = ou.decode(lp, which=which, beam=K)
    for d, sts, what in ((dec, states, "the saved streams"), (dec2, new, "the restored streams")):
        for b, F in enumerate(ages):
            out = d.decode(x[b:b + 1, F:], [sts[b]], [True])
            ou.assert_same(_final(out, 0, K, T, su.one(final, b)), su.one(final, b), "%s: stream %d" % (what, b))


def test_commit_save_restore_commit(torch_mod):
    import ctcdecode_amd

    which = pu.which_oracle()
    case = pu.five_classes()[0]
    lp, K = case["lp"][:, :160], case["kw"]["beam"]
    T = 160
    dec, dec2 = _dec(29, K), _dec(29, K)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(3)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec.decode(x[:, :80], states, [False] * 3, check=False)
    first = dec.commit(states)
    C = [len(t) for t, _ in first]
    assert max(C) > 0 and [s.committed_len for s in states] == C
    w80 = [pu.oracle_prefix(lp[b:b + 1], 80, which, beam=K) for b in range(3)]
    blobs = dec.save(states)
    _assert_images(blobs, K, False, w80, [80] * 3, "after a commit", committed=C)
    assert [ctcdecode_amd.snapshot_info(b)["committed"] for b in blobs] == C
    del states
    new = dec2.restore(blobs)
    assert [s.committed_len for s in new] == C
    _assert_peeks(dec2, new, K, w80, None, "after commit, save, restore", committed=C)
    dec2.decode(x[:, 80:120], new, [False] * 3, check=False)
    w120 = [pu.oracle_prefix(lp[b:b + 1], 120, which, beam=K) for b in range(3)]
    second = dec2.commit(new)
    for b in range(3):
        m = max(0, pu.common_prefix_len(w120[b], 0) - 1 - C[b])
        assert len(second[b][0]) == m
        assert np.array_equal(second[b][0].numpy(), w120[b]["tokens"][0, 0, C[b]:C[b] + m]), "stream %d: the commit after the restore" % b
        assert np.array_equal(second[b][1].numpy(), w120[b]["timesteps"][0, 0, C[b]:C[b] + m])
        C[b] += m
    assert sum(len(t) for t, _ in second) > 0
    out = dec2.decode(x[:, 120:], new, [True] * 3)
    _ends(out, K, T, ou.decode(lp, which=which, beam=K), "commit, save, restore, commit", committed=C)


@pytest.mark.parametrize("policy", [None, 64])
def test_restore_into_a_small_block_that_grows(torch_mod, policy):
    import ctcdecode_amd

    which = pu.which_oracle()
    lp = ou.synth_logprobs(2, 140, 29, 69)
    K, T = 20, 140
    dec = _dec(29, K)
    dec2 = _dec(29, K, **({} if policy is None else dict(compact_pool_above=policy)))
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec.decode(x[:, :40], states, [False] * 2, check=False)
    blobs = dec.save(states)
    M = [ctcdecode_amd.snapshot_info(b)["nodes"] for b in blobs]
    new = dec2.restore(blobs, frames_hint=4)
    assert [_capacity(s) for s in new] == [max(4, (2 * m - 1 + K - 1) // K) * K + 1 for m in M]
    assert [s.pool_nodes for s in new] == M
    small = [s.nbytes for s in new]
    assert all(a < b.nbytes for a, b in zip(small, states))
    for lo in range(40, 140, 10):
        out = dec2.decode(x[:, lo:lo + 10], new, [lo == 130] * 2, check=False)
        if lo == 120:
            assert all(s.nbytes > a for s, a in zip(new, small)), "the blocks did not grow"
            if policy:
                assert all(s.pool_nodes < m + 90 * K for s, m in zip(new, M)), "the compaction policy did not continue after the restore"
    _ends(out, K, T, ou.decode(lp, which=which, beam=K), "grown after a restore (policy %s)" % policy)


def test_hand_over_from_1024_threads_to_512(torch_mod):
    import ctcdecode_amd

    which = pu.which_oracle()
    case = pu.five_classes()[0]
    lp, K = case["lp"][:, :160], case["kw"]["beam"]
    dec, dec2 = _dec(29, K), _dec(29, K)
    dec.set_threads(1024)
    dec2.set_threads(512)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(3)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    for lo in (0, 40):
        dec.decode(x[:, lo:lo + 40], states, [False] * 3)
        assert dec.last_kernel() == FIXED_1024, dec.last_kernel()
    new = dec2.restore(dec.save(states))
    for lo in (80, 120):
        out = dec2.decode(x[:, lo:lo + 40], new, [lo == 120] * 3)
        assert dec2.last_kernel() == FIXED_RUNTIME_THREADS, dec2.last_kernel()
    _ends(out, K, 160, ou.decode(lp, which=which, beam=K), "1024 threads, then 512")


@pytest.mark.parametrize("c", [pu.LM_PEEK_CASES[0], pu.LM_PEEK_CASES[3]], ids=lambda c: c["name"])
def test_builtin_scorer_streams_travel(torch_mod, c):
    lp, kw = pu.lm_case_inputs(c)
    path = os.path.join(pu.DATA, c["arpa"])
    sc = ou.Scorer(c["alpha"], c["beta"], path, c["labels"], pu.which_oracle())
    mk = dict(model_path=path, alpha=c["alpha"], beta=c["beta"])  # (each decoder builds its scorer from the file on its own)
    nodes = _walk(torch_mod, lp, kw, 20, (2, 3), labels=c["labels"], dec_kw=mk, scorer=sc)
    assert len(nodes) == 6


def test_scorer_mismatches_and_callback_streams_are_refused(torch_mod):
    import ctcdecode_amd
    from test_gpu_lm import _BuiltinBehindCallback

    which = pu.which_oracle()
    c = pu.LM_PEEK_CASES[0]
    lp, kw = pu.lm_case_inputs(c)
    lp = lp[:2]
    path = os.path.join(pu.DATA, c["arpa"])
    K, T = kw["beam"], lp.shape[1]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    osc = ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which)
    want = pu.oracle_prefix(lp, T, which, scorer=osc, **kw)
    dec = _dec(c["labels"], K, cutoff_top_n=kw["cutoff_top_n"], model_path=path, alpha=c["alpha"], beta=c["beta"])
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
    dec.decode(x[:, :60], states, [False, False])
    blobs = dec.save(states)
    assert all(ctcdecode_amd.snapshot_info(b)["scorer_kind"] == 1 and ctcdecode_amd.snapshot_info(b)["fingerprint"] != 0 for b in blobs)
    other_model = _dec(c["labels"], K, cutoff_top_n=kw["cutoff_top_n"], model_path=os.path.join(pu.DATA, "chars.arpa"), alpha=0.6, beta=0.2)
    no_model = _dec(c["labels"], K, cutoff_top_n=kw["cutoff_top_n"])
    for d, word in ((other_model, "fingerprint"), (no_model, "scorer kind")):
        with pytest.raises(ValueError, match=word):
            d.restore(blobs)
    plain = [ctcdecode_amd.DecoderState(no_model)]
    no_model.decode(x[:1, :60], plain, [False])
    with pytest.raises(ValueError, match="scorer kind"):
        dec.restore(no_model.save(plain))
    # other alpha / beta: the same tables, the same fingerprint -- the image is taken (reset_params may change them mid-stream)
    tuned = _dec(c["labels"], K, cutoff_top_n=kw["cutoff_top_n"], model_path=path, alpha=0.1, beta=0.1)
    assert len(tuned.restore(blobs)) == 2
    out = dec.decode(x[:, 60:], states, [True, True])
    _ends(out, K, T, want, "the saved scorer streams decode on")
    inner = _BuiltinBehindCallback(dict(labels=c["labels"], lm_path=path))
    try:
        cs = ctcdecode_amd.CallbackScorer(inner, inner.vocabulary, inner.order, c["labels"], alpha=c["alpha"], beta=c["beta"], device="cuda:0")
        cdec = ctcdecode_amd.OnlineCTCBeamDecoder(c["labels"], beam_width=K, cutoff_top_n=kw["cutoff_top_n"], blank_id=0, log_probs_input=True,
                                                  device="cuda:0", scorer=cs)
        cstates = [ctcdecode_amd.DecoderState(cdec) for _ in range(2)]
        cdec.decode(x[:, :60], cstates, [False, False])
        nodes = [s.pool_nodes for s in cstates]
        with pytest.raises(NotImplementedError):
            cdec.save(cstates)
        with pytest.raises(NotImplementedError):
            cdec.restore(blobs)
        assert [s.pool_nodes for s in cstates] == nodes, "the refused save touched the streams"
        out = cdec.decode(x[:, 60:], cstates, [True, True])
        _ends(out, K, T, want, "callback-scorer streams after the refused save")
    finally:
        inner.close()


def test_64_streams_saved_in_random_subsets_behind_unchecked_chunks(torch_mod):
    import ctcdecode_amd

    which = pu.which_oracle()
    B, T, K = 64, 60, 20
    lp = ou.synth_logprobs(B, T, 29, 70)
    dec, dec2 = _dec(29, K), _dec(29, K)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    home = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    where = [0] * B  # the decoder a stream lives in
    states = list(home)
    rng = np.random.default_rng(5)
    moved = 0
    out = {}
    for c in range(6):
        for side, d in ((0, dec), (1, dec2)):
            idx = [b for b in range(B) if where[b] == side]
            if idx:
                res = d.decode(x[idx, c * 10:(c + 1) * 10], [states[b] for b in idx], [c == 5] * len(idx), check=False)
                if c == 5:
                    out[side] = (idx, res)
        if c == 5:
            break
        pick = [b for b in rng.permutation(B)[:int(rng.integers(8, 24))] if where[b] == 0]
        blobs = dec.save([states[b] for b in pick])
        go = pick[::2]  # half are restored into the second decoder, half continue in place
        new = dec2.restore([blobs[i] for i in range(0, len(pick), 2)])
        for b, st in zip(go, new):
            states[b], where[b] = st, 1
        moved += len(go)
    assert moved >= 16 and 0 in out and 1 in out
    want = ou.decode(lp, which=which, beam=K)
    for side in (0, 1):
        idx, res = out[side]
        for i, b in enumerate(idx):
            ou.assert_same(_final(res, i, K, T, su.one(want, b)), su.one(want, b), "stream %d (decoder %d)" % (b, side))


def test_save_restore_on_both_sides_of_frame_65535(torch_mod):
    """A beam-4 stream with a commit, a save and a restore at frames 65000 and 65600: the committed and the kept time steps past frame
    65535 are the oracle's (the high parts of the kept nodes' time steps travel)."""
    import ctcdecode_amd

    which = pu.which_oracle()
    T, K = 65536 + 300, 4
    lp = ou.synth_logprobs(1, T, 3, 17, blank_bias=2.5)
    decs = [_dec(3, K), _dec(3, K)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    states = [ctcdecode_amd.DecoderState(decs[0])]
    tok, ts = np.zeros((0,), np.int32), np.zeros((0,), np.int32)
    cur = 0
    for lo, hi in ((0, 65000), (65000, 65600)):
        decs[cur].decode(x[:, lo:hi], states, [False], check=False)
        g = decs[cur].commit(states)[0]
        tok, ts = np.concatenate([tok, g[0].numpy()]), np.concatenate([ts, g[1].numpy()])
        want = pu.oracle_prefix(lp, hi, which, beam=K)
        before = _assert_peeks(decs[cur], states, K, [want], None, "F=%d" % hi, committed=[len(tok)])
        blobs = decs[cur].save(states)
        _assert_images(blobs, K, False, [want], [hi], "F=%d" % hi, committed=[len(tok)])
        del states
        cur = 1 - cur
        states = decs[cur].restore(blobs, frames_hint=4)
        now = _assert_peeks(decs[cur], states, K, [want], before, "restored at F=%d" % hi, committed=[len(tok)])
        if hi > 65536:
            assert int(now[-1][1][2].max()) > 65535, "no kept time step lies past frame 65535"
    out = decs[cur].decode(x[:, 65600:], states, [True])
    final = pu.oracle_prefix(lp, T, which, beam=K)
    mu.assert_committed_prefix(final, 0, tok, ts, "T > 65536: committed")
    mu.assert_final(_final(out, 0, K, T, dict(nres=final["nres"])), final, 0, len(tok), "T > 65536 after two restores")
    assert int(out[2].max()) > 65535


def test_refusals_leave_the_decoder_usable(torch_mod):
    import ctcdecode_amd

    which = pu.which_oracle()
    lp = ou.synth_logprobs(2, 80, 29, 72)
    K, T = 20, 80
    dec, other = _dec(29, K), _dec(29, K)
    wide, more_labels = _dec(29, K + 1), _dec(30, K)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec.decode(x[:, :40], states, [False, False])
    with pytest.raises(ValueError):
        dec.save([states[0], states[0]])
    with pytest.raises(ValueError):
        dec.save([states[0], ctcdecode_amd.DecoderState(other)])
    with pytest.raises(ValueError):
        other.save(states)
    blobs = dec.save(states)
    good = bytes(blobs[0].numpy().tobytes())
    w = su.words(good)
    M, n = int(w[su.W_NODES]), int(w[su.HDR_WORDS + su.S_N])

    def put(i, v):
        m = w.copy()
        m[i] = v
        return m.tobytes()

    bad = [("truncated", good[:-4]), ("truncated", good[:30]), ("magic", put(su.W_MAGIC, 0)), ("version", put(su.W_VERSION, 7)),
           ("beam pool index", put(su.array_word(K, su.A_NODE, 1), M)), ("node parent", put(su.node_word(K, False, M, 5), 5)),
           ("express word", put(su.node_word(K, False, M, 5, 1), 6)), ("order array", put(su.array_word(K, su.A_FIN, 0), n)),
           ("header word", put(su.HDR_WORDS + su.S_POOL, M + 1)), ("node layout", put(su.array_word(K, su.A_NODE, 1), int(w[su.array_word(K, su.A_NODE, 1)]) - 1))]
    from ctcdecode_amd import _native

    free0 = torch_mod.cuda.mem_get_info()[0]
    for word, blob in bad:
        with pytest.raises(ValueError, match=word):
            other.restore([blob])
        # all or nothing: one bad image among good ones creates no stream
        with pytest.raises(ValueError, match="item 1"):
            other.restore([blobs[0], blob, blobs[1]])
    for d in (wide, more_labels):
        with pytest.raises(ValueError):
            d.restore(blobs)
    assert torch_mod.cuda.mem_get_info()[0] >= free0 - (1 << 20), "refused restores left memory allocated"
    assert _native is not None
    new = other.restore(blobs)
    want = ou.decode(lp, which=which, beam=K)
    for d, sts, what in ((dec, states, "the saved streams"), (other, new, "restored after the refusals")):
        _ends(d.decode(x[:, 40:], sts, [True, True]), K, T, want, what)


def test_the_device_image_is_the_host_twins_image(torch_mod):
    """The same rows in the same chunks through the device and through the host twin (tests/native/snapshot_host.cpp): identical
    bytes, for a plain stream, a stream with fewer entries than its beam holds, and a committed one."""
    import ctcdecode_amd

    lp = ou.synth_logprobs(2, 60, 29, 73)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    for K, bounds, commit in ((20, (0, 20, 40), False), (100, (0, 1, 2), False), (20, (0, 30, 50), True)):
        dec = _dec(29, K)
        states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
        twins = [su.HostStream(29, K, 1024) for _ in range(2)]
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            dec.decode(x[:, lo:hi], states, [False, False], check=False)
            for b in range(2):
                twins[b].feed(lp[b, lo:hi])
        if commit:
            dec.commit(states)
            for t in twins:
                t.commit()
        blobs = dec.save(states)
        for b in range(2):
            mine, theirs = bytes(blobs[b].numpy().tobytes()), twins[b].save()
            if mine != theirs:
                a, o = su.words(mine), su.words(theirs)
                diff = np.nonzero(a[:min(len(a), len(o))] != o[:min(len(a), len(o))])[0]
                raise AssertionError("K=%d stream %d: %d vs %d bytes, first differing words %s" % (K, b, len(mine), len(theirs), diff[:12].tolist()))
        # ... and each side takes the other's image
        assert [s.frames for s in dec.restore([twins[0].save(), twins[1].save()])] == [bounds[-1]] * 2
        assert twins[0].restore(bytes(blobs[0].numpy().tobytes()), 4, committed=(twins[0].tokens, twins[0].timesteps)).frames == bounds[-1]
