"""-m gpu: OnlineCTCBeamDecoder.commit on the device -- the ctc_stream_commit_* kernels on the parked states of live streams.  A commit
hands out the oracle's row 0 at the newly final positions and keeps the oracle's live trie below the new root; afterwards every
peek and every final result are the oracle's one-shot decode with the committed labels removed from the front of every row, bit for
bit (streams of three ages and a stream without frames in one call, check=False chunks queued in front of it, kernels of other
layouts and workgroup sizes continuing a committed state, commits on both sides of frame 65535); a block shrinks when the rule says
so; streams with a scorer are refused and decode on.  _walk_device is also the walk of test_gpu_stream_matrix.py, which puts a
committed state in front of every scorer-free instantiation of the decode kernel a stream can launch."""
import os

import commit_util as mu
import compact_util as cu
import numpy as np
import oracle_util as ou
import peek_util as pu
import pytest
from test_gpu_stream_compact import _capacity, _final, _peek_view, _state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _plain_switches(dec):
    """The switches the kernel assertions rely on: no subtree search, one workgroup per CU, the fixed layout where it applies."""
    from ctcdecode_amd import _native

    _native.check(_native.lib.ctcd_set_subtree_search(dec._handle, 0))
    _native.check(_native.lib.ctcd_set_cu_sharing(dec._handle, 0))


def _walk_device(torch_mod, lp, kw, every, chunk=None, starts=None, frames_hint=0, before=None, kernel_of=None, bounds=None, seq_lens=None,
                 configure=None, kernel=None, layout=None, blank_id=0, cutoff_prob=1.0):
    """B streams, stream b first fed at call starts[b] (default 0, 1, 2, ...: streams of different ages), and one more that is never
    fed.  Chunks go in with check=False; after every `every`-th call ALL streams are committed together, twice: counts, labels, time
    steps and kept nodes against the oracle at each stream's own age; the second call commits nothing.  Peeks (n_best in {1, K},
    since in {0, stable'}) after every call against the oracle with the offset applied; every stream's end: committed ++ rows == the
    one-shot decode.  before(c, dec): called in front of call c; kernel_of(c): what last_kernel() must report after it.

    bounds: the chunk boundaries instead of `chunk` (an empty chunk is fed as one); every stream is then fed from call 0 on and ends
    at the last call.  seq_lens: per-item lengths of a ragged batch (every chunk carries its own seq_lens; a stream's age is the
    frames of its item fed so far).  configure(dec): sets the new decoder's switches (default: _plain_switches); kernel / layout: what
    last_kernel() / last_layout() must report after every chunk that held a frame; blank_id, cutoff_prob: for the decoder and the
    oracle alike.  With bounds the ends are compared with both oracles where the compiled reference was built.
    -> labels committed per stream."""
    import ctcdecode_amd

    which = pu.which_oracle()
    B, T, V = lp.shape
    K = kw["beam"]
    okw = dict(kw)
    if blank_id != 0:
        okw["blank_id"] = blank_id
    if cutoff_prob != 1.0:
        okw["cutoff_prob"] = cutoff_prob
    dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, cutoff_top_n=kw.get("cutoff_top_n", 40), cutoff_prob=cutoff_prob,
                                             blank_id=blank_id, log_probs_input=True, device="cuda:0")
    if configure is None:
        _plain_switches(dec)
    else:
        configure(dec)
    states = [_state(dec, frames_hint) for _ in range(B)]
    idle = _state(dec, frames_hint)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    cache = {}

    def want_at(b, F, oracle=which):
        if (b, F, oracle) not in cache:
            cache[(b, F, oracle)] = pu.oracle_prefix(lp[b:b + 1], F, oracle, **okw)
        return cache[(b, F, oracle)]

    item_len = [T] * B if seq_lens is None else [int(v) for v in seq_lens]
    if bounds is None:
        starts = list(range(B)) if starts is None else starts
        assert (T // chunk) * chunk == T and seq_lens is None
        steps = T // chunk + max(starts)
    else:
        assert chunk is None and starts is None and bounds[0] == 0 and bounds[-1] == T
        starts = [0] * B
        steps = len(bounds) - 1
    frames = [0] * B  # frames a stream has decoded
    pos = [0] * B     # rows of its item that have been handed over (past a short item's end too)
    tok = [np.zeros((0,), np.int32) for _ in range(B)]
    ts = [np.zeros((0,), np.int32) for _ in range(B)]
    ended = {}
    events = 0
    for c in range(steps):
        idx = [b for b in range(B) if starts[b] <= c and b not in ended]
        if before is not None:
            before(c, dec)
        n = chunk if bounds is None else bounds[c + 1] - bounds[c]
        lens = [max(0, min(item_len[b] - pos[b], n)) for b in idx]
        ends = [pos[b] + n == T for b in idx] if bounds is None else [c == steps - 1] * len(idx)
        out = dec.decode(torch_mod.stack([x[b, pos[b]:pos[b] + n] for b in idx]), [states[b] for b in idx], ends,
                         seq_lens=None if seq_lens is None else torch_mod.tensor(lens, dtype=torch_mod.int32), check=False)
        if kernel_of is not None and kernel_of(c) is not None:
            assert dec.last_kernel() == tuple(kernel_of(c)), "call %d launched %s, expected %s" % (c, dec.last_kernel(), tuple(kernel_of(c)))
        if n > 0 and kernel is not None:
            assert dec.last_kernel() == tuple(kernel), "call %d launched %s, expected %s" % (c, dec.last_kernel(), tuple(kernel))
        if n > 0 and layout is not None:
            assert dec.last_layout() == layout, "call %d ran layout %d, expected %d" % (c, dec.last_layout(), layout)
        for i, b in enumerate(idx):
            pos[b] += n
            frames[b] += lens[i]
            if ends[i]:
                ended[b] = _final(out, i, K, frames[b], want_at(b, frames[b]))
        live_ones = [b for b in range(B) if b not in ended]
        if not live_ones:
            break
        if c % every == every - 1:
            sizes = [states[b].nbytes for b in live_ones]
            got = dec.commit([states[b] for b in live_ones] + [idle])
            assert len(got[-1][0]) == 0 and len(got[-1][1]) == 0 and idle.pool_nodes == 1 and idle.committed_len == 0, "a stream without frames commits nothing"
            for i, b in enumerate(live_ones):
                what = "call %d stream %d F=%d" % (c, b, frames[b])
                want = want_at(b, frames[b])
                C = len(tok[b])
                m = max(0, pu.common_prefix_len(want, 0) - 1 - C)
                g_tok, g_ts = got[i][0].numpy(), got[i][1].numpy()
                assert g_tok.dtype == np.int32 and g_ts.dtype == np.int32 and not got[i][0].is_cuda
                assert len(g_tok) == m == len(g_ts), "%s: %d labels committed, want %d" % (what, len(g_tok), m)
                assert np.array_equal(g_tok, want["tokens"][0, 0, C:C + m]), "%s: committed tokens differ from the oracle's row 0" % what
                assert np.array_equal(g_ts, want["timesteps"][0, 0, C:C + m]), "%s: committed time steps differ from the oracle's row 0" % what
                tok[b], ts[b] = np.concatenate([tok[b], g_tok]), np.concatenate([ts[b], g_ts])
                assert states[b].committed_len == C + m, what
                if frames[b] > 0:
                    assert states[b].pool_nodes == cu.oracle_live_count(want, 0) - (C + m), "%s: nodes kept" % what
                assert states[b].nbytes <= sizes[i]
                events += 1 if m else 0
            sizes = [states[b].nbytes for b in live_ones]
            nodes = [states[b].pool_nodes for b in live_ones]
            again = dec.commit([states[b] for b in live_ones] + [idle])
            assert all(len(t) == 0 for t, _ in again), "a second commit committed labels"
            assert [states[b].nbytes for b in live_ones] == sizes and [states[b].pool_nodes for b in live_ones] == nodes
        for nb in sorted({1, K}):
            for use_stable in (False, True):
                shs = [mu.shifted(want_at(b, frames[b]), 0, len(tok[b])) for b in live_ones]
                since = [pu.common_prefix_len(sh, 0) if use_stable else 0 for sh in shs]
                res = dec.peek([states[b] for b in live_ones], n_best=nb, since=since)
                for i, b in enumerate(live_ones):
                    pu.assert_peek_equals(_peek_view(res, i), shs[i], 0, nb, since[i],
                                          "call %d stream %d F=%d C=%d n_best=%d since=%d" % (c, b, frames[b], len(tok[b]), nb, since[i]))
    assert sorted(ended) == list(range(B))
    for b in range(B):
        for oracle in sorted({which, "restated"} if bounds is not None else {which}):
            want = want_at(b, frames[b], oracle)
            mu.assert_committed_prefix(want, 0, tok[b], ts[b], "stream %d: committed (%s oracle)" % (b, oracle))
            mu.assert_final(ended[b], want, 0, len(tok[b]), "stream %d: the final result after the commits (%s oracle)" % (b, oracle))
    assert events > 0
    return [len(t) for t in tok]


FIXED_1024 = (0, 0, 1, 0, 1024, 0, 0)
FIXED_RUNTIME_THREADS = (0, 0, 1, 0, 0, 0, 0)
WIDE_BEAM = (0, 1, 3, 0, 1024, 0, 0)


def test_commit_device_randn(torch_mod):
    case = pu.five_classes()[0]  # B 3, T 240, V 29, beam 50
    done = _walk_device(torch_mod, case["lp"], case["kw"], 1, 20)
    assert sum(1 for n in done if n > 0) >= 2 and max(done) > 64, done


def test_commit_device_peaky_k20_every_third_call(torch_mod):
    case = pu.five_classes()[4]
    done = _walk_device(torch_mod, case["lp"], case["kw"], 3, 20)
    assert sum(1 for n in done if n > 0) >= 2, done


def test_commit_device_pruned(torch_mod):
    case = pu.pruned_class()  # V 64, beam 16, top_n 8
    done = _walk_device(torch_mod, case["lp"], case["kw"], 1, 10)
    assert sum(1 for n in done if n > 0) >= 2, done


def test_commit_device_small_blocks_grow_between_commits(torch_mod):
    """frames_hint = 4: the blocks double between the commits (the grow path copies a re-rooted pool)."""
    case = pu.five_classes()[0]
    _walk_device(torch_mod, case["lp"][:, :120], case["kw"], 2, 20, frames_hint=4)


def test_commit_device_wide_beam(torch_mod):
    """Beam 500 over 29 labels (B 2, T 120): the parked state the wide-beam layout writes and continues."""
    lp = pu.peaky_logprobs(2, 120, 29, 75, hold=2, p_weak=0.05)
    done = _walk_device(torch_mod, lp, dict(beam=500), 1, 30, starts=[0, 0], kernel_of=lambda c: WIDE_BEAM)
    assert all(n > 0 for n in done), done


def test_commit_device_fixed_layout_1024_threads_then_512(torch_mod):
    """set_threads(1024): the fixed-layout kernel continues committed states (commits after calls 1 .. 4); from call 5 on 512 threads:
    another kernel takes the re-rooted streams over."""
    case = pu.five_classes()[0]

    def before(c, dec):
        if c == 0:
            dec.set_threads(1024)
        if c == 5:
            dec.set_threads(512)

    done = _walk_device(torch_mod, case["lp"][:, :160], case["kw"], 1, 20, starts=[0, 0, 0], before=before,
                        kernel_of=lambda c: FIXED_1024 if c < 5 else FIXED_RUNTIME_THREADS)
    assert min(done) >= 23, done  # (committed while the first kernel ran: the oracle's stable lengths at frame 100 are 40, 53, 24)


def test_commit_device_64_streams_at_random_boundaries(torch_mod):
    """64 streams in one decoder; after every chunk (queued with check=False) a random subset is committed in one call."""
    import ctcdecode_amd

    which = pu.which_oracle()
    B, T, V, K, chunk = 64, 120, 29, 20, 10
    lp = np.concatenate([ou.synth_logprobs(B // 2, T, V, 72), ou.synth_logprobs(B // 2, T, V, 73, blank_bias=4)])
    dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    rng = np.random.default_rng(74)
    tok = [np.zeros((0,), np.int32) for _ in range(B)]
    ts = [np.zeros((0,), np.int32) for _ in range(B)]
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
        got = dec.commit([states[b] for b in pick])
        want = pu.oracle_prefix(lp, lo + chunk, which, beam=K)
        for i, b in enumerate(pick):
            C = len(tok[b])
            m = max(0, pu.common_prefix_len(want, b) - 1 - C)
            g_tok, g_ts = got[i][0].numpy(), got[i][1].numpy()
            assert len(g_tok) == m, "F=%d stream %d: %d labels committed, want %d" % (lo + chunk, b, len(g_tok), m)
            assert np.array_equal(g_tok, want["tokens"][b, 0, C:C + m]) and np.array_equal(g_ts, want["timesteps"][b, 0, C:C + m]), (lo, b)
            assert states[b].pool_nodes == cu.oracle_live_count(want, b) - (C + m) and states[b].committed_len == C + m, (lo, b)
            tok[b], ts[b] = np.concatenate([tok[b], g_tok]), np.concatenate([ts[b], g_ts])
            events += 1 if m else 0
    assert events > B // 2, events
    want = ou.decode(lp, which=which, beam=K)
    for b in range(B):
        mu.assert_committed_prefix(want, b, tok[b], ts[b], "stream %d of 64: committed" % b)
        mu.assert_final(_final(out, b, K, T, dict(nres=want["nres"][b:b + 1])), want, b, len(tok[b]), "stream %d of 64" % b)


@pytest.mark.parametrize("beam", [4, 1])
def test_commit_device_timesteps_beyond_16_bits(torch_mod, beam):
    """test_commit_host_timesteps_beyond_16_bits on the device, at the shape of test_time_steps_beyond_16_bits (3 labels): one stream
    across frame 65535, chunks queued with check=False, a commit at frame 65000 and one at frame 65600 -- behind the second the
    gather kernel assembles the committed time steps from the nodes' 16 bits and their high parts, and the kept nodes keep theirs.
    frames_hint = 16: the live set below the new root is a few nodes, so the stream moves to a smaller block at both commits, at the
    second one with the high parts.  Committed labels, absolute time steps (some past frame 65535), kept nodes and a full peek
    against the oracle after each commit; the end: committed ++ rows == the one-shot decode."""
    import ctcdecode_amd

    which = pu.which_oracle()
    T = 65536 + 300
    lp = ou.synth_logprobs(1, T, 3, 17, blank_bias=2.5)
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(["0", "1", "2"], beam_width=beam, blank_id=0, log_probs_input=True, device="cuda:0")
    hint = 16
    st = _state(dec, hint)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    tok, ts = np.zeros((0,), np.int32), np.zeros((0,), np.int32)
    seen = 0
    for lo, hi in ((0, 65000), (65000, 65600)):
        dec.decode(x[:, lo:hi], [st], [False], check=False)
        want = pu.oracle_prefix(lp, hi, which, beam=beam)
        C = len(tok)
        m = max(0, pu.common_prefix_len(want, 0) - 1 - C)
        need = max(hint * beam + 1, 2 * (cu.oracle_live_count(want, 0) - (C + m)))
        assert 4 * need <= _capacity(st), "F=%d: the inputs do not exercise the shrink rule" % hi
        before = st.nbytes
        (g_tok, g_ts), = dec.commit([st])
        assert need <= _capacity(st) < need + beam and st.nbytes < before // 4, "F=%d: the block did not move to one of %d nodes" % (hi, need)
        g_tok, g_ts = g_tok.numpy(), g_ts.numpy()
        assert len(g_tok) == m > 0 and len(g_ts) == m, "F=%d: %d labels committed, want %d" % (hi, len(g_tok), m)
        assert np.array_equal(g_tok, want["tokens"][0, 0, C:C + m]), "F=%d: committed tokens differ from the oracle's row 0" % hi
        assert np.array_equal(g_ts, want["timesteps"][0, 0, C:C + m]), "F=%d: committed time steps differ from the oracle's row 0" % hi
        tok, ts = np.concatenate([tok, g_tok]), np.concatenate([ts, g_ts])
        assert st.committed_len == C + m and st.pool_nodes == cu.oracle_live_count(want, 0) - (C + m), "F=%d: nodes kept" % hi
        (t2, _), = dec.commit([st])
        assert len(t2) == 0 and st.committed_len == C + m, "F=%d: a second commit committed labels" % hi
        res = dec.peek([st], n_best=beam)
        pu.assert_peek_equals(_peek_view(res, 0), mu.shifted(want, 0, C + m), 0, beam, 0, "F=%d after the commit" % hi)
        seen = int(res[2].max())
    assert seen > 65535, "no kept node's time step lies past frame 65535"
    assert int(ts.max()) > 65535, "no committed time step lies past frame 65535"
    out = dec.decode(x[:, 65600:], [st], [True], check=False)
    final = pu.oracle_prefix(lp, T, which, beam=beam)
    mu.assert_committed_prefix(final, 0, tok, ts, "T > 65536: committed")
    mu.assert_final(_final(out, 0, beam, T, final), final, 0, len(tok), "T > 65536 after the commits")
    assert int(out[2].max()) > 65535


def test_commit_device_block_shrinks_when_the_rule_says_so(torch_mod):
    """frames_hint = 50 at beam 10, 1000 blank-dominated frames in 100-frame chunks: the block holds 1600 frames' nodes; the commit
    leaves live' nodes, the need max(501, 2 * live') is at most a quarter of the capacity, and the stream moves to a block of that
    size (DecoderState.nbytes falls); a commit directly after changes nothing.  The stream ends with the oracle's result."""
    import ctcdecode_amd

    which = pu.which_oracle()
    T, V, K, chunk, hint, at = 1200, 29, 10, 100, 50, 1000
    lp = cu.blank_dominated_long(1500, V)[:, :T]
    dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    st = _state(dec, hint)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    out = None
    C = 0
    for lo in range(0, T, chunk):
        end = lo + chunk == T
        out = dec.decode(x[:, lo:lo + chunk], [st], [end], check=False)
        if lo + chunk == at:
            before, cap = st.nbytes, _capacity(st)
            assert cap == 1600 * K + 1
            want = pu.oracle_prefix(lp, at, which, beam=K)
            (g_tok, g_ts), = dec.commit([st])
            C = max(0, pu.common_prefix_len(want, 0) - 1)
            assert C > 0 and len(g_tok) == C
            assert np.array_equal(g_tok.numpy(), want["tokens"][0, 0, :C]) and np.array_equal(g_ts.numpy(), want["timesteps"][0, 0, :C])
            live = cu.oracle_live_count(want, 0) - C
            assert st.pool_nodes == live
            need = max(hint * K + 1, 2 * live)
            assert 4 * need <= cap, "the inputs do not exercise the rule"
            assert need <= _capacity(st) < need + K and st.nbytes < before // 4, (need, _capacity(st), st.nbytes, before)
            after = st.nbytes
            (t2, _), = dec.commit([st])
            assert len(t2) == 0 and st.nbytes == after and st.pool_nodes == live
    want = pu.oracle_prefix(lp, T, which, beam=K)
    mu.assert_final(_final(out, 0, K, T, want), want, 0, C, "after the move to a smaller block")


def test_commit_refusals_leave_the_decoder_usable(torch_mod):
    """A state twice in the batch and a state of another decoder: ValueError.  Streams behind the built-in scorer and behind a
    callback scorer: NotImplementedError, nothing committed, and they decode on to the oracle's result."""
    import ctcdecode_amd
    from test_gpu_lm import _BuiltinBehindCallback

    which = pu.which_oracle()
    V, K, T = 29, 20, 40
    lp = ou.synth_logprobs(2, T, V, 69)
    labels = [str(i) for i in range(V)]
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    other = ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec.decode(x[:, :20], states, [False, False], check=False)
    assert dec.commit([]) == []
    with pytest.raises(ValueError):
        dec.commit([states[0], states[0]])
    with pytest.raises(ValueError):
        dec.commit([states[0], ctcdecode_amd.DecoderState(other)])
    assert [s.committed_len for s in states] == [0, 0]
    got = dec.commit(states)
    want20 = pu.oracle_prefix(lp, 20, which, beam=K)
    done = [max(0, pu.common_prefix_len(want20, b) - 1) for b in range(2)]
    assert [len(t) for t, _ in got] == done
    out = dec.decode(x[:, 20:], states, [True, True])
    want = ou.decode(lp, which=which, beam=K)
    for b in range(2):
        mu.assert_final(_final(out, b, K, T, dict(nres=want["nres"][b:b + 1])), want, b, done[b], "after the refused commits")

    c = pu.LM_PEEK_CASES[0]
    lp, kw = pu.lm_case_inputs(c)
    lp = lp[:2]
    path = os.path.join(pu.DATA, c["arpa"])
    osc = ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which)
    want = pu.oracle_prefix(lp, c["T"], which, scorer=osc, **kw)
    K, T = kw["beam"], lp.shape[1]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    inner = _BuiltinBehindCallback(dict(labels=c["labels"], lm_path=path))
    try:
        cs = ctcdecode_amd.CallbackScorer(inner, inner.vocabulary, inner.order, c["labels"], alpha=c["alpha"], beta=c["beta"], device="cuda:0")
        for name, extra in (("built-in", dict(model_path=path, alpha=c["alpha"], beta=c["beta"])), ("callback", dict(scorer=cs))):
            dec = ctcdecode_amd.OnlineCTCBeamDecoder(c["labels"], beam_width=K, cutoff_top_n=kw["cutoff_top_n"], blank_id=0, log_probs_input=True,
                                                     device="cuda:0", **extra)
            states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
            dec.decode(x[:, :60], states, [False, False])
            nodes = [s.pool_nodes for s in states]
            with pytest.raises(NotImplementedError):
                dec.commit(states)
            assert [s.committed_len for s in states] == [0, 0] and [s.pool_nodes for s in states] == nodes, name
            out = dec.decode(x[:, 60:], states, [True, True])
            for b in range(2):
                one = dict((k, v[b:b + 1]) for k, v in want.items())
                ou.assert_same(_final(out, b, K, T, one), one, "%s-scorer stream %d after the refused commit" % (name, b))
    finally:
        inner.close()
