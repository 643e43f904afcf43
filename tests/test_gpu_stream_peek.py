"""-m gpu: OnlineCTCBeamDecoder.peek on the device -- the interim results of live streams (ctc_stream_peek_kernel on the parked states)
against the oracle's one-shot decode of the frames each stream has been fed so far, streams of different ages in one peek, chunks
queued with check=False in front of it; the streams then end through the normal decode(..., is_eos) path and must equal the one-shot
oracle: peeks disturb nothing."""
import ctypes
import os

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


def _stream_view(res, b):
    tok, sc, ts, ln, stable = res
    n = tok.shape[1]
    lens = ln[b].numpy()
    scores = sc[b].numpy()
    nres = n
    while nres > 0 and lens[nres - 1] == 0 and scores[nres - 1] == 0:  # (rows beyond a stream's own n_results are zero)
        nres -= 1
    return dict(tokens=tok[b].numpy(), timesteps=ts[b].numpy(), scores=scores, lens=lens, nres=nres, stable=int(stable[b]))


def _check_peeks(dec, states, idx, frames, want_at, prev, K, tag, n_bests=None):
    """Peek the live streams idx (their states, frames fed) with every n_best / since combination; compare each stream with the oracle
    at ITS age; the stable prefix's properties against prev[b] = (stable_len, tokens, timesteps)."""
    n_bests = n_bests or sorted({1, min(3, K), K})
    for nb in n_bests:
        for use_prev in (False, True):
            since = [prev[b][0] if use_prev else 0 for b in idx]
            res = dec.peek([states[b] for b in idx], n_best=nb, since=since if use_prev else None)
            assert res[0].shape[1] <= nb and all(not t.is_cuda for t in res)
            for i, b in enumerate(idx):
                want = want_at(b, frames[b])
                got = _stream_view(res, i)
                if int(want["nres"][0]) >= 1 and got["nres"] == 0:  # (a root-only result: length 0, score -0.0)
                    got["nres"] = 1
                pu.assert_peek_equals(got, want, 0, nb, since[i], "%s stream %d F=%d n_best=%d since=%d" % (tag, b, frames[b], nb, since[i]))
    full = dec.peek([states[b] for b in idx], n_best=K)
    for i, b in enumerate(idx):
        g = _stream_view(full, i)
        st = g["stable"]
        assert st >= prev[b][0], "%s stream %d: stable_len fell from %d to %d" % (tag, b, prev[b][0], st)
        m = prev[b][0]
        for p in range(g["nres"]):
            assert np.array_equal(g["tokens"][p, :m], prev[b][1]) and np.array_equal(g["timesteps"][p, :m], prev[b][2]), \
                "%s stream %d row %d leaves the stable prefix" % (tag, b, p)
        prev[b] = (st, g["tokens"][0, :st].copy(), g["timesteps"][0, :st].copy())


def _walk_device(torch_mod, lp, kw, chunk=10, labels=None, lm=None, scorer=None, which=None, late=2):
    """B streams; the last one starts `late` chunks after the others.  Chunks go in with check=False, a round of peeks follows every
    call; all streams end in the call that feeds the older ones their last chunk."""
    import ctcdecode_amd

    which = which or pu.which_oracle()
    B, T, V = lp.shape
    K = kw["beam"]
    labels = labels or [str(i) for i in range(V)]
    dkw = dict(beam_width=K, cutoff_top_n=kw.get("cutoff_top_n", 40), blank_id=0, log_probs_input=True, device="cuda:0")
    if lm is not None:
        dkw.update(model_path=lm[2], alpha=lm[0], beta=lm[1])
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, **dkw)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    cache = {}

    def want_at(b, F):
        if (b, F) not in cache:
            cache[(b, F)] = pu.oracle_prefix(lp[b:b + 1], F, which, scorer=scorer, **kw)
        return cache[(b, F)]

    frames = [0] * B
    prev = [(0, np.zeros((0,), np.int32), np.zeros((0,), np.int32)) for _ in range(B)]
    _check_peeks(dec, states, list(range(B)), frames, want_at, prev, K, "no frames yet", n_bests=[1, K])
    steps = T // chunk
    assert steps * chunk == T and steps > late
    for c in range(steps):
        idx = [b for b in range(B) if b < B - 1 or c >= late]
        rows = torch_mod.stack([x[b, frames[b]:frames[b] + chunk] for b in idx])
        end = c == steps - 1
        out = dec.decode(rows, [states[b] for b in idx], [end] * len(idx), check=False)
        for b in idx:
            frames[b] += chunk
        if not end:
            _check_peeks(dec, states, idx, frames, want_at, prev, K, "step %d" % c)
    tok, sc, ts, ln = out
    for b in range(B):
        want = want_at(b, frames[b])
        F = frames[b]
        got = dict(tokens=np.zeros((1, K, F), np.int32), timesteps=np.zeros((1, K, F), np.int32), scores=sc[b:b + 1].numpy(), lens=ln[b:b + 1].numpy(),
                   nres=want["nres"])
        w = min(F, tok.shape[2])
        got["tokens"][0, :tok.shape[1], :w] = tok[b, :, :w].numpy()
        got["timesteps"][0, :ts.shape[1], :w] = ts[b, :, :w].numpy()
        ou.assert_same(got, want, "stream %d: the final result after the peeks" % b)
        pu.assert_starts_with(want, 0, prev[b][1], prev[b][2], "stream %d: final result" % b)


@pytest.mark.parametrize("case", pu.five_classes() + [pu.pruned_class()], ids=lambda c: c["name"])
def test_peek_device_streams_of_different_ages(torch_mod, case):
    _walk_device(torch_mod, case["lp"], case["kw"])


def test_peek_device_ragged_and_empty_chunks(torch_mod):
    """Chunk ends that differ per stream (seq_lens), empty chunks among them, a stream that is still without frames beside live ones."""
    import ctcdecode_amd

    which = pu.which_oracle()
    B, T, V, K = 3, 100, 29, 30
    lp = ou.synth_logprobs(B, T, V, 66)
    dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    frames = [0] * B
    prev = [(0, np.zeros((0,), np.int32), np.zeros((0,), np.int32)) for _ in range(B)]

    def want_at(b, F):
        return pu.oracle_prefix(lp[b:b + 1], F, which, beam=K)

    plan = [(0, 0, 0), (7, 0, 3), (0, 0, 0), (12, 0, 12), (1, 5, 0), (12, 12, 12)]  # frames per stream and call (stream 1 idles for four calls)
    for step, lens in enumerate(plan):
        W = 12
        rows = torch_mod.zeros((B, W, V), device="cuda:0")
        for b in range(B):
            rows[b, :lens[b]] = x[b, frames[b]:frames[b] + lens[b]]
        dec.decode(rows, states, [False] * B, seq_lens=torch_mod.tensor(lens, dtype=torch_mod.int32), check=False)
        for b in range(B):
            frames[b] += lens[b]
        _check_peeks(dec, states, list(range(B)), frames, want_at, prev, K, "call %d" % step)
    rest = max(T - f for f in frames)
    rows = torch_mod.zeros((B, rest, V), device="cuda:0")
    lens = [T - f for f in frames]
    for b in range(B):
        rows[b, :lens[b]] = x[b, frames[b]:]
    tok, sc, ts, ln = dec.decode(rows, states, [True] * B, seq_lens=torch_mod.tensor(lens, dtype=torch_mod.int32))
    want = ou.decode(lp, which=which, beam=K)
    got = dict(tokens=np.zeros((B, K, T), np.int32), timesteps=np.zeros((B, K, T), np.int32), scores=sc.numpy(), lens=ln.numpy(), nres=want["nres"])
    got["tokens"][:, :tok.shape[1], :tok.shape[2]] = tok.numpy()
    got["timesteps"][:, :ts.shape[1], :ts.shape[2]] = ts.numpy()
    ou.assert_same(got, want, "ragged streams after the peeks")


def test_peek_device_wide_beam(torch_mod):
    """Beam 500 over 29 labels: the parked state the wide-beam layout writes, 500 entries through both sort routes."""
    _walk_device(torch_mod, ou.synth_logprobs(3, 80, 29, 68, quant=0.25), dict(beam=500), chunk=20, late=1)


def test_peek_device_timesteps_beyond_16_bits(torch_mod):
    """A stream that crosses frame 65535 at a small beam: peeked before and after, time steps from the pool's high-part array."""
    import ctcdecode_amd

    which = pu.which_oracle()
    T = 66500
    lp = ou.synth_logprobs(2, T, 3, 17, blank_bias=2.5)
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(["0", "1", "2"], beam_width=4, blank_id=0, log_probs_input=True, device="cuda:0")
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
    x = torch_mod.from_numpy(lp)
    bounds = [0, 65000, 65600, T]
    prev = [(0, np.zeros((0,), np.int32), np.zeros((0,), np.int32)) for _ in range(2)]
    seen = 0
    cache = {}

    def want_at(b, F):
        if (b, F) not in cache:
            cache[(b, F)] = pu.oracle_prefix(lp[b:b + 1], F, which, beam=4)
        return cache[(b, F)]

    for i in range(len(bounds) - 1):
        end = i == len(bounds) - 2
        out = dec.decode(x[:, bounds[i]:bounds[i + 1]], states, [end] * 2, check=False)
        if not end:
            F = bounds[i + 1]
            _check_peeks(dec, states, [0, 1], [F, F], want_at, prev, 4, "F=%d" % F)
            full = dec.peek(states, n_best=4)
            seen = max(seen, int(full[2].max()))
    assert seen > 65535
    tok, sc, ts, ln = out
    want = ou.decode(lp, which=which, beam=4)
    got = dict(tokens=np.zeros((2, 4, T), np.int32), timesteps=np.zeros((2, 4, T), np.int32), scores=sc.numpy(), lens=ln.numpy(), nres=want["nres"])
    got["tokens"][:, :tok.shape[1], :tok.shape[2]] = tok.numpy()
    got["timesteps"][:, :ts.shape[1], :ts.shape[2]] = ts.numpy()
    ou.assert_same(got, want, "T > 65536 after peeks")


@pytest.mark.parametrize("c", pu.LM_PEEK_CASES, ids=lambda c: c["name"])
def test_peek_device_with_the_built_in_scorer(torch_mod, c):
    lp, kw = pu.lm_case_inputs(c)
    path = os.path.join(pu.DATA, c["arpa"])
    which = pu.which_oracle()
    sc = ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which)
    _walk_device(torch_mod, lp, kw, labels=c["labels"], lm=(c["alpha"], c["beta"], path), scorer=sc, which=which)


def test_peek_refusals_leave_the_decoder_usable(torch_mod):
    import ctcdecode_amd
    from ctcdecode_amd import _native
    from test_gpu_lm import _BuiltinBehindCallback

    V, K, T = 29, 20, 40
    lp = ou.synth_logprobs(2, T, V, 69)
    labels = [str(i) for i in range(V)]
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    other = ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0")
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
    foreign = ctcdecode_amd.DecoderState(other)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec.decode(x[:, :20], states, [False, False], check=False)
    with pytest.raises(ValueError):
        dec.peek(states, n_best=0)
    with pytest.raises(ValueError):
        dec.peek(states, n_best=K + 1)
    with pytest.raises((ValueError, _native.NativeError)):
        dec.peek([states[0], foreign])
    with pytest.raises((ValueError, _native.NativeError)):
        dec.peek([states[0], states[0]])
    with pytest.raises(ValueError):
        dec.peek(states, since=[0])
    # through the raw ABI: a state created for another beam width; an L_cap too small for a row, with guard words around the buffers
    wide = ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=K + 5, blank_id=0, log_probs_input=True, device="cuda:0")
    wide_state = ctcdecode_amd.DecoderState(wide)
    full = dec.peek(states, n_best=3)
    longest = int(full[3].max())
    assert longest > 2
    G = 64
    stream = torch_mod.cuda.current_stream().cuda_stream

    def raw_peek(ptrs, B, n_best, L_cap):
        bufs = [torch_mod.full((G + B * n_best * L_cap + G,), -77, dtype=torch_mod.int32, device="cuda:0") for _ in range(2)]
        bufs.append(torch_mod.full((G + B * n_best + G,), -77.0, dtype=torch_mod.float32, device="cuda:0"))
        bufs += [torch_mod.full((G + n + G,), -77, dtype=torch_mod.int32, device="cuda:0") for n in (B * n_best, B, B)]
        arr = (ctypes.c_void_p * B)(*ptrs)
        rc = _native.lib.ctcd_stream_peek(dec._handle, arr, B, n_best, None, bufs[0][G:].data_ptr(), bufs[1][G:].data_ptr(), L_cap,
                                          bufs[2][G:].data_ptr(), bufs[3][G:].data_ptr(), bufs[4][G:].data_ptr(), bufs[5][G:].data_ptr(), stream)
        return rc, bufs

    rc, _ = raw_peek([states[0].state.value, wide_state.state.value], 2, 1, 8)
    assert rc == -1, rc  # CTCD_EINVAL
    rc, bufs = raw_peek([s.state.value for s in states], 2, 3, longest - 1)
    assert rc == 0
    with pytest.raises(ValueError):
        _native.check(_native.lib.ctcd_check_status(dec._handle, 0))
    torch_mod.cuda.synchronize()
    for t in bufs:
        h = t.cpu()
        assert bool((h[:G] == -77).all()) and bool((h[-G:] == -77).all()), "a peek wrote outside its buffers"
    rc, bufs = raw_peek([s.state.value for s in states], 2, 3, longest)
    assert rc == 0
    _native.check(_native.lib.ctcd_check_status(dec._handle, 0))
    tok = bufs[0][G:G + 2 * 3 * longest].view(2, 3, longest).cpu()
    assert np.array_equal(tok[:, :full[0].shape[1], :full[0].shape[2]].numpy(), full[0].numpy())
    for t in bufs:
        h = t.cpu()
        assert bool((h[:G] == -77).all()) and bool((h[-G:] == -77).all()), "a peek wrote outside its buffers"
    # a callback scorer's streams
    path = os.path.join(pu.DATA, "test.arpa")
    inner = _BuiltinBehindCallback(dict(labels=pu.LABELS29, lm_path=path))
    try:
        cs = ctcdecode_amd.CallbackScorer(inner, inner.vocabulary, inner.order, pu.LABELS29, alpha=0.5, beta=1.0, device="cuda:0")
        cdec = ctcdecode_amd.OnlineCTCBeamDecoder(pu.LABELS29, beam_width=K, blank_id=0, log_probs_input=True, device="cuda:0", scorer=cs)
        cstates = [ctcdecode_amd.DecoderState(cdec) for _ in range(2)]
        with pytest.raises(NotImplementedError):
            cdec.peek(cstates)
        arr = (ctypes.c_void_p * 2)(*[s.state.value for s in cstates])
        one = torch_mod.zeros((16,), dtype=torch_mod.int32, device="cuda:0")
        f = torch_mod.zeros((16,), dtype=torch_mod.float32, device="cuda:0")
        rc = _native.lib.ctcd_stream_peek(cdec._handle, arr, 2, 1, None, one.data_ptr(), one.data_ptr(), 1, f.data_ptr(), one.data_ptr(), one.data_ptr(),
                                          one.data_ptr(), stream)
        assert rc == -2, rc  # CTCD_EUNSUPPORTED
        tok, sc, ts, ln = cdec.decode(x, cstates, [True, True])
        want = ou.decode(lp, scorer=ou.Scorer(0.5, 1.0, path, pu.LABELS29, "restated"), beam=K)
        assert np.array_equal(ln.numpy()[:, 0], want["lens"][:, 0])
    finally:
        inner.close()
    # ... and the decoder of the refused calls still decodes correctly
    tok, sc, ts, ln = dec.decode(x[:, 20:], states, [True, True])
    want = ou.decode(lp, which=pu.which_oracle(), beam=K)
    got = dict(tokens=np.zeros((2, K, T), np.int32), timesteps=np.zeros((2, K, T), np.int32), scores=sc.numpy(), lens=ln.numpy(), nres=want["nres"])
    got["tokens"][:, :tok.shape[1], :tok.shape[2]] = tok.numpy()
    got["timesteps"][:, :ts.shape[1], :ts.shape[2]] = ts.numpy()
    ou.assert_same(got, want, "after the refused peeks")
