"""-m gpu: OnlineCTCBeamDecoder.set_blank_skip(thr) on the device -- the chunk scan with carry, the gather, the decode of the kept rows and
the remaps of stream_blank_skip.hip behind every streaming call.  The contract: however a stream's frames are cut into chunks, what it
reports -- at its end, from peek and from commit -- equals ``blank_skip_util.decode`` of the concatenation, bit for bit (tokens, scores,
lengths, result counts, time steps as indices among the frames seen), and so equals the one-shot ``CTCBeamDecoder(blank_skip=thr)``."""
import os

import blank_skip_util as bu
import numpy as np
import oracle_util as ou
import peek_util as pu
import pytest
from test_gpu_stream_compact import _final, _peek_view

pytestmark = pytest.mark.gpu
_WANT = {}


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _online(V, beam, thr, mode="log", **kw):
    import ctcdecode_amd

    labels = kw.pop("labels", None) or [str(i) for i in range(V)]
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, beam_width=beam, blank_id=0, log_probs_input=mode == "log", logits_input=mode == "logits",
                                             device="cuda:0", **kw)
    assert dec.last_blank_skip() is None
    if thr is not None:
        dec.set_blank_skip(thr)
    return dec


def _item(res, b):
    return {k: v[b:b + 1] for k, v in res.items()}


def _chunk(torch_mod, x, b, a, T):
    """Rows [a, a + T) of item b, zero rows where the item has none."""
    out = torch_mod.zeros((T,) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
    z = min(a + T, x.shape[1])
    if z > a:
        out[:z - a] = x[b, a:z]
    return out


def _run(torch_mod, dec, x, sizes, seq_lens=None, states=None, check=True, lens_of=None, between=None):
    """Feeds x [B, N, V] (device tensor) to B streams in chunk calls of ``sizes`` frames; stream b has seq_lens[b] frames (default N) and
    consumes lens_of(call, b, left, T) of them per call (default: as many as the chunk holds).  The last call ends every stream.
    between(call, states): called after every call but the last.  -> (the last call's result tuple, states, frames seen per stream)."""
    import ctcdecode_amd

    B, N = x.shape[:2]
    total = [N] * B if seq_lens is None else [int(v) for v in seq_lens]
    states = states or [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    pos = [0] * B
    out = None
    for c, T in enumerate(sizes):
        last = c == len(sizes) - 1
        lens = [min(total[b] - pos[b], T) if lens_of is None else lens_of(c, b, total[b] - pos[b], T) for b in range(B)]
        if last:
            assert all(pos[b] + lens[b] == total[b] for b in range(B)), "the cut does not cover the streams"
        rows = torch_mod.stack([_chunk(torch_mod, x, b, pos[b], T) for b in range(B)]) if T else x[:, :0]
        out = dec.decode(rows, states, [last] * B, seq_lens=torch_mod.tensor(lens, dtype=torch_mod.int32), check=check or last)
        for b in range(B):
            pos[b] += lens[b]
            assert states[b].frames_seen == pos[b] or last
        if not last and between is not None:
            between(c, states)
    return out, states, pos


def _same_as(out, want, K, seen, what):
    for b in range(len(seen)):
        wb = _item(want, b)
        got = _final(out, b, K, max(seen[b], 1), wb)
        ou.assert_same(got, wb, "%s item %d" % (what, b))
        n = int(wb["nres"][0])
        assert not got["lens"][0, n:].any() and not got["scores"][0, n:].any(), "%s item %d: rows beyond n_results" % (what, b)


def _oneshot(torch_mod, x, seq_lens, V, K, thr, mode="log"):
    import ctcdecode_amd

    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=mode == "log", logits_input=mode == "logits",
                                       device="cuda:0", blank_skip=thr)
    tok, sc, ts, ln = dec.decode(x, None if seq_lens is None else torch_mod.tensor(seq_lens, dtype=torch_mod.int32))
    return dict(tokens=tok.numpy(), timesteps=ts.numpy(), scores=sc.numpy(), lens=ln.numpy())


# ---- anchor chunkings --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", ["one", "50", "3", "ragged"])
def test_anchor_chunkings(torch_mod, cut):
    a = bu.ANCHOR
    lp, sl = bu.anchor_input()
    want, kept, n2 = bu.anchor_want()
    assert n2.tolist() == [77, 57, 0, 40]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec = _online(a["V"], a["beam"], a["thr"])
    lens_of = None
    if cut == "ragged":
        rng = np.random.default_rng(5)
        sizes = [40] * 9 + [150]
        lens_of = lambda c, b, left, T: left if c == len(sizes) - 1 else int(rng.integers(0, min(left, T) + 1))  # noqa: E731
    else:
        size = {"one": 150, "50": 50, "3": 3}[cut]
        sizes = [size] * (150 // size)
    if cut == "3":
        k0 = set(kept[0, :n2[0]].tolist())
        assert any(not (k0 & set(range(s, s + 3))) for s in range(0, 150, 3)), "no 3-frame chunk of item 0 is skipped whole"
        skipped = [t not in k0 for t in range(150)]
        run = best = 0
        for s in skipped:
            run = run + 1 if s else 0
            best = max(best, run)
        assert best == 7
    out, states, seen = _run(torch_mod, dec, x, sizes, seq_lens=sl, lens_of=lens_of)
    assert seen == sl.tolist() and [st.frames for st in states] == n2.tolist() and [st.frames_seen for st in states] == sl.tolist()
    _same_as(out, want, a["beam"], seen, "anchor/" + cut)
    got2 = _final(out, 2, a["beam"], 1, _item(want, 2))
    bu.assert_root_only(got2, 0, "item 2 must end with the root alone")
    assert int(want["nres"][2]) == 1
    considered, kept_last = dec.last_blank_skip()
    assert 0 <= kept_last <= considered <= sum(sl.tolist())
    if cut == "one":
        assert (considered, kept_last) == (int(sl.sum()), int(n2.sum()))
        one = _oneshot(torch_mod, x, sl, a["V"], a["beam"], a["thr"])
        one["nres"] = want["nres"]
        ou.assert_same(one, want, "one-shot blank_skip")


# ---- threshold cases ---------------------------------------------------------------------------------------------------------------
def test_a_threshold_that_skips_every_frame(torch_mod):
    lp = ou.synth_logprobs(2, 90, 29, 21, blank_bias=4.0)
    thr = 1e-7
    assert (lp[:, :, 0] > np.float32(np.log(thr))).all()
    want, kept, n2 = bu.decode(lp, None, thr, beam=8)
    assert n2.tolist() == [0, 0]
    dec = _online(29, 8, thr)
    out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [32, 32, 26])
    assert [st.frames for st in states] == [0, 0] and [st.frames_seen for st in states] == [90, 90]
    _same_as(out, want, 8, seen, "all skipped")
    for b in range(2):
        bu.assert_root_only(_final(out, b, 8, 1, _item(want, b)), 0, "a stream whose frames were all skipped ends with the root alone")


def test_threshold_one_equals_no_filter(torch_mod):
    lp = ou.synth_logprobs(2, 90, 29, 22, blank_bias=4.0)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    outs = []
    for thr in (1.0, None):
        dec = _online(29, 8, thr)
        out, states, _ = _run(torch_mod, dec, x, [32, 32, 26])
        assert [st.frames for st in states] == [90, 90]
        outs.append(out)
    for g, w in zip(*outs):
        assert g.shape == w.shape and np.array_equal(g.numpy().view(np.int32), w.numpy().view(np.int32))


# ---- input forms and gather word sizes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,dtype,V", [("prob", "f32", 29), ("log", "f32", 29), ("logits", "f32", 29), ("log", "f16", 29), ("log", "bf16", 29),
                                          ("log", "f32", 32), ("log", "bf16", 31), ("logits", "bf16", 32)])
def test_input_forms_and_gather_word_sizes(torch_mod, mode, dtype, V):
    """V 32 float32: rows of whole 16-byte words; V 29 float32: 4-byte words; an odd V in bf16: 2-byte words."""
    thr, K, N = 0.6, 8, 90
    vals = bu.to_dtype_values(bu.synth(2, N, V, 31 + V, mode=mode), dtype)
    want, kept, n2 = bu.decode(vals, None, thr, mode=mode, beam=K)
    assert 0 < n2.min() and n2.max() < N
    tdt = {"f32": torch_mod.float32, "f16": torch_mod.float16, "bf16": torch_mod.bfloat16}[dtype]
    x = torch_mod.from_numpy(vals).to("cuda:0").to(tdt)
    assert np.array_equal(x.float().cpu().numpy(), vals)
    dec = _online(V, K, thr, mode=mode)
    out, states, seen = _run(torch_mod, dec, x, [32, 32, 26])
    assert [st.frames for st in states] == n2.tolist()
    _same_as(out, want, K, seen, "%s/%s/V%d" % (mode, dtype, V))
    if dtype == "f32" and V == 29:
        one = _oneshot(torch_mod, x, None, V, K, thr, mode)
        one["nres"] = want["nres"]
        ou.assert_same(one, want, "one-shot blank_skip " + mode)


# ---- scan carry, map growth ----------------------------------------------------------------------------------------------------------
def test_scan_carry_across_1024_frame_passes(torch_mod):
    lp = ou.synth_logprobs(2, 2200, 5, 7, blank_bias=4.0)
    want, kept, n2 = bu.decode(lp, None, 0.6, beam=4)
    assert n2.tolist() == [102, 108]
    dec = _online(5, 4, 0.6)
    out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [1025, 1023, 64, 65, 23])
    assert [st.frames for st in states] == [102, 108]
    _same_as(out, want, 4, seen, "scan carry")


def test_map_growth(torch_mod):
    """Forty chunks of 37 frames into streams created with no hint: the maps start with room for the 1024 frames the pools start with,
    and double when the kept frames outgrow them."""
    from ctcdecode_amd import _native

    lp = ou.synth_logprobs(2, 1480, 5, 9, blank_bias=2.0)
    want, kept, n2 = bu.decode(lp, None, 0.9, beam=4)
    assert n2.min() > 1024, n2
    dec = _online(5, 4, 0.9)
    sizes_seen = []
    out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [37] * 40,
                             between=lambda c, sts: sizes_seen.append(int(_native.lib.ctcd_stream_map_bytes(sts[0].state))))
    assert sizes_seen[0] == 1024 * 4 and sorted(set(sizes_seen)) == [4096, 8192], sorted(set(sizes_seen))
    assert sizes_seen == sorted(sizes_seen), "a map shrank"
    _same_as(out, want, 4, seen, "map growth")


# ---- staggered batch -------------------------------------------------------------------------------------------------------------------
def test_streams_that_joined_the_batch_at_different_calls(torch_mod):
    import ctcdecode_amd

    B, N, V, K, thr, C = 3, 120, 29, 8, 0.6, 30
    lp = ou.synth_logprobs(B, N, V, 41, blank_bias=4.0)
    want, kept, n2 = bu.decode(lp, None, thr, beam=K)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec = _online(V, K, thr)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    ended = {}
    for c in range(N // C + B - 1):
        idx = [b for b in range(B) if b <= c < b + N // C]  # stream b takes its chunks at calls b .. b + 3
        rows = torch_mod.stack([x[b, (c - b) * C:(c - b + 1) * C] for b in idx])
        out = dec.decode(rows, [states[b] for b in idx], [c == b + N // C - 1 for b in idx], check=False)
        assert [states[b].frames_seen for b in idx] == [(c - b + 1) * C for b in idx]
        for i, b in enumerate(idx):
            if c == b + N // C - 1:
                ended[b] = _final(out, i, K, N, _item(want, b))
    for b in range(B):
        ou.assert_same(ended[b], _item(want, b), "staggered item %d" % b)


# ---- peek, commit ----------------------------------------------------------------------------------------------------------------------
def _prefix_want(lp, F, thr, K):
    key = (lp.ctypes.data, F, thr, K)
    if key not in _WANT:
        _WANT[key] = bu.decode(np.ascontiguousarray(lp[:, :F]), None, thr, beam=K)[0]
    return _WANT[key]


def test_peek_after_every_chunk(torch_mod):
    B, N, V, K, thr, C = 2, 120, 29, 8, 0.6, 30
    lp = pu.peaky_logprobs(B, N, V, 65)
    dec = _online(V, K, thr)

    def look(c, states):
        w = _prefix_want(lp, (c + 1) * C, thr, K)
        first = dec.peek(states, n_best=2)
        stable = [int(v) for v in first[4]]
        again = dec.peek(states, n_best=2, since=stable)
        for b in range(B):
            pu.assert_peek_equals(_peek_view(first, b), w, b, 2, 0, "peek after call %d stream %d" % (c, b))
            pu.assert_peek_equals(_peek_view(again, b), w, b, 2, stable[b], "peek since stable after call %d stream %d" % (c, b))
            assert states[b].frames < states[b].frames_seen == (c + 1) * C
            stable_seen.append(stable[b])

    stable_seen = []
    out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [C] * (N // C), check=False, between=look)
    assert max(stable_seen) > 2, "no stable prefix to ask beyond: the since path was not exercised"
    _same_as(out, _prefix_want(lp, N, thr, K), K, seen, "end after peeks")


def test_commit_reports_seen_frame_numbers(torch_mod):
    B, N, V, K, thr, C = 2, 200, 29, 8, 0.6, 40
    lp = pu.peaky_logprobs(B, N, V, 64)
    dec = _online(V, K, thr)
    tok = [np.zeros((0,), np.int32) for _ in range(B)]
    ts = [np.zeros((0,), np.int32) for _ in range(B)]
    committed = [0]

    def rows_match(got_view, w, b, what):
        n = int(w["nres"][b])
        assert got_view["nres"] == n, what
        for p in range(n):
            L, r = int(w["lens"][b, p]), int(got_view["lens"][p])
            assert r + len(tok[b]) == L, "%s row %d: %d + %d labels, want %d" % (what, p, len(tok[b]), r, L)
            assert np.array_equal(np.concatenate([tok[b], got_view["tokens"][p, :r]]), w["tokens"][b, p, :L]), "%s row %d: tokens" % (what, p)
            assert np.array_equal(np.concatenate([ts[b], got_view["timesteps"][p, :r]]), w["timesteps"][b, p, :L]), "%s row %d: time steps" % (what, p)
        assert np.array_equal(np.asarray(got_view["scores"][:n], np.float32).view(np.uint32), w["scores"][b, :n].view(np.uint32)), what

    def step(c, states):
        w = _prefix_want(lp, (c + 1) * C, thr, K)
        before = dec.peek(states, n_best=K)
        for b in range(B):  # (what an earlier commit took is still gone after a further chunk)
            rows_match(_peek_view(before, b), w, b, "before commit %d stream %d" % (c, b))
        got = dec.commit(states)
        for b in range(B):
            g_tok, g_ts = got[b][0].numpy(), got[b][1].numpy()
            C0 = len(tok[b])
            assert np.array_equal(g_tok, w["tokens"][b, 0, C0:C0 + len(g_tok)]) and np.array_equal(g_ts, w["timesteps"][b, 0, C0:C0 + len(g_ts)]), (c, b)
            tok[b], ts[b] = np.concatenate([tok[b], g_tok]), np.concatenate([ts[b], g_ts])
            assert states[b].committed_len == len(tok[b])
            committed[0] += len(g_tok)
        after = dec.peek(states, n_best=K)
        for b in range(B):
            rows_match(_peek_view(after, b), w, b, "after commit %d stream %d" % (c, b))

    out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [C] * (N // C), check=False, between=step)
    assert committed[0] > 0 and any(len(t) and t.max() > len(t) for t in ts), "nothing was committed, or no committed time step was moved by the map"
    w = _prefix_want(lp, N, thr, K)
    for b in range(B):
        wb = _item(w, b)
        got = _final(out, b, K, N, wb)
        view = dict(tokens=got["tokens"][0], timesteps=got["timesteps"][0], scores=got["scores"][0], lens=got["lens"][0], nres=int(wb["nres"][0]))
        rows_match(view, w, b, "end stream %d" % b)


def test_a_larger_batch_fed_while_a_small_batch_s_peek_is_still_queued(torch_mod):
    """ctcd_stream_peek is asynchronous: its remap kernel reads the call's pointer table when the stream gets there.  Four streams are
    peeked through the C entry behind work that keeps the stream busy, and at once a chunk call of eight streams fills in its own,
    longer argument tables; the peek must still report the four streams' rows, and all eight must end like the one-shot decode."""
    import ctypes

    import ctcdecode_amd
    from ctcdecode_amd import _native

    B, N, V, K, thr, C = 8, 60, 29, 8, 0.6, 30
    lp = pu.peaky_logprobs(B, N, V, 71)
    want = bu.decode(lp, None, thr, beam=K)[0]
    first = bu.decode(np.ascontiguousarray(lp[:4, :C]), None, thr, beam=K)[0]
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec = _online(V, K, thr)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    dec.decode(x[:4, :C], states[:4], [False] * 4)
    kept4 = [st.frames for st in states[:4]]
    L_cap, n_best = max(kept4), 2
    tok = torch_mod.full((4, n_best, L_cap), -5, dtype=torch_mod.int32, device="cuda:0")
    ts = torch_mod.full((4, n_best, L_cap), -5, dtype=torch_mod.int32, device="cuda:0")
    sc = torch_mod.zeros((4, n_best), dtype=torch_mod.float32, device="cuda:0")
    meta = torch_mod.zeros((4 * (n_best + 2),), dtype=torch_mod.int32, device="cuda:0")
    ln, nres, stable = meta[:4 * n_best], meta[4 * n_best:4 * n_best + 4], meta[4 * n_best + 4:]
    ptrs = (ctypes.c_void_p * 4)(*[st.state.value for st in states[:4]])
    busy = torch_mod.randn((4096, 4096), device="cuda:0")
    stream = torch_mod.cuda.current_stream().cuda_stream
    for _ in range(20):  # (some tens of milliseconds of work in front of the peek)
        busy = busy @ busy
        busy = busy / busy.abs().max()
    _native.check(_native.lib.ctcd_stream_peek(dec._handle, ptrs, 4, n_best, None, tok.data_ptr(), ts.data_ptr(), L_cap, sc.data_ptr(), ln.data_ptr(),
                                               nres.data_ptr(), stable.data_ptr(), stream))
    # the larger batch, while the peek and its remap are still queued: streams 0..3 take their second chunk, 4..7 their first
    rows = torch_mod.stack([x[b, C:2 * C] if b < 4 else x[b, :C] for b in range(B)])
    dec.decode(rows, states, [False] * B, check=False)
    torch_mod.cuda.synchronize()
    _native.check(_native.lib.ctcd_check_status(dec._handle, 0))
    got = (tok.cpu(), sc.cpu(), ts.cpu(), ln.view(4, n_best).cpu(), stable.cpu())
    for b in range(4):
        pu.assert_peek_equals(_peek_view(got, b), first, b, n_best, 0, "queued peek, stream %d" % b)
    assert any(int(first["timesteps"][b, 0, :int(first["lens"][b, 0])].max(initial=0)) >= kept4[b] for b in range(4)), "no reported time step was moved by a map"
    # every stream ends (the first four have all their frames already), and everything matches the one-shot decode
    out = dec.decode(x[:, C:], states, [True] * B, seq_lens=torch_mod.tensor([0] * 4 + [C] * 4, dtype=torch_mod.int32))
    _same_as(out, want, K, [N] * B, "after the queued peek")


# ---- compact and the policy; unchecked chunks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["compact", "policy"])
def test_compaction_changes_nothing(torch_mod, how):
    B, N, V, K, thr, C = 2, 160, 29, 8, 0.6, 20
    lp = ou.synth_logprobs(B, N, V, 45, blank_bias=3.0)
    want, kept, n2 = bu.decode(lp, None, thr, beam=K)
    dec = _online(V, K, thr, **(dict(compact_pool_above=1) if how == "policy" else {}))
    states = None
    if how == "policy":  # (blocks of 8 frames: every other chunk outgrows its pool)
        from test_gpu_stream_compact import _state

        states = [_state(dec, 8) for _ in range(B)]
    maps = []

    def between(c, sts):
        from ctcdecode_amd import _native

        if how == "compact":
            dec.compact(sts)
        maps.append(int(_native.lib.ctcd_stream_map_bytes(sts[0].state)))

    out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [C] * (N // C), states=states, check=False, between=between)
    assert maps == sorted(maps) and [st.frames for st in states] == n2.tolist()
    _same_as(out, want, K, seen, how)


# ---- built-in scorer -------------------------------------------------------------------------------------------------------------------
def test_built_in_scorer(torch_mod):
    c = dict(pu.LM_PEEK_CASES[0], B=2, T=80, K=16)
    lp, kw = pu.lm_case_inputs(c)
    x0 = lp.copy()
    x0[:, :, 0] += np.float32(4.0)  # (a dominant blank, so that the filter has frames to drop)
    m = x0.max(-1, keepdims=True)
    lp = np.ascontiguousarray((x0 - (m + np.log(np.exp(x0 - m).sum(-1, keepdims=True)))).astype(np.float32))
    path = os.path.join(pu.DATA, c["arpa"])
    which = bu.which_oracle()
    want, kept, n2 = bu.decode(lp, None, 0.6, scorer=ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which=which), which=which, **kw)
    assert 0 < n2.min() and n2.max() < c["T"]
    dec = _online(len(c["labels"]), c["K"], 0.6, labels=c["labels"], model_path=path, alpha=c["alpha"], beta=c["beta"], cutoff_top_n=kw["cutoff_top_n"])
    out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [30, 30, 20])
    _same_as(out, want, c["K"], seen, "built-in scorer")


def test_callback_scorer_streams_take_the_filter(torch_mod):
    """The built-in tables behind the callback hook: the stream ends through ctcd_stream_decode's rounds, on the kept rows."""
    import ctcdecode_amd
    from test_gpu_lm import _BuiltinBehindCallback

    c = dict(pu.LM_PEEK_CASES[0], B=2, T=60, K=16)
    lp, kw = pu.lm_case_inputs(c)
    x0 = lp.copy()
    x0[:, :, 0] += np.float32(4.0)
    m = x0.max(-1, keepdims=True)
    lp = np.ascontiguousarray((x0 - (m + np.log(np.exp(x0 - m).sum(-1, keepdims=True)))).astype(np.float32))
    path = os.path.join(pu.DATA, c["arpa"])
    want, kept, n2 = bu.decode(lp, None, 0.6, scorer=ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which="restated"), which="restated", **kw)
    assert 0 < n2.min() and n2.max() < c["T"]
    inner = _BuiltinBehindCallback(dict(labels=c["labels"], lm_path=path))
    try:
        cs = ctcdecode_amd.CallbackScorer(inner, inner.vocabulary, inner.order, c["labels"], alpha=c["alpha"], beta=c["beta"], device="cuda:0")
        dec = _online(len(c["labels"]), c["K"], 0.6, labels=c["labels"], scorer=cs, cutoff_top_n=kw["cutoff_top_n"])
        out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [30, 30])
        assert [st.frames for st in states] == n2.tolist()
        _same_as(out, want, c["K"], seen, "callback scorer")
    finally:
        inner.close()


# ---- unchecked chunks --------------------------------------------------------------------------------------------------------------
def test_unchecked_chunks_then_a_checked_end(torch_mod):
    """A run of check=False chunks (the wait for the kept counts stays, the wait for the status words goes) and a checked stream end."""
    B, N, V, K, thr = 3, 140, 29, 8, 0.6
    lp = ou.synth_logprobs(B, N, V, 51, blank_bias=4.0)
    want, kept, n2 = bu.decode(lp, None, thr, beam=K)
    dec = _online(V, K, thr)
    seen_counts = []
    out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [20] * 7, check=False,
                             between=lambda c, sts: seen_counts.append(dec.last_blank_skip()))
    for c, (considered, k) in enumerate(seen_counts):  # the counts are on the host when the call returns
        assert considered == B * 20 and k == int(((kept >= c * 20) & (kept < (c + 1) * 20) & (np.arange(N)[None] < n2[:, None])).sum()), c
    assert [st.frames for st in states] == n2.tolist()
    _same_as(out, want, K, seen, "unchecked chunks")


# ---- beyond frame 65535 ----------------------------------------------------------------------------------------------------------------
def test_beyond_frame_65535(torch_mod, monkeypatch):
    from ctcdecode_amd import _native

    lp = ou.synth_logprobs(1, 66000, 5, 3, blank_bias=4.0)
    want, kept, n2 = bu.decode(lp, None, 0.6, beam=4)
    assert int(n2[0]) == 3417 and int((kept[0, :3417] >= 65536).sum()) == 33
    calls = []
    real = _native.lib.ctcd_stream_decode_to_host

    def counted(*args):
        calls.append(1)
        return real(*args)

    monkeypatch.setattr(_native.lib, "ctcd_stream_decode_to_host", counted)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec = _online(5, 4, 0.6)
    out, states, seen = _run(torch_mod, dec, x, [6000] * 11, check=False)
    assert calls == [], "a stream that has seen more than 65536 frames must not end on the compact route"
    assert states[0].frames == 3417 and states[0].frames_seen == 66000
    _same_as(out, want, 4, seen, "66000 frames")
    assert int(out[2][0, 0].max()) > 65535 and int(want["timesteps"][0, 0].max()) > 65535
    # 60 000 frames: frames seen + T stays within 16 bits, the stream ends on the compact route
    want2, kept2, n22 = bu.decode(np.ascontiguousarray(lp[:, :60000]), None, 0.6, beam=4)
    out2, states2, seen2 = _run(torch_mod, dec, x[:, :60000], [6000] * 10, check=False)
    assert calls == [1], "the 60 000-frame stream did not end on the compact route"
    _same_as(out2, want2, 4, seen2, "60000 frames")


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_save_and_restore_are_refused_and_the_stream_decodes_on(torch_mod):
    import ctcdecode_amd

    B, N, V, K, thr = 2, 90, 29, 8, 0.6
    lp = ou.synth_logprobs(B, N, V, 47, blank_bias=4.0)
    want, kept, n2 = bu.decode(lp, None, thr, beam=K)
    dec = _online(V, K, thr)

    def between(c, states):
        with pytest.raises(NotImplementedError):
            dec.save(states)

    out, states, seen = _run(torch_mod, dec, torch_mod.from_numpy(lp).to("cuda:0"), [32, 32, 26], between=between)
    _same_as(out, want, K, seen, "after a refused save")
    plain = _online(V, K, None)
    st = ctcdecode_amd.DecoderState(plain)
    plain.decode(torch_mod.from_numpy(lp[:1, :30]).to("cuda:0"), [st], [False])
    blobs = plain.save([st])
    with pytest.raises(NotImplementedError):
        dec.restore(blobs)


def test_native_refusals_leave_the_stream_as_it_was(torch_mod):
    """The C layer's own refusals (the Python class raises before it gets there): ctcd_stream_save of a filtered stream, and a stream
    with frames under the other setting on every streaming call."""
    import ctypes

    import ctcdecode_amd
    from ctcdecode_amd import _native

    V, K, thr = 29, 8, 0.6
    lp = ou.synth_logprobs(1, 90, V, 49, blank_bias=4.0)
    x = torch_mod.from_numpy(lp).to("cuda:0")
    dec = _online(V, K, thr)
    st = ctcdecode_amd.DecoderState(dec)
    dec.decode(x[:, :30], [st], [False])
    frames, seen = st.frames, st.frames_seen
    assert 0 < frames < seen == 30
    ptrs = (ctypes.c_void_p * 1)(st.state.value)
    sizes = (ctypes.c_ulonglong * 1)()
    cb = _native.BYTES_ALLOC_FN(lambda _u, _n: None)
    assert _native.lib.ctcd_stream_save(dec._handle, ptrs, 1, cb, None, sizes, None) == -2
    # the filter off on this decoder: the filtered stream is refused by a chunk, a peek and a commit, and is unchanged
    _native.check(_native.lib.ctcd_set_stream_blank_skip(dec._handle, 0, 0.0, 0.0))
    with pytest.raises(ValueError, match="blank-frame filter"):
        dec.decode(x[:, 30:60], [st], [False])
    with pytest.raises(ValueError, match="blank-frame filter"):
        dec.peek([st])
    with pytest.raises(ValueError, match="blank-frame filter"):
        dec.commit([st])
    assert (st.frames, st.frames_seen) == (frames, seen)
    # ... and the other way round: a stream that took frames without the filter is refused once it is on
    other = ctcdecode_amd.DecoderState(dec)
    dec.decode(x[:, :30], [other], [False])
    assert other.frames == other.frames_seen == 30
    _native.check(_native.lib.ctcd_set_stream_blank_skip(dec._handle, 1, float(bu.bound(thr, "prob")), float(bu.bound(thr, "log"))))
    with pytest.raises(ValueError, match="blank-frame filter"):
        dec.decode(x[:, 30:60], [other], [False])
    assert other.frames == other.frames_seen == 30
    # the filtered stream decodes on and matches
    want = bu.decode(lp, None, thr, beam=K)[0]
    dec.decode(x[:, 30:60], [st], [False])
    out = dec.decode(x[:, 60:], [st], [True])
    _same_as(out, want, K, [90], "after the refusals")
