"""-m gpu tests of ``CTCBeamDecoder(blank_skip=thr)``: every one-shot route, bit for bit against the definition restated in
tests/blank_skip_util.py (the filter in numpy, the oracle's decode of the kept rows, the time steps mapped back)."""
import blank_skip_util as bs
import numpy as np
import oracle_util as ou
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _labels(V):
    return [str(i) for i in range(V)]


def _dec(V, **kw):
    import ctcdecode_amd

    kw.setdefault("log_probs_input", True)
    kw.setdefault("cutoff_top_n", V)
    return ctcdecode_amd.CTCBeamDecoder(_labels(V), **kw)


def _dict(res, want):
    out, scores, ts, lens = [t.cpu().numpy() for t in res]
    return dict(tokens=out, timesteps=ts, scores=scores, lens=lens, nres=want["nres"])


def _check(res, want, what):
    got = _dict(res, want)
    assert got["tokens"].shape == want["tokens"].shape and got["timesteps"].shape == want["timesteps"].shape, what
    ou.assert_same(got, want, what)
    B, K = got["lens"].shape
    for b in range(B):
        for p in range(K):
            L = int(got["lens"][b, p]) if p < int(want["nres"][b]) else 0
            assert not got["tokens"][b, p, L:].any() and not got["timesteps"][b, p, L:].any(), "%s: item %d row %d is not zero beyond its prefix" % (what, b, p)
    return got


def _torch_half(torch, values, dtype):
    t = torch.from_numpy(np.ascontiguousarray(values, np.float32))
    return t if dtype == "f32" else t.to(torch.float16 if dtype == "f16" else torch.bfloat16)


ROUTES = ["decode_device", "decode_cpu", "decode_dev", "decode_padded", "compact", "compact_async", "pipeline"]


@pytest.mark.parametrize("route", ROUTES)
def test_anchor_case_through_every_route(torch_mod, route):
    import ctcdecode_amd

    torch = torch_mod
    a = bs.ANCHOR
    lp, sl = bs.anchor_input()
    want, kept, n2 = bs.anchor_want()
    x, xs = torch.from_numpy(lp), torch.from_numpy(sl)
    dec = _dec(a["V"], beam_width=a["beam"], blank_skip=a["thr"])
    if route == "decode_device":
        res = dec.decode_device(x, xs)
    elif route == "decode_cpu":
        res = dec.decode(x, xs)
        assert not res[0].is_cuda
    elif route == "decode_dev":
        res = dec.decode(x.cuda(), xs.cuda())
    elif route == "decode_padded":
        res = dec.decode_padded(x, xs)
    elif route in ("compact", "compact_async"):
        if route == "compact":
            hdr, ent, labels, scores, lens = dec.decode_compact(x, xs)
        else:
            hdr, ent, labels, scores, lens = dec.finish_compact(dec.decode_compact_async(x, xs))
        out, ts = dec.expand_compact(hdr, ent, labels, a["T"])
        res = (out, scores, ts, lens)
    else:
        pipe = ctcdecode_amd.DecodePipeline(lambda: _dec(a["V"], beam_width=a["beam"], blank_skip=a["thr"]), inflight=2)
        tickets = [pipe.submit(x, xs), pipe.submit(x.flip(0).contiguous(), xs.flip(0).contiguous()), pipe.submit(x, xs)]
        rs = [pipe.result(t) for t in tickets]
        pipe.drain()
        _check(rs[2], want, "pipeline, third batch")
        flipped = {k: v[::-1].copy() for k, v in want.items()}
        _check(rs[1], flipped, "pipeline, second batch (items reversed)")
        res = rs[0]
    _check(res, want, route)
    if route != "pipeline":
        assert dec.last_blank_skip() == (int(sl.sum()), int(n2.sum())), dec.last_blank_skip()


def test_skip_blank_frames_alone(torch_mod):
    torch = torch_mod
    a = bs.ANCHOR
    lp, sl = bs.anchor_input()
    _, kept, n2 = bs.anchor_want()
    dec = _dec(a["V"], beam_width=a["beam"], blank_skip=a["thr"])
    rows, lens, k = dec.skip_blank_frames(torch.from_numpy(lp), torch.from_numpy(sl))
    assert rows.is_cuda and rows.shape == lp.shape and rows.dtype == torch.float32 and k.shape == (a["B"], a["T"])
    assert np.array_equal(lens.cpu().numpy(), n2) and np.array_equal(k.cpu().numpy(), kept), "n' or kept (zero tail included) differ"
    rows = rows.cpu().numpy()
    for b in range(a["B"]):
        assert np.array_equal(rows[b, :n2[b]].view(np.uint32), lp[b, kept[b, :n2[b]]].view(np.uint32)), b
    assert dec.last_blank_skip() == (int(sl.sum()), int(n2.sum()))
    rows, lens, k = dec.skip_blank_frames(torch.from_numpy(lp))  # no seq_lens: every frame of T
    kept_all, n_all = bs.filter_frames(lp, None, 0, a["thr"], "log")
    assert np.array_equal(lens.cpu().numpy(), n_all) and np.array_equal(k.cpu().numpy(), kept_all)
    with pytest.raises(ValueError):
        _dec(a["V"]).skip_blank_frames(torch.from_numpy(lp))


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("V", [29, 31, 32])
def test_dtypes_and_row_alignments(torch_mod, dtype, V):
    """Half rows at 2-, 2- and 16-byte alignment, float32 rows at 4 and 16: the 16-byte gather and the element-wise one."""
    torch = torch_mod
    B, T, K = 3, 70, 4
    vals = bs.to_dtype_values(bs.synth(B, T, V, 40 + V), dtype)
    sl = np.asarray([T, 41, 9], np.int32)
    want, kept, n2 = bs.decode(vals, sl, 0.6, beam=K, cutoff_top_n=V)
    assert 0 < n2.sum() < sl.sum()
    x = _torch_half(torch, vals, dtype).cuda()
    dec = _dec(V, beam_width=K, blank_skip=0.6)
    rows, lens, k = dec.skip_blank_frames(x, torch.from_numpy(sl))
    assert rows.dtype == x.dtype and np.array_equal(k.cpu().numpy(), kept) and np.array_equal(lens.cpu().numpy(), n2)
    rows = rows.float().cpu().numpy()
    for b in range(B):
        assert np.array_equal(rows[b, :n2[b]].view(np.uint32), vals[b, kept[b, :n2[b]]].view(np.uint32)), "kept rows of item %d differ" % b
    _check(dec.decode_device(x, torch.from_numpy(sl)), want, "%s V=%d" % (dtype, V))


def test_pruned_class(torch_mod):
    torch = torch_mod
    B, T, V, K = 3, 90, 64, 8
    lp = bs.synth(B, T, V, 71)
    sl = np.asarray([T, 50, 77], np.int32)
    want, kept, n2 = bs.decode(lp, sl, 0.6, beam=K, cutoff_top_n=8)
    dec = _dec(V, beam_width=K, cutoff_top_n=8, blank_skip=0.6)
    _check(dec.decode_device(torch.from_numpy(lp), torch.from_numpy(sl)), want, "V=64, cutoff_top_n=8")
    _check(dec.decode(torch.from_numpy(lp), torch.from_numpy(sl)), want, "V=64, cutoff_top_n=8, decode()")


def test_logits_input_equals_the_log_softmax_composition(torch_mod):
    torch = torch_mod
    B, T, V, K = 3, 80, 29, 8
    z = bs.synth(B, T, V, 72, mode="logits")
    sl = np.asarray([T, 33, 60], np.int32)
    want, kept, n2 = bs.decode(z, sl, 0.6, mode="logits", beam=K, cutoff_top_n=V)
    assert 0 < n2.sum() < sl.sum()
    x, xs = torch.from_numpy(z), torch.from_numpy(sl)
    dec = _dec(V, beam_width=K, log_probs_input=False, logits_input=True, blank_skip=0.6)
    got = _check(dec.decode_device(x, xs), want, "logits_input")
    _check(dec.decode(x, xs), want, "logits_input, decode()")
    # the composition by hand: the log-softmax pass, then a log-probability decoder with the same threshold
    lsm = dec.log_softmax(x, xs)
    comp = _dict(_dec(V, beam_width=K, blank_skip=0.6).decode_device(lsm, xs), want)
    for k in ("tokens", "timesteps", "lens"):
        assert np.array_equal(got[k], comp[k]), k
    assert np.array_equal(got["scores"].view(np.uint32), comp["scores"].view(np.uint32))
    rows, lens, kk = dec.skip_blank_frames(x, xs)
    assert rows.dtype == torch.float32 and np.array_equal(kk.cpu().numpy(), kept)
    # bfloat16 logits: filtered on the float32 log-softmax of the widened rows
    zb = bs.to_dtype_values(z, "bf16")
    want_b, _, _ = bs.decode(zb, sl, 0.6, mode="logits", beam=K, cutoff_top_n=V)
    _check(dec.decode_device(_torch_half(torch, zb, "bf16").cuda(), xs), want_b, "bfloat16 logits")


def test_probability_input_and_last_label_as_blank(torch_mod):
    torch = torch_mod
    B, T, V, K = 3, 80, 29, 8
    sl = np.asarray([T, 0, 45], np.int32)
    p = bs.synth(B, T, V, 73, mode="prob")
    want, kept, n2 = bs.decode(p, sl, 0.6, mode="prob", beam=K, cutoff_top_n=V)
    assert 0 < n2.sum() < sl.sum()
    dec = _dec(V, beam_width=K, log_probs_input=False, blank_skip=0.6)
    _check(dec.decode_device(torch.from_numpy(p), torch.from_numpy(sl)), want, "probabilities")
    _check(dec.decode(torch.from_numpy(p), torch.from_numpy(sl)), want, "probabilities, decode()")
    lp = bs.synth(B, T, V, 74, blank_id=V - 1)
    want, kept, n2 = bs.decode(lp, sl, 0.6, blank_id=V - 1, beam=K, cutoff_top_n=V)
    assert 0 < n2.sum() < sl.sum()
    dec = _dec(V, beam_width=K, blank_id=V - 1, blank_skip=0.6)
    _check(dec.decode_device(torch.from_numpy(lp), torch.from_numpy(sl)), want, "blank_id = V - 1")


def test_scan_crosses_chunks(torch_mod):
    torch = torch_mod
    T, V, K = 2 * 1024 + 37, 29, 4
    lp = bs.synth(2, T, V, 75)
    sl = np.asarray([T, 2 * 1024 - 1], np.int32)
    want, kept, n2 = bs.decode(lp, sl, 0.6, beam=K, cutoff_top_n=V)
    assert n2[0] > 1024 and kept[0, n2[0] - 1] > 2 * 1024
    dec = _dec(V, beam_width=K, blank_skip=0.6)
    rows, lens, k = dec.skip_blank_frames(torch.from_numpy(lp), torch.from_numpy(sl))
    assert np.array_equal(lens.cpu().numpy(), n2) and np.array_equal(k.cpu().numpy(), kept)
    _check(dec.decode_device(torch.from_numpy(lp), torch.from_numpy(sl)), want, "T = 2 * 1024 + 37")


def test_edges(torch_mod):
    torch = torch_mod
    B, T, V, K = 3, 60, 29, 8
    lp = bs.synth(B, T, V, 76)
    sl = np.asarray([T, 0, 37], np.int32)
    x, xs = torch.from_numpy(lp), torch.from_numpy(sl)
    # thr = 1.0 on normalised log-probabilities skips nothing: blank_skip=None bit for bit, whole tensors
    a = [t.cpu().numpy() for t in _dec(V, beam_width=K, blank_skip=1.0).decode_device(x, xs)]
    b = [t.cpu().numpy() for t in _dec(V, beam_width=K).decode_device(x, xs)]
    for g, w in zip(a, b):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), "thr = 1.0 differs from blank_skip=None"
    a = _dec(V, beam_width=K, blank_skip=1.0).decode(x, xs)
    b = _dec(V, beam_width=K).decode(x, xs)
    for g, w in zip(a, b):
        assert np.array_equal(g.numpy().view(np.uint32), w.numpy().view(np.uint32)), "thr = 1.0 differs from blank_skip=None, decode()"
    # a bias that skips every frame: root-only results, as for the item with seq_lens = 0
    hot = bs.synth(B, T, V, 77, blank_bias=30.0)
    want, kept, n2 = bs.decode(hot, sl, 0.6, beam=K, cutoff_top_n=V)
    assert not n2.any()
    dec = _dec(V, beam_width=K, blank_skip=0.6)
    got = _check(dec.decode_device(torch.from_numpy(hot), xs), want, "every frame skipped")
    for i in range(B):
        bs.assert_root_only(got, i, "item %d" % i)
    assert dec.last_blank_skip() == (int(sl.sum()), 0)
    _check(dec.decode(torch.from_numpy(hot), xs), want, "every frame skipped, decode()")
    # a blank value exactly equal to the bound is kept, the next float above it is skipped; a blank-dominated frame directly at
    # seq_lens[b] is not counted
    c = bs.bound(0.6, "log")
    e = lp.copy()
    e[0, :, 0] = np.float32(-1e-3)
    e[0, 10:20, 0] = c
    e[0, 25, 0] = np.nextafter(c, np.float32(0))
    e[2, :37, 0] = np.float32(-3)
    e[2, 37, 0] = np.float32(-1e-3)
    want, kept, n2 = bs.decode(e, sl, 0.6, beam=K, cutoff_top_n=V)
    assert kept[0, :n2[0]].tolist() == list(range(10, 20)) and n2[2] == 37
    _check(dec.decode_device(torch.from_numpy(e), xs), want, "values at the bound")
    assert dec.last_blank_skip() == (int(sl.sum()), int(n2.sum()))


def test_nan_and_infinities_at_the_blank_follow_the_ordered_compare(torch_mod):
    """The filter alone (a NaN row is not a decodable input): NaN is kept -- every compare with it is false --, -inf is kept, and +inf,
    greater than any bound, is skipped, as the restated definition has it; in float32 and in both half formats."""
    torch = torch_mod
    B, T, V = 2, 40, 29
    lp = bs.synth(B, T, V, 78)
    lp[0, :, 0] = np.float32(-1e-3)
    lp[0, 5, 0] = np.float32("nan")
    lp[0, 6, 0] = np.float32("inf")
    lp[0, 7, 0] = np.float32("-inf")
    lp[1, 0, 0] = np.float32("nan")
    for dtype in ("f32", "f16", "bf16"):
        vals = bs.to_dtype_values(lp, dtype)
        kept, n2 = bs.filter_frames(vals, None, 0, 0.6, "log")
        assert kept[0, :n2[0]].tolist() == [5, 7]
        rows, lens, k = _dec(V, blank_skip=0.6).skip_blank_frames(_torch_half(torch, vals, dtype).cuda())
        assert np.array_equal(lens.cpu().numpy(), n2) and np.array_equal(k.cpu().numpy(), kept), dtype


@pytest.mark.parametrize("kind", ["builtin", "callback"])
def test_scorers(torch_mod, kind):
    """The composition sits outside the scorer's relaunch logic: the built-in ARPA scorer, and a CallbackScorer over the same tables."""
    import ctcdecode_amd
    from test_gpu_scorer_batch import _Builtin, _scorer
    from test_lm import LABELS29, TEST_ARPA

    torch = torch_mod
    B, T, V, K = 2, 60, 29, 8
    lp = ou.synth_logprobs(B, T, V, 79, blank_bias=3.5)
    lp[:, :, LABELS29.index(" ")] += np.float32(1.5)
    lp = ou.log_softmax_rows(lp)
    sl = np.asarray([T, 41], np.int32)
    which = bs.which_oracle()
    want, kept, n2 = bs.decode(lp, sl, 0.6, beam=K, cutoff_top_n=V, which=which, scorer=ou.Scorer(0.7, 0.9, TEST_ARPA, LABELS29, which=which))
    assert 0 < n2.sum() < sl.sum()
    x, xs = torch.from_numpy(lp), torch.from_numpy(sl)
    inner = None
    try:
        if kind == "builtin":
            dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, model_path=TEST_ARPA, alpha=0.7, beta=0.9, beam_width=K, cutoff_top_n=V, log_probs_input=True,
                                               blank_skip=0.6)
        else:
            inner = _Builtin(LABELS29, TEST_ARPA)
            sc = _scorer("python", inner, LABELS29, 0.7, 0.9)
            dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, scorer=sc, beam_width=K, cutoff_top_n=V, log_probs_input=True, blank_skip=0.6)
        _check(dec.decode_device(x, xs), want, kind)
        _check(dec.decode(x, xs), want, kind + ", decode()")
    finally:
        if inner is not None:
            del dec, sc
            inner.close()


def test_unchecked_calls_back_to_back(torch_mod):
    """check=False: two calls queued on one stream, nothing waits for the host in between, one ctcd_check_status at the end."""
    from ctcdecode_amd import _native

    torch = torch_mod
    a = bs.ANCHOR
    lp, sl = bs.anchor_input()
    want, _, _ = bs.anchor_want()
    lp2 = bs.synth(a["B"], a["T"], a["V"], 80)
    want2, _, _ = bs.decode(lp2, sl, a["thr"], beam=a["beam"], cutoff_top_n=a["V"])
    x, x2, xs = torch.from_numpy(lp).cuda(), torch.from_numpy(lp2).cuda(), torch.from_numpy(sl).cuda()
    dec = _dec(a["V"], beam_width=a["beam"], blank_skip=a["thr"])
    r1 = dec.decode_device(x, xs, check=False)
    r2 = dec.decode_device(x2, xs, check=False)
    _native.check(_native.lib.ctcd_check_status(dec._handle, a["B"]))
    _check(r1, want, "first unchecked call")
    _check(r2, want2, "second unchecked call")


def test_length_order_ranks_by_kept_frames(torch_mod):
    torch = torch_mod
    B, T, V, K = 4, 100, 29, 8
    lp = bs.synth(B, T, V, 81)
    lp[1, :, 0] = np.float32(-1e-3)  # the longest utterance keeps the fewest frames
    lp[1, ::9, 0] = np.float32(-4)
    sl = np.asarray([60, T, 80, 40], np.int32)
    want, kept, n2 = bs.decode(lp, sl, 0.6, beam=K, cutoff_top_n=V)
    order = sorted(range(B), key=lambda b: (-int(n2[b]), b))
    assert order != sorted(range(B), key=lambda b: (-int(sl[b]), b)), "the kept counts rank as the lengths do"
    dec = _dec(V, beam_width=K, blank_skip=0.6)
    dec.set_launch_order("length")
    _check(dec.decode_device(torch.from_numpy(lp), torch.from_numpy(sl)), want, "length order")
    assert dec.last_launch_order().tolist() == order, (dec.last_launch_order(), order, n2)
    dec.set_launch_order("batch")
    _check(dec.decode_device(torch.from_numpy(lp), torch.from_numpy(sl)), want, "batch order")
