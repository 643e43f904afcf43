"""-m gpu tests of ``n_best`` on every one-shot route: the [B, n, ...] tensors against rows [:, :n] of the oracle's, bit for bit on
the region the full call defines (oracle_util.assert_same), and the zeros the n-best tensors add (tests/nbest_util.py)."""
import nbest_util as nb
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


def _check(res, full, n, what):
    """The four tensors of a product call at ``n`` against the oracle's full result."""
    want = nb.want_nbest(full, n)
    got = nb.as_dict(*res, want)
    nb.assert_nbest(got, want, "%s, n_best=%d" % (what, n))
    return got


def _check_full_slices(res_n, res_full, full, n, what):
    """... and against the product's own full call, restricted to [:, :n], on everything the full call defines."""
    got = nb.as_dict(*res_n, nb.want_nbest(full, n))
    mine = nb.as_dict(*res_full, full)
    ou.assert_same(got, {k: (v[:, :n] if k != "nres" else np.minimum(v, n)) for k, v in mine.items()}, what + ": against the full call's slices")


# ---- the anchor shape: B 5, T 67, V 29, beam 16, ragged lengths with a 0 --------------------------------------------------------------
ANCHOR = dict(B=5, T=67, V=29, beam=16, seed=41, seq_lens=[67, 40, 0, 66, 13])


def _anchor():
    a = ANCHOR
    lp = ou.synth_logprobs(a["B"], a["T"], a["V"], a["seed"])
    sl = np.asarray(a["seq_lens"], np.int32)
    return lp, sl, nb.cached("anchor", lambda: ou.decode(lp, sl, beam=a["beam"], cutoff_top_n=a["V"], which=nb.which_oracle()))


ROUTES = ["decode_cpu", "decode_dev", "decode_padded", "decode_device", "compact", "pipeline"]


@pytest.mark.parametrize("n", [1, 3, 15, 16])
@pytest.mark.parametrize("route", ROUTES)
def test_every_route_agrees_with_the_oracle_and_the_full_call(torch_mod, route, n):
    import ctcdecode_amd

    torch = torch_mod
    a = ANCHOR
    lp, sl, full = _anchor()
    dec = _dec(a["V"], beam_width=a["beam"])
    x, xs = torch.from_numpy(lp), torch.from_numpy(sl)
    if route == "decode_cpu":
        res, res_full = dec.decode(x, xs, n_best=n), dec.decode(x, xs)
    elif route == "decode_dev":
        res, res_full = dec.decode(x.cuda(), xs.cuda(), n_best=n), dec.decode(x.cuda(), xs.cuda())
    elif route == "decode_padded":
        res, res_full = dec.decode_padded(x, xs, n_best=n), dec.decode_padded(x, xs)
    elif route == "decode_device":
        res, res_full = dec.decode_device(x, xs, n_best=n), dec.decode_device(x, xs)
        assert all(t.is_cuda for t in res)
    elif route == "compact":
        hdr, ent, labels, scores, lens = dec.decode_compact(x, xs)
        out, ts = dec.expand_compact(hdr, ent, labels, a["T"], n_best=n)
        fout, fts = dec.expand_compact(hdr, ent, labels, a["T"])
        # (the scores and lengths of the compact form are the full call's: columns [:n]; rows without a result are zero there already)
        res, res_full = (out, scores[:, :n], ts, lens[:, :n]), (fout, scores, fts, lens)
    else:
        pipe = ctcdecode_amd.DecodePipeline(lambda: _dec(a["V"], beam_width=a["beam"]), inflight=2)
        tickets = [pipe.submit(x, xs, n_best=n), pipe.submit(x, xs), pipe.submit(x, xs, n_best=n)]
        res, res_full, again = (pipe.result(t) for t in tickets)
        pipe.drain()
        _check(again, full, n, route + ", second submit")
    assert tuple(res[0].shape) == (a["B"], n, a["T"]) and tuple(res[2].shape) == (a["B"], n, a["T"])
    assert tuple(res[1].shape) == (a["B"], n) and tuple(res[3].shape) == (a["B"], n)
    if route in ("decode_cpu", "decode_dev"):
        assert not res[0].is_cuda and res[0].is_pinned(), "decode() returns page-locked [B, n, T] tensors"
    _check(res, full, n, route)
    _check_full_slices(res, res_full, full, n, route)


def test_fewer_results_than_n(torch_mod):
    """T 2, V 3, beam 8, n 8: fewer than eight prefixes exist; the rows beyond them are zero, with length 0 and score 0."""
    torch = torch_mod
    lp = ou.synth_logprobs(2, 2, 3, 4)
    full = ou.decode(lp, None, beam=8, cutoff_top_n=3, which=nb.which_oracle())
    assert (full["nres"] < 8).all(), full["nres"]
    dec = _dec(3, beam_width=8)
    x = torch.from_numpy(lp)
    for name, res in (("decode", dec.decode(x, n_best=8)), ("decode_device", dec.decode_device(x, n_best=8)), ("decode_padded", dec.decode_padded(x, n_best=8))):
        _check(res, full, 8, "nres < n, " + name)
    hdr, ent, labels, scores, lens = dec.decode_compact(x)
    out, ts = dec.expand_compact(hdr, ent, labels, 2, n_best=8)
    _check((out, scores, ts, lens), full, 8, "nres < n, expand_compact")


def test_blank_dominated_row_whose_best_result_is_empty(torch_mod):
    torch = torch_mod
    B, T, V, K = 3, 40, 29, 8
    lp = ou.synth_logprobs(B, T, V, 43, blank_bias=9.0)
    full = ou.decode(lp, None, beam=K, cutoff_top_n=V, which=nb.which_oracle())
    assert (full["lens"][:, 0] == 0).all() and (full["lens"][:, 1] > 0).all(), "the best result is not the empty one"
    dec = _dec(V, beam_width=K)
    x = torch.from_numpy(lp)
    for n in (1, 2):
        _check(dec.decode(x, n_best=n), full, n, "empty best row, decode")
        _check(dec.decode_device(x, n_best=n), full, n, "empty best row, decode_device")


@pytest.mark.parametrize("T", [64, 67])
def test_both_store_paths(torch_mod, T):
    """T 64: rows of whole 16-byte words (the vector stores); T 67: element stores.  Three rows: more rows than one wave writes at a time
    is covered by n = 15 above; here one and three waves."""
    torch = torch_mod
    B, V, K = 3, 29, 16
    lp = ou.synth_logprobs(B, T, V, 44 + T)
    sl = np.asarray([T, T - 9, 1], np.int32)
    full = ou.decode(lp, sl, beam=K, cutoff_top_n=V, which=nb.which_oracle())
    dec = _dec(V, beam_width=K)
    x, xs = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    for n in (1, 3, 16):
        res = dec.decode_device(x, xs, n_best=n)
        assert nb.host_vec16(T, res[0].data_ptr(), res[2].data_ptr()) == (T == 64), "the case does not take the store path it is named for"
        _check(res, full, n, "T=%d" % T)


def test_pruned_class(torch_mod):
    torch = torch_mod
    B, T, V, K = 2, 50, 64, 20
    lp = ou.synth_logprobs(B, T, V, 45)
    full = ou.decode(lp, None, beam=K, cutoff_top_n=8, which=nb.which_oracle())
    dec = _dec(V, beam_width=K, cutoff_top_n=8)
    x = torch.from_numpy(lp)
    _check(dec.decode_device(x, n_best=2), full, 2, "pruned, decode_device")
    _check(dec.decode(x, n_best=2), full, 2, "pruned, decode")


@pytest.mark.parametrize("kind", ["builtin", "callback"])
def test_scorers(torch_mod, kind):
    """The built-in scorer (the row order comes from the LM sorts and differs from trie order): the word model of tests/data, n 1 and 4;
    a callback scorer (the full decode on the device, rows [:, :n] delivered): n 2."""
    import ctcdecode_amd
    from test_gpu_scorer_batch import _Builtin, _scorer
    from test_lm import LABELS29, TEST_ARPA

    torch = torch_mod
    B, T, V, K = 2, 60, 29, 8
    lp = ou.synth_logprobs(B, T, V, 79, blank_bias=2.0)
    lp[:, :, LABELS29.index(" ")] += np.float32(1.5)
    lp = ou.log_softmax_rows(lp)
    sl = np.asarray([T, 41], np.int32)
    which = nb.which_oracle()
    full = ou.decode(lp, sl, beam=K, cutoff_top_n=V, which=which, scorer=ou.Scorer(0.7, 0.9, TEST_ARPA, LABELS29, which=which))
    x, xs = torch.from_numpy(lp), torch.from_numpy(sl)
    inner = None
    try:
        if kind == "builtin":
            dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, model_path=TEST_ARPA, alpha=0.7, beta=0.9, beam_width=K, cutoff_top_n=V, log_probs_input=True)
            ns = (1, 4)
            hdr, ent, _, _, _ = dec.decode_compact(x, xs)
            rows = ent.cpu().numpy()[0, :int(hdr.cpu().numpy()[0, 0]), 0]
            assert rows.tolist() != sorted(rows.tolist()), "the result rows come in trie order: the case does not test a permuted one"
        else:
            inner = _Builtin(LABELS29, TEST_ARPA)
            sc = _scorer("python", inner, LABELS29, 0.7, 0.9)
            dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, scorer=sc, beam_width=K, cutoff_top_n=V, log_probs_input=True)
            ns = (2,)
        for n in ns:
            _check(dec.decode_device(x, xs, n_best=n), full, n, kind + ", decode_device")
            _check(dec.decode(x, xs, n_best=n), full, n, kind + ", decode")
    finally:
        if inner is not None:
            del dec, sc
            inner.close()


def test_bf16_input(torch_mod):
    torch = torch_mod
    B, T, V, K = 2, 50, 29, 8
    xb = torch.from_numpy(ou.synth_logprobs(B, T, V, 46)).to(torch.bfloat16)
    full = ou.decode(xb.float().numpy(), None, beam=K, cutoff_top_n=V, which=nb.which_oracle())
    dec = _dec(V, beam_width=K)
    _check(dec.decode_device(xb.cuda(), n_best=3), full, 3, "bf16, decode_device")
    _check(dec.decode(xb.cuda(), n_best=3), full, 3, "bf16, decode")
    assert dec._in_dtype == 2, "the rows were not read as bfloat16"


def test_logits_input(torch_mod):
    torch = torch_mod
    B, T, V, K = 2, 50, 29, 8
    logits = (ou.synth_logprobs(B, T, V, 47) + np.random.default_rng(47).standard_normal((B, T, 1)).astype(np.float32) * np.float32(3)).astype(np.float32)
    full = ou.decode(ou.log_softmax_rows(logits), None, beam=K, cutoff_top_n=V, which=nb.which_oracle())
    dec = _dec(V, beam_width=K, log_probs_input=False, logits_input=True)
    x = torch.from_numpy(logits)
    _check(dec.decode_device(x, n_best=2), full, 2, "logits, decode_device")
    _check(dec.decode(x, n_best=2), full, 2, "logits, decode")


def test_blank_skip_reports_original_frames(torch_mod):
    """blank_skip 0.9 on blank-dominated rows: the n-best time steps are original frame numbers on every route."""
    import blank_skip_util as bs

    torch = torch_mod
    B, T, V, K = 3, 80, 29, 8
    lp = bs.synth(B, T, V, 48, blank_bias=6.0)  # (blank posteriors around 0.9: about half of the frames go)
    sl = np.asarray([T, 55, 0], np.int32)
    full, kept, n2 = bs.decode(lp, sl, 0.9, beam=K, cutoff_top_n=V)
    assert 0 < n2.sum() < sl.sum(), "the filter drops nothing or everything"
    raw = ou.decode(bs.gather_rows(lp, kept, n2), n2, beam=K, cutoff_top_n=V, which=nb.which_oracle())
    assert not np.array_equal(raw["timesteps"][:, :2], full["timesteps"][:, :2]), "no time step of the first rows moves under the map"
    dec = _dec(V, beam_width=K, blank_skip=0.9)
    x, xs = torch.from_numpy(lp), torch.from_numpy(sl)
    for n in (1, 2):
        _check(dec.decode_device(x, xs, n_best=n), full, n, "blank_skip, decode_device")
        _check(dec.decode(x, xs, n_best=n), full, n, "blank_skip, decode")
        _check(dec.decode_padded(x, xs, n_best=n), full, n, "blank_skip, decode_padded")
        hdr, ent, labels, scores, lens = dec.decode_compact(x, xs)
        out, ts = dec.expand_compact(hdr, ent, labels, T, n_best=n)
        _check((out, scores[:, :n], ts, lens[:, :n]), full, n, "blank_skip, expand_compact")


def test_length_order_with_more_items_than_resident_workgroups(torch_mod):
    torch = torch_mod
    B, T, V, K = 600, 20, 29, 8
    lp = ou.synth_logprobs(B, T, V, 49)
    sl = np.random.default_rng(49).integers(0, T + 1, B).astype(np.int32)
    full = ou.decode(lp, sl, beam=K, cutoff_top_n=V, which=nb.which_oracle())
    dec = _dec(V, beam_width=K)
    dec.set_launch_order("length")
    x, xs = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    _check(dec.decode_device(x, xs, n_best=2), full, 2, "length order, decode_device")
    assert dec.last_launch_order() is not None, "the launch did not run in length order"
    _check(dec.decode(x, xs, n_best=2), full, 2, "length order, decode")


def test_beyond_the_compact_form(torch_mod):
    """T 65537: the compact records cannot hold the frame numbers; the call decodes in full on the device and delivers row 0."""
    torch = torch_mod
    T = 65537
    lp = ou.synth_logprobs(1, T, 3, 17, blank_bias=2.5)
    full = ou.decode(lp, None, beam=4, cutoff_top_n=3, which=nb.which_oracle())
    dec = _dec(3, beam_width=4)
    x = torch.from_numpy(lp)
    _check(dec.decode_device(x, n_best=1), full, 1, "T 65537, decode_device")
    _check(dec.decode(x, n_best=1), full, 1, "T 65537, decode")


def test_no_frames(torch_mod):
    """T == 0: the other case without compact records -- one empty result per item."""
    torch = torch_mod
    dec = _dec(5, beam_width=4)
    x = torch.zeros((2, 0, 5))
    for res in (dec.decode_device(x, n_best=2), dec.decode(x, n_best=2)):
        full = [t.cpu().numpy() for t in (dec.decode_device(x))]
        assert tuple(res[0].shape) == (2, 2, 0) and tuple(res[2].shape) == (2, 2, 0)
        assert np.array_equal(res[1].cpu().numpy().view(np.uint32), full[1][:, :2].view(np.uint32)) and np.array_equal(res[3].cpu().numpy(), full[3][:, :2])
        assert not res[3].cpu().numpy().any()


def test_unchecked_calls_back_to_back(torch_mod):
    """check=False twice on one decoder before any sync: the second call's records overwrite the decoder's scratch behind the first
    call's expansion on the stream; the first result is intact."""
    from ctcdecode_amd import _native

    torch = torch_mod
    a = ANCHOR
    lp, sl, full = _anchor()
    lp2 = ou.synth_logprobs(a["B"], a["T"], a["V"], 50)
    full2 = ou.decode(lp2, sl, beam=a["beam"], cutoff_top_n=a["V"], which=nb.which_oracle())
    x, x2, xs = torch.from_numpy(lp).cuda(), torch.from_numpy(lp2).cuda(), torch.from_numpy(sl).cuda()
    dec = _dec(a["V"], beam_width=a["beam"])
    r1 = dec.decode_device(x, xs, check=False, n_best=3)
    r2 = dec.decode_device(x2, xs, check=False, n_best=3)
    _native.check(_native.lib.ctcd_check_status(dec._handle, a["B"]))
    _check(r1, full, 3, "first unchecked call")
    _check(r2, full2, 3, "second unchecked call")


@pytest.mark.parametrize("bad", [0, 17, 2.5])
def test_invalid_n_best_raises_and_the_decoder_stays_usable(torch_mod, bad):
    import ctcdecode_amd

    torch = torch_mod
    a = ANCHOR
    lp, sl, full = _anchor()
    dec = _dec(a["V"], beam_width=a["beam"])
    x, xs = torch.from_numpy(lp), torch.from_numpy(sl)
    pipe = ctcdecode_amd.DecodePipeline(lambda: _dec(a["V"], beam_width=a["beam"]), inflight=1)
    hdr, ent, labels, _, _ = dec.decode_compact(x, xs)
    for call in (lambda: dec.decode(x, xs, n_best=bad), lambda: dec.decode_device(x, xs, n_best=bad), lambda: dec.decode_padded(x, xs, n_best=bad),
                 lambda: dec.decode_device(x, xs, check=False, n_best=bad), lambda: dec.expand_compact(hdr, ent, labels, a["T"], n_best=bad),
                 lambda: pipe.submit(x, xs, n_best=bad)):
        with pytest.raises(ValueError, match="n_best"):
            call()
    _check(dec.decode(x, xs, n_best=3), full, 3, "decode after a refused call")
    _check(dec.decode_device(x, xs, n_best=3), full, 3, "decode_device after a refused call")
    _check(pipe.result(pipe.submit(x, xs, n_best=3)), full, 3, "pipeline after a refused call")


def test_malformed_records_on_the_device(torch_mod):
    """An offset beyond the label buffer and a row index at the beam width, through expand_compact(n_best): reported, and the rows that
    would have drawn on them come out zero (checked through the C entry point, which leaves the tensors to the caller)."""
    import ctypes

    from ctcdecode_amd import NativeError, _native

    torch = torch_mod
    T = 8
    lab = lambda seq, t0=0: [(c, t0 + 2 * i) for i, c in enumerate(seq)]  # noqa: E731
    entries = [(1, 0, lab([5, 6, 7])), (2, 3, lab([8, 9], 6)), (0, 4, lab([3, 4], 8)), (3, 0, lab([2], 1))]
    hdr, ent, labels = nb.trie(entries)
    want = nb.expand_py(hdr, ent, labels, T)
    dec = _dec(29, beam_width=4)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()  # noqa: E731
    out, ts = dec.expand_compact(dev(hdr), dev(ent), dev(labels), T, n_best=4)
    assert np.array_equal(out.cpu().numpy(), want["tokens"]) and np.array_equal(ts.cpu().numpy(), want["timesteps"])
    for what, (j, field, value), zero_rows in (("offset", (1, 3, labels.size + 100), [0, 2]), ("row index", (2, 0, 4), [0])):
        e = ent.copy()
        e[0, j, field] = value
        with pytest.raises(NativeError, match="malformed"):
            dec.expand_compact(dev(hdr), dev(e), dev(labels), T, n_best=4)
        h, ee, ll = dev(hdr), dev(e), dev(labels)
        tok = torch.full((1, 4, T), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        tss = torch.full((1, 4, T), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        status = torch.zeros((1,), dtype=torch.int32, device="cuda")
        _native.check(_native.lib.ctcd_expand_compact_nbest(dec._handle, h.data_ptr(), ee.data_ptr(), ll.data_ptr(), int(ll.numel()), 1, 4, T, 4, tok.data_ptr(),
                                                            tss.data_ptr(), status.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        assert status.cpu().tolist() == [nb.BAD_RECORD], what
        tok, tss = tok.cpu().numpy(), tss.cpu().numpy()
        ht, hs, ok, st = nb.host_nbest(hdr, e, labels, T, 4, 1)
        assert np.array_equal(tok, ht) and np.array_equal(tss, hs), what + ": the device rows differ from the host twin's"
        for p in zero_rows:
            assert not tok[0, p].any() and not tss[0, p].any(), "%s: row %d is not zero" % (what, p)
