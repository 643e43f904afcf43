"""-m gpu tests of the greedy decode (``CTCBeamDecoder.greedy_decode`` / ``greedy_decode_device`` / ``ctcd_greedy_decode``): device
output == the numpy / Python restatement of the header's definition (tests/greedy_util.py), bit for bit -- scores and label scores as
uint32, labels and frames exactly -- at the shapes where the kernels can go wrong.  The cases are those of tests/test_greedy_host.py;
a reference is computed once per process."""
import greedy_util as gu
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _dec(V, blank=0, mode=1, **kw):
    import ctcdecode_amd

    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, beam_width=kw.pop("beam_width", 8), log_probs_input=mode == 1,
                                        logits_input=mode == 2, **kw)


def _numpy(outs):
    tok, sc, st, lens, en, ls = (o.cpu().numpy() for o in outs)
    return dict(tokens=tok[:, 0], scores=sc[:, 0], starts=st[:, 0], lens=lens[:, 0], ends=en[:, 0], label_scores=ls[:, 0])


def _decode(torch, c, rows=None):
    """dec.greedy_decode_device(details=True) on the case's rows (``rows``: another tensor of them) -> result dict (numpy)."""
    dec = _dec(c["x"].shape[2], c["blank"], c["mode"])
    x = gu.to_torch(torch, c["stored"], c["dtype"]) if rows is None else rows
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    outs = dec.greedy_decode_device(x, seq, details=True)
    B, T = c["x"].shape[:2]
    assert [tuple(o.shape) for o in outs] == [(B, 1, T), (B, 1), (B, 1, T), (B, 1), (B, 1, T), (B, 1, T)] and all(o.is_cuda for o in outs)
    assert [o.dtype for o in outs] == [torch.int32, torch.float32, torch.int32, torch.int32, torch.int32, torch.float32]
    return _numpy(outs)


def _check(torch, c, what, rows=None):
    want = gu.cached(("ref", what), lambda: gu.case_reference(c))
    gu.assert_same(_decode(torch, c, rows), want, what)
    return want


@pytest.mark.parametrize("V", gu.V_LIST)
def test_device_equals_the_restatement_over_the_label_counts(torch_mod, V):
    """1 .. 64 labels: 1 .. 64 lanes per frame; 65 .. 256: a wave per frame; from 260 on, where rows are whole vectors: a workgroup
    per frame (1024 / 1028 / 2056 / 4104 / 10000 / 10248: every count of float4s a thread holds of a logit row); 4098: no whole vectors."""
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            _check(torch_mod, gu.shape_case(V, mode, dtype), "V %d mode %d dtype %d" % (V, mode, dtype))


@pytest.mark.parametrize("T", gu.T_LIST)
def test_device_equals_the_restatement_over_the_frame_counts(torch_mod, T):
    for mode in gu.MODES:
        _check(torch_mod, gu.shape_case(3, mode, 0, T=T), "T %d mode %d" % (T, mode))


def test_seq_lens(torch_mod):
    """0, 1, ragged, T, above T, negative; None is every other test."""
    for mode in gu.MODES:
        c = gu.shape_case(5, mode, 0, T=12, B=6)
        c["seq_lens"] = np.asarray([0, 1, 7, 12, 40, -3], np.int32)
        _check(torch_mod, c, "seq_lens mode %d" % mode)
    c = gu.shape_case(1024, 2, 2, T=6, B=3)  # (the workgroup kernels skip frames too)
    c["seq_lens"] = np.asarray([2, 0, 9], np.int32)
    _check(torch_mod, c, "seq_lens V 1024 logits")
    c = gu.shape_case(1024, 1, 0, T=6, B=3)
    c["seq_lens"] = np.asarray([2, 0, 9], np.int32)
    _check(torch_mod, c, "seq_lens V 1024 log-probabilities")


def test_input_off_the_16_byte_boundary(torch_mod):
    """A contiguous input whose base pointer is one element off a 16-byte boundary, V = 1024: the element path."""
    torch = torch_mod
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            c = gu.shape_case(1024, mode, dtype)
            x = gu.to_torch(torch, c["stored"], dtype)
            flat = torch.empty((x.numel() + 8,), dtype=x.dtype, device="cuda")
            off = 1 + (-flat.data_ptr() % 16) // x.element_size()
            rows = flat[off:off + x.numel()].view(x.shape)
            rows.copy_(x)
            assert rows.is_contiguous() and rows.data_ptr() % 16 == x.element_size()
            _check(torch, c, "V 1024 mode %d dtype %d" % (mode, dtype), rows=rows)


@pytest.mark.parametrize("V", sorted(gu.TIE_PATTERNS))
def test_among_equal_maxima_the_smallest_index_wins(torch_mod, V):
    """Two and three equal maxima in different lanes, waves and vector words; -0.0 against +0.0; a frame of -inf (label 0, the blank being
    the last label)."""
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            _check(torch_mod, gu.tie_case(V, mode, dtype), "ties V %d mode %d dtype %d" % (V, mode, dtype))


@pytest.mark.parametrize("V", [29, 1024, 10000])
def test_rounded_rows_tie_in_most_frames(torch_mod, V):
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            c = gu.coarse_case(V, mode, dtype, B=1 if V > 5000 else 2, T=4 if V > 5000 else 6)
            _check(torch_mod, c, "coarse V %d mode %d dtype %d" % (V, mode, dtype))


@pytest.mark.parametrize("blank", [0, 3, 5])
def test_emission(torch_mod, blank):
    """All frames blank (L = 0); no blank and no repeat (L = T); a a _ a (two labels); a a a (one)."""
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            want = _check(torch_mod, gu.emission_case(blank, mode, dtype)[0], "emission blank %d mode %d dtype %d" % (blank, mode, dtype))
            assert want["lens"].tolist() == [0, 12, 4, 1]


@pytest.mark.parametrize("mode", gu.MODES)
def test_runs_across_the_chunk_boundaries(torch_mod, mode):
    """Runs that end at frame 63 / 1023 and start at 64 / 1024, runs across frame 1024 (one of 1191 frames): ends and label_scores."""
    _check(torch_mod, gu.long_run_case(mode), "long runs mode %d" % mode)


@pytest.mark.parametrize("kind", ["neg_inf_log", "neg_inf_logits", "dominant", "prob_exact"])
def test_scores_at_the_edges_of_float32(torch_mod, kind):
    for V in (29, 1024):
        for dtype in gu.DTYPES:
            _check(torch_mod, gu.score_case(kind, V, dtype), "score %s V %d dtype %d" % (kind, V, dtype))


def test_cpu_results_and_the_drop_in_name(torch_mod):
    """greedy_decode: four CPU tensors in decode's order; CPU input; the methods under the ``ctcdecode`` import name."""
    import ctcdecode

    torch = torch_mod
    assert hasattr(ctcdecode.CTCBeamDecoder, "greedy_decode") and hasattr(ctcdecode.CTCBeamDecoder, "greedy_decode_device")
    c = gu.shape_case(29, 1, 0)
    want = gu.cached(("ref", "V 29 mode 1 dtype 0"), lambda: gu.case_reference(c))
    dec = ctcdecode.CTCBeamDecoder([str(i) for i in range(29)], blank_id=c["blank"], log_probs_input=True)
    for x in (torch.from_numpy(c["stored"]), torch.from_numpy(c["stored"]).cuda()):
        tok, sc, st, lens = dec.greedy_decode(x)
        assert not (tok.is_cuda or sc.is_cuda or st.is_cuda or lens.is_cuda)
        assert tuple(tok.shape) == (2, 1, 9) and tuple(sc.shape) == (2, 1) and tuple(st.shape) == (2, 1, 9) and tuple(lens.shape) == (2, 1)
        gu.assert_same(dict(tokens=tok.numpy()[:, 0], scores=sc.numpy()[:, 0], starts=st.numpy()[:, 0], lens=lens.numpy()[:, 0]), want, "greedy_decode")
    assert len(dec.greedy_decode_device(x)) == 4
    with pytest.raises(ValueError):
        dec.greedy_decode(x[:, :, :7])
    with pytest.raises(ValueError):
        dec.greedy_decode(x[0])
    with pytest.raises(ValueError):
        dec.greedy_decode(x, torch.zeros((3,), dtype=torch.int32))


def _raw(torch, dec, c, details=True, mode=None):
    """Once through the raw ABI: output tensors pre-filled with a sentinel."""
    from ctcdecode_amd import _native

    B, T, V = c["x"].shape
    x = gu.to_torch(torch, c["stored"], c["dtype"])
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"]).cuda()
    tok, st, en, ls_bits = (torch.full((B, T), gu.SENTINEL, dtype=torch.int32, device="cuda") for _ in range(4))
    ls = ls_bits.view(torch.float32)
    sc = torch.full((B,), -123.0, dtype=torch.float32, device="cuda")
    lens = torch.full((B,), gu.SENTINEL, dtype=torch.int32, device="cuda")
    _native.check(_native.lib.ctcd_set_input_dtype(dec._handle, c["dtype"]))
    _native.check(_native.lib.ctcd_greedy_decode(dec._handle, x.data_ptr(), seq.data_ptr() if seq is not None else None, B, T, V, c["blank"],
                                                 c["mode"] if mode is None else mode, tok.data_ptr(), st.data_ptr(), en.data_ptr() if details else None,
                                                 ls.data_ptr() if details else None, sc.data_ptr(), lens.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return dict(tokens=tok.cpu().numpy(), starts=st.cpu().numpy(), ends=en.cpu().numpy(), label_scores=ls.cpu().numpy(), scores=sc.cpu().numpy(),
                lens=lens.cpu().numpy())


def test_raw_abi_writes_every_position(torch_mod):
    """Output buffers pre-filled with a sentinel: every position is written, the tails as zeros; NULL ends / label_scores are left alone."""
    torch = torch_mod
    cases = [gu.emission_case(3, 1, 0)[0], gu.shape_case(29, 2, 2), gu.shape_case(1025, 0, 1)]
    seq = gu.shape_case(5, 1, 0, T=12, B=6)
    seq["seq_lens"] = np.asarray([0, 1, 7, 12, 40, -3], np.int32)
    for i, c in enumerate(cases + [seq]):
        dec = _dec(c["x"].shape[2], c["blank"], c["mode"])
        want = gu.case_reference(c)
        got = _raw(torch, dec, c)
        for k in ("tokens", "starts", "ends", "lens"):
            assert not (got[k] == gu.SENTINEL).any(), "case %d: a position of %s was not written" % (i, k)
        assert not (got["label_scores"].view(np.int32) == gu.SENTINEL).any(), "case %d: a position of label_scores was not written" % i
        gu.assert_same(got, want, "raw ABI, case %d" % i)
        got = _raw(torch, dec, c, details=False)
        assert (got["ends"] == gu.SENTINEL).all() and (got["label_scores"].view(np.int32) == gu.SENTINEL).all()
        gu.assert_same(dict(got, ends=None, label_scores=None), want, "raw ABI without details, case %d" % i)


def test_raw_abi_refuses_bad_shapes(torch_mod):
    from ctcdecode_amd import _native

    torch = torch_mod
    c = gu.shape_case(8, 1, 0, T=4)
    dec = _dec(8)
    x = gu.to_torch(torch, c["stored"], 0)
    tok, st, lens = (torch.full((64,), 7, dtype=torch.int32, device="cuda") for _ in range(3))
    sc = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")

    def call(B=2, T=4, V=8, blank=0, mode=1, probs=x.data_ptr(), tokens=tok.data_ptr(), starts=st.data_ptr(), scores=sc.data_ptr(), out_lens=lens.data_ptr()):
        return _native.lib.ctcd_greedy_decode(dec._handle, probs, None, B, T, V, blank, mode, tokens, starts, None, None, scores, out_lens, None)

    _native.check(_native.lib.ctcd_set_input_dtype(dec._handle, 0))
    assert call() == 0
    for kw in (dict(B=-1), dict(T=-1), dict(V=0), dict(blank=8), dict(blank=-1), dict(mode=3), dict(mode=-1), dict(probs=None), dict(tokens=None),
               dict(starts=None), dict(scores=None), dict(out_lens=None)):
        assert call(**kw) == -1, kw
    assert _native.lib.ctcd_greedy_decode(None, x.data_ptr(), None, 2, 4, 8, 0, 1, tok.data_ptr(), st.data_ptr(), None, None, sc.data_ptr(), lens.data_ptr(), None) == -1
    assert call(V=(1 << 28) + 1, blank=0) == -2, "beyond the V bound of ctcd_ctc_loglik"
    torch.cuda.synchronize()
    lens.fill_(7)
    sc.fill_(7.0)
    assert call(B=0) == 0
    torch.cuda.synchronize()
    assert (lens == 7).all() and (sc == 7.0).all(), "B == 0 launches nothing"
    assert call(B=3, T=0, probs=None, tokens=None, starts=None) == 0
    torch.cuda.synchronize()
    assert lens[:4].tolist() == [0, 0, 0, 7] and sc[:4].tolist() == [0.0, 0.0, 0.0, 7.0], "T == 0: lens and scores are zeros"
    # ... and the decoder is usable afterwards
    gu.assert_same(_decode(torch, c), gu.case_reference(c), "after the refused calls")
    outs = dec.greedy_decode_device(torch.zeros((0, 4, 8), device="cuda"))
    assert [tuple(o.shape) for o in outs] == [(0, 1, 4), (0, 1), (0, 1, 4), (0, 1)]
    outs = dec.greedy_decode(torch.zeros((2, 0, 8), device="cuda"))
    assert tuple(outs[0].shape) == (2, 1, 0) and outs[1].tolist() == [[0.0], [0.0]] and outs[3].tolist() == [[0], [0]]


@pytest.mark.parametrize("mode", gu.MODES)
def test_align_of_the_greedy_row_has_the_greedy_score(torch_mod, mode):
    """No path sums to more than the greedy one (float32 addition is monotone and c*(t) carries the frame's greatest lp): align of the
    greedy row returns the score with equal bits, and log_likelihood a value >= it.  Random rows, B = 8, T = 200, V = 29."""
    torch = torch_mod
    rng = np.random.default_rng(11 + mode)
    raw = gu.random_rows(rng, 8, 200, 29, mode, scale=3.0)
    seq = torch.tensor([200, 199, 150, 64, 1, 0, 200, 77], dtype=torch.int32)
    dec = _dec(29, 0, mode)
    for dtype in gu.DTYPES:
        x = gu.to_torch(torch, gu.as_dtype(raw, dtype)[0], dtype)
        tok, sc, st, lens = dec.greedy_decode_device(x, seq)
        assert int(lens.max()) > 20
        starts, ends, asc = dec.align(x, seq, tok, lens)
        g, a = sc.cpu().numpy(), asc.cpu().numpy()
        print("mode %d dtype %d: greedy %s align %s" % (mode, dtype, g[:3, 0].tolist(), a[:3, 0].tolist()))
        assert np.array_equal(gu.bits(g), gu.bits(a)), "mode %d dtype %d: greedy %s, align %s" % (mode, dtype, g.tolist(), a.tolist())
        assert tuple(starts.shape) == tuple(st.shape) == tuple(ends.shape)
        ll = dec.log_likelihood(x, seq, tok, lens).cpu().numpy()
        assert (ll >= g).all(), "mode %d dtype %d: log-likelihood %s below the greedy score %s" % (mode, dtype, ll.tolist(), g.tolist())
        peaks, occ, conf, ll2 = dec.label_posteriors(x, seq, tok, lens)
        assert np.array_equal(gu.bits(ll2.cpu().numpy()), gu.bits(ll))


def test_a_beam_decode_is_the_same_before_and_after(torch_mod):
    """Regression guard: a decode_device call before and after a greedy call returns identical tensors."""
    torch = torch_mod
    rng = np.random.default_rng(3)
    x = torch.from_numpy(gu.random_rows(rng, 4, 60, 29, 1)).cuda()
    seq = torch.tensor([60, 41, 60, 7], dtype=torch.int32)
    dec = _dec(29, 0, 1, beam_width=16)
    before = [o.clone() for o in dec.decode_device(x, seq)]
    dec.greedy_decode_device(x, seq, details=True)
    dec.greedy_decode_device(x.to(torch.bfloat16), seq)
    after = dec.decode_device(x, seq)
    for b, a in zip(before, after):
        assert torch.equal(b, a)
