"""-m gpu tests of half-precision input: a HIP tensor of dtype bfloat16 / float16 is decoded without a float32 copy, and the result
is that of the same decoder on ``x.float()`` -- tokens, timesteps, lengths and scores bit for bit, and the vocabulary prune's kept
candidates as well.  Widening is exact, so there is no tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest

import oracle_util as ou

pytestmark = pytest.mark.gpu

KINDS = ("logp", "prob", "logits")
HALVES = ("bfloat16", "float16")


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _rows(torch, B, T, V, seed, kind, dtype, scale=2.0):
    """Seeded float32 logits -> log_softmax / softmax / as they are, in float32, then rounded to `dtype` on the device."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, T, V), generator=g) * scale
    if kind == "logp":
        x = torch.log_softmax(x, -1)
    elif kind == "prob":
        x = torch.softmax(x, -1)
    return x.to(getattr(torch, dtype)).cuda()


def _decoder(V, kind, **kw):
    import ctcdecode_amd

    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], log_probs_input=kind == "logp", logits_input=kind == "logits",
                                        device="cuda:0", **kw)


def _np(ts):
    return [t.cpu().numpy() for t in ts]


def _assert_bits(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert u.dtype == v.dtype and u.shape == v.shape, what
        if u.dtype == np.float32:
            u, v = u.view(np.int32), v.view(np.int32)
        assert np.array_equal(u, v), "%s: output %d differs" % (what, i)


def _assert_prune_rows(p, q, what):
    (c1, l1, v1), (c2, l2, v2) = p, q
    assert np.array_equal(c1, c2), what + ": kept counts"
    for r in range(c1.shape[0]):
        k = int(c1[r])
        assert np.array_equal(l1[r, :k], l2[r, :k]), "%s: labels of frame %d" % (what, r)
        assert np.array_equal(v1[r, :k].view(np.int32), v2[r, :k].view(np.int32)), "%s: values of frame %d" % (what, r)


def _flagged(dec):
    import ctcdecode_amd._native as n

    return int(n.lib.ctcd_last_prune_flagged_rows(dec._handle))


def _in_dtype(dec):
    import ctcdecode_amd._native as n

    return int(n.lib.ctcd_last_input_dtype(dec._handle))


def _oracle_check(x, got, kind, **kw):
    """The oracle on x.float() (log-probabilities or probabilities; the oracle has no logits input)."""
    want = ou.decode(x.float().cpu().numpy(), log_input=kind == "logp", **kw)
    g = dict(tokens=got[0], scores=got[1], timesteps=got[2], lens=got[3], nres=want["nres"])
    ou.assert_same(g, want, "oracle")


@pytest.mark.parametrize("dtype", HALVES)
@pytest.mark.parametrize("kind", KINDS)
def test_unpruned_north_star_class(torch_mod, dtype, kind):
    """Beam 100 over 29 labels, blank 0: the shape of the exact-shape twin (ctcd_set_exact_shape).  Log-probability rows run in both
    modes -- the planned kernel (0) and the twin required (1) -- and say which ran; probabilities and logits run as a caller gets
    them (test_gpu_exact_shape.py::test_rows_that_pass_a_prepass_first holds both kernels behind those pre-passes)."""
    x = _rows(torch_mod, 8, 300, 29, 11, kind, dtype)
    dec = _decoder(29, kind, beam_width=100)
    dec.set_subtree_search(0)  # (the automatic choice follows the last checked launch: every call here plans the plain build)
    res = {}
    for mode in ((0, 1) if kind == "logp" else (-1,)):
        dec.set_exact_shape(mode)
        got = _np(dec.decode_device(x))
        assert _in_dtype(dec) == (1 if dtype == "float16" else 2)
        ran = dec.last_exact_shape()
        want = _np(dec.decode_device(x.float()))
        assert _in_dtype(dec) == 0
        assert ran == dec.last_exact_shape() == (1 if mode else 0), (mode, ran, dec.last_exact_shape())
        _assert_bits(got, want, "%s %s, exact-shape mode %d" % (dtype, kind, mode))
        res[mode] = got
    if kind == "logp":
        _assert_bits(res[1], res[0], "%s %s: the twin against the planned kernel" % (dtype, kind))
        if dtype == "bfloat16":
            for mode in (0, 1):
                dec.set_exact_shape(mode)
                _oracle_check(x[:2], _np(dec.decode_device(x[:2])), kind, beam=100)
                assert dec.last_exact_shape() == mode


@pytest.mark.parametrize("V", [10000, 1001])
@pytest.mark.parametrize("cutoff_prob", [0.99, 0.5])
@pytest.mark.parametrize("kind", KINDS)
def test_pruned(torch_mod, V, cutoff_prob, kind):
    B, T = 4, 60
    x = _rows(torch_mod, B, T, V, 100 + V, kind, "bfloat16", scale=4.0)
    dec = _decoder(V, kind, beam_width=16, cutoff_top_n=40, cutoff_prob=cutoff_prob)
    got = _np(dec.decode_device(x))
    got_rows = dec.last_prune_rows(B * T, 40)
    want = _np(dec.decode_device(x.float()))
    want_rows = dec.last_prune_rows(B * T, 40)
    what = "V%d p%.2f %s" % (V, cutoff_prob, kind)
    _assert_bits(got, want, what)
    _assert_prune_rows(got_rows, want_rows, what)
    if V == 1001 and kind != "logits":
        _oracle_check(x[:1, :30], _np(dec.decode_device(x[:1, :30])), kind, beam=16, cutoff_top_n=40, cutoff_prob=cutoff_prob)
    # fp16 through the same kernels
    y = _rows(torch_mod, B, T, V, 200 + V, kind, "float16", scale=4.0)
    _assert_bits(_np(dec.decode_device(y)), _np(dec.decode_device(y.float())), what + " fp16")


# (V=64: prune_rows_kernel's pre-filter; 1024: the workgroup kernel and the fused logits kernel; cutoff_top_n=100 > 64 at V=1001 and
#  V=10241 (R == 0): prune_rows_kernel's threshold search, where a group straddling cutoff_top_n sets the first tie)
@pytest.mark.parametrize("V,kind,top_n", [(64, "prob", 40), (1024, "prob", 40), (1024, "logits", 40), (1001, "prob", 100), (10241, "prob", 40)])
def test_tie_rule_flags_only_ties_inside_the_cut(torch_mod, V, kind, top_n):
    """One label far ahead and a tail whose bf16 values tie: with cutoff_prob = 0.5 the cut keeps one label (log(1 + 0.9) = 0.64 >= 0.5),
    so the tail's ties cannot change the result.  The half route settles these frames in the fast pass; the float32 rule flags them."""
    B, T = 2, 50
    tail = torch_mod.randn((B, T, V), generator=torch_mod.Generator().manual_seed(V))
    x = torch_mod.softmax(tail, -1) * 0.1 if kind == "prob" else tail
    for t in range(T):
        x[:, t, (t * 7) % V] = 0.9 if kind == "prob" else 12.0
    x = x.to(torch_mod.bfloat16).cuda()
    dec = _decoder(V, kind, beam_width=8, cutoff_top_n=top_n, cutoff_prob=0.5)
    got = _np(dec.decode_device(x))
    got_rows = dec.last_prune_rows(B * T, top_n)
    half_flagged = _flagged(dec)
    want = _np(dec.decode_device(x.float()))
    want_rows = dec.last_prune_rows(B * T, top_n)
    float_flagged = _flagged(dec)
    _assert_bits(got, want, "tie rule V%d %s" % (V, kind))
    _assert_prune_rows(got_rows, want_rows, "tie rule V%d %s" % (V, kind))
    assert (got_rows[0] == 1).all()
    assert half_flagged == 0 and float_flagged > 0, (half_flagged, float_flagged)


def test_pruned_bf16_allocates_no_float_copy(torch_mod):
    B, T, V = 4, 200, 10000
    x = _rows(torch_mod, B, T, V, 5, "logp", "bfloat16")
    dec = _decoder(V, "logp", beam_width=16, cutoff_top_n=40)
    dec.decode_device(x)  # (warm: the decoder's own workspace is allocated by the library, not by torch)
    torch_mod.cuda.synchronize()
    base = torch_mod.cuda.memory_allocated()
    torch_mod.cuda.reset_peak_memory_stats()
    out = dec.decode_device(x)
    torch_mod.cuda.synchronize()
    assert torch_mod.cuda.max_memory_allocated() - base < B * T * V * 4
    assert _in_dtype(dec) == 2
    del out


@pytest.mark.parametrize("V", [64, 1024])  # (1024: the workgroup kernels and their 8-byte loads)
@pytest.mark.parametrize("pruned", [False, True])
def test_special_values(torch_mod, pruned, V):
    B, T = 3, 80
    lp = torch_mod.log_softmax(torch_mod.randn((B, T, V), generator=torch_mod.Generator().manual_seed(3)) * 2, -1)
    lp[0, 5] = -float("inf")                 # a frame without a finite value
    lp[0, 6, 3] = float("inf")
    lp[1, 7, 10] = -float("inf")
    lp[1, ::3, 50:] = float("nan")           # NaN entries: below every number
    lp[2, 9, :] = float("nan")
    seq_lens = torch_mod.tensor([80, 41, 7], dtype=torch_mod.int32)
    kw = dict(beam_width=16, cutoff_top_n=8) if pruned else dict(beam_width=16, cutoff_top_n=V)
    dec = _decoder(V, "logp", **kw)
    for dtype in HALVES:
        x = lp.to(getattr(torch_mod, dtype)).cuda()
        _assert_bits(_np(dec.decode_device(x, seq_lens)), _np(dec.decode_device(x.float(), seq_lens)), "special %s" % dtype)
    # fp16 values that overflowed to inf (raw logits beyond 65504), through the logits route
    lg = torch_mod.randn((B, T, V), generator=torch_mod.Generator().manual_seed(4)) * 2
    lg[:, 3, 5] = 1e5
    lg[:, 4, 6] = -1e5
    x = lg.to(torch_mod.float16).cuda()
    assert torch_mod.isinf(x).any()
    dec = _decoder(V, "logits", **kw)
    _assert_bits(_np(dec.decode_device(x, seq_lens)), _np(dec.decode_device(x.float(), seq_lens)), "fp16 overflow")


def test_lm_tier(torch_mod):
    import ctcdecode_amd
    import ctcdecode_amd._native as n
    from test_lm import LABELS29, TEST_ARPA

    x = _rows(torch_mod, 2, 40, 29, 21, "logp", "bfloat16")
    dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, model_path=TEST_ARPA, alpha=0.6, beta=0.8, beam_width=16, log_probs_input=True, device="cuda:0")
    _assert_bits(_np(dec.decode_device(x)), _np(dec.decode_device(x.float())), "LM tier")
    probs = _rows(torch_mod, 2, 40, 29, 22, "prob", "bfloat16")
    dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, model_path=TEST_ARPA, alpha=0.6, beta=0.8, beam_width=16, device="cuda:0")
    _assert_bits(_np(dec.decode_device(probs)), _np(dec.decode_device(probs.float())), "LM tier, probabilities")
    # the same tables behind the scorer hook (ctcd_scorer_cond_log10 has the callback's signature)
    arr = (ctypes.c_char_p * 29)(*[s.encode("utf-8") for s in LABELS29])
    inner = ctypes.c_void_p()
    n.check(n.lib.ctcd_scorer_create(ctypes.byref(inner), 0.0, 0.0, TEST_ARPA.encode(), arr, 29, 0))
    try:
        words = [line.split("\t")[1] for line in open(TEST_ARPA, encoding="utf-8").read().split("\\1-grams:")[1].split("\\2-grams:")[0].splitlines()
                 if "\t" in line]
        fn = ctypes.cast(n.lib.ctcd_scorer_cond_log10, ctypes.c_void_p).value
        sc = ctcdecode_amd.CallbackScorer.from_c(fn, inner.value, words, int(n.lib.ctcd_scorer_max_order(inner)), LABELS29, alpha=0.6, beta=0.8)
        dec = ctcdecode_amd.CTCBeamDecoder(LABELS29, scorer=sc, beam_width=16, log_probs_input=True, device="cuda:0")
        _assert_bits(_np(dec.decode_device(x)), _np(dec.decode_device(x.float())), "scorer hook")
        del dec, sc
    finally:
        n.lib.ctcd_scorer_destroy(inner)


def test_streaming_chunks_across_the_epoch_wrap(torch_mod):
    """bf16 chunks of 50 frames with a boundary at frame 1023 (where the rank table's epoch wraps), pruned, against the same chunks in
    float32."""
    import ctcdecode_amd

    B, T, V = 2, 1100, 29
    x = _rows(torch_mod, B, T, V, 31, "logp", "bfloat16")
    bounds = list(range(0, 1001, 50)) + [1023, 1050, 1100]
    res = []
    for conv in (lambda c: c, lambda c: c.float()):
        dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], cutoff_top_n=10, beam_width=16, log_probs_input=True, device="cuda:0")
        states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
        for a, b in zip(bounds[:-1], bounds[1:]):
            out = dec.decode(conv(x[:, a:b]), states, [b == T] * B)
        res.append([t.numpy() for t in out])
    _assert_bits(res[0], res[1], "streaming")


def test_other_entry_points(torch_mod):
    x = _rows(torch_mod, 3, 120, 29, 41, "logp", "bfloat16")
    dec = _decoder(29, "logp", beam_width=32)
    _assert_bits([t.numpy() for t in dec.decode(x)], [t.numpy() for t in dec.decode(x.float())], "decode()")
    # a CPU half tensor is cast on the host, as the reference does
    _assert_bits([t.numpy() for t in dec.decode(x.cpu())], [t.numpy() for t in dec.decode(x.float().cpu())], "decode() CPU bf16")
    c1 = dec.decode_compact(x)
    e1 = dec.expand_compact(c1[0], c1[1], c1[2], 120)
    c2 = dec.decode_compact(x.float())
    e2 = dec.expand_compact(c2[0], c2[1], c2[2], 120)
    _assert_bits(_np(c1) + _np(e1), _np(c2) + _np(e2), "decode_compact")
    lg = _rows(torch_mod, 2, 30, 1000, 42, "logits", "float16")
    ldec = _decoder(1000, "logits")
    a = ldec.log_softmax(lg)
    assert a.dtype == torch_mod.float32 and _in_dtype(ldec) == 1
    b = ldec.log_softmax(lg.float())
    assert _in_dtype(ldec) == 0
    assert np.array_equal(a.cpu().numpy().view(np.int32), b.cpu().numpy().view(np.int32))
    # in place is float32 only: half logits overlapping the output are refused
    import ctcdecode_amd._native as n

    buf = torch_mod.zeros((2, 30, 1000), dtype=torch_mod.float32, device="cuda:0")
    half = buf.view(torch_mod.float16)[..., :1000]
    n.check(n.lib.ctcd_set_input_dtype(ldec._handle, 1))
    ldec._in_dtype = 1
    assert n.lib.ctcd_log_softmax(ldec._handle, half.data_ptr(), None, 2, 30, 1000, buf.data_ptr(), None) == -1
