"""-m gpu tests of the launch order (ctcd_set_launch_order / CTCBeamDecoder.set_launch_order): the order pass on the device ranks the
clamped seq_lens as numpy's stable argsort does, and a decode whose workgroups take their utterances longest first returns what batch
order returns -- every tensor bit for bit, scores compared as uint32 -- on every route the one-shot entry points take."""
import ctypes

import numpy as np
import pytest

import fake_kenlm
import oracle_util as ou
from test_lm import LABELS29, TEST_ARPA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _decoder(V, **kw):
    import ctcdecode_amd

    kw.setdefault("log_probs_input", True)
    return ctcdecode_amd.CTCBeamDecoder(kw.pop("labels", [str(i) for i in range(V)]), device="cuda:0", **kw)


def _want_order(lens, T):
    return np.argsort(-np.clip(np.asarray(lens, np.int64), 0, T), kind="stable").astype(np.int32)


def _ragged(B, T, seed, lo=None):
    rng = np.random.default_rng(seed)
    return rng.integers(T // 4 if lo is None else lo, T + 1, size=B).astype(np.int32)


def _np(ts):
    return [np.asarray(t.cpu().numpy() if hasattr(t, "cpu") else t) for t in ts]


def _assert_bits(a, b, what):
    assert len(a) == len(b), what
    for i, (u, v) in enumerate(zip(_np(a), _np(b))):
        assert u.dtype == v.dtype and u.shape == v.shape, "%s: output %d: %s %s vs %s %s" % (what, i, u.dtype, u.shape, v.dtype, v.shape)
        if u.dtype == np.float32:
            u, v = u.view(np.uint32), v.view(np.uint32)
        assert np.array_equal(u, v), "%s: output %d differs between length and batch order" % (what, i)


def _both_orders(dec, run, lens, T, what):
    """`run()` under length order, then under batch order, on the same decoder: equal bit for bit, and the order non-trivial."""
    dec.set_launch_order("length")
    got = run()
    order = dec.last_launch_order()
    assert order is not None and order.dtype == np.int32, what
    B = len(lens) if lens is not None else len(order)
    assert np.array_equal(np.sort(order), np.arange(B)), what + ": not a permutation"
    assert not np.array_equal(order, np.arange(B)), what + ": the order is the identity (nothing was reordered)"
    dec.set_launch_order("batch")
    want = run()
    assert dec.last_launch_order() is None, what
    _assert_bits(got, want, what)
    return got, order


# ---------------------------------------------------------------------------------------------------------------- the order pass

# (16384: the largest batch the single-workgroup sort takes; 20000: the multi-workgroup ranking beyond it)
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 1000, 4096, 16384, 20000])
def test_order_pass_equals_numpy_stable_argsort(torch_mod, B):
    torch = torch_mod
    T, V = 12, 5
    rng = np.random.default_rng(B)
    # heavy ties (a handful of distinct values), lengths 0, past T and negative
    lens = rng.choice(np.array([-7, -1, 0, 0, 3, 5, 5, 12, 12, 13, 40], np.int32), size=B)
    probs = torch.from_numpy(ou.synth_logprobs(1, T, V, 7)).expand(B, T, V).contiguous().cuda()
    dec = _decoder(V, beam_width=2)
    dec.set_launch_order("length")
    dec.decode_device(probs, torch.from_numpy(lens))
    assert np.array_equal(dec.last_launch_order(), _want_order(lens, T)), B
    # equal lengths and no seq_lens: the identity
    dec.decode_device(probs, torch.full((B,), 9, dtype=torch.int32))
    assert np.array_equal(dec.last_launch_order(), np.arange(B, dtype=np.int32))
    dec.decode_device(probs)
    assert np.array_equal(dec.last_launch_order(), np.arange(B, dtype=np.int32))


def test_order_pass_random_lengths(torch_mod):
    torch = torch_mod
    T, V, B = 300, 4, 3000
    lens = np.random.default_rng(5).integers(-20, T + 20, size=B).astype(np.int32)
    probs = torch.from_numpy(ou.synth_logprobs(B, 2, V, 8)).repeat(1, T // 2, 1).contiguous().cuda()
    dec = _decoder(V, beam_width=1)
    dec.set_launch_order("length")
    dec.decode_device(probs, torch.from_numpy(lens))
    assert np.array_equal(dec.last_launch_order(), _want_order(lens, T))


# ---------------------------------------------------------------------------------------------------------------- bit identity

def test_north_star_layout_more_workgroups_than_slots(torch_mod):
    """B = 600 > the 512 workgroups the two-per-CU build keeps resident: the tail of the launch queues."""
    torch = torch_mod
    B, T, V = 600, 60, 29
    lens = _ragged(B, T, 11)
    probs = torch.from_numpy(ou.synth_logprobs(B, T, V, 11)).cuda()
    sl = torch.from_numpy(lens).cuda()
    dec = _decoder(V, beam_width=16)
    _, order = _both_orders(dec, lambda: dec.decode_device(probs, sl), lens, T, "north-star layout")
    assert dec.last_layout() == 1
    assert np.array_equal(order, _want_order(lens, T))
    dec.set_cu_sharing(0)  # (the default build at one workgroup per CU: 256 resident)
    _both_orders(dec, lambda: dec.decode_device(probs, sl), lens, T, "north-star layout, one workgroup per CU")


def test_cu_sharing_on(torch_mod):
    torch = torch_mod
    B, T, V = 40, 50, 29
    lens = _ragged(B, T, 12, lo=0)
    probs = torch.from_numpy(ou.synth_logprobs(B, T, V, 12)).cuda()
    dec = _decoder(V, beam_width=24)
    dec.set_cu_sharing(1)
    _both_orders(dec, lambda: dec.decode_device(probs, torch.from_numpy(lens)), lens, T, "cu_sharing")


def test_pruned_mid_layout_and_runtime_layout(torch_mod):
    torch = torch_mod
    B, T, V = 48, 50, 1000
    lens = _ragged(B, T, 13)
    probs = torch.from_numpy(ou.synth_logprobs(B, T, V, 13)).cuda()
    dec = _decoder(V, beam_width=40, cutoff_top_n=40)  # (beam 40: 1024 threads, which the compile-time layout needs)
    _both_orders(dec, lambda: dec.decode_device(probs, torch.from_numpy(lens)), lens, T, "pruned mid layout")
    assert dec.last_layout() == 2
    dec.set_fixed_layout(False)
    _both_orders(dec, lambda: dec.decode_device(probs, torch.from_numpy(lens)), lens, T, "pruned, run-time layout")
    assert dec.last_layout() == 0
    dec2 = _decoder(29, beam_width=16)
    dec2.set_fixed_layout(False)
    p29 = torch.from_numpy(ou.synth_logprobs(B, T, 29, 14)).cuda()
    _both_orders(dec2, lambda: dec2.decode_device(p29, torch.from_numpy(lens)), lens, T, "run-time layout")
    assert dec2.last_layout() == 0


def test_wide_beam_layout(torch_mod):
    torch = torch_mod
    B, T, V = 6, 40, 29
    lens = np.array([10, 40, 3, 25, 40, 0], np.int32)
    probs = torch.from_numpy(ou.synth_logprobs(B, T, V, 15)).cuda()
    dec = _decoder(V, beam_width=300)
    _both_orders(dec, lambda: dec.decode_device(probs, torch.from_numpy(lens)), lens, T, "wide-beam layout")
    assert dec.last_layout() == 3


def test_host_tensors_and_compact(torch_mod):
    """decode() from CPU tensors (the rows large enough to be streamed in while the kernel runs) and decode_compact after expansion."""
    torch = torch_mod
    B, T, V = 72, 160, 29
    lens = _ragged(B, T, 16)
    lp = torch.from_numpy(ou.synth_logprobs(B, T, V, 16))
    sl = torch.from_numpy(lens)
    dec = _decoder(V, beam_width=16)
    _both_orders(dec, lambda: dec.decode(lp, sl), lens, T, "decode() from host tensors")
    dev = lp.cuda()

    def compact():
        hdr, ent, labels, scores, out_len = dec.decode_compact(dev, sl)
        tok, ts = dec.expand_compact(hdr, ent, labels, T)
        return tok, ts, scores, out_len

    _both_orders(dec, compact, lens, T, "decode_compact, expanded")


def test_bf16_input_and_logits(torch_mod):
    torch = torch_mod
    B, T, V = 40, 60, 29
    lens = _ragged(B, T, 17)
    g = torch.Generator().manual_seed(17)
    x = torch.randn((B, T, V), generator=g) * 2.0
    sl = torch.from_numpy(lens).cuda()
    half = torch.log_softmax(x, -1).to(torch.bfloat16).cuda()
    dec = _decoder(V, beam_width=16)
    _both_orders(dec, lambda: dec.decode_device(half, sl), lens, T, "bf16 input")
    dec_l = _decoder(V, beam_width=16, log_probs_input=False, logits_input=True)
    logits = x.cuda()
    _both_orders(dec_l, lambda: dec_l.decode_device(logits, sl), lens, T, "logits_input")


def test_builtin_lm_tier(torch_mod):
    torch = torch_mod
    B, T, V = 24, 80, 29
    lens = _ragged(B, T, 18)
    probs = torch.from_numpy(ou.synth_logprobs(B, T, V, 18, blank_bias=1.0)).cuda()
    dec = _decoder(V, labels=LABELS29, beam_width=16, model_path=TEST_ARPA, alpha=0.5, beta=1.0)
    _both_orders(dec, lambda: dec.decode_device(probs, torch.from_numpy(lens)), lens, T, "LM tier (test.arpa)")
    _both_orders(dec, lambda: dec.decode(probs.cpu(), torch.from_numpy(lens)), lens, T, "LM tier, host tensors")


class _Builtin(object):
    """test.arpa's built-in tables behind the batched callback interface (a cold cache for a new CallbackScorer)."""

    def __init__(self, labels, lm_path):
        from ctcdecode_amd import _native as n

        self.n = n
        arr = (ctypes.c_char_p * len(labels))(*[x.encode("utf-8") for x in labels])
        self.handle = ctypes.c_void_p()
        n.check(n.lib.ctcd_scorer_create(ctypes.byref(self.handle), 0.0, 0.0, lm_path.encode(), arr, len(labels), 0))
        self.order = int(n.lib.ctcd_scorer_max_order(self.handle))
        self.vocabulary = fake_kenlm.arpa_words(lm_path)
        self.cond_log10 = fake_kenlm.library_backend(n.lib, self.handle)

    def batch(self, windows):
        return [self.cond_log10(w) for w in windows]

    def close(self):
        self.n.lib.ctcd_scorer_destroy(self.handle)


def test_callback_scorer_cold_cache(torch_mod):
    import ctcdecode_amd

    torch = torch_mod
    B, T, V = 16, 70, 29
    lens = _ragged(B, T, 19)
    probs = torch.from_numpy(ou.synth_logprobs(B, T, V, 19, blank_bias=1.0)).cuda()
    sl = torch.from_numpy(lens)
    inner = _Builtin(LABELS29, TEST_ARPA)
    try:
        sc = ctcdecode_amd.CallbackScorer.batched(inner.batch, inner.vocabulary, inner.order, LABELS29, alpha=0.5, beta=1.0, device="cuda:0")
        dec = _decoder(V, labels=LABELS29, beam_width=16, scorer=sc)
        got, order = _both_orders(dec, lambda: dec.decode_device(probs, sl), lens, T, "callback scorer, cold cache")
        assert np.array_equal(order, _want_order(lens, T))
        ref = _decoder(V, labels=LABELS29, beam_width=16, model_path=TEST_ARPA, alpha=0.5, beta=1.0)
        _assert_bits(got, ref.decode_device(probs, sl), "callback scorer vs built-in tables")
        del dec, sc
    finally:
        inner.close()


def test_callback_scorer_resumed_launches(torch_mod):
    """Without the waiting launch every miss ends the utterance's launch: the decode takes launch after launch, and the resumed ones
    take the second permutation (by the frames each utterance has left).  Cold caches for both orders: a new scorer per order."""
    import ctcdecode_amd

    torch = torch_mod
    B, T, V = 12, 60, 29
    lens = _ragged(B, T, 23)
    probs = torch.from_numpy(ou.synth_logprobs(B, T, V, 23, blank_bias=1.0)).cuda()
    sl = torch.from_numpy(lens)
    inner = _Builtin(LABELS29, TEST_ARPA)
    outs, rounds = {}, {}
    try:
        for mode in ("length", "batch"):
            sc = ctcdecode_amd.CallbackScorer.batched(inner.batch, inner.vocabulary, inner.order, LABELS29, alpha=0.5, beta=1.0, device="cuda:0")
            dec = _decoder(V, labels=LABELS29, beam_width=16, scorer=sc)
            dec.set_scorer_wait(False)
            dec.set_launch_order(mode)
            outs[mode] = dec.decode_device(probs, sl)
            rounds[mode] = dec.last_scorer_launches()[0]
            order = dec.last_launch_order()
            if mode == "length":
                assert np.array_equal(order, _want_order(lens, T))
            else:
                assert order is None
            del dec, sc
    finally:
        inner.close()
    assert rounds["length"] > 1 and rounds["batch"] > 1, rounds  # (launches counted: more than one, so resumed launches ran)
    _assert_bits(outs["length"], outs["batch"], "callback scorer, resumed launches")


# ---------------------------------------------------------------------------------------------------------------- oracle, default

def test_length_order_against_oracle(torch_mod):
    torch = torch_mod
    B, T, V, K = 32, 90, 29, 12
    lens = _ragged(B, T, 20)
    lens[5], lens[17] = T, 1  # (the longest and the shortest of the batch)
    lp = ou.synth_logprobs(B, T, V, 20)
    dec = _decoder(V, beam_width=K)
    dec.set_launch_order("length")
    out, scores, ts, out_len = dec.decode(torch.from_numpy(lp), torch.from_numpy(lens))
    order = dec.last_launch_order()
    assert order[0] == 5 and order[-1] == 17
    which = "reference" if ou.have_reference() else "restated"
    want = ou.decode(lp, seq_lens=lens, beam=K, which=which)
    got = dict(tokens=out.numpy(), timesteps=ts.numpy(), scores=scores.numpy(), lens=out_len.numpy(), nres=want["nres"])
    ou.assert_same(got, want, "length order vs the %s oracle" % which)


def test_default_is_batch_order(torch_mod):
    torch = torch_mod
    B, T, V = 8, 40, 29
    lens = _ragged(B, T, 21)
    lp = ou.synth_logprobs(B, T, V, 21)
    dec = _decoder(V, beam_width=8)
    assert dec.last_launch_order() is None
    out, scores, ts, out_len = dec.decode(torch.from_numpy(lp), torch.from_numpy(lens))
    assert dec.last_launch_order() is None
    want = ou.decode(lp, seq_lens=lens, beam=8, which="restated")
    ou.assert_same(dict(tokens=out.numpy(), timesteps=ts.numpy(), scores=scores.numpy(), lens=out_len.numpy(), nres=want["nres"]), want, "default")
    with pytest.raises(ValueError):
        dec.set_launch_order("fastest")
    with pytest.raises(ValueError):
        dec.set_launch_order(1)
