"""-m gpu tests of the pruned default's compile-time layout (kernel <0,0,2,true,1024>: beam <= 112, cutoff_top_n <= 40, <= 10240
labels, 1024 threads) across frame 1023 mod 1024, where its rank table's tags wrap (ctcdecode_amd/csrc/beam_core.h kRankEpoch; the
inputs: rank_epoch_util.py).  Every decode asserts through the layout hook that this kernel ran, and compares bit for bit with the
oracle and, where named, with the run-time layout's kernel."""
import numpy as np
import pytest

import oracle_util as ou
import rank_epoch_util as reu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _decoder(V, beam, top_n, cutoff_prob=1.0, threads=None, fixed_layout=True, **kw):
    import ctcdecode_amd

    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=beam, cutoff_top_n=top_n, cutoff_prob=cutoff_prob,
                                       device="cuda:0", **kw)
    if threads:
        dec.set_threads(threads)
    if not fixed_layout:
        dec.set_fixed_layout(False)
    return dec


def _result(outs, nres):
    out, sc, ts, ln = [t.cpu().numpy() for t in outs]
    return dict(tokens=out, scores=sc, timesteps=ts, lens=ln, nres=nres)


def _assert_bits(a, b, what):
    for key in ("tokens", "timesteps", "lens"):
        assert np.array_equal(a[key], b[key]), "%s: %s" % (what, key)
    assert np.array_equal(a["scores"].view(np.uint32), b["scores"].view(np.uint32)), what + ": scores"


def _decode_both_layouts(torch, lp, beam, top_n, cutoff_prob=1.0, threads=None, sl=None):
    """The compile-time layout (asserted) and the run-time layout's kernel on the same rows: identical tensors."""
    x = torch.from_numpy(np.ascontiguousarray(lp))
    s = torch.from_numpy(sl) if sl is not None else None
    dec = _decoder(lp.shape[2], beam, top_n, cutoff_prob, threads, log_probs_input=True)
    got = [t.numpy() for t in dec.decode(x, s)]
    assert dec.last_layout() == 2
    rt = _decoder(lp.shape[2], beam, top_n, cutoff_prob, threads, fixed_layout=False, log_probs_input=True)
    ref = [t.numpy() for t in rt.decode(x, s)]
    assert rt.last_layout() == 0
    a = dict(tokens=got[0], scores=got[1], timesteps=got[2], lens=got[3])
    _assert_bits(a, dict(tokens=ref[0], scores=ref[1], timesteps=ref[2], lens=ref[3]), "compile-time vs run-time layout")
    return a


def test_default_decoder_on_a_large_vocabulary_runs_the_layout(torch_mod):
    """Guard: the reference's default decoder (beam 100, cutoff_top_n 40) on a BPE-sized vocabulary is this layout's, so the tests
    of this file cannot drift to another kernel unnoticed."""
    import ctcdecode_amd

    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(10000)], beam_width=100, cutoff_top_n=40, log_probs_input=True, device="cuda:0")
    assert dec.last_layout() == -1
    lp = ou.synth_logprobs(1, 20, 10000, 5)
    dec.decode(torch_mod.from_numpy(lp))
    assert dec.last_layout() == 2


@pytest.mark.parametrize("kind", reu.KINDS)
def test_offline_across_three_wraps(torch_mod, kind):
    """The host build's cases at T = 3100 (frames 1023, 2047 and 3071): the blank pruned in every frame, pruned around the wraps
    only, and labels that are candidates in one frame and prefix-final labels 1024 frames later.  K * (top_n + 2) = 660 slots: the
    automatic choice runs 512 threads and the run-time layout, so the decoder asks for 1024."""
    lp = reu.epoch_case(kind, 3100)
    want = ou.decode(lp, beam=reu.K, cutoff_top_n=reu.TOP_N)
    got = _decode_both_layouts(torch_mod, lp, reu.K, reu.TOP_N, threads=1024)
    ou.assert_same(dict(got, nres=want["nres"]), want, kind)


def test_configs3_decoder_across_two_wraps(torch_mod):
    """BASELINE configs[3]'s decoder (V = 10000, beam 100, cutoff_top_n 40, cutoff_prob 0.99; automatic thread choice) on two
    utterances of 2100 frames: the blank pushed out of the candidates around the wraps (item 0) and in every frame (item 1)."""
    V, T = 10000, 2100
    lp = ou.synth_logprobs(2, T, V, 3003)
    reu.strong_wrap_frames(lp, 40, 7)
    reu.prune_blank(lp[:1], 40, reu.wrap_frames(T))
    reu.prune_blank(lp[1:], 40)
    kw = dict(beam=100, cutoff_top_n=40, cutoff_prob=0.99)
    want = ou.decode(lp, **kw)
    got = _decode_both_layouts(torch_mod, lp, 100, 40, cutoff_prob=0.99)
    ou.assert_same(dict(got, nres=want["nres"]), want, "configs[3] decoder, T=2100")


def _stream(torch, dec, lp, bounds, nres):
    import ctcdecode_amd

    B, T, _ = lp.shape
    x = torch.from_numpy(lp)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    edges = [0] + list(bounds) + [T]
    for a, b in zip(edges[:-1], edges[1:]):
        outs = dec.decode(x[:, a:b], states, [b == T] * B)
        assert dec.last_layout() == 2, (a, b)
    out, sc, ts, ln = [t.numpy() for t in outs]
    K = ln.shape[1]
    res = dict(tokens=np.zeros((B, K, T), np.int32), timesteps=np.zeros((B, K, T), np.int32), scores=sc, lens=ln, nres=nres)
    res["tokens"][:, : out.shape[1], : out.shape[2]] = out
    res["timesteps"][:, : out.shape[1], : out.shape[2]] = ts
    return res


def test_streamed_across_the_wraps(torch_mod):
    """Streams with the automatic thread choice (beam 100, cutoff_top_n 40: 4200 slots, 1024 threads): every chunk starts with a
    wiped rank table, so a chunk starting at frame 1023 or 2047 looks up every label outside its first frame's candidates in a wiped
    table.  Chunk bounds at the wraps and one-frame chunks across them: the one-shot result and the oracle."""
    import ctcdecode_amd

    T, K, top_n = 2100, 100, 40
    lp = np.concatenate([reu.epoch_case("blank_pruned_at_wraps", T, top_n=top_n), reu.epoch_case("stale_tag", T, top_n=top_n)])
    want = ou.decode(lp, beam=K, cutoff_top_n=top_n)
    one = _decoder(reu.V, K, top_n, log_probs_input=True)
    oneshot = _result(one.decode(torch_mod.from_numpy(lp)), want["nres"])
    assert one.last_layout() == 2
    ou.assert_same(oneshot, want, "one launch")
    for bounds in ([1023, 2047], [1024, 2048], list(range(1021, 1027)) + list(range(2045, 2051))):
        dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(reu.V)], beam_width=K, cutoff_top_n=top_n, log_probs_input=True,
                                                 device="cuda:0")
        got = _stream(torch_mod, dec, lp, bounds, want["nres"])
        ou.assert_same(got, want, "chunks %s" % bounds)
        _assert_bits(got, oneshot, "chunks %s vs one launch" % bounds)


def test_fused_logits_input_across_the_wraps(torch_mod):
    """Raw logits (V % 4 == 0, V > 256: the fused log_softmax + prune pass feeds the kernel its candidates) across frames 1023 and 2047,
    the blank out of the candidates around the wraps; against the oracle on the host twin of the log_softmax."""
    T, K, top_n = 2100, 100, 40
    logits = reu.epoch_case("blank_pruned_at_wraps", T, top_n=top_n)
    dec = _decoder(reu.V, K, top_n, logits_input=True)
    dec.set_fused_logits(True)
    got = _result(dec.decode(torch_mod.from_numpy(logits)), None)
    assert dec.last_layout() == 2
    want = ou.decode(ou.log_softmax_rows(logits), beam=K, cutoff_top_n=top_n)
    got["nres"] = want["nres"]
    ou.assert_same(got, want, "fused logits")


def test_bf16_rows_across_the_wraps(torch_mod):
    """bfloat16 log-probabilities decoded without a float32 copy across frames 1023 and 2047: the result of the same decoder on the
    widened rows, and the oracle's on them."""
    torch = torch_mod
    T, K, top_n = 2100, 100, 40
    lp = reu.epoch_case("blank_pruned_at_wraps", T, top_n=top_n)
    x = torch.from_numpy(lp).to(torch.bfloat16).cuda()
    dec = _decoder(reu.V, K, top_n, log_probs_input=True)
    got = _result(dec.decode_device(x), None)
    assert dec.last_layout() == 2
    wide = _result(dec.decode_device(x.float()), None)
    assert dec.last_layout() == 2
    _assert_bits(got, wide, "bf16 vs float32 rows")
    want = ou.decode(x.float().cpu().numpy(), beam=K, cutoff_top_n=top_n)
    got["nres"] = want["nres"]
    ou.assert_same(got, want, "bf16 rows")
