"""Keyword search on the device (include/ctcdecode_amd.h "Keyword search"): ``find_keywords`` against the numpy restatement of
tests/keyword_util.py, bit for bit, on the case table the host twin runs on the CPU."""
import numpy as np
import pytest
import torch

import greedy_util as gu
import keyword_util as ku

pytestmark = pytest.mark.gpu
KEYS = ("scores", "starts", "ends", "end_scores", "end_starts")


def _decoder(V, blank, mode=1, **kw):
    import ctcdecode_amd

    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, log_probs_input=mode == 1, device="cuda:0", **kw)


def _find(dec, c, kws=None, details=True, probs=None):
    k, lens = ku.kw_tensors(kws or c["kws"])
    sl = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    probs = gu.to_torch(torch, c["stored"], c["dtype"]) if probs is None else probs
    outs = dec.find_keywords(probs, sl, torch.from_numpy(k).cuda(), torch.from_numpy(lens), details=details)
    assert all(o.is_cuda for o in outs)
    return dict(zip(KEYS, (o.cpu().numpy() for o in outs)))


@pytest.mark.parametrize("c", ku.CASES, ids=lambda c: c["name"])
def test_equals_restatement(c):
    dec = _decoder(c["x"].shape[2], c["blank"], c["mode"])
    assert dec.last_keyword_kernel() is None
    ku.assert_same(_find(dec, c), ku.reference_of(c), c["name"])
    assert dec.last_keyword_kernel() == c["kernel"]


def test_keyword_count_changes_nothing():
    """Q on both sides of the keywords per wave (8) and per workgroup (32) of an 8-lane group: every keyword's result stays what it is."""
    rng = np.random.default_rng(5)
    c = ku.case("Q edge", T=40, kws=[ku._keyword(rng, 1 + q % 8, 29, 0) for q in range(33)])
    dec, want = _decoder(29, c["blank"]), ku.reference_of(c)
    for Q in (1, 8, 9, 32, 33):
        got = _find(dec, c, kws=c["kws"][:Q], details=False)
        assert len(got) == 3
        ku.assert_same(got, {k: want[k][:, :Q] for k in KEYS[:3]}, "Q = %d" % Q)


def test_logits_equal_log_softmax_rows():
    c = ku.case("logits", T=37)
    logits = torch.from_numpy(gu.random_rows(np.random.default_rng(3), 2, 37, 29, 2)).cuda()
    dec = _decoder(29, c["blank"], 0, logits_input=True)
    got = _find(dec, c, probs=logits)
    want = _find(_decoder(29, c["blank"]), c, probs=dec.log_softmax(logits))
    ku.assert_same(got, want, "logits")


@pytest.mark.parametrize("mode", (0, 1))
def test_greedy_transcript_scores_zero_and_greedy_is_unchanged(mode):
    """One-hot rows: every run of up to 4 labels of the greedy transcript scores 0.0f at greedy's frames; the greedy decode behind a
    keyword call, which shares its frame records, returns what it returned before."""
    path = [1, 1, 0, 2, 3, 3, 0, 0, 4, 5, 5, 6, 0, 7, 7] * 5  # 75 frames: the labels recur, the latest run wins
    x = np.full((1, len(path), 8), 0.0 if mode == 0 else -np.inf, np.float32)
    x[0, np.arange(len(path)), path] = 1.0 if mode == 0 else 0.0
    dec, probs = _decoder(8, 0, mode), torch.from_numpy(x).cuda()
    before = [o.cpu() for o in dec.greedy_decode_device(probs, details=True)]
    tok, st, en, n = before[0][0, 0].tolist(), before[2][0, 0].tolist(), before[4][0, 0].tolist(), int(before[3][0, 0])
    runs = [(i, j) for i in range(n - 7, n) for j in range(i, min(i + 4, n))]  # (runs that do not recur behind themselves)
    got = _find(dec, dict(stored=x, dtype=0, seq_lens=None), kws=[tok[i:j + 1] for i, j in runs])
    assert (got["scores"].view(np.uint32) == 0).all()
    assert got["starts"][0].tolist() == [st[i] for i, _ in runs] and got["ends"][0].tolist() == [en[j] for _, j in runs]
    assert all(torch.equal(a, b.cpu()) for a, b in zip(before, dec.greedy_decode_device(probs, details=True)))


def test_invalid_keywords_raise_and_the_decoder_stays_usable():
    c = ku.case("usable", V=9, T=6)  # blank 0
    dec, probs = _decoder(9, 0), torch.from_numpy(c["stored"]).cuda()
    for kws, lens in (([[3, 0]], [2]), ([[3, 9]], [2]), ([[3, 4]], [0]), ([[3, 4], [5, 6]], [2, 3])):
        with pytest.raises(ValueError):
            dec.find_keywords(probs, None, torch.tensor(kws, dtype=torch.int32), torch.tensor(lens, dtype=torch.int32))
    with pytest.raises(NotImplementedError):
        dec.find_keywords(probs, None, torch.ones((1, 65), dtype=torch.int32), torch.tensor([1], dtype=torch.int32))
    outs = dec.find_keywords(probs, None, *map(torch.from_numpy, ku.kw_tensors(c["kws"])), details=True)
    assert not any(o.is_cuda for o in outs)
    ku.assert_same(dict(zip(KEYS, (o.numpy() for o in outs))), ku.reference_of(c), "after the errors")
