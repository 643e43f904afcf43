"""Keywords of 65 .. 2048 labels (include/ctcdecode_amd.h "Keyword search", ``set_long_keywords``): ``find_keywords`` on the long keyword
kernel against a vectorised numpy float32 restatement of the definition, bit for bit.  The restatement itself is held against
tests/keyword_util.py's scalar one without a GPU."""
import numpy as np
import pytest
import torch

import greedy_util as gu
import keyword_util as ku

gpu = pytest.mark.gpu
KEYS = ("scores", "starts", "ends", "end_scores", "end_starts")
NEG_INF = ku.NEG_INF
STEP4 = {True: 16, False: 4}  # the frames of a step of the four-wave class, staged / gathered (keyword_long.h kwl_step)


# ---- the definition, on arrays over the 2L - 1 states --------------------------------------------------------------------------------
def find_item(x, n, blank, mode, kw):
    """ku.find_item, a frame at a time: every operation is a float32 add, subtract or compare of the same operands."""
    T, kw = x.shape[0], np.asarray(kw)
    S = 2 * len(kw) - 1
    z = np.full(S, blank)
    z[0::2] = kw
    skip = np.zeros(S, bool)
    skip[2::2] = kw[1:] != kw[:-1]
    tv, ts, best = np.zeros(T, np.float32), np.zeros(T, np.int32), (NEG_INF, -1, -1)
    with np.errstate(all="ignore"):
        lp = (lambda a: a if mode == 1 else np.log(a.astype(np.float64) + gu.FLT_MIN).astype(np.float32))
        rows, m = lp(x[:n][:, z]), lp(x[:n].max(1))
        r = np.where(rows == NEG_INF, NEG_INF, rows - m[:, None]).astype(np.float32)
        v, st = np.full(S, NEG_INF, np.float32), np.full(S, -1, np.int32)
        for t in range(n):
            bv, bs = v.copy(), st.copy()  # stay
            for back, allowed in ((1, True), (2, skip)):  # s - 1, then s - 2 where the entry rule allows it
                pv, ps = np.concatenate([np.full(back, NEG_INF, np.float32), v[:-back]]), np.concatenate([np.full(back, -1, np.int32), st[:-back]])
                take = allowed & (pv > bv)
                bv, bs = np.where(take, pv, bv), np.where(take, ps, bs)
            if np.float32(0.0) > bv[0]:  # the entry
                bv[0], bs[0] = 0.0, t
            v, st = r[t] + bv, bs
            if v[-1] >= best[0]:
                best = (v[-1], st[-1], t)
            tv[t], ts[t] = v[-1], st[-1]
    return (best if best[0] > NEG_INF else (best[0], -1, -1)) + (tv, ts)


def reference(c):
    x, (B, T, _), Q = c["x"], c["x"].shape, len(c["kws"])
    out = dict(scores=np.zeros((B, Q), np.float32), starts=np.zeros((B, Q), np.int32), ends=np.zeros((B, Q), np.int32),
               end_scores=np.zeros((B, Q, T), np.float32), end_starts=np.zeros((B, Q, T), np.int32))
    for b in range(B):
        n = T if c["seq_lens"] is None else min(max(int(c["seq_lens"][b]), 0), T)
        for q, kw in enumerate(c["kws"]):
            out["scores"][b, q], out["starts"][b, q], out["ends"][b, q], out["end_scores"][b, q], out["end_starts"][b, q] = find_item(x[b], n, c["blank"], c["mode"], kw)
    return out


def _repeat_rows(raw):
    raw[0, 4] = -np.inf  # a frame of all -inf
    raw[:, :, 7] = -np.inf  # a column of -inf


@pytest.mark.parametrize("c", [ku.case("vec L%d m%d" % (L, mode), mode=mode, T=90, L=(L,)) for L in (3, 70) for mode in (0, 1)]
                         + [ku.case("vec repeat", T=30, kws=[[5, 5, 7, 3, 3], [7, 2], [9, 9]], edit=_repeat_rows)], ids=lambda c: c["name"])
def test_vectorised_restatement_equals_the_scalar_one(c):
    ku.assert_same(reference(c), ku.reference(c), c["name"])


# ---- the device ----------------------------------------------------------------------------------------------------------------------
def _decoder(V, blank, mode=1, on=True):
    import ctcdecode_amd

    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, log_probs_input=mode == 1, device="cuda:0")
    if on:
        dec.set_long_keywords()
    return dec


def _find(dec, c, Lk, kws=None, details=True):
    k, lens = ku.kw_tensors(kws or c["kws"], Lk)
    sl = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    outs = dec.find_keywords(gu.to_torch(torch, c["stored"], c["dtype"]), sl, torch.from_numpy(k).cuda(), torch.from_numpy(lens), details=details)
    return dict(zip(KEYS, (o.cpu().numpy() for o in outs)))


def _check(c, Lk, dec=None):
    """The call on a case equals the restatement, and ran the long kernel of Lk's class."""
    dec = dec or _decoder(c["x"].shape[2], c["blank"], c["mode"])
    got = _find(dec, c, Lk)
    ku.assert_same(got, reference(c), c["name"])
    waves = 1 if Lk <= 512 else 2 if Lk <= 1024 else 4
    assert dec.last_keyword_kernel() == c["kernel"][:3] + (128 + waves,)
    return got


@gpu
@pytest.mark.parametrize("Lk", (65, 72, 73, 512, 513, 1024, 1025, 2048))
def test_lengths_on_both_sides_of_every_edge(Lk):
    """len = Lk and Lk - 1; the second item is shorter than either keyword: -inf, -1, -1, traces of -inf below n and 0 beyond."""
    c = ku.case("long L%d" % Lk, T=Lk + 40, L=(Lk, Lk - 1), seq_lens=[Lk + 40, Lk - 5])
    got = _check(c, Lk)
    assert np.isfinite(got["scores"][0]).all() and (got["scores"][1] == NEG_INF).all() and (got["starts"][1] == -1).all() and (got["ends"][1] == -1).all()
    assert (got["end_scores"][1, :, :Lk - 5] == NEG_INF).all() and (got["end_scores"][1, :, Lk - 5:].view(np.uint32) == 0).all()


@gpu
@pytest.mark.parametrize("dtype,mode,V,Lk", [(dt, mode, V, 70) for dt in gu.DTYPES for mode in (0, 1) for V in (29, 130)] + [(0, 1, 130, 520), (2, 0, 130, 520)])
def test_every_instantiation(dtype, mode, V, Lk):
    _check(ku.case("long inst %d %d %d %d" % (dtype, mode, V, Lk), dtype=dtype, mode=mode, V=V, T=Lk + 40, L=(Lk, Lk - 7)), Lk)


@gpu
@pytest.mark.parametrize("V", (29, 130))
@pytest.mark.parametrize("steps,extra", [(1, -1), (1, 0), (1, 1), (4, 1)])
def test_pipeline_fill_and_drain(V, steps, extra):
    """Four waves with the last label in wave 0 or 1 while later waves idle, T around the class's step, ragged lengths.  (A third
    keyword of 5 labels is the one short enough to score on these T.)"""
    T = steps * STEP4[V <= 128] + extra
    got = _check(ku.case("drain V%d T%d" % (V, T), V=V, T=T, B=3, L=(66, 700, 5), seq_lens=[0, 1, T]), 1025)
    assert np.isfinite(got["scores"][2, 2]) == (T >= 5)


@gpu
@pytest.mark.parametrize("mode", (0, 1))
def test_planted_phrase_in_closed_form(mode):
    """One-hot rows spell a 600-label keyword from frame 17 on, a blank frame between its repeated labels at positions (7, 8) -- a lane
    edge -- and (511, 512) -- a wave edge: score 0.0f at the planted frames.  Item 1 lacks the blank frame between 511 and 512: on
    log-probabilities the keyword cannot be spelt (-inf); on probabilities a zero is log(FLT_MIN), so its score is finite and below 0."""
    kw = [1 + (i % 6) for i in range(600)]
    kw[8], kw[512] = kw[7], kw[511]
    spelt = [0] * 17 + kw[:8] + [0] + kw[8:512] + [0] + kw[512:] + [0] * 5
    broken = [0] * 17 + kw[:8] + [0] + kw[8:] + [0] * 6
    x = np.full((2, len(spelt), 8), 0.0 if mode == 0 else -np.inf, np.float32)
    for b, path in enumerate((spelt, broken)):
        x[b, np.arange(len(path)), path] = 1.0 if mode == 0 else 0.0
    c = dict(name="planted", stored=x, x=x, dtype=0, seq_lens=None, blank=0, mode=mode, kws=[kw], kernel=(0, mode == 0, True))
    got = _check(c, 600, _decoder(8, 0, mode))
    assert got["scores"].view(np.uint32)[0, 0] == 0 and (got["starts"][0, 0], got["ends"][0, 0]) == (17, 17 + 601)
    assert got["scores"][1, 0] == NEG_INF if mode == 1 else NEG_INF < got["scores"][1, 0] < 0


@gpu
@pytest.mark.parametrize("Q,Lk", [(5, 100), (3, 600)])
def test_keywords_per_workgroup(Q, Lk):
    """More keywords than a workgroup holds (4 of one wave, 2 of two): every keyword's result is its result alone."""
    c = ku.case("long Q%d L%d" % (Q, Lk), T=Lk + 30, L=tuple(Lk - 3 * q for q in range(Q)))
    dec = _decoder(29, c["blank"])
    got = _check(c, Lk, dec)
    for q in range(Q):
        ku.assert_same(_find(dec, c, Lk, kws=[c["kws"][q]]), {k: got[k][:, q:q + 1] for k in KEYS}, "keyword %d alone" % q)


@gpu
def test_the_switch():
    c = ku.case("long switch", T=40, L=(33, 20))
    off, on, probs = _decoder(29, c["blank"], on=False), _decoder(29, c["blank"]), torch.from_numpy(c["stored"]).cuda()
    ones = lambda Lk: (torch.ones((1, Lk), dtype=torch.int32), torch.tensor([1], dtype=torch.int32))  # noqa: E731
    for dec, Lk in ((off, 65), (on, 2049)):
        with pytest.raises(NotImplementedError):
            dec.find_keywords(probs, None, *ones(Lk))
    with pytest.raises(ValueError):
        on.set_long_keywords(2)
    ku.assert_same(_find(on, c, 33), _find(off, c, 33), "Lk = 33")
    assert on.last_keyword_kernel() == off.last_keyword_kernel() == c["kernel"]
    bad = torch.ones((1, 800), dtype=torch.int32)
    bad[0, 700] = c["blank"]  # (28) the blank label at position 700 of 800
    with pytest.raises(ValueError):
        on.find_keywords(probs, None, bad, torch.tensor([800], dtype=torch.int32))
    after = ku.case("long after the errors", T=110, L=(70,))
    assert after["blank"] == c["blank"]
    _check(after, 70, on)


@gpu
def test_neg_inf_rows():
    """Frames of all -inf and a label ruled out everywhere (7): a keyword that avoids it, and one that has it at position 40."""
    kw = [1 + i % 6 for i in range(130)]
    got = _check(ku.case("long neg inf", T=170, kws=[kw, kw[:40] + [7] + kw[41:66]], edit=ku._neg_inf_rows), 130)
    assert np.isfinite(got["scores"][:, 0]).all() and (got["scores"][:, 1] == NEG_INF).all()
