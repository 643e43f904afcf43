"""-m gpu tests of long rows (``CTCBeamDecoder.set_long_rows`` / ``ctcd_set_long_rows``): ``align`` and ``log_likelihood`` of rows
beyond a band, bit for bit against the restatements of the header's definitions (tests/align_util.py, tests/loglik_util.py) at band
256, identical across band widths, and beyond the 2047 labels of the register kernels at the default band."""
import align_util as au
import lattice_matrix_util as mu
import loglik_util as lu
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
KEYS = ("start", "end", "scores", "loglik")


@pytest.fixture(scope="module", autouse=True)
def _torch():
    global torch
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"


def _dec(V, band, blank=0, **kw):
    import ctcdecode_amd

    kw.setdefault("log_probs_input", True)
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, beam_width=8, **kw)
    dec.set_long_rows(band)
    return dec


def _run(dec, x, c):
    """``align`` and ``log_likelihood`` of the case's labels over the rows ``x`` (a device tensor) -> dict of numpy arrays."""
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    tok, lens = torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()
    st, en, sc = dec.align(x, seq, tok, lens)
    bands = [dec.last_long_rows()]
    ll = dec.log_likelihood(x, seq, tok, lens)
    return dict(start=st.cpu().numpy(), end=en.cpu().numpy(), scores=sc.cpu().numpy(), loglik=ll.cpu().numpy(), bands=bands + [dec.last_long_rows()])


def _raw(dec, c):
    """The same through the raw ABI on float32 log-probabilities, outputs pre-filled: invalid rows leave their status word and zeros."""
    from ctcdecode_amd import _native

    (B, T, V), (R, Ls) = c["lp"].shape, c["tokens"].shape[1:]
    x, tok, lens = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("lp", "tokens", "lens"))
    st, en = (torch.full((B, R, Ls), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for _ in range(2))
    sc, ll = (torch.full((B, R), -123.0, dtype=torch.float32, device="cuda") for _ in range(2))
    s1, s2 = (torch.zeros((B,), dtype=torch.int32, device="cuda") for _ in range(2))
    _native.check(_native.lib.ctcd_set_input_dtype(dec._handle, 0))
    head = (dec._handle, x.data_ptr(), None, B, T, V, c["blank"], 1, tok.data_ptr(), lens.data_ptr(), R, Ls)
    _native.check(_native.lib.ctcd_ctc_align(*head, st.data_ptr(), en.data_ptr(), sc.data_ptr(), s1.data_ptr(), None))
    _native.check(_native.lib.ctcd_ctc_loglik(*head, ll.data_ptr(), s2.data_ptr(), None))
    torch.cuda.synchronize()
    assert s1.tolist() == s2.tolist()
    return dict(start=st.cpu().numpy(), end=en.cpu().numpy(), scores=sc.cpu().numpy(), loglik=ll.cpu().numpy(), status=s1.cpu().numpy())


def _edge_case(L, T, seq=None, V=6):
    """Three rows around the band edge at state 256: y[127] == y[128] (state 257 has no third predecessor: its look-back crosses the
    edge), distinct labels there, and a random row with repeats."""
    rng = np.random.default_rng(au.hash_name("long_rows_%d_%d" % (L, T)))
    rep = au.cycle(L, V)
    if L > 128:
        rep[128] = rep[127]
    tok, lens = au.pack_rows([[rep, au.cycle(L, V, first=1), au.random_rows(rng, 1, 1, L, V)[0][0]]], R=3, Ls=max(L, T))
    return dict(lp=au.log_softmax_rows(rng, 1, T, V, scale=1.0), seq_lens=seq, tokens=tok, lens=lens, blank=0)


def _check_band_256(dec, x, lp, c, what):
    got = _run(dec, x, c)
    assert got["bands"] == [256, 256], what
    au.assert_same(got, au.reference(lp, c["seq_lens"], c["tokens"], c["lens"], c["blank"]), what)
    lu.assert_same(got["loglik"], lu.reference(lp, c["seq_lens"], c["tokens"], c["lens"], c["blank"]), what)


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("L", [128, 129, 255, 256, 257, 384])
def test_band_edges_at_band_256(L, tight):
    """S = 257: S - 1 alone in band 1, S - 2 in band 0; 259: two states there; 511 / 513 / 515: a third band of none, one and three states;
    769: a fourth band of one state.  T = L + 7: few alignments; T = min(2L, 300): many (or, below L, none)."""
    c = _edge_case(L, L + 7 if tight else min(2 * L, 300))
    _check_band_256(_dec(c["lp"].shape[2], 256), torch.from_numpy(c["lp"]).cuda(), c["lp"], c, "L %d T %d" % (L, c["lp"].shape[1]))


@pytest.mark.parametrize("mode", ["prob", "logits", "bfloat16", "float16", "seq_lens"])
def test_input_modes_at_band_256(mode):
    """Probabilities and raw logits in float32; half log-probabilities (the reference on the widened values); an item shorter than T."""
    c = _edge_case(129, 136, np.asarray([133], np.int32) if mode == "seq_lens" else None)
    V, x = c["lp"].shape[2], torch.from_numpy(c["lp"]).cuda()
    if mode == "prob":
        dec, x = _dec(V, 256, log_probs_input=False), torch.exp(x)
        lp = au.prob_to_lp(x.cpu().numpy())
    elif mode == "logits":
        dec, x = _dec(V, 256, log_probs_input=False, logits_input=True), x * 3.0 + 1.0
        lp = dec.log_softmax(x, None).cpu().numpy()
    else:
        dec = _dec(V, 256)
        x = x.to(getattr(torch, mode)) if mode != "seq_lens" else x
        lp = x.float().cpu().numpy()
    _check_band_256(dec, x, lp, c, mode)


def _every_class_case():
    """Rows of every class in one launch: a group of one-wave rows; S = 201 / 901 / 3001 and L > n; an invalid row (a label = V at
    position 1400), S = 1401, another L > n and S = 261."""
    rng = np.random.default_rng(au.hash_name("long_rows_classes"))
    T, V, cy = 1510, 5, au.cycle
    bad = cy(1505, V)
    bad[1400] = V
    rows = [au.random_rows(rng, 1, 4, 25, V)[0], [cy(100, V), cy(450, V, first=1), cy(1500, V), cy(1600, V)], [bad, cy(700, V, first=2), cy(1511, V), cy(130, V)]]
    tok, lens = au.pack_rows(rows, R=4, Ls=1600)
    return dict(lp=au.log_softmax_rows(rng, 3, T, V, scale=1.0), seq_lens=None, tokens=tok, lens=lens, blank=0)


@pytest.mark.parametrize("budget", [0, 1])
@pytest.mark.parametrize("name", ["third_wave", "every_class"])
def test_band_width_never_changes_a_result(name, budget):
    """Mode off and bands 256 / 1024 / 4096 agree bit for bit; budget 1: one workgroup reuses its slot and edge columns for every row."""
    c = mu.case("third_wave") if name == "third_wave" else _every_class_case()
    off = None
    for band in (0, 256, 1024, 4096):
        dec = _dec(c["lp"].shape[2], band)
        dec.set_align_scratch(budget)
        got = _raw(dec, c)
        assert dec.last_long_rows() == (band if 0 < band < 2 * min(c["lp"].shape[1], c["tokens"].shape[2]) + 1 else 0)  # (the shape alone)
        off = off or got
        assert all(np.array_equal(got[k].view(np.uint32), off[k].view(np.uint32)) for k in KEYS + ("status",)), "%s band %d" % (name, band)
    assert np.isfinite(off["loglik"]).any() and off["status"].any() == (name == "every_class")


@pytest.mark.parametrize("L", [2048, 2049])
def test_single_alignment_beyond_the_old_limit(L):
    """L = n = T = L_stride: S = 4097 (a second band of one state) and 4099.  The only alignment is in state 2t + 1 at frame t, and
    lse3(x, -inf, -inf) = x exactly: both scores are the left-to-right float32 sum of the path's lp."""
    c = mu.single_path_case(L)
    dec, x = _dec(c["lp"].shape[2], 0), torch.from_numpy(c["lp"]).cuda()
    with pytest.raises(NotImplementedError, match="2047"):
        _run(dec, x, c)
    dec.set_long_rows()
    got = _run(dec, x, c)
    assert got["bands"] == [4096, 4096]
    want = np.asarray([[lu.path_sum(c, 0, r, L) for r in range(2)]], np.float32)
    assert np.array_equal(got["loglik"].view(np.uint32), want.view(np.uint32)) and np.array_equal(got["scores"].view(np.uint32), want.view(np.uint32))
    assert (got["start"] == np.arange(L)).all() and (got["end"] == np.arange(L)).all()


def _viterbi32(lp, y, blank):
    """The header's recurrence in float32, a frame at a time: exact maxima, one addition, ties to the largest state index."""
    n, L = lp.shape[0], len(y)
    z, skip, ninf = np.full(2 * L + 1, blank), np.zeros(2 * L + 1, bool), np.float32(-np.inf)
    z[1::2] = y
    skip[3::2] = z[3::2] != z[1:-2:2]
    d = np.full(z.size, ninf, np.float32)
    d[:2] = lp[0, z[:2]]
    bp = np.zeros((n, z.size), np.int8)
    for t in range(1, n):
        p1, p2 = np.concatenate(([ninf], d[:-1])), np.where(skip, np.concatenate(([ninf, ninf], d[:-2])), ninf)
        best = np.maximum(np.maximum(d, p1), p2)
        bp[t] = np.where(d == best, 0, np.where(p1 == best, 1, 2))
        d = (lp[t, z] + best).astype(np.float32)
    s = z.size - 2 if d[-2] > d[-1] else z.size - 1
    score, st, en = d[s], np.zeros(L, np.int32), np.full(L, -1, np.int32)
    for t in range(n - 1, -1, -1):
        if s & 1:
            st[s >> 1] = t
            if en[s >> 1] < 0:
                en[s >> 1] = t
        s -= int(bp[t, s]) if t else 0
    return score, st, en


def test_many_alignments_beyond_the_old_limit():
    """L = 2050 in 2060 frames at band 4096: align against the vectorised float32 Viterbi, log_likelihood against the float64 forward
    pass within n x 2^-23 x (A + 3) (tests/test_loglik_host.py); a second row with a label = V at position 2049 is zeroed and raised."""
    rng = np.random.default_rng(au.hash_name("long_rows_2050"))
    T, V, L = 2060, 5, 2050
    bad = au.cycle(L, V)
    bad[2049] = V
    tok, lens = au.pack_rows([[au.cycle(L, V), bad]], R=2, Ls=T)
    c = dict(lp=au.log_softmax_rows(rng, 1, T, V, scale=1.0), seq_lens=None, tokens=tok, lens=lens, blank=0)
    got = _raw(_dec(V, 4096), c)
    score, st, en = _viterbi32(c["lp"][0], tok[0, 0, :L], 0)
    assert np.isfinite(score) and got["scores"][0, 0].view(np.uint32) == score.view(np.uint32)
    assert np.array_equal(got["start"][0, 0, :L], st) and np.array_equal(got["end"][0, 0, :L], en) and not got["start"][0, 0, L:].any()
    ll64, A = lu.forward64(c["lp"][0], T, tok[0, 0, :L], 0)
    print("ll32 %r ll64 %r bound %r" % (float(got["loglik"][0, 0]), ll64, T * 2.0 ** -23 * (A + 3.0)))
    assert abs(float(got["loglik"][0, 0]) - ll64) <= T * 2.0 ** -23 * (A + 3.0)
    assert got["status"].tolist() == [au.BAD_ROW] and not any(got[k][0, 1].any() for k in KEYS)


def test_edges_of_the_contract():
    c = mu.single_path_case(2048)
    dec, x = _dec(c["lp"].shape[2], 4096), torch.from_numpy(c["lp"]).cuda()
    with pytest.raises(ValueError):
        dec.set_long_rows(300)
    tok, lens = torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()
    with pytest.raises(NotImplementedError, match="2047"):
        dec.label_posteriors(x, None, tok, lens)
    big = torch.zeros((1, 1 << 20, x.shape[2]), device="cuda")  # one step beyond 2^20 - 1
    for fn in (dec.align, dec.log_likelihood):
        with pytest.raises(NotImplementedError, match="2\\^20"):
            fn(big, None, torch.zeros((1, 1, 1 << 20), dtype=torch.int32), torch.zeros((1, 1), dtype=torch.int32))
    assert _run(dec, x, c)["bands"] == [4096, 4096], "the decoder afterwards"
    dec.set_long_rows(0)
    with pytest.raises(NotImplementedError, match="2047"):
        dec.align(x, None, tok, lens)
