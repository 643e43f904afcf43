"""-m gpu tests of long posteriors (``CTCBeamDecoder.set_long_posteriors`` / ``ctcd_set_long_posteriors``): ``label_posteriors`` of rows
beyond a band, bit for bit against the restatement of the header's definition (tests/posterior_util.py) at band 256 and block 16,
identical across bands, blocks and the mode itself, and beyond the 2047 labels of the register kernels."""
import align_util as au
import lattice_matrix_util as mu
import numpy as np
import posterior_util as pu
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _torch():
    global torch
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"


def _dec(V, band, block=0, blank=0, **kw):
    import ctcdecode_amd

    kw.setdefault("log_probs_input", True)
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, beam_width=8, **kw)
    dec.set_long_posteriors(band, block)
    return dec


def _run(dec, x, c):
    """``label_posteriors`` of the case's labels over the rows ``x`` (a device tensor) -> dict of numpy arrays."""
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    outs = dec.label_posteriors(x, seq, torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda())
    return dict(zip(pu.KEYS, (o.cpu().numpy() for o in outs)))


def _raw(dec, c):
    """The same through the raw ABI on float32 log-probabilities, outputs pre-filled: invalid rows leave their status word and zeros."""
    from ctcdecode_amd import _native

    (B, T, V), (R, Ls) = c["lp"].shape, c["tokens"].shape[1:]
    x, tok, lens = (torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ("lp", "tokens", "lens"))
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"]).cuda()
    pk = torch.full((B, R, Ls), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    oc, cf = (torch.full((B, R, Ls), -123.0, dtype=torch.float32, device="cuda") for _ in range(2))
    ll, status = torch.full((B, R), -123.0, dtype=torch.float32, device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda")
    _native.check(_native.lib.ctcd_set_input_dtype(dec._handle, 0))
    _native.check(_native.lib.ctcd_ctc_posteriors(dec._handle, x.data_ptr(), seq.data_ptr() if seq is not None else None, B, T, V, c["blank"], 1, tok.data_ptr(),
                                                  lens.data_ptr(), R, Ls, pk.data_ptr(), oc.data_ptr(), cf.data_ptr(), ll.data_ptr(), status.data_ptr(), None))
    torch.cuda.synchronize()
    return dict(peaks=pk.cpu().numpy(), occupancy=oc.cpu().numpy(), confidence=cf.cpu().numpy(), loglik=ll.cpu().numpy(), status=status.cpu().numpy())


def _same(got, want, what, keys=pu.KEYS):
    for k in keys:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)


def _edge_case(L, T, V=6):
    """Four rows around the band edges at band 256: y[127] == y[128] (forward state 257 has no third predecessor: its look-back crosses
    state 256), y[L-129] == y[L-128] (the same for the reversed walk, whose state 256 is the row's state S - 1 - 256), distinct labels at
    both places, and a random row with repeats."""
    rng = np.random.default_rng(au.hash_name("long_posteriors_%d_%d" % (L, T)))
    fwd, rev = au.cycle(L, V), au.cycle(L, V)
    if L > 128:
        fwd[128] = fwd[127]
        rev[L - 129] = rev[L - 128]
    tok, lens = au.pack_rows([[fwd, rev, au.cycle(L, V, first=1), au.random_rows(rng, 1, 1, L, V)[0][0]]], R=4, Ls=max(L, T))
    return dict(lp=au.log_softmax_rows(rng, 1, T, V, scale=1.0), seq_lens=None, tokens=tok, lens=lens, blank=0)


def _check_restatement(dec, x, lp, c, mode, what):
    got = _run(dec, x, c)
    assert dec.last_long_posteriors() == mode, what
    pu.assert_same(got, pu.reference(lp, c["seq_lens"], c["tokens"], c["lens"], c["blank"]), what)
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    ll = dec.log_likelihood(x, seq, torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()).cpu().numpy()
    assert np.array_equal(got["loglik"].view(np.uint32), ll.view(np.uint32)), what
    return got


@pytest.mark.parametrize("tight", [True, False])
@pytest.mark.parametrize("L", [128, 129, 255, 256, 257, 384])
def test_band_edges_at_band_256_block_16(L, tight):
    """S = 257: a second band of one state; 259: of three; 511 / 513 / 515: a third band of none, one and three states; 769: a fourth of one.
    T = L + 7: few alignments; T = min(2L, 300): many (or, below L, none).  Blocks of 16 frames: every row crosses many block edges."""
    c = _edge_case(L, L + 7 if tight else min(2 * L, 300))
    _check_restatement(_dec(c["lp"].shape[2], 256, 16), torch.from_numpy(c["lp"]).cuda(), c["lp"], c, (256, 16), "L %d T %d" % (L, c["lp"].shape[1]))


@pytest.mark.parametrize("n, block", [(143, 16), (144, 16), (145, 16), (144, 8), (144, 512)])
def test_block_edges(n, block):
    """L = 130: a last block of 15, 16 and 1 frames; blocks of 8; one block longer than the row."""
    c = _edge_case(130, n)
    got = _check_restatement(_dec(c["lp"].shape[2], 256, block), torch.from_numpy(c["lp"]).cuda(), c["lp"], c, (256, block), "n %d block %d" % (n, block))
    assert np.isfinite(got["loglik"][0, :3]).all() and (got["occupancy"][0, 2, :130] > 0).all()


def test_ragged_items_and_a_bad_label():
    """One launch at block 16: n = 145, n = 0, n = 100 < L and, at n = 144, a row with a label = V -- zeroed, its item's status raised."""
    rng = np.random.default_rng(au.hash_name("long_posteriors_ragged"))
    V, bad = 6, au.cycle(130, 6)
    bad[129] = V
    tok, lens = au.pack_rows([[au.cycle(130, V)], [au.cycle(130, V)], [au.cycle(130, V, first=1)], [bad]], R=1, Ls=145)
    c = dict(lp=au.log_softmax_rows(rng, 4, 145, V, scale=1.0), seq_lens=np.asarray([145, 0, 100, 144], np.int32), tokens=tok, lens=lens, blank=0)
    got = _raw(_dec(V, 256, 16), c)
    pu.assert_same(got, pu.reference(c["lp"], c["seq_lens"], tok, lens, 0), "ragged")
    assert got["status"].tolist() == [0, 0, 0, au.BAD_ROW] and np.isfinite(got["loglik"][0, 0]) and not any(got[k][1:].any() for k in pu.KEYS[:3])


def _every_class_case():
    """S = 201, 261, 901, 1401, 3001 and 4095 in one launch of 2050 frames (L_stride 2047: the mode-off launch takes it)."""
    rng = np.random.default_rng(au.hash_name("long_posteriors_classes"))
    tok, lens = au.pack_rows([[au.cycle(L, 5, first=i) for i, L in enumerate((100, 130, 450, 700, 1500, 2047))]], R=6, Ls=2047)
    return dict(lp=au.log_softmax_rows(rng, 1, 2050, 5, scale=1.0), seq_lens=None, tokens=tok, lens=lens, blank=0)


@pytest.mark.parametrize("budget", [0, 1])
def test_neither_knob_changes_a_bit(budget):
    """Mode off, bands 256 / 1024 / 4096 and blocks 8 / 64 / automatic agree bit for bit; budget 1: one workgroup reuses its slot for
    every row.  The register kernels of the mode-off launch are pinned to the restatement by tests/test_gpu_posterior.py."""
    c = _every_class_case()
    off = None
    for band, block in [(0, 0)] + [(w, f) for w in (256, 1024, 4096) for f in (8, 64, 0)]:
        dec = _dec(5, band, block)
        dec.set_posterior_scratch(budget)
        got = _raw(dec, c)
        w, f = dec.last_long_posteriors()
        assert w == (band if 0 < band < 4095 else 0) and (f == 0 if w == 0 else (f == block if block else 32 <= f <= 1024)), (band, block)  # (the shape alone)
        assert dec.last_posterior_grid() == (1 if budget else 6)
        off = off or got
        _same(got, off, "band %d block %d" % (band, block), pu.KEYS + ("status",))
    assert np.isfinite(off["loglik"]).all() and (off["occupancy"][0, 5] > 0).all() and not off["status"].any()


@pytest.mark.parametrize("L", [2048, 2049])
def test_single_alignment_beyond_the_old_limit(L):
    """L = n = T = L_stride: S = 4097 and 4099.  The only alignment is in state 2t + 1 at frame t: the closed form of
    lattice_matrix_util.single_path_expected, at one band of 4096 states and a second of one or three, and at seventeen bands of 256."""
    c = mu.single_path_case(L)
    x, want = torch.from_numpy(c["lp"]).cuda(), mu.single_path_expected(c)["posteriors"]
    for band in (4096, 256):
        dec = _dec(c["lp"].shape[2], band)
        pu.assert_same(_run(dec, x, c), want, "L %d band %d" % (L, band))
        assert dec.last_long_posteriors()[0] == band


def _beyond_case():
    """L = 2050 in 2060 frames: many alignments, beyond every register class."""
    rng = np.random.default_rng(au.hash_name("long_posteriors_2050"))
    tok, lens = au.pack_rows([[au.cycle(2050, 5)]], R=1, Ls=2060)
    return dict(lp=au.log_softmax_rows(rng, 1, 2060, 5, scale=1.0), seq_lens=None, tokens=tok, lens=lens, blank=0)


def _three_bands(x, c, what, **kw):
    first = None
    for band in (256, 1024, 4096):
        dec = _dec(x.shape[2], band, **kw)
        got = _run(dec, x, c)
        assert dec.last_long_posteriors()[0] == band, what
        first = first or got
        _same(got, first, "%s band %d" % (what, band))
    assert np.isfinite(first["loglik"]).all() and (first["occupancy"][0, 0, :2050] > 0).all(), what
    return first


def test_many_alignments_beyond_the_old_limit():
    c = _beyond_case()
    x = torch.from_numpy(c["lp"]).cuda()
    got = _three_bands(x, c, "L 2050")
    dec = _dec(5, 0)
    dec.set_long_rows(4096)
    ll = dec.log_likelihood(x, None, torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()).cpu().numpy()
    assert np.array_equal(got["loglik"].view(np.uint32), ll.view(np.uint32))


@pytest.mark.parametrize("prob", [False, True])
@pytest.mark.parametrize("dtype", mu.DTYPES)
def test_every_instantiation(dtype, prob):
    """Each element type and mode: the L = 2050 row at the three bands (1, 4 and 16 states per lane) is identical, and at band 256 the
    rows of L = 129 in 136 frames equal the restatement on the rows' float32 copies."""
    kw = dict(log_probs_input=not prob)
    for c, small in ((_beyond_case(), False), (_edge_case(129, 136), True)):
        x = torch.from_numpy(c["lp"]).cuda()
        x = (torch.exp(x) if prob else x).to(getattr(torch, dtype))
        if not small:
            _three_bands(x, c, "%s prob %d" % (dtype, prob), **kw)
            continue
        lp = au.prob_to_lp(x.float().cpu().numpy()) if prob else x.float().cpu().numpy()
        _check_restatement(_dec(x.shape[2], 256, 16, **kw), x, lp, c, (256, 16), "%s prob %d" % (dtype, prob))


def test_logits_input():
    c = _edge_case(129, 136)
    dec = _dec(c["lp"].shape[2], 256, 16, log_probs_input=False, logits_input=True)
    x = torch.from_numpy(c["lp"]).cuda() * 3.0 + 1.0
    _check_restatement(dec, x, dec.log_softmax(x, None).cpu().numpy(), c, (256, 16), "logits")


def test_edges_of_the_contract():
    c = mu.single_path_case(2048)
    x, tok, lens = torch.from_numpy(c["lp"]).cuda(), torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()
    dec = _dec(c["lp"].shape[2], 0)
    for _ in range(2):  # mode off; set_long_rows alone
        with pytest.raises(NotImplementedError, match="2047"):
            dec.label_posteriors(x, None, tok, lens)
        dec.set_long_rows(4096)
    for bad in ((300, 0), (256, 12), (256, 4104), (256, -8)):
        with pytest.raises(ValueError):
            dec.set_long_posteriors(*bad)
    dec.set_long_posteriors()
    with pytest.raises(NotImplementedError, match="2\\^20"):  # one step beyond 2^20 - 1
        dec.label_posteriors(torch.zeros((1, 1 << 20, x.shape[2]), device="cuda"), None, torch.zeros((1, 1, 1 << 20), dtype=torch.int32),
                             torch.zeros((1, 1), dtype=torch.int32))
    pu.assert_same(_run(dec, x, c), mu.single_path_expected(c)["posteriors"], "the decoder afterwards")
    assert dec.last_long_posteriors()[0] == 4096
    dec.set_long_posteriors(0)
    with pytest.raises(NotImplementedError, match="2047"):
        dec.label_posteriors(x, None, tok, lens)
