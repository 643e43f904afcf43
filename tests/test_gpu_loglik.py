"""-m gpu tests of the CTC log-likelihood (``CTCBeamDecoder.log_likelihood`` / ``ctcd_ctc_loglik``): device output == the Python
restatement of the header's definition (tests/loglik_util.py), bit for bit as uint32, at the shapes where the kernel can go wrong.  The
cases and their references are those of tests/test_loglik_host.py, computed once per process."""
import align_util as au
import loglik_util as lu
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _references_released_afterwards():
    """The cases and their references live for this module's tests only: the tests that run after it find the process as it was."""
    yield
    import gc

    lu.release()
    gc.collect()


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _dec(V, blank=0, **kw):
    import ctcdecode_amd

    kw.setdefault("log_probs_input", True)
    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, beam_width=kw.pop("beam_width", 8), **kw)


def _loglik(torch, dec, rows, c, device=True):
    """``rows``: the tensor the decoder is given.  -> float32 [B, R] (numpy) of dec.log_likelihood on the case's labels."""
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    tok, lens = torch.from_numpy(c["tokens"]), torch.from_numpy(c["lens"])
    if device:
        tok, lens = tok.cuda(), lens.cuda()
    ll = dec.log_likelihood(rows, seq, tok, lens)
    assert ll.is_cuda == device and ll.dtype == torch.float32 and tuple(ll.shape) == tuple(c["lens"].shape)
    return ll.cpu().numpy()


@pytest.mark.parametrize("name", lu.CASES)
def test_device_equals_the_restatement(torch_mod, name):
    """align_util's cases -- edges, one_frame, wave_edge (S = 63 / 65), workgroup_edge (S = 255 / 257 / 259), many_per_lane (S = 1023 /
    1025, T = 514: no multiple of the prefetch depth), ties_*, neg_inf, blank_* (blank_id != 0, L_stride < T), forty_rows, mixed_group (a
    group the workgroup runs row by row that also holds a row without a path, and a partial last group of that kind) -- and zeros
    (+0.0 / -0.0 values: the logf(1) + m rule), far_apart (differences around -88: an expf term vanishes or only just does not),
    positive (log_input == 1 rows with positive entries), overflow (finite values near -3e38 whose sums overflow to -inf)."""
    torch = torch_mod
    c, want = lu.case(name)
    dec = _dec(c["lp"].shape[2], c["blank"])
    lu.assert_same(_loglik(torch, dec, torch.from_numpy(c["lp"]).cuda(), c), want, name)


def test_cpu_tensors_in_cpu_tensors_out(torch_mod):
    torch = torch_mod
    c, want = lu.case("edges")
    dec = _dec(c["lp"].shape[2], c["blank"])
    lu.assert_same(_loglik(torch, dec, torch.from_numpy(c["lp"]), c, device=False), want, "CPU tensors")


def test_half_rows_equal_their_float_copies(torch_mod):
    torch = torch_mod
    c, _ = lu.case("blank_last")
    dec = _dec(c["lp"].shape[2], c["blank"])
    for dt in (torch.float16, torch.bfloat16):
        h = torch.from_numpy(c["lp"]).cuda().to(dt)
        want = lu.reference(h.float().cpu().numpy(), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
        assert np.isfinite(want["loglik"]).any()
        lu.assert_same(_loglik(torch, dec, h, c), want, str(dt))
        lu.assert_same(_loglik(torch, dec, h.float(), c), want, str(dt) + " as float32")


def test_the_three_input_modes(torch_mod):
    """Probabilities: float32(math.log(float64(p) + FLT_MIN)) per element; logits: the restatement on log_softmax()'s own output."""
    torch = torch_mod
    c, _ = lu.case("ties_half")
    V = c["lp"].shape[2]
    rng = np.random.default_rng(5)
    p = rng.random(c["lp"].shape).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    p[0, 3, 1] = 0.0
    p[1, 2, :] = 0.0
    dec = _dec(V, c["blank"], log_probs_input=False)
    want = lu.reference(au.prob_to_lp(p), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    lu.assert_same(_loglik(torch, dec, torch.from_numpy(p).cuda(), c), want, "probabilities")
    logits = (rng.standard_normal(c["lp"].shape) * 3).astype(np.float32)
    dec = _dec(V, c["blank"], log_probs_input=False, logits_input=True)
    seq = torch.from_numpy(c["seq_lens"])
    for x in (torch.from_numpy(logits).cuda(), torch.from_numpy(logits).cuda().to(torch.bfloat16)):
        lsm = dec.log_softmax(x, seq).cpu().numpy()
        want = lu.reference(lsm, c["seq_lens"], c["tokens"], c["lens"], c["blank"])
        assert np.isfinite(want["loglik"]).any()
        lu.assert_same(_loglik(torch, dec, x, c), want, "logits %s" % x.dtype)


def test_the_grid_cap_changes_nothing(torch_mod):
    """set_loglik_grid(3) and (1) on 40 rows: the launches take 3 and 1 workgroups, and the results are the default's."""
    torch = torch_mod
    c, want = lu.case("forty_rows")
    dec = _dec(c["lp"].shape[2], c["blank"])
    x = torch.from_numpy(c["lp"]).cuda()
    full = _loglik(torch, dec, x, c)
    assert dec.last_loglik_grid() == 40, "40 rows on a device that holds more workgroups than that"
    dec.set_loglik_grid(3)
    few = _loglik(torch, dec, x, c)
    assert dec.last_loglik_grid() == 3
    dec.set_loglik_grid(1)
    one = _loglik(torch, dec, x, c)
    assert dec.last_loglik_grid() == 1
    dec.set_loglik_grid(0)
    for got, what in ((full, "default cap"), (few, "three workgroups"), (one, "one workgroup")):
        lu.assert_same(got, want, what)
    assert np.array_equal(few.view(np.uint32), full.view(np.uint32)) and np.array_equal(one.view(np.uint32), full.view(np.uint32))


def _raw_loglik(torch, dec, c, tok, lens, log_input=1):
    """Once through the raw ABI: the output pre-filled, status zeroed by the caller.  -> dict(loglik, status)."""
    from ctcdecode_amd import _native

    B, T, V = c["lp"].shape
    R, Ls = tok.shape[1:]
    x = torch.from_numpy(c["lp"]).cuda()
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"]).cuda()
    dtok, dlens = torch.from_numpy(tok).cuda(), torch.from_numpy(lens).cuda()
    out = torch.full((B, R), -123.0, dtype=torch.float32, device="cuda")
    status = torch.zeros((B,), dtype=torch.int32, device="cuda")
    _native.check(_native.lib.ctcd_set_input_dtype(dec._handle, 0))
    rc = _native.lib.ctcd_ctc_loglik(dec._handle, x.data_ptr(), seq.data_ptr() if seq is not None else None, B, T, V, c["blank"], log_input, dtok.data_ptr(),
                                     dlens.data_ptr(), R, Ls, out.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _native.check(rc)
    torch.cuda.synchronize()
    return dict(loglik=out.cpu().numpy(), status=status.cpu().numpy())


def test_raw_abi_writes_every_row(torch_mod):
    torch = torch_mod
    for name in ("edges", "blank_mid", "wave_edge"):
        c, want = lu.case(name)
        dec = _dec(c["lp"].shape[2], c["blank"])
        got = _raw_loglik(torch, dec, c, c["tokens"], c["lens"])
        assert not (got["loglik"] == -123.0).any(), "a row of the output was not written"
        lu.assert_same(got, want, "raw ABI, " + name)


def test_raw_abi_refuses_bad_shapes(torch_mod):
    from ctcdecode_amd import _native

    torch = torch_mod
    c, _ = lu.case("edges")
    dec = _dec(c["lp"].shape[2])
    x = torch.from_numpy(c["lp"]).cuda()
    a, lens = (torch.zeros((64,), dtype=torch.int32, device="cuda") for _ in range(2))
    f = torch.full((64,), -123.0, dtype=torch.float32, device="cuda")

    def call(B=1, T=2, V=8, blank=0, mode=1, R=2, Ls=2, probs=x.data_ptr(), tok=a.data_ptr(), out=f.data_ptr()):
        return _native.lib.ctcd_ctc_loglik(dec._handle, probs, None, B, T, V, blank, mode, tok, lens.data_ptr(), R, Ls, out, None, None)

    for kw in (dict(B=-1), dict(T=-1), dict(V=0), dict(blank=8), dict(blank=-1), dict(mode=3), dict(R=-1), dict(Ls=-1), dict(probs=None), dict(tok=None),
               dict(out=None)):
        assert call(**kw) == -1, kw
    assert call(T=5000, Ls=5000, R=1) == -2, "rows beyond the states one workgroup holds are refused, not cut"
    assert call(T=2048, Ls=2048, R=1) == -2, "min(L_stride, T) = 2048: one label more than a workgroup holds"
    assert call(V=(1 << 28) + 1) == -2
    assert call(B=0) == 0 and call(R=0) == 0
    torch.cuda.synchronize()
    assert (f == -123.0).all(), "a refused call, or one without rows, launches nothing"
    assert call() == 0
    torch.cuda.synchronize()
    assert (f[:2] != -123.0).all() and (f[2:] == -123.0).all()
    # the limit itself is accepted: min(L_stride, T) = 2047 (tensors of that shape: the call launches, on one row without labels)
    x2 = torch.zeros((1, 2048, 8), dtype=torch.float32, device="cuda")
    t2 = torch.zeros((2047,), dtype=torch.int32, device="cuda")
    assert call(T=2048, Ls=2047, R=1, probs=x2.data_ptr(), tok=t2.data_ptr()) == 0
    torch.cuda.synchronize()


def _check_invalid_row(torch, dec, c, want, what, pos, val):
    b1, r1 = pos[:2]
    blank = c["blank"]
    tok, lens = c["tokens"].copy(), c["lens"].copy()
    (tok if len(pos) == 3 else lens)[pos] = val
    got = _raw_loglik(torch, dec, c, tok, lens)
    ref = lu.reference(c["lp"], c["seq_lens"], tok, lens, blank)
    assert ref["status"].tolist() == [lu.BAD_ROW if b == b1 else 0 for b in range(2)]
    lu.assert_same(got, ref, what)
    assert got["loglik"][b1, r1] == 0, what
    keep = np.ones(c["lens"].shape, bool)
    keep[b1, r1] = False
    assert np.array_equal(got["loglik"][keep].view(np.uint32), want["loglik"][keep].view(np.uint32)), what
    with pytest.raises(ValueError, match=r"items \[%d\].*CTCD_ALIGN_BAD_ROW" % b1):
        dec.log_likelihood(torch.from_numpy(c["lp"]), None, torch.from_numpy(tok), torch.from_numpy(lens))
    lu.assert_same(_loglik(torch, dec, torch.from_numpy(c["lp"]).cuda(), c), want, "the decoder afterwards")


def test_invalid_rows_raise_their_item_alone(torch_mod):
    """A label = V, a label = blank, a negative length and one beyond L_stride each raise CTCD_ALIGN_BAD_ROW for that item only; the other
    rows are unchanged and the decoder is usable afterwards.  mixed_group: the invalid row lies in a group whose rows the workgroup
    runs one by one."""
    torch = torch_mod
    c, want = lu.case("blank_mid")
    V, blank = c["lp"].shape[2], c["blank"]
    dec = _dec(V, blank)
    r0 = int(np.argmax(c["lens"][1] > 1))
    for what, pos, val in (("label = V", (1, r0, 1), V), ("label = blank", (1, r0, 0), blank), ("length < 0", (1, r0), -1), ("length > L_stride", (1, r0), 13)):
        _check_invalid_row(torch, dec, c, want, what, pos, val)
    c, want = lu.case("mixed_group")
    V = c["lp"].shape[2]
    _check_invalid_row(torch, _dec(V, c["blank"]), c, want, "label = V in a long group", (0, 1, 1), V)


@pytest.mark.parametrize("name", ["edges", "wave_edge", "workgroup_edge", "ties_half", "neg_inf", "blank_mid", "forty_rows", "far_apart", "positive"])
def test_against_align_on_the_device(torch_mod, name):
    """Two consequences of the definitions, device against device: logf of a sum >= 1 is >= 0 and float addition is monotone, so
    log_likelihood >= align score exactly in float32 for every valid row; and on single-path rows (L == 0, or L == n without adjacent
    repeats) the bits are equal."""
    torch = torch_mod
    c, _ = lu.case(name)
    dec = _dec(c["lp"].shape[2], c["blank"])
    x = torch.from_numpy(c["lp"]).cuda()
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    tok, lens = torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()
    ll = dec.log_likelihood(x, seq, tok, lens).cpu().numpy()
    sc = dec.align(x, seq, tok, lens)[2].cpu().numpy()
    assert (ll >= sc).all(), np.argwhere(~(ll >= sc))[:4].tolist()
    assert np.array_equal(np.isneginf(ll), np.isneginf(sc)), "a row has alignments or it has none"
    single = lu.single_path_rows(c)
    for b, r, _n in single:
        assert ll[b, r].view(np.uint32) == sc[b, r].view(np.uint32), (b, r, ll[b, r], sc[b, r])
    if name in ("edges", "neg_inf", "far_apart"):
        assert len(single) >= 2, "the case has single-path rows"
    if name in ("ties_half", "forty_rows"):
        assert (ll > sc).any(), "rows with more than one alignment score strictly more than their best one"


def test_decode_rows_fed_straight_back(torch_mod):
    """End to end: the rows of decode_device(..., n_best=4) on 3 items (T 40, V 8) are scored as they are, against the restatement.
    (log_likelihood against beam_scores is NOT asserted: beam_scores follows the reference's sign convention -- the negated sum of the
    alignments that survived the beam -- so the two are not the same quantity with an inequality between them.)"""
    torch = torch_mod
    rng = np.random.default_rng(40)
    lp = au.log_softmax_rows(rng, 3, 40, 8)
    sl = np.asarray([40, 33, 17], np.int32)
    dec = _dec(8, 0, beam_width=16)
    x, xs = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    out, _scores, _ts, lens = dec.decode_device(x, xs, n_best=4)
    ll = dec.log_likelihood(x, xs, out, lens)
    assert ll.is_cuda and tuple(ll.shape) == (3, 4)
    tok, ln = out.cpu().numpy(), lens.cpu().numpy()
    assert (ln > 0).sum() >= 6, "the input decodes to labels"
    want = lu.reference(lp, sl, tok, ln, 0)
    lu.assert_same(ll.cpu().numpy(), want, "decode rows")
    assert np.isfinite(want["loglik"]).all() and (want["loglik"] < 0).all(), "every row of a decode has alignments"
    # the same through decode()'s CPU tensors and the full beam
    o2, _, _, l2 = dec.decode(torch.from_numpy(lp), torch.from_numpy(sl))
    ll2 = dec.log_likelihood(torch.from_numpy(lp), torch.from_numpy(sl), o2, l2)
    assert not ll2.is_cuda and tuple(ll2.shape) == (3, 16)
    assert np.array_equal(ll2.numpy()[:, :4].view(np.uint32), want["loglik"].view(np.uint32))
