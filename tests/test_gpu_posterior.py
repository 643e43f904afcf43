"""-m gpu tests of the label posteriors (``CTCBeamDecoder.label_posteriors`` / ``ctcd_ctc_posteriors``): device output == the Python
restatement of the header's definition (tests/posterior_util.py), bit for bit as uint32, at the shapes where the kernel can go wrong.
The cases and their references are those of tests/test_posterior_host.py, computed once per process."""
import align_util as au
import numpy as np
import posterior_util as pu
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _references_released_afterwards():
    """The cases and their references live for this module's tests only: the tests that run after it find the process as it was."""
    yield
    import gc

    pu.release()
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


def _post(torch, dec, rows, c, device=True):
    """``rows``: the tensor the decoder is given.  -> dict of numpy arrays of dec.label_posteriors on the case's labels."""
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    tok, lens = torch.from_numpy(c["tokens"]), torch.from_numpy(c["lens"])
    if device:
        tok, lens = tok.cuda(), lens.cuda()
    outs = dec.label_posteriors(rows, seq, tok, lens)
    assert len(outs) == 4 and all(o.is_cuda == device for o in outs)
    assert [o.dtype for o in outs] == [torch.int32, torch.float32, torch.float32, torch.float32]
    assert [tuple(o.shape) for o in outs] == [tuple(c["tokens"].shape)] * 3 + [tuple(c["lens"].shape)]
    return dict(zip(pu.KEYS, (o.cpu().numpy() for o in outs)))


@pytest.mark.parametrize("name", pu.CASES)
def test_device_equals_the_restatement(torch_mod, name):
    """loglik_util's cases -- edges, one_frame, wave_edge (S = 63 / 65), workgroup_edge (S = 255 / 257 / 259), many_per_lane (S = 1023 /
    1025, T = 514: no multiple of the prefetch depth), ties_*, neg_inf, blank_* (blank_id != 0, L_stride < T), forty_rows, mixed_group,
    zeros, far_apart, positive, overflow -- and dyadic_single_path (exact sums: occupancy 1.0f, peaks i, confidence expf(lp)), clamped
    (a + b - lp - ll above 0), subnormal (a subnormal product g * e80(lp))."""
    torch = torch_mod
    c, want = pu.case(name)
    dec = _dec(c["lp"].shape[2], c["blank"])
    pu.assert_same(_post(torch, dec, torch.from_numpy(c["lp"]).cuda(), c), want, name)


def test_cpu_tensors_in_cpu_tensors_out(torch_mod):
    torch = torch_mod
    c, want = pu.case("edges")
    dec = _dec(c["lp"].shape[2], c["blank"])
    pu.assert_same(_post(torch, dec, torch.from_numpy(c["lp"]), c, device=False), want, "CPU tensors")


def test_half_rows_equal_their_float_copies(torch_mod):
    torch = torch_mod
    c, _ = pu.case("blank_last")
    dec = _dec(c["lp"].shape[2], c["blank"])
    for dt in (torch.float16, torch.bfloat16):
        h = torch.from_numpy(c["lp"]).cuda().to(dt)
        want = pu.reference(h.float().cpu().numpy(), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
        assert np.isfinite(want["loglik"]).any() and (want["occupancy"] > 0).any()
        pu.assert_same(_post(torch, dec, h, c), want, str(dt))
        pu.assert_same(_post(torch, dec, h.float(), c), want, str(dt) + " as float32")


def test_the_three_input_modes(torch_mod):
    """Probabilities: float32(math.log(float64(p) + FLT_MIN)) per element; logits: the restatement on log_softmax()'s own output."""
    torch = torch_mod
    c, _ = pu.case("ties_half")
    V = c["lp"].shape[2]
    rng = np.random.default_rng(5)
    p = rng.random(c["lp"].shape).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    p[0, 3, 1] = 0.0
    p[1, 2, :] = 0.0
    dec = _dec(V, c["blank"], log_probs_input=False)
    want = pu.reference(au.prob_to_lp(p), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    pu.assert_same(_post(torch, dec, torch.from_numpy(p).cuda(), c), want, "probabilities")
    logits = (rng.standard_normal(c["lp"].shape) * 3).astype(np.float32)
    dec = _dec(V, c["blank"], log_probs_input=False, logits_input=True)
    seq = torch.from_numpy(c["seq_lens"])
    for x in (torch.from_numpy(logits).cuda(), torch.from_numpy(logits).cuda().to(torch.bfloat16)):
        lsm = dec.log_softmax(x, seq).cpu().numpy()
        want = pu.reference(lsm, c["seq_lens"], c["tokens"], c["lens"], c["blank"])
        assert np.isfinite(want["loglik"]).any()
        pu.assert_same(_post(torch, dec, x, c), want, "logits %s" % x.dtype)


def test_the_scratch_budget_changes_nothing(torch_mod):
    """set_posterior_scratch at 3 slots and at 1 slot for the 40 rows of forty_rows: the grids are 3 and 1, and the results are the
    default's bits."""
    torch = torch_mod
    c, want = pu.case("forty_rows")
    T = c["lp"].shape[1]
    dec = _dec(c["lp"].shape[2], c["blank"])
    x = torch.from_numpy(c["lp"]).cuda()
    slot = pu.host_slot_bytes(T, c["tokens"].shape[2])
    full = _post(torch, dec, x, c)
    assert dec.last_posterior_grid() == 40, "40 rows within the default budget"
    dec.set_posterior_scratch(3 * slot + slot // 2)
    few = _post(torch, dec, x, c)
    assert dec.last_posterior_grid() == 3
    dec.set_posterior_scratch(slot)
    one = _post(torch, dec, x, c)
    assert dec.last_posterior_grid() == 1
    dec.set_posterior_scratch(0)
    for got, what in ((full, "default budget"), (few, "three slots"), (one, "one slot")):
        pu.assert_same(got, want, what)
        for k in pu.KEYS:
            assert np.array_equal(got[k].view(np.uint32), full[k].view(np.uint32)), (what, k)


def _raw(torch, dec, c, tok, lens, log_input=1):
    """Once through the raw ABI: the outputs pre-filled, status zeroed by the caller.  -> dict(peaks, occupancy, confidence, loglik, status)."""
    from ctcdecode_amd import _native

    B, T, V = c["lp"].shape
    R, Ls = tok.shape[1:]
    x = torch.from_numpy(c["lp"]).cuda()
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"]).cuda()
    dtok, dlens = torch.from_numpy(tok).cuda(), torch.from_numpy(lens).cuda()
    pk = torch.full((B, R, Ls), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    oc, cf = (torch.full((B, R, Ls), -123.0, dtype=torch.float32, device="cuda") for _ in range(2))
    ll = torch.full((B, R), -123.0, dtype=torch.float32, device="cuda")
    status = torch.zeros((B,), dtype=torch.int32, device="cuda")
    _native.check(_native.lib.ctcd_set_input_dtype(dec._handle, 0))
    rc = _native.lib.ctcd_ctc_posteriors(dec._handle, x.data_ptr(), seq.data_ptr() if seq is not None else None, B, T, V, c["blank"], log_input, dtok.data_ptr(),
                                         dlens.data_ptr(), R, Ls, pk.data_ptr(), oc.data_ptr(), cf.data_ptr(), ll.data_ptr(), status.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
    _native.check(rc)
    torch.cuda.synchronize()
    return dict(peaks=pk.cpu().numpy(), occupancy=oc.cpu().numpy(), confidence=cf.cpu().numpy(), loglik=ll.cpu().numpy(), status=status.cpu().numpy())


def test_raw_abi_writes_every_row(torch_mod):
    torch = torch_mod
    for name in ("edges", "blank_mid", "wave_edge", "mixed_group"):
        c, want = pu.case(name)
        dec = _dec(c["lp"].shape[2], c["blank"])
        got = _raw(torch, dec, c, c["tokens"], c["lens"])
        assert not (got["peaks"] == 0x5A5A5A5A).any() and not any((got[k] == -123.0).any() for k in pu.KEYS[1:]), "a position of the outputs was not written"
        pu.assert_same(got, want, "raw ABI, " + name)


def test_raw_abi_refuses_bad_shapes(torch_mod):
    from ctcdecode_amd import _native

    torch = torch_mod
    c, _ = pu.case("edges")
    dec = _dec(c["lp"].shape[2])
    x = torch.from_numpy(c["lp"]).cuda()
    a, lens = (torch.zeros((64,), dtype=torch.int32, device="cuda") for _ in range(2))
    pk = torch.full((64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    oc, cf, f = (torch.full((64,), -123.0, dtype=torch.float32, device="cuda") for _ in range(3))

    def call(B=1, T=2, V=8, blank=0, mode=1, R=2, Ls=2, probs=x.data_ptr(), tok=a.data_ptr(), peaks=pk.data_ptr(), occ=oc.data_ptr(), conf=cf.data_ptr(), out=f.data_ptr()):
        return _native.lib.ctcd_ctc_posteriors(dec._handle, probs, None, B, T, V, blank, mode, tok, lens.data_ptr(), R, Ls, peaks, occ, conf, out, None, None)

    for kw in (dict(B=-1), dict(T=-1), dict(V=0), dict(blank=8), dict(blank=-1), dict(mode=3), dict(R=-1), dict(Ls=-1), dict(probs=None), dict(tok=None),
               dict(peaks=None), dict(occ=None), dict(conf=None), dict(out=None)):
        assert call(**kw) == -1, kw
    assert call(T=5000, Ls=5000, R=1) == -2, "rows beyond the states one workgroup holds are refused, not cut"
    assert call(T=2048, Ls=2048, R=1) == -2, "min(L_stride, T) = 2048: one label more than a workgroup holds"
    assert call(V=(1 << 28) + 1) == -2
    assert call(B=0) == 0 and call(R=0) == 0
    torch.cuda.synchronize()
    assert (f == -123.0).all() and (oc == -123.0).all() and (cf == -123.0).all() and (pk == 0x5A5A5A5A).all(), "a refused call, or one without rows, launches nothing"
    assert call() == 0
    torch.cuda.synchronize()
    assert (f[:2] != -123.0).all() and (f[2:] == -123.0).all()
    for o in (oc, cf):
        assert (o[:4] == 0).all() and (o[4:] == -123.0).all(), "two empty rows of stride 2: zero tails, and nothing beyond them"
    assert (pk[:4] == 0).all() and (pk[4:] == 0x5A5A5A5A).all()
    # the limit itself is accepted: min(L_stride, T) = 2047 (tensors of that shape: the call launches, on one row without labels)
    x2 = torch.zeros((1, 2048, 8), dtype=torch.float32, device="cuda")
    t2, p2 = (torch.zeros((2047,), dtype=torch.int32, device="cuda") for _ in range(2))
    o2, c2 = (torch.zeros((2047,), dtype=torch.float32, device="cuda") for _ in range(2))
    assert call(T=2048, Ls=2047, R=1, probs=x2.data_ptr(), tok=t2.data_ptr(), peaks=p2.data_ptr(), occ=o2.data_ptr(), conf=c2.data_ptr()) == 0
    torch.cuda.synchronize()


def _check_invalid_row(torch, dec, c, want, what, pos, val):
    b1, r1 = pos[:2]
    blank = c["blank"]
    tok, lens = c["tokens"].copy(), c["lens"].copy()
    (tok if len(pos) == 3 else lens)[pos] = val
    got = _raw(torch, dec, c, tok, lens)
    ref = pu.reference(c["lp"], c["seq_lens"], tok, lens, blank)
    assert ref["status"].tolist() == [pu.BAD_ROW if b == b1 else 0 for b in range(2)]
    pu.assert_same(got, ref, what)
    keep = np.ones(c["lens"].shape, bool)
    keep[b1, r1] = False
    for k in pu.KEYS:
        assert not got[k][b1, r1].any(), (what, k)
        assert np.array_equal(got[k][keep].view(np.uint32), want[k][keep].view(np.uint32)), (what, k)
    with pytest.raises(ValueError, match=r"items \[%d\].*CTCD_ALIGN_BAD_ROW" % b1):
        dec.label_posteriors(torch.from_numpy(c["lp"]), None, torch.from_numpy(tok), torch.from_numpy(lens))
    pu.assert_same(_post(torch, dec, torch.from_numpy(c["lp"]).cuda(), c), want, "the decoder afterwards")


def test_invalid_rows_raise_their_item_alone(torch_mod):
    """A label = V, a label = blank, a negative length and one beyond L_stride each raise CTCD_ALIGN_BAD_ROW for that item only; the other
    rows are unchanged and the decoder is usable afterwards.  mixed_group: the invalid row lies in a group whose rows the workgroup
    runs one by one."""
    torch = torch_mod
    c, want = pu.case("blank_mid")
    V, blank = c["lp"].shape[2], c["blank"]
    dec = _dec(V, blank)
    r0 = int(np.argmax(c["lens"][1] > 1))
    for what, pos, val in (("label = V", (1, r0, 1), V), ("label = blank", (1, r0, 0), blank), ("length < 0", (1, r0), -1), ("length > L_stride", (1, r0), 13)):
        _check_invalid_row(torch, dec, c, want, what, pos, val)
    c, want = pu.case("mixed_group")
    V = c["lp"].shape[2]
    _check_invalid_row(torch, _dec(V, c["blank"]), c, want, "label = V in a long group", (0, 1, 1), V)


@pytest.mark.parametrize("name", ["edges", "wave_edge", "workgroup_edge", "many_per_lane", "neg_inf", "blank_mid", "forty_rows", "mixed_group", "far_apart", "overflow"])
def test_loglik_equals_log_likelihood_on_the_device(torch_mod, name):
    """The fourth output and dec.log_likelihood, device against device, with equal bits."""
    torch = torch_mod
    c, _ = pu.case(name)
    dec = _dec(c["lp"].shape[2], c["blank"])
    x = torch.from_numpy(c["lp"]).cuda()
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    tok, lens = torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()
    ll = dec.log_likelihood(x, seq, tok, lens)
    got = dec.label_posteriors(x, seq, tok, lens)[3]
    assert torch.equal(ll.view(torch.int32), got.view(torch.int32)), name


def test_peaks_lie_inside_the_alignment_on_single_path_rows(torch_mod):
    """dyadic_single_path: a row's only alignment is align's, and every label's posterior peaks inside its span -- here the span is one
    frame, frame i."""
    torch = torch_mod
    c, _ = pu.case("dyadic_single_path")
    dec = _dec(c["lp"].shape[2], c["blank"])
    x, seq = torch.from_numpy(c["lp"]).cuda(), torch.from_numpy(c["seq_lens"])
    tok, lens = torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()
    starts, ends, scores = (o.cpu().numpy() for o in dec.align(x, seq, tok, lens))
    peaks, occ, _conf, ll = (o.cpu().numpy() for o in dec.label_posteriors(x, seq, tok, lens))
    assert np.isfinite(scores).all() and np.array_equal(scores.view(np.uint32), ll.view(np.uint32)), "one alignment holds all of the mass"
    for b, r in np.ndindex(*c["lens"].shape):
        L = int(c["lens"][b, r])
        assert L >= 1 and ((starts[b, r, :L] <= peaks[b, r, :L]) & (peaks[b, r, :L] <= ends[b, r, :L])).all(), (b, r)
        assert (occ[b, r, :L] == 1).all() and not occ[b, r, L:].any() and not peaks[b, r, L:].any()


def test_decode_rows_fed_straight_back(torch_mod):
    """End to end: the rows of decode_device(..., n_best=4) on 3 items (T 40, V 8) are scored as they are, against the restatement."""
    torch = torch_mod
    rng = np.random.default_rng(40)
    lp = au.log_softmax_rows(rng, 3, 40, 8)
    sl = np.asarray([40, 33, 17], np.int32)
    dec = _dec(8, 0, beam_width=16)
    x, xs = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    out, _scores, _ts, lens = dec.decode_device(x, xs, n_best=4)
    outs = dec.label_posteriors(x, xs, out, lens)
    assert all(o.is_cuda for o in outs) and tuple(outs[0].shape) == (3, 4, 40) and tuple(outs[3].shape) == (3, 4)
    tok, ln = out.cpu().numpy(), lens.cpu().numpy()
    assert (ln > 0).sum() >= 6, "the input decodes to labels"
    want = pu.reference(lp, sl, tok, ln, 0)
    pu.assert_same(dict(zip(pu.KEYS, (o.cpu().numpy() for o in outs))), want, "decode rows")
    assert np.isfinite(want["loglik"]).all() and (want["occupancy"][want["peaks"] > 0] >= 0.9).all(), "every label of a decoded row occupies about a frame or more"
