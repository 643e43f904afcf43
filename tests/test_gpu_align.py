"""-m gpu tests of the forced alignment (``CTCBeamDecoder.align`` / ``ctcd_ctc_align``): device output == the numpy restatement of the
header's definition (tests/align_util.py), bit for bit -- scores as uint32, spans exactly -- at the shapes where the kernel can go
wrong.  The cases and their references are those of tests/test_align_host.py, computed once per process."""
import align_util as au
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _dec(V, blank=0, **kw):
    import ctcdecode_amd

    kw.setdefault("log_probs_input", True)
    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, beam_width=kw.pop("beam_width", 8), **kw)


def _align(torch, dec, rows, c, device=True):
    """``rows``: the tensor the decoder is given.  -> result dict (numpy) of dec.align on the case's labels."""
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    tok, lens = torch.from_numpy(c["tokens"]), torch.from_numpy(c["lens"])
    if device:
        tok, lens = tok.cuda(), lens.cuda()
    st, en, sc = dec.align(rows, seq, tok, lens)
    assert st.is_cuda == device and en.is_cuda == device and sc.is_cuda == device
    assert st.dtype == torch.int32 and en.dtype == torch.int32 and sc.dtype == torch.float32
    return dict(start=st.cpu().numpy(), end=en.cpu().numpy(), scores=sc.cpu().numpy())


@pytest.mark.parametrize("name", au.CASES)
def test_device_equals_the_restatement(torch_mod, name):
    """edges: L = 0 at n = 0 and 1, L = 1 at n = 1, L = n distinct / with a repeat, "a a" at n = 3, ragged seq_lens with a 0, rows of length
    0; one_frame: T = 1; wave_edge: S = 63 / 65; workgroup_edge: S = 255 / 257 / 259; many_per_lane: S = 1023 / 1025, T no multiple of 16;
    ties_*: the tie rules alone decide; neg_inf: a label ruled out over a stretch, a whole frame of -inf; blank_*: blank_id != 0,
    L_stride < T; forty_rows: rows of both kinds in every group; mixed_group: a group the workgroup runs row by row that also holds a row
    without a path, and a partial last group of that kind."""
    torch = torch_mod
    c, want = au.case(name)
    dec = _dec(c["lp"].shape[2], c["blank"])
    au.assert_same(_align(torch, dec, torch.from_numpy(c["lp"]).cuda(), c), want, name)


def test_cpu_tensors_in_cpu_tensors_out(torch_mod):
    torch = torch_mod
    c, want = au.case("edges")
    dec = _dec(c["lp"].shape[2], c["blank"])
    au.assert_same(_align(torch, dec, torch.from_numpy(c["lp"]), c, device=False), want, "CPU tensors")


def test_half_rows_equal_their_float_copies(torch_mod):
    torch = torch_mod
    c, _ = au.case("blank_last")
    dec = _dec(c["lp"].shape[2], c["blank"])
    for dt in (torch.float16, torch.bfloat16):
        h = torch.from_numpy(c["lp"]).cuda().to(dt)
        want = au.reference(h.float().cpu().numpy(), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
        assert want["aligned"].any()
        au.assert_same(_align(torch, dec, h, c), want, str(dt))
        au.assert_same(_align(torch, dec, h.float(), c), want, str(dt) + " as float32")


def test_the_three_input_modes(torch_mod):
    """Probabilities: float32(math.log(float64(p) + FLT_MIN)) per element; logits: the restatement on log_softmax()'s own output."""
    torch = torch_mod
    c, _ = au.case("ties_half")
    V = c["lp"].shape[2]
    rng = np.random.default_rng(5)
    p = rng.random(c["lp"].shape).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    p[0, 3, 1] = 0.0
    p[1, 2, :] = 0.0
    dec = _dec(V, c["blank"], log_probs_input=False)
    want = au.reference(au.prob_to_lp(p), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    au.assert_same(_align(torch, dec, torch.from_numpy(p).cuda(), c), want, "probabilities")
    logits = (rng.standard_normal(c["lp"].shape) * 3).astype(np.float32)
    dec = _dec(V, c["blank"], log_probs_input=False, logits_input=True)
    seq = torch.from_numpy(c["seq_lens"])
    for x in (torch.from_numpy(logits).cuda(), torch.from_numpy(logits).cuda().to(torch.bfloat16)):
        lsm = dec.log_softmax(x, seq).cpu().numpy()
        want = au.reference(lsm, c["seq_lens"], c["tokens"], c["lens"], c["blank"])
        assert want["aligned"].any()
        au.assert_same(_align(torch, dec, x, c), want, "logits %s" % x.dtype)


def test_more_hypotheses_than_scratch_slots(torch_mod):
    """ctcd_set_align_scratch set so that the grid is 3 for 40 rows: identical to the default budget's results."""
    torch = torch_mod
    c, want = au.case("forty_rows")
    T, Ls = c["lp"].shape[1], c["tokens"].shape[2]
    dec = _dec(c["lp"].shape[2], c["blank"])
    x = torch.from_numpy(c["lp"]).cuda()
    full = _align(torch, dec, x, c)
    assert dec.last_align_grid() == 40
    dec.set_align_scratch(3 * au.host_slot_bytes(T, Ls))
    few = _align(torch, dec, x, c)
    assert dec.last_align_grid() == 3
    dec.set_align_scratch(1)  # (less than a slot: one workgroup takes every group)
    one = _align(torch, dec, x, c)
    assert dec.last_align_grid() == 1
    dec.set_align_scratch(0)
    for got, what in ((full, "default budget"), (few, "three slots"), (one, "one slot")):
        au.assert_same(got, want, what)


def _raw_align(torch, dec, c, tok, lens, log_input=1):
    """Once through the raw ABI: output tensors pre-filled, status zeroed by the caller.  -> result dict with status."""
    from ctcdecode_amd import _native

    B, T, V = c["lp"].shape
    R, Ls = tok.shape[1:]
    x = torch.from_numpy(c["lp"]).cuda()
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"]).cuda()
    dtok, dlens = torch.from_numpy(tok).cuda(), torch.from_numpy(lens).cuda()
    st = torch.full((B, R, Ls), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    en = torch.full((B, R, Ls), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    sc = torch.full((B, R), -123.0, dtype=torch.float32, device="cuda")
    status = torch.zeros((B,), dtype=torch.int32, device="cuda")
    _native.check(_native.lib.ctcd_set_input_dtype(dec._handle, 0))
    rc = _native.lib.ctcd_ctc_align(dec._handle, x.data_ptr(), seq.data_ptr() if seq is not None else None, B, T, V, c["blank"], log_input, dtok.data_ptr(),
                                    dlens.data_ptr(), R, Ls, st.data_ptr(), en.data_ptr(), sc.data_ptr(), status.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    _native.check(rc)
    torch.cuda.synchronize()
    return dict(start=st.cpu().numpy(), end=en.cpu().numpy(), scores=sc.cpu().numpy(), status=status.cpu().numpy())


def test_raw_abi_writes_every_position(torch_mod):
    torch = torch_mod
    for name in ("edges", "blank_mid", "wave_edge"):
        c, want = au.case(name)
        dec = _dec(c["lp"].shape[2], c["blank"])
        got = _raw_align(torch, dec, c, c["tokens"], c["lens"])
        assert not (got["start"] == 0x5A5A5A5A).any() and not (got["end"] == 0x5A5A5A5A).any(), "a position of the outputs was not written"
        au.assert_same(got, want, "raw ABI, " + name)


def test_raw_abi_refuses_bad_shapes(torch_mod):
    from ctcdecode_amd import _native

    torch = torch_mod
    c, _ = au.case("edges")
    dec = _dec(c["lp"].shape[2])
    x = torch.from_numpy(c["lp"]).cuda()
    a, lens, st, en = (torch.zeros((64,), dtype=torch.int32, device="cuda") for _ in range(4))
    f = torch.zeros((64,), dtype=torch.float32, device="cuda")

    def call(B=1, T=2, V=8, blank=0, mode=1, R=2, Ls=2, probs=x.data_ptr(), tok=a.data_ptr()):
        return _native.lib.ctcd_ctc_align(dec._handle, probs, None, B, T, V, blank, mode, tok, lens.data_ptr(), R, Ls, st.data_ptr(), en.data_ptr(), f.data_ptr(),
                                          None, None)

    assert call() == 0
    for kw in (dict(B=-1), dict(T=-1), dict(V=0), dict(blank=8), dict(blank=-1), dict(mode=3), dict(R=-1), dict(Ls=-1), dict(probs=None), dict(tok=None)):
        assert call(**kw) == -1, kw
    assert call(T=5000, Ls=5000, R=1) == -2, "rows beyond the states one workgroup holds are refused, not cut"
    assert call(T=2048, Ls=2048, R=1) == -2, "min(L_stride, T) = 2048: one label more than a workgroup holds"
    assert call(B=0) == 0 and call(R=0) == 0
    torch.cuda.synchronize()
    # the limit itself is accepted: min(L_stride, T) = 2047 (tensors of that shape: the call launches, on one row without labels)
    x2 = torch.zeros((1, 2048, 8), dtype=torch.float32, device="cuda")
    t2, s2, e2 = (torch.zeros((2047,), dtype=torch.int32, device="cuda") for _ in range(3))
    assert _native.lib.ctcd_ctc_align(dec._handle, x2.data_ptr(), None, 1, 2048, 8, 0, 1, t2.data_ptr(), lens.data_ptr(), 1, 2047, s2.data_ptr(), e2.data_ptr(),
                                      f.data_ptr(), None, None) == 0
    torch.cuda.synchronize()


def _check_invalid_row(torch, dec, c, want, what, pos, val):
    b1, r1 = pos[:2]
    blank = c["blank"]
    tok, lens = c["tokens"].copy(), c["lens"].copy()
    (tok if len(pos) == 3 else lens)[pos] = val
    got = _raw_align(torch, dec, c, tok, lens)
    ref = au.reference(c["lp"], c["seq_lens"], tok, lens, blank)
    assert ref["status"].tolist() == [au.BAD_ROW if b == b1 else 0 for b in range(2)]
    au.assert_same(got, ref, what)
    assert not got["start"][b1, r1].any() and not got["end"][b1, r1].any() and got["scores"][b1, r1] == 0, what
    keep = np.ones(c["lens"].shape, bool)
    keep[b1, r1] = False
    assert np.array_equal(got["start"][keep], want["start"][keep]) and np.array_equal(got["end"][keep], want["end"][keep]), what
    with pytest.raises(ValueError, match="CTCD_ALIGN_BAD_ROW"):
        dec.align(torch.from_numpy(c["lp"]), None, torch.from_numpy(tok), torch.from_numpy(lens))
    au.assert_same(_align(torch, dec, torch.from_numpy(c["lp"]).cuda(), c), want, "the decoder afterwards")


def test_invalid_rows_raise_their_item_alone(torch_mod):
    """A label = V, a label = blank and a negative length each raise CTCD_ALIGN_BAD_ROW for that item only; the other rows are unchanged
    and the decoder is usable afterwards.  mixed_group: the invalid row lies in a group whose rows the workgroup runs one by one."""
    torch = torch_mod
    c, want = au.case("blank_mid")
    V, blank = c["lp"].shape[2], c["blank"]
    dec = _dec(V, blank)
    r0 = int(np.argmax(c["lens"][1] > 1))
    for what, pos, val in (("label = V", (1, r0, 1), V), ("label = blank", (1, r0, 0), blank), ("length < 0", (1, r0), -1), ("length > L_stride", (1, r0), 13)):
        _check_invalid_row(torch, dec, c, want, what, pos, val)
    c, want = au.case("mixed_group")
    V = c["lp"].shape[2]
    _check_invalid_row(torch, _dec(V, c["blank"]), c, want, "label = V in a long group", (0, 1, 1), V)


def test_decode_rows_fed_straight_back(torch_mod):
    """End to end on a tests/golden input: the rows of decode_device(..., n_best=3) are aligned as they are.  Every row is aligned,
    start <= end, spans strictly increase along a row, and the result is the restatement's.  (start <= timesteps is NOT asserted: the
    frame the search appended a label at and the frame the best path puts it on are different notions.)"""
    torch = torch_mod
    import golden_util as gu

    args, _ = gu.load("ragged_b5_t60_k16")  # (log-probabilities, seq_lens 60, 0, 1, 37, 99)
    assert args["log_input"] and args["blank_id"] == 0
    lp, sl = np.ascontiguousarray(args["probs"], np.float32), np.asarray(args["seq_lens"], np.int32)
    B, T, V = lp.shape
    dec = _dec(V, 0, beam_width=args["beam"], cutoff_top_n=args["cutoff_top_n"])
    x, xs = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    out, scores, ts, lens = dec.decode_device(x, xs, n_best=3)
    st, en, sc = dec.align(x, xs, out, lens)
    assert st.is_cuda and tuple(st.shape) == (B, 3, T) and tuple(sc.shape) == (B, 3)
    c = dict(lp=lp, seq_lens=sl, tokens=out.cpu().numpy(), lens=lens.cpu().numpy(), blank=0)
    want = au.reference(lp, sl, c["tokens"], c["lens"], 0)
    got = dict(start=st.cpu().numpy(), end=en.cpu().numpy(), scores=sc.cpu().numpy())
    au.assert_same(got, want, "decode rows")
    assert (c["lens"] > 0).sum() >= 6, "the golden input decodes to labels"
    assert np.isfinite(got["scores"]).all() and want["aligned"].all(), "every row of a decode is aligned"
    for b in range(B):
        for r in range(3):
            L = int(c["lens"][b, r])
            s, e = got["start"][b, r, :L], got["end"][b, r, :L]
            assert (s <= e).all() and (e < min(int(sl[b]), T)).all() and (s[1:] > e[:-1]).all(), (b, r)
    # the same through decode()'s CPU tensors and the full beam
    o2, _, _, l2 = dec.decode(torch.from_numpy(lp), torch.from_numpy(sl))
    st2, en2, sc2 = dec.align(torch.from_numpy(lp), torch.from_numpy(sl), o2, l2)
    assert not st2.is_cuda and tuple(st2.shape) == (B, 16, T)
    assert np.array_equal(st2.numpy()[:, :3], got["start"]) and np.array_equal(sc2.numpy()[:, :3].view(np.uint32), got["scores"].view(np.uint32))
