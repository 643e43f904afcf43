"""-m gpu tests of the exact-shape twin of the north-star decode kernel (ctcd_set_exact_shape / CTCBeamDecoder.set_exact_shape):
beam 100 over 29 labels, blank 0.  The twin against the planned kernel -- every output tensor and the status words, bit for bit --
and against the oracle, over the inputs the CPU test settled (exact_shape_util.cases: T <= 40, B <= 8); every route that takes the
twin, each through _both() -- the twin REQUIRED, then the planned kernel, which ran asserted, the outputs equal by bits: the kernel
matrix's recipe (select paths, overflow frames), rows behind each pre-pass, the blank-frame filter, the result routes (n_best,
decode() of device and host rows), a batch that outnumbers the CUs under length order, time steps past frame 65535; and the near
misses, each of which must keep the planned kernel (and be refused in mode 1)."""
import numpy as np
import pytest

import exact_shape_util as xs
import oracle_util as ou

pytestmark = pytest.mark.gpu

CASES = xs.cases()
LABELS = [str(i) for i in range(xs.LABELS)]


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _decoder(labels=xs.LABELS, cls=None, **kw):
    import ctcdecode_amd

    kw.setdefault("log_probs_input", True)
    kw.setdefault("beam_width", xs.BEAM)
    kw.setdefault("blank_id", xs.BLANK)
    lab = kw.pop("label_names", [str(i) for i in range(labels)])
    dec = (cls or ctcdecode_amd.CTCBeamDecoder)(lab, device="cuda:0", **kw)
    # (the automatic choice between the plain build and the subtree build follows the beam shape of the last checked launch: pinned
    #  to the plain build, so that every call of a test plans the same kernel -- the subtree build is one of the near misses)
    if cls is None:
        dec.set_subtree_search(0)
    return dec


def _status(torch, dec, B):
    from ctcdecode_amd import _native

    st = torch.full((max(B, 1),), -7, dtype=torch.int32).pin_memory()
    _native.check(_native.lib.ctcd_fetch_status_async(dec._handle, B, st.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return st[:B].clone()


def _run(torch, dec, probs, sl, mode, n_best=None):
    dec.set_exact_shape(mode)
    out = dec.decode_device(probs, sl, n_best=n_best)
    return out, _status(torch, dec, probs.shape[0]), dec.last_exact_shape()


def _as_dict(out, B):
    tok, sc, ts, ln = [t.cpu().numpy() for t in out]
    return dict(tokens=tok, timesteps=ts, scores=sc, lens=ln, nres=np.full((B,), -1, np.int32))


def _assert_oracle(out, want, what):
    """oracle_util.assert_same on the rows the oracle defines (decode_device reports no result count: the oracle's is taken)."""
    got = _as_dict(out, len(want["nres"]))
    got["nres"] = want["nres"]
    ou.assert_same(got, want, what)


@pytest.mark.parametrize("name,lp,sl", CASES, ids=[c[0] for c in CASES])
def test_twin_equals_planned_kernel_and_oracle(torch_mod, name, lp, sl):
    torch = torch_mod
    B = lp.shape[0]
    probs = torch.from_numpy(lp).cuda()
    lens = torch.from_numpy(sl).cuda() if sl is not None else None
    dec = _decoder()
    on, st_on, ran_on = _run(torch, dec, probs, lens, -1)
    kernel_on = dec.last_kernel()
    off, st_off, ran_off = _run(torch, dec, probs, lens, 0)
    assert ran_on == 1 and ran_off == 0, (ran_on, ran_off)
    assert kernel_on == dec.last_kernel() == (0, 0, 1, 0, 1024, 0, 0)  # (the record stays the planned key)
    for i, (a, b) in enumerate(zip(on, off)):
        assert torch.equal(a, b), "%s: output %d differs between the twin and the planned kernel" % (name, i)
        if a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name
    assert torch.equal(st_on, st_off) and int(st_on.abs().sum()) == 0, (st_on, st_off)
    _assert_oracle(on, xs.oracle(name, lp, sl), name + " twin vs oracle:")
    req, st_req, ran_req = _run(torch, dec, probs, lens, 1)  # required: the same launch
    assert ran_req == 1 and all(torch.equal(a, b) for a, b in zip(req, on)) and torch.equal(st_req, st_on)


def _both(torch, dec, run, B, what):
    """run() -- one decode call of `dec`, returning its tensors -- in mode 1 (the twin REQUIRED: a call that does not qualify is
    refused, so a route that silently stopped taking the twin fails here) and in mode 0 (the planned kernel).  Asserts which kernel
    ran, and that every output and the status words are equal, float32 by bits.  -> the mode-1 outputs, for the oracle.  The decoder
    is left in automatic mode."""
    res = []
    for mode in (1, 0):
        dec.set_exact_shape(mode)
        out = run()
        st = _status(torch, dec, B)
        assert dec.last_exact_shape() == mode, "%s: mode %d ran %s" % (what, mode, "the twin" if dec.last_exact_shape() else "the planned kernel")
        res.append((out, st))
    dec.set_exact_shape(-1)
    (on, st_on), (off, st_off) = res
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        assert a.dtype == b.dtype and a.shape == b.shape and a.device == b.device, "%s: output %d" % (what, i)
        assert torch.equal(a, b), "%s: output %d differs between the twin and the planned kernel" % (what, i)
        if a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "%s: output %d differs by bits" % (what, i)
    assert torch.equal(st_on, st_off) and int(st_on.abs().sum()) == 0, (what, st_on, st_off)
    return on


def _want(lp, sl, **kw):
    """The oracle (the compiled reference where it was built) on float32 rows."""
    kw.setdefault("beam", xs.BEAM)
    kw.setdefault("blank_id", xs.BLANK)
    return ou.decode(lp, sl, cutoff_prob=1.0, cutoff_top_n=40, which="reference" if ou.have_reference() else "restated", **kw)


def _in_dtype(dec):
    from ctcdecode_amd import _native

    return int(_native.lib.ctcd_last_input_dtype(dec._handle))


def _same_rows(torch, part, full, n, what):
    """A result of n rows per item (any device) against rows [:n] of the padded result."""
    assert len(part) == 4
    for i, (a, b) in enumerate(zip(part, full)):
        b = b[:, :n].to(a.device)
        assert a.shape == b.shape and torch.equal(a, b), "%s: output %d is not rows [:%d] of the padded result" % (what, i, n)
        if a.dtype == torch.float32:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


def test_select_paths_and_overflow_frames(torch_mod):
    """The kernel matrix's recipe at the twin's shape (exact_shape_util.matrix_inputs; test_exact_shape_host.py certifies on the CPU
    which select paths it reaches): every wave-parallel select routine of Decoder::step<true>, and danger mode entered from finite
    inputs -- two frames of -3e38 overflow every score to -inf."""
    torch = torch_mod
    lp, sl = xs.matrix_inputs()
    c = xs.matrix_case()
    probs, lens = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    dec = _decoder()
    dec.set_threads(c["threads"])
    on = _both(torch, dec, lambda: dec.decode_device(probs, lens), lp.shape[0], "matrix inputs")
    assert dec.last_kernel() == c["kernel"] == xs.PARENT_KERNEL
    _assert_oracle(on, _want(lp, sl), "matrix inputs, twin vs oracle:")


PREPASS_LENS = np.array([40, 0, 17, 49], np.int32)  # (one empty item, one length beyond T)


@pytest.mark.parametrize("kind,dtype", [("logp", "bfloat16"), ("logp", "float16"), ("prob", "float32"), ("prob", "bfloat16"),
                                        ("logits", "float32"), ("logits", "bfloat16")])
def test_rows_that_pass_a_prepass_first(torch_mod, kind, dtype):
    """Half log-probabilities (widened), probabilities (their logarithm taken) and raw logits (log-softmax) reach the decode kernel
    through a pre-pass that writes float32 rows into the workspace: the twin reads those as its parent does."""
    torch = torch_mod
    B, T = 4, 40
    x = torch.randn((B, T, xs.LABELS), generator=torch.Generator().manual_seed(77)) * 2.0
    if kind == "logp":
        x = torch.log_softmax(x, -1)
    elif kind == "prob":
        x = torch.softmax(x, -1)
    x = x.to(getattr(torch, dtype)).cuda()
    lens = torch.from_numpy(PREPASS_LENS).cuda()
    dec = _decoder(log_probs_input=kind == "logp", logits_input=kind == "logits")
    what = "%s %s" % (dtype, kind)
    on = _both(torch, dec, lambda: dec.decode_device(x, lens), B, what)
    assert _in_dtype(dec) == {"float32": 0, "float16": 1, "bfloat16": 2}[dtype]
    stages = dec.last_prepass()
    assert stages["prune"] is None and stages["resolve"] is None
    if kind == "logits":
        assert stages["log_softmax"] is not None and stages["elementwise"] is None, stages
    else:
        assert stages["elementwise"] is not None and stages["log_softmax"] is None, stages
    wide = x.float().cpu().numpy()  # (widening is exact)
    if kind == "logits":
        want = _want(ou.log_softmax_rows(wide), PREPASS_LENS)
    else:
        want = _want(wide, PREPASS_LENS, log_input=kind == "logp")
    _assert_oracle(on, want, what + ", twin vs oracle:")


def test_blank_frame_filter_in_front_of_the_twin(torch_mod):
    """CTCBeamDecoder(blank_skip=thr): the filter is a pass of its own in front of the decode (ctcd_blank_skip gathers the kept rows,
    ctcd_remap_timesteps maps the time steps back behind it), and the decode call sees whole utterances of kept rows in HBM -- no
    stream state, no streamed rows.  So the route QUALIFIES: it takes the twin, on the device route and on the host route."""
    import blank_skip_util as bs

    torch = torch_mod
    B, T, thr = 4, 60, 0.9
    lp = xs.rows("blank", B, T, 4242)
    sl = np.array([60, 0, 31, 64], np.int32)
    want, kept, n2 = bs.decode(lp, sl, thr, beam=xs.BEAM, cutoff_top_n=40)
    considered = int(np.clip(sl, 0, T).sum())
    assert 0 < int(n2.sum()) < considered and all(0 < n2[b] < min(sl[b], T) for b in (0, 2, 3)), n2  # some frames dropped, not all
    probs, lens = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    dec = _decoder(blank_skip=thr)
    on = _both(torch, dec, lambda: dec.decode_device(probs, lens), B, "blank_skip, decode_device")
    assert dec.last_blank_skip() == (considered, int(n2.sum()))
    _assert_oracle(on, want, "blank_skip, twin vs the oracle on the kept frames:")
    host = _both(torch, dec, lambda: dec.decode(probs, lens), B, "blank_skip, decode")
    _same_rows(torch, host, on, xs.BEAM, "blank_skip, decode")


@pytest.mark.parametrize("kind", ["randn", "quant"])
def test_n_best_route_and_ragged_batch_under_length_order(torch_mod, kind):
    """A ragged batch under length order, and every result route behind the twin: n_best rows through the compact records
    (n < beam) and as the whole beam (n = 100), decode() of device rows (compact records through mapped host memory) and decode() of a
    small CPU tensor (uploaded whole) -- each in both modes, each equal to the slices of the padded result."""
    torch = torch_mod
    name = kind + "_ragged"
    lp, sl = [(l, s) for n, l, s in CASES if n == name][0]
    B = len(sl)
    probs, lens = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    dec = _decoder()
    dec.set_launch_order("length")
    on, st_on, ran = _run(torch, dec, probs, lens, -1)
    order = dec.last_launch_order()
    assert ran == 1 and order is not None and not np.array_equal(order, np.arange(len(sl)))
    assert sorted(order.tolist()) == list(range(B))
    off, st_off, ran0 = _run(torch, dec, probs, lens, 0)
    assert ran0 == 0 and all(torch.equal(a, b) for a, b in zip(on, off)) and torch.equal(st_on, st_off)
    _assert_oracle(on, xs.oracle(name, lp, sl), name + " length order, twin vs oracle:")
    for n in (1, 7, xs.BEAM):
        nb = _both(torch, dec, lambda: dec.decode_device(probs, lens, n_best=n), B, "%s n_best=%d" % (name, n))
        _same_rows(torch, nb, on, n, "%s n_best=%d" % (name, n))
    dec.set_launch_order("batch")
    dec.set_exact_shape(-1)
    host = dec.decode(probs, lens)  # (compact results to the host: the twin behind another entry point)
    assert dec.last_exact_shape() == 1
    assert all(torch.equal(a, b.cpu()) for a, b in zip(host, on))
    for what, run in (("decode() of device rows", lambda: dec.decode(probs, lens)),
                      ("decode() of a CPU tensor", lambda: dec.decode(torch.from_numpy(lp), torch.from_numpy(sl))),
                      ("decode(n_best=7) of device rows", lambda: dec.decode(probs, lens, n_best=7))):
        res = _both(torch, dec, run, B, "%s, %s" % (name, what))
        assert not res[0].is_cuda
        _same_rows(torch, res, on, res[0].shape[1], "%s, %s" % (name, what))


def test_more_workgroups_than_cus(torch_mod):
    """A batch that outnumbers the CUs with one workgroup per CU: the ticket counter of the length order runs past the first round of
    workgroups, and a late workgroup starts on the LDS an earlier twin workgroup left behind.  Left to itself (set_cu_sharing(-1))
    the same call plans the two-workgroups-per-CU build, which has no twin."""
    torch = torch_mod
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    B, T = ncu + 44, 12
    lp = ou.synth_logprobs(B, T, xs.LABELS, 5150, quant=1.0)
    sl = np.random.default_rng(5151).integers(0, T + 1, size=B).astype(np.int32)
    sl[:4] = [T, 0, 1, T + 3]
    probs, lens = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    dec = _decoder()
    dec.set_cu_sharing(0)
    dec.set_launch_order("length")
    orders = []

    def run():
        out = dec.decode_device(probs, lens)
        orders.append(dec.last_launch_order())
        return out

    on = _both(torch, dec, run, B, "B = #CUs + 44")
    assert dec.last_kernel() == xs.PARENT_KERNEL
    for order in orders:
        assert order is not None and sorted(order.tolist()) == list(range(B)), "the launch order is not a permutation of the batch"
        assert not np.array_equal(order, np.arange(B))
    _assert_oracle(on, _want(lp, sl), "B = #CUs + 44, twin vs oracle:")
    dec.set_cu_sharing(-1)
    _near_miss(torch, dec, probs, "more utterances than CUs: the two-workgroups-per-CU build", run=lambda: dec.decode_device(probs, lens))
    assert dec.last_kernel() == xs.PARENT_KERNEL[:6] + (1,)


LONG_T = 66500


@pytest.fixture(scope="module")
def long_case():
    """One utterance of 66500 frames and the oracle's decode of it (host time only: tens of seconds on one thread), computed once
    for the module and left unchanged."""
    lp = ou.synth_logprobs(1, LONG_T, xs.LABELS, 17, blank_bias=2.5)
    want = _want(lp, None)
    n = int(want["lens"][0, 0])
    assert n > 0 and int(want["timesteps"][0, 0, :n].max()) > 65535, "no time step past frame 65535 in the best row: change the seed"
    return lp, want


def test_time_steps_past_frame_65535(torch_mod, long_case):
    """Past frame 65535 a node's time step keeps its high part in a side array (beam_core.h long_t): in the twin those stores
    sit in Decoder::step<true>.  decode_device, and the two padded fallbacks that T > 65536 sends past the compact records
    (n_best, decode())."""
    torch = torch_mod
    lp, want = long_case
    probs = torch.from_numpy(lp).cuda()
    dec = _decoder()
    on = _both(torch, dec, lambda: dec.decode_device(probs), 1, "T = %d" % LONG_T)
    _assert_oracle(on, want, "T = %d, twin vs oracle:" % LONG_T)
    nb = _both(torch, dec, lambda: dec.decode_device(probs, n_best=3), 1, "T = %d, n_best=3" % LONG_T)
    _same_rows(torch, nb, on, 3, "T = %d, n_best=3" % LONG_T)
    host = _both(torch, dec, lambda: dec.decode(probs), 1, "T = %d, decode()" % LONG_T)
    assert not host[0].is_cuda
    _same_rows(torch, host, on, xs.BEAM, "T = %d, decode()" % LONG_T)


def _near_miss(torch, dec, probs, what, run=None):
    """The call keeps the planned kernel in automatic mode, and mode 1 refuses it without launching anything."""
    run = run or (lambda: dec.decode_device(probs))
    dec.set_exact_shape(-1)
    run()
    assert dec.last_exact_shape() == 0, what
    before = dec.last_kernel()
    dec.set_exact_shape(1)
    with pytest.raises(Exception, match="exact"):
        run()
    assert dec.last_kernel() == before and dec.last_exact_shape() == 0, what
    dec.set_exact_shape(-1)


def test_near_misses_keep_the_planned_kernel(torch_mod):
    torch = torch_mod
    T, B = 12, 2

    def rows(V, seed=3):
        return torch.from_numpy(ou.synth_logprobs(B, T, V, seed)).cuda()

    p29 = rows(29)
    ok = _decoder()
    ok.decode_device(p29)
    assert ok.last_exact_shape() == 1  # (the shape that qualifies, for contrast)
    for beam in (99, 101):
        _near_miss(torch, _decoder(beam_width=beam), p29, "beam %d" % beam)
    for V in (28, 30, 32):
        _near_miss(torch, _decoder(labels=V), rows(V), "%d labels" % V)
    _near_miss(torch, _decoder(blank_id=1), p29, "blank 1")
    _near_miss(torch, _decoder(blank_id=28), p29, "blank 28")
    _near_miss(torch, _decoder(cutoff_top_n=28), p29, "cutoff_top_n 28")
    _near_miss(torch, _decoder(cutoff_prob=0.99), p29, "cutoff_prob 0.99")
    d = _decoder()
    d.set_cu_sharing(1)
    _near_miss(torch, d, p29, "two workgroups per CU")
    d = _decoder()
    d.set_threads(512)
    _near_miss(torch, d, p29, "512 threads")
    d = _decoder()
    d.set_subtree_search(1)
    _near_miss(torch, d, p29, "the subtree build")


def test_near_miss_scorer(torch_mod):
    torch = torch_mod
    from test_lm import LABELS29, TEST_ARPA

    probs = torch.from_numpy(ou.synth_logprobs(2, 12, 29, 4)).cuda()
    dec = _decoder(label_names=LABELS29, model_path=TEST_ARPA, alpha=0.5, beta=1.0)
    _near_miss(torch, dec, probs, "a scorer")


def test_near_miss_streamed_host_rows(torch_mod):
    """decode() of a CPU tensor of a megabyte or more with T >= 128: the rows cross PCIe while the kernel runs (its PROF 4 build)."""
    torch = torch_mod
    B, T = 8, 1140  # 8 * 1140 * 29 * 4 B = 1.01 MiB
    probs = torch.from_numpy(ou.synth_logprobs(B, T, 29, 5))
    dec = _decoder()
    _near_miss(torch, dec, probs, "streamed rows", run=lambda: dec.decode(probs))
    assert dec.last_kernel()[0] == 4
    small = probs[:, :64].contiguous()  # (the same route with rows that are uploaded whole: the twin)
    dec.decode(small)
    assert dec.last_exact_shape() == 1


def test_near_miss_online_chunk(torch_mod):
    torch = torch_mod
    import ctcdecode_amd
    from ctcdecode_amd import _native

    probs = torch.from_numpy(ou.synth_logprobs(2, 12, 29, 6)).cuda()
    dec = _decoder(cls=ctcdecode_amd.OnlineCTCBeamDecoder)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(2)]
    dec.decode(probs, states, [False, False])
    assert int(_native.lib.ctcd_last_exact_shape(dec._handle)) == 0
    _native.check(_native.lib.ctcd_set_exact_shape(dec._handle, 1))
    with pytest.raises(Exception, match="exact"):
        dec.decode(probs, states, [True, True])
    _native.check(_native.lib.ctcd_set_exact_shape(dec._handle, -1))
    dec.decode(probs, states, [True, True])
    assert int(_native.lib.ctcd_last_exact_shape(dec._handle)) == 0


def test_mode_is_validated(torch_mod):
    dec = _decoder()
    for bad in (-2, 2):
        with pytest.raises(Exception):
            dec.set_exact_shape(bad)
    assert dec.last_exact_shape() == 0  # (no launch yet)
