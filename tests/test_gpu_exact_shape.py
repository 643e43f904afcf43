"""-m gpu tests of the exact-shape twin of the north-star decode kernel (ctcd_set_exact_shape / CTCBeamDecoder.set_exact_shape):
beam 100 over 29 labels, blank 0.  The twin against the planned kernel -- every output tensor and the status words, bit for bit --
and against the oracle, over the inputs the CPU test settled (exact_shape_util.cases: T <= 40, B <= 8); the n_best route, a ragged
batch under length order; and the near misses, each of which must keep the planned kernel (and be refused in mode 1)."""
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


@pytest.mark.parametrize("kind", ["randn", "quant"])
def test_n_best_route_and_ragged_batch_under_length_order(torch_mod, kind):
    torch = torch_mod
    name = kind + "_ragged"
    lp, sl = [(l, s) for n, l, s in CASES if n == name][0]
    probs, lens = torch.from_numpy(lp).cuda(), torch.from_numpy(sl).cuda()
    dec = _decoder()
    dec.set_launch_order("length")
    on, st_on, ran = _run(torch, dec, probs, lens, -1)
    order = dec.last_launch_order()
    assert ran == 1 and order is not None and not np.array_equal(order, np.arange(len(sl)))
    off, st_off, ran0 = _run(torch, dec, probs, lens, 0)
    assert ran0 == 0 and all(torch.equal(a, b) for a, b in zip(on, off)) and torch.equal(st_on, st_off)
    _assert_oracle(on, xs.oracle(name, lp, sl), name + " length order, twin vs oracle:")
    for n in (1, 7):
        nb_on, st1, ran1 = _run(torch, dec, probs, lens, 1, n_best=n)
        nb_off, st2, ran2 = _run(torch, dec, probs, lens, 0, n_best=n)
        assert ran1 == 1 and ran2 == 0
        assert all(torch.equal(a, b) for a, b in zip(nb_on, nb_off)) and torch.equal(st1, st2)
        assert torch.equal(nb_on[0], on[0][:, :n]) and torch.equal(nb_on[1], on[1][:, :n]) and torch.equal(nb_on[3], on[3][:, :n])
    dec.set_launch_order("batch")
    dec.set_exact_shape(-1)
    host = dec.decode(probs, lens)  # (compact results to the host: the twin behind another entry point)
    assert dec.last_exact_shape() == 1
    assert all(torch.equal(a, b.cpu()) for a, b in zip(host, on))


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
