"""-m gpu: every pre-pass kernel instantiation, launched and checked against the reference.  One case per row of the build's pre-pass
table (tests/prepass_matrix_util.py; test_abi.py proves the cases cover the table exactly), plus the global-memory route of
prune_resolve_kernel per input dtype.  Each case must launch exactly the kernels the dispatch prescribes (ctcd_debug_last_prepass, read
back from the pointers that were launched); its vocabulary prune must equal the reference's get_pruned_log_probs frame by frame, bit for
bit (count, labels in order, float values; where oracle/_ref predates the per-frame entry, the restatement, which tests/test_oracle.py
pins to the reference: ou.have_reference_prune); its log-softmax rows must equal the host twin bit for bit and lie within a float64
bound; and its decode must equal the oracle."""
import numpy as np
import pytest

import oracle_util as ou
import prepass_matrix_util as pm
from test_gpu_decode import _with_nres

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _device_rows(torch, x, c):
    """x on the device in the case's dtype; a misaligned case gets a contiguous view one element past an aligned base (storage offset 1:
    4 bytes for float32, 2 for half rows), which .contiguous() does not copy."""
    dt = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[c["dt"]]
    rows = torch.from_numpy(x).to(device="cuda:0", dtype=dt)
    if not c["misaligned"]:
        return rows
    buf = torch.zeros(x.size + 8, dtype=dt, device="cuda:0")
    view = buf[1:1 + x.size].view(x.shape)
    view.copy_(rows)
    assert view.is_contiguous() and view.contiguous().data_ptr() == view.data_ptr()
    assert view.data_ptr() % (16 if c["dt"] == "f32" else 8) != 0
    return view


def _check_log_softmax(torch, dec, c, x, xt, sl, what):
    """The case's log-softmax kernel, run on its own through ctcd_log_softmax (the same dispatch): its rows equal the host twin bit for
    bit and a float64 log-softmax within rounding."""
    y = dec.log_softmax(xt, torch.from_numpy(sl)).cpu().numpy()
    assert dec.last_prepass() == dict(elementwise=None, log_softmax=pm.expected_prepass(c)["log_softmax"], prune=None, resolve=None)
    twin = ou.log_softmax_rows(x)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        x64 = x.astype(np.float64)
        m = x64.max(-1, keepdims=True)
        exact = x64 - m - np.log(np.exp(x64 - m).sum(-1, keepdims=True))
    tol = 2e-6 * (1 + np.log(c["V"]))
    for b in range(pm.B):
        for t in range(int(sl[b])):
            d = y[b, t].view(np.uint32) != twin[b, t].view(np.uint32)
            assert not d.any(), "%s log_softmax frame (%d, %d) differs from the host twin at %s" % (what, b, t, np.nonzero(d)[0][:6])
            ok = np.isfinite(exact[b, t])
            assert np.all(np.isneginf(y[b, t][~ok])), "%s frame (%d, %d)" % (what, b, t)
            # (relative to the row's spread: a row of logits near 9 +- 1e-3 has every value near -log V)
            err = np.abs(y[b, t][ok] - exact[b, t][ok]) / (1.0 + np.abs(exact[b, t][ok]))
            assert np.all(err <= tol), "%s frame (%d, %d): %g from a float64 log_softmax" % (what, b, t, err.max())


@pytest.mark.parametrize("c", pm.CASES, ids=pm.case_id)
def test_prepass_instantiation(torch_mod, c):
    import ctcdecode_amd
    import ctcdecode_amd._native as n

    torch = torch_mod
    V, K, li, top_n, cp = c["V"], c["K"], c["li"], c["top_n"], c["cp"]
    what = "%s %s" % (pm.case_id(c), {k: v for k, v in c.items() if k not in ("target", "seed")})
    x, sl, nans = pm.inputs(c)
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=K, cutoff_top_n=top_n, cutoff_prob=cp,
                                       log_probs_input=li == 1, logits_input=li == 2, device="cuda:0")
    assert dec.last_prepass() == dict(elementwise=None, log_softmax=None, prune=None, resolve=None)
    dec.set_fused_logits(c["fused"])
    dec.set_prune_registers(c["reg"])
    n.check(n.lib.ctcd_debug_set_prune_resolve(dec._handle, 0 if c["resolve_global"] else 1))
    xt = _device_rows(torch, x, c)
    assert np.array_equal(xt.float().cpu().numpy(), x, equal_nan=True)  # (the oracle reads exactly the rows the kernels widen)
    out, sc, ts, ln = dec.decode_device(xt, torch.from_numpy(sl))
    got = dict(tokens=out.cpu().numpy(), timesteps=ts.cpu().numpy(), scores=sc.cpu().numpy(), lens=ln.cpu().numpy())
    want_pp = pm.expected_prepass(c)
    assert dec.last_prepass() == want_pp, what
    assert c["target"] in want_pp.values()

    which = "reference" if ou.have_reference() else "restated"
    which_prune = "reference" if ou.have_reference_prune() else "restated"
    # the rows the prune read, as the oracle takes them: raw logits through the host twin of the log-softmax; a NaN (defined by the
    # library as below every number) as -inf / 0
    xo = ou.log_softmax_rows(x) if li == 2 else x.copy()
    for b, t, v in nans:
        xo[b, t, v] = 0.0 if li == 0 else -np.inf
    if want_pp["prune"]:
        rows = [b * pm.T + t for b in range(pm.B) for t in range(int(sl[b]))]
        got_rows = dec.last_prune_rows(pm.B * pm.T, min(top_n, V))
        ou.assert_same_pruned(got_rows, ou.pruned_rows(xo, cp, top_n, li != 0, which=which_prune), what, rows)
        if c["ties"]:
            assert n.lib.ctcd_last_prune_flagged_rows(dec._handle) > 0, "%s: no frame reached prune_resolve_kernel" % what
    if want_pp["log_softmax"]:
        _check_log_softmax(torch, dec, c, x, xt, sl, what)
    want = ou.decode(xo, sl, beam=K, cutoff_prob=cp, cutoff_top_n=top_n, log_input=li != 0, which=which)
    ou.assert_same(_with_nres(got, want), want, what)


def test_negative_cutoff_prob_keeps_top_n(torch_mod):
    """A negative cutoff_prob: the reference's log(cutoff_prob) is NaN, so it makes no cumulative cut and keeps cutoff_top_n candidates
    per frame.  (The library once took any cutoff_prob < 1 for a cut, and kept one candidate per frame.)"""
    import ctcdecode_amd

    torch = torch_mod
    V, top_n, K = 300, 40, 8
    x = ou.synth_logprobs(2, 20, V, 5)
    which = "reference" if ou.have_reference() else "restated"
    which_prune = "reference" if ou.have_reference_prune() else "restated"
    for cp in (-0.5, -1e-300, float("-inf")):
        dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=K, cutoff_top_n=top_n, cutoff_prob=cp, log_probs_input=True,
                                           device="cuda:0")
        out, sc, ts, ln = dec.decode(torch.from_numpy(x))
        cnt, lab, val = dec.last_prune_rows(40, top_n)
        assert np.all(cnt == top_n), (cp, cnt)
        ou.assert_same_pruned((cnt, lab, val), ou.pruned_rows(x, cp, top_n, True, which=which_prune), "cutoff_prob %r" % cp)
        want = ou.decode(x, beam=K, cutoff_prob=cp, cutoff_top_n=top_n, which=which)
        ou.assert_same(_with_nres(dict(tokens=out.numpy(), timesteps=ts.numpy(), scores=sc.numpy(), lens=ln.numpy()), want), want,
                       "cutoff_prob %r" % cp)
