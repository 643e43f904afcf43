"""-m gpu: the prune's std::sort replay (prune_resolve_kernel -> stl_emul.h sort_prefix_parallel / sort_parallel) driven into its
depth-limit heap fallbacks by rows only an adversary builds (tests/prune_adversary_util.py; test_prune_adversary.py certifies on the CPU
what each row makes the replay do).  Every case: the device's per-frame prune -- count, labels in order, value bits -- equals the
reference's get_pruned_log_probs (the restatement where oracle/_ref lacks the per-frame entry), the short decode equals the oracle, the
kernels launched are the ones the dispatch prescribes, nothing goes to the host, and at least the frames that tie across the cut are
flagged for the replay (nothing else can settle those)."""
import numpy as np
import pytest

import oracle_util as ou
import prepass_matrix_util as pm
import prune_adversary_util as pa
from test_gpu_decode import _with_nres
from test_gpu_prepass_matrix import _device_rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _decoder(V, top_n, cp, li, resolve_global, reg=True, fused=True):
    import ctcdecode_amd
    import ctcdecode_amd._native as n

    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=pa.K, cutoff_top_n=top_n, cutoff_prob=cp,
                                       log_probs_input=li == 1, logits_input=li == 2, device="cuda:0")
    dec.set_fused_logits(fused)
    dec.set_prune_registers(reg)
    n.check(n.lib.ctcd_debug_set_prune_resolve(dec._handle, 0 if resolve_global else 1))  # (0: the sort's arrays in global memory)
    return dec


def _oracles():
    return "reference" if ou.have_reference() else "restated", "reference" if ou.have_reference_prune() else "restated"


def _run_and_check(torch, dec, xt, xo, sl, V, top_n, cp, li, min_flagged, what):
    """One call: per-frame prune and decode against the oracles; the replay's bookkeeping."""
    import ctcdecode_amd._native as n

    Bc, Tc = xo.shape[:2]
    out, sc, ts, ln = dec.decode_device(xt, torch.from_numpy(sl) if sl is not None else None)
    got = dict(tokens=out.cpu().numpy(), timesteps=ts.cpu().numpy(), scores=sc.cpu().numpy(), lens=ln.cpu().numpy())
    which, which_prune = _oracles()
    rows = pa.live_rows(sl if sl is not None else [Tc] * Bc, Tc)
    got_rows = dec.last_prune_rows(Bc * Tc, min(top_n, V))
    ou.assert_same_pruned(got_rows, ou.pruned_rows(xo, cp, top_n, li != 0, which=which_prune), what, rows)
    assert n.lib.ctcd_last_prune_host_rows(dec._handle) == 0
    flagged = n.lib.ctcd_last_prune_flagged_rows(dec._handle)
    assert flagged >= min_flagged, "%s: %d frames flagged, %d tie across the cut" % (what, flagged, min_flagged)
    want = ou.decode(xo, sl, beam=pa.K, cutoff_prob=cp, cutoff_top_n=top_n, log_input=li != 0, which=which)
    ou.assert_same(_with_nres(got, want), want, what)
    return flagged


@pytest.mark.parametrize("c", pa.CASES, ids=pa.case_id)
def test_adversarial_rows(torch_mod, c):
    torch = torch_mod
    V, top_n, cp, li = c["V"], c["top_n"], c["cp"], c["li"]
    what = pa.case_id(c)
    x, xo, shift = pa.inputs(c)
    certs = pa.certificates(c)
    sl = pa.SEQ_LENS
    dec = _decoder(V, top_n, cp, li, c["resolve_global"], c["reg"], c["fused"])
    xt = _device_rows(torch, np.array(x), c)
    assert np.array_equal(xt.float().cpu().numpy(), x)  # (the oracle reads exactly the rows the kernels widen)
    ties = sum(certs[b][t]["tie_at_cut"] for b in range(pa.B) for t in range(int(sl[b])))
    # (two equal best labels: float32 rows flag every tie inside the kept labels, half rows do when there is no cumulative cut)
    if c["tie_top"] and cp >= 1.0:
        ties = int(sl.sum())
    _run_and_check(torch, dec, xt, np.array(xo), sl, V, top_n, cp, li, ties, what)
    assert dec.last_prepass() == pm.expected_prepass(c), what


@pytest.mark.parametrize("c", pa.CARRY, ids=lambda c: "frames%d_%s" % (c["frames"], "far" if c["resolve_global"] else "lds"))
def test_state_carried_from_row_to_row(torch_mod, c):
    """More flagged frames than the replay has workgroups: a workgroup goes from a heap-sorted row straight into a benign or a constant one
    (bstack, the task lists and the counters start over).  Once whole, once with seq_lens that leave out frames, killer rows among them."""
    torch = torch_mod
    x, kinds = pa.carry_inputs(c)
    Tc = x.shape[1]
    dec = _decoder(c["V"], c["top_n"], 1.0, 1, c["resolve_global"])
    xt = torch.from_numpy(x).to("cuda:0")
    flagged = _run_and_check(torch, dec, xt, x, None, c["V"], c["top_n"], 1.0, 1, c["frames"], "carry, whole")
    assert flagged == c["frames"] > (64 if c["resolve_global"] else 256)
    assert dec.last_prepass()["resolve"] == ("resolve", 0, int(c["resolve_global"]), "f32")
    sl = np.array([Tc, Tc - Tc // 3], np.int32)
    assert "adversarial" in kinds[1][int(sl[1]):]
    _run_and_check(torch, dec, xt, x, sl, c["V"], c["top_n"], 1.0, 1, int(sl.sum()), "carry, seq_lens %s" % sl)
