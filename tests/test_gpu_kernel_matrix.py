"""-m gpu: every instantiation of the decode kernel, launched and checked.  One case per item of CTC_KERNEL_LIST
(tests/kernel_matrix_util.py; test_abi.py proves the table covers the list): the decoder arguments and switches of the case must
launch exactly the expected kernel (ctcd_debug_last_kernel, read back from the pointer that was launched), and that kernel must decode
ragged batches with ties, degenerate frames and one-frame utterances bit for bit like the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_matrix_util as km
import oracle_util as ou
from test_gpu_decode import _with_nres

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def wide99(tmp_path_factory):
    from test_lm import make_wide_label_lm

    return make_wide_label_lm(tmp_path_factory.mktemp("kernel_matrix_lm"))


def _decoder(c, labels, lm, callback_scorer=None):
    import ctcdecode_amd
    from ctcdecode_amd import _native

    kw = dict(cutoff_top_n=c["top_n"], cutoff_prob=c["cutoff_prob"], beam_width=c["K"], blank_id=c["blank"], log_probs_input=True,
              device="cuda:0")
    if callback_scorer is not None:
        dec = ctcdecode_amd.CTCBeamDecoder(labels, scorer=callback_scorer, **kw)
    elif lm is not None:
        dec = ctcdecode_amd.CTCBeamDecoder(labels, model_path=lm[0], alpha=lm[2], beta=lm[3], **kw)
    else:
        dec = ctcdecode_amd.CTCBeamDecoder(labels, **kw)
    if c["threads"]:
        dec.set_threads(c["threads"])
    dec.set_subtree_search(c["subtree"])
    dec.set_cu_sharing(c["cu_sharing"])
    if not c["fixed"]:
        dec.set_fixed_layout(False)
    dec.set_host_path(input_streaming=c["streamed"])
    if c["profile"]:  # (as tools/phase_profile.py and tools/barrier_timeline.py do)
        _native.check(_native.lib.ctcd_debug_set_profile(dec._handle, 1))
    if c["profile"] == 2:
        _native.check(_native.lib.ctcd_debug_timeline(dec._handle, 0, min(8, c["T"]), None))
    assert dec.last_kernel() is None and dec.last_layout() == -1
    return dec


def _run(torch, dec, c, lp, sl):
    out, sc, ts, ln = dec.decode(torch.from_numpy(lp), torch.from_numpy(sl))
    assert dec.last_kernel() == c["kernel"], "launched %s, expected %s" % (dec.last_kernel(), c["kernel"])
    assert dec.last_layout() == km.expected_layout(c["kernel"])
    return dict(tokens=out.numpy(), timesteps=ts.numpy(), scores=sc.numpy(), lens=ln.numpy())


def _child_main(index, directory):
    """A streamed-input case's decode, in a process of its own (see _run_in_child)."""
    import torch

    c = km.CASES[index]
    z = np.load(os.path.join(directory, "in.npz"))
    dec = _decoder(c, [str(i) for i in range(c["V"])] if not c["lm"] else km.lm_spec(c)[1], km.lm_spec(c) if c["lm"] else None)
    out, sc, ts, ln = dec.decode(torch.from_numpy(z["lp"]), torch.from_numpy(z["sl"]))
    np.savez(os.path.join(directory, "out.npz"), tokens=out.numpy(), timesteps=ts.numpy(), scores=sc.numpy(), lens=ln.numpy(),
             kernel=np.array(dec.last_kernel() or (), np.int32), layout=np.int32(dec.last_layout()))


def _run_in_child(c, lp, sl, directory):
    """The streamed-input cases decode in a fresh process, so that what earlier tests did to this process cannot change the route.  In
    one run of the whole GPU suite, the first of these cases launched the plain kernel: its streamed rows had not reached the kernel in
    time, the call gave up on streaming after about a second and decoded again from rows copied up front (correct results, but not
    the twin under test; the fallback in ctcdecode_amd.hip ctcd_beam_decode_to_host).  The cause is not established -- twelve streams made
    in one process did not reproduce it.  The hook, read in the child, still catches such a fallback."""
    np.savez(os.path.join(directory, "in.npz"), lp=lp, sl=sl)
    tests = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_kernel_matrix as m; m._child_main(%d, %r)" % (
        tests, os.path.dirname(tests), km.CASES.index(c), directory)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    z = np.load(os.path.join(directory, "out.npz"))
    assert tuple(int(v) for v in z["kernel"]) == c["kernel"], "launched %s, expected %s" % (z["kernel"], c["kernel"])
    assert int(z["layout"]) == km.expected_layout(c["kernel"])
    return dict(tokens=z["tokens"], timesteps=z["timesteps"], scores=z["scores"], lens=z["lens"])


@pytest.mark.parametrize("c", km.CASES, ids=km.case_id)
def test_kernel_instantiation(torch_mod, wide99, monkeypatch, tmp_path, c):
    if c["general"]:  # (read when the decoder is created)
        monkeypatch.setenv("CTCD_GENERAL_LM_KERNEL", "1")
    lm = km.lm_spec(c, *wide99) if c["lm"] else None
    labels = lm[1] if lm else [str(i) for i in range(c["V"])]
    assert len(labels) == c["V"]
    lp, sl = km.inputs(c, labels)
    what = "%s %s" % (km.case_id(c), {k: v for k, v in c.items() if v not in (None, False, 0) and k != "kernel"})
    args = dict(beam=c["K"], cutoff_prob=c["cutoff_prob"], cutoff_top_n=c["top_n"], blank_id=c["blank"])
    if lm is None:
        wants = [ou.decode(lp, sl, which="restated", **args)]
        if ou.have_reference():
            wants.append(ou.decode(lp, sl, which="reference", **args))
        got = _run_in_child(c, lp, sl, str(tmp_path)) if c["streamed"] else _run(torch_mod, _decoder(c, labels, None), c, lp, sl)
        for want in wants:
            ou.assert_same(_with_nres(got, want), want, what)
        return
    want = ou.decode(lp, sl, scorer=ou.Scorer(lm[2], lm[3], lm[0], labels, "restated"), **args)
    if not c["callback"]:
        got = _run_in_child(c, lp, sl, str(tmp_path)) if c["streamed"] else _run(torch_mod, _decoder(c, labels, lm), c, lp, sl)
        ou.assert_same(_with_nres(got, want), want, what)
        return
    import ctcdecode_amd
    from test_gpu_lm import _BuiltinBehindCallback

    inner = _BuiltinBehindCallback(dict(labels=labels, lm_path=lm[0]))
    try:
        for wait in (True, False):  # (a launch that waits on the GPU for the answers, and a launch per round of misses)
            sc = ctcdecode_amd.CallbackScorer(inner, inner.vocabulary, inner.order, labels, alpha=lm[2], beta=lm[3], device="cuda:0")
            dec = _decoder(c, labels, lm, callback_scorer=sc)
            dec.set_scorer_wait(wait)
            got = _run(torch_mod, dec, c, lp, sl)
            ou.assert_same(_with_nres(got, want), want, what + " wait=%s" % wait)
            assert sc.callback_calls() > 0
    finally:
        inner.close()
