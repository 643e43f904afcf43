"""-m gpu: every instantiation <DT, PROB, CLS> of the align, log-likelihood and posterior kernels, run and compared with the
restatements of the header's definitions bit for bit -- floats as uint32, spans and peaks exactly (tests/lattice_matrix_util.py).

  matrix       one launch with rows of all four classes (tests/test_lattice_matrix_host.py proves the census), over values that float32,
               float16 and bfloat16 hold exactly: feature x element type x input mode = 18 tests of four kernels each, 72 instantiations;
               and the same launch squeezed into one scratch slot / one workgroup
  max_states   S = 4095, the limit: one alignment through every lane and all three wave hand-overs, against its closed form
  third_wave   S = 2061 with many alignments: real states in the workgroup's third wave
  big_vocab    V = 70001: labels beyond 2^8 and 2^16, byte offsets up to 280000, a frame's gathers in different cache lines

The references are those of tests/test_lattice_matrix_host.py, computed once per process."""
import align_util as au
import lattice_matrix_util as mu
import numpy as np
import posterior_util as pu
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _references_released_afterwards():
    """The cases and their references live for this module's tests only: the tests that run after it find the process as it was."""
    yield
    import gc

    mu.release()
    gc.collect()


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


def _dec(V, blank=0, **kw):
    import ctcdecode_amd

    kw.setdefault("log_probs_input", True)
    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, beam_width=8, **kw)


def _device_rows(torch, x, dtype="float32"):
    """x as a HIP tensor of the element type; the tensor widened back is what the reference was computed on."""
    rows = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda().to(getattr(torch, dtype))
    assert rows.is_cuda and rows.dtype == getattr(torch, dtype)
    return rows


def _run(torch, dec, feature, rows, c):
    """Every output of the feature's Python front end on the case's labels, as numpy arrays (a raised status word raises there)."""
    seq = None if c["seq_lens"] is None else torch.from_numpy(c["seq_lens"])
    tok, lens = torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()
    if feature == "align":
        outs, keys = dec.align(rows, seq, tok, lens), ("start", "end", "scores")
    elif feature == "loglik":
        outs, keys = (dec.log_likelihood(rows, seq, tok, lens),), ("loglik",)
    else:
        outs, keys = dec.label_posteriors(rows, seq, tok, lens), pu.KEYS
    assert len(outs) == len(keys) and all(o.is_cuda for o in outs)
    return dict(zip(keys, (o.cpu().numpy() for o in outs)))


def _same_bits(got, other, what):
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), other[k].view(np.uint32)), (what, k)


@pytest.mark.parametrize("mode", mu.MODES)
@pytest.mark.parametrize("dtype", mu.DTYPES)
@pytest.mark.parametrize("feature", mu.FEATURES)
def test_every_instantiation_on_the_matrix(torch_mod, feature, dtype, mode):
    """One launch = the kernels <dtype, mode, 0 / 1 / 4 / 16>, each with rows of its own; every output against the restatement."""
    torch = torch_mod
    c = mu.case("matrix")
    want = mu.want("matrix", feature, mode)
    x = c["lp"] if mode == "log" else c["p"]
    rows = _device_rows(torch, x, dtype)
    assert np.array_equal(rows.float().cpu().numpy().view(np.uint32), x.view(np.uint32)), "the element type holds the values exactly"
    dec = _dec(x.shape[2], c["blank"], log_probs_input=mode == "log")
    mu.ASSERT_SAME[feature](_run(torch, dec, feature, rows, c), want, "matrix %s %s %s" % (feature, dtype, mode))
    print("reference times (s):", {k: round(v, 2) for k, v in mu.TIMES.items()})


@pytest.mark.parametrize("feature", mu.FEATURES)
def test_one_slot_and_one_workgroup_on_the_matrix(torch_mod, feature):
    """The scratch budget at exactly one slot (align, posteriors) and the grid cap at 1 (log-likelihood): one workgroup runs the class-16
    row, the class-4 rows and the class-1 rows one after the other in the same slot, each with a row pitch of its own.  The bits are the
    default run's, and the restatement's."""
    torch = torch_mod
    c = mu.case("matrix")
    T, Ls = c["lp"].shape[1], c["tokens"].shape[2]
    dec = _dec(c["lp"].shape[2], c["blank"])
    rows = _device_rows(torch, c["lp"])
    squeeze, last = {"align": (lambda on: dec.set_align_scratch(au.host_slot_bytes(T, Ls) if on else 0), dec.last_align_grid),
                     "loglik": (lambda on: dec.set_loglik_grid(1 if on else 0), dec.last_loglik_grid),
                     "posteriors": (lambda on: dec.set_posterior_scratch(pu.host_slot_bytes(T, Ls) if on else 0), dec.last_posterior_grid)}[feature]
    full = _run(torch, dec, feature, rows, c)
    assert last() > 1, "the default run spreads the rows over workgroups"
    squeeze(True)
    try:
        one = _run(torch, dec, feature, rows, c)
        assert last() == 1
    finally:
        squeeze(False)
    again = _run(torch, dec, feature, rows, c)
    assert last() > 1, "the default is back"
    _same_bits(one, full, "one slot")
    _same_bits(again, full, "the default restored")
    mu.ASSERT_SAME[feature](one, mu.want("matrix", feature, "log"), "matrix %s in one slot" % feature)


@pytest.mark.parametrize("dtype", mu.DTYPES)
@pytest.mark.parametrize("feature", mu.FEATURES)
def test_the_limit(torch_mod, feature, dtype):
    """max_states: two rows of L = n = 2047 labels, S = 4095.  The only alignment is in state 2t + 1 at frame t: it crosses every lane
    and all three wave boundaries, the reversed labels fill 2047 of the stage's 2048 words, and a posterior row takes the largest slot
    there is (2047 x 4095 floats)."""
    torch = torch_mod
    c = mu.case("max_states")
    assert mu.exact_in(c["lp"], dtype)
    dec = _dec(c["lp"].shape[2], c["blank"])
    got = _run(torch, dec, feature, _device_rows(torch, c["lp"], dtype), c)
    if feature == "posteriors":
        assert dec.last_posterior_grid() == 2
    mu.ASSERT_SAME[feature](got, mu.max_states_expected()[feature], "max_states %s %s" % (feature, dtype))


@pytest.mark.parametrize("feature", mu.FEATURES)
def test_the_third_wave(torch_mod, feature):
    """third_wave: L = 1030 in 1040 frames, S = 2061 -- many alignments, and states 2048 .. 2060 on lane 128."""
    torch = torch_mod
    c = mu.case("third_wave")
    want = mu.want("third_wave", feature)
    print("reference time (s): %.2f" % mu.TIMES[("third_wave", feature, "log")])
    dec = _dec(c["lp"].shape[2], c["blank"])
    mu.ASSERT_SAME[feature](_run(torch, dec, feature, _device_rows(torch, c["lp"]), c), want, "third_wave " + feature)


@pytest.mark.parametrize("variant", ["log", "prob", "float16", "bfloat16"])
@pytest.mark.parametrize("feature", mu.FEATURES)
def test_the_wide_vocabulary(torch_mod, feature, variant):
    """big_vocab: V = 70001, blank 69999, labels 1, 2, 255, 256, 65535, 65536, 65537 and 70000 -- on float32 rows, on probabilities,
    and on float16 / bfloat16 copies, whose reference is the restatement on the copy widened back."""
    torch = torch_mod
    c = mu.case("big_vocab")
    if variant in ("log", "prob"):
        want = mu.want("big_vocab", feature, variant)
        rows = _device_rows(torch, c["lp"] if variant == "log" else c["p"])
    else:
        rows = _device_rows(torch, c["lp"], variant)
        want = mu.reference_on("big_vocab", feature, variant + " as the device rounds it", rows.float().cpu().numpy())
    finite = want["scores"] if feature == "align" else want["loglik"]
    assert np.isfinite(finite).sum() >= 8 and np.isfinite(finite[0, 0]), "rows with alignments, the one of all eight labels among them"
    dec = _dec(c["lp"].shape[2], c["blank"], log_probs_input=variant != "prob")
    mu.ASSERT_SAME[feature](_run(torch, dec, feature, rows, c), want, "big_vocab %s %s" % (feature, variant))
