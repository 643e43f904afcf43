"""-m gpu tests of the log-likelihood gradient (``CTCBeamDecoder.log_likelihood_grad`` / ``differentiable_log_likelihood`` /
``ctcd_ctc_loglik_grad``): the device against the float64 numpy forward-backward of tests/loglik_grad_util.py -- and, through autograd
in logits mode, against ``torch.nn.functional.ctc_loss`` in float64 on the CPU -- within eight times the float32 reference's own
deviation on the same inputs (loglik_grad_util.BOUND), and against itself bit for bit where the header promises bits."""
import loglik_grad_util as gu
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

    if not kw:
        kw["log_probs_input"] = True
    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, beam_width=8, **kw)


def _grad(torch, dec, c, tokens=None, lens=None, weights=None):
    """-> (grad, loglik) of dec.log_likelihood_grad on the case's float32 log-probabilities, as numpy arrays."""
    tokens, lens = c["tokens"] if tokens is None else tokens, c["lens"] if lens is None else lens
    weights = c["weights"] if weights is None else weights
    grad, ll = dec.log_likelihood_grad(torch.from_numpy(c["lp"]).cuda(), torch.from_numpy(c["seq_lens"]), torch.from_numpy(tokens).cuda(),
                                       torch.from_numpy(lens).cuda(), torch.from_numpy(weights))
    assert grad.dtype == ll.dtype == torch.float32 and tuple(grad.shape) == c["lp"].shape and tuple(ll.shape) == lens.shape
    return grad.cpu().numpy(), ll.cpu().numpy()


def _check(c, grad, ll, bound, what):
    """grad within ``bound`` of the float64 reference; the sum rule; loglik's -inf where the reference's are."""
    ref = c["ref"]
    dev = np.abs(grad.astype(np.float64) - ref["grad"]).max()
    print("%s: max |device - float64| = %.3e (bound %.3e)" % (what, dev, bound))
    assert dev <= bound, what
    assert np.array_equal(np.isfinite(ll), np.isfinite(ref["loglik"])), what
    for b, n in enumerate(c["seq_lens"]):
        assert not grad[b, n:].any(), (what, b, "frames beyond the item")
        nnz = (grad[b, :n] != 0).sum(-1)
        assert np.all(np.abs(grad[b, :n].astype(np.float64).sum(-1) - ref["weight_sum"][b]) <= nnz * bound), (what, b, "the sum rule")


@pytest.mark.parametrize("R", (1, 3))
@pytest.mark.parametrize("V", (5, 300))
@pytest.mark.parametrize("L", gu.ROW_LS)
def test_against_float64(torch_mod, L, V, R):
    """S = 63, 65, 255, 257, 1023, 1025: both sides of the one-wave, 1, 4 and 16 states-per-lane classes; V = 5: long chains; V = 300:
    short ones; weights (1.5, -2.0, 0.0)."""
    c = gu.rows_case(L, V, R)
    grad, ll = _grad(torch_mod, _dec(V), c)
    _check(c, grad, ll, gu.BOUND["rows_V%d" % V], "L=%d V=%d R=%d" % (L, V, R))


def test_every_class_in_one_launch_and_the_bits(torch_mod):
    """Rows of every class in one call, against float64; then what the header promises bit for bit: loglik is log_likelihood's, a
    second call and a call with the scratch cut down to one slot change nothing, and weights (1, 0, 0) give the call on row 0 alone."""
    torch = torch_mod
    c = gu.mixed_case()
    dec = _dec(300)
    grad, ll = _grad(torch, dec, c)
    _check(c, grad, ll, gu.BOUND["mixed"], "mixed")
    want_ll = dec.log_likelihood(torch.from_numpy(c["lp"]).cuda(), torch.from_numpy(c["seq_lens"]), torch.from_numpy(c["tokens"]).cuda(),
                                 torch.from_numpy(c["lens"]).cuda()).cpu().numpy()
    assert np.array_equal(ll.view(np.uint32), want_ll.view(np.uint32))
    again, _ = _grad(torch, dec, c)
    assert np.array_equal(grad.view(np.uint32), again.view(np.uint32)), "the same call twice"
    grid = dec.last_posterior_grid()
    dec.set_posterior_scratch(1)
    one, ll_one = _grad(torch, dec, c)
    assert grid > 1 and dec.last_posterior_grid() == 1
    dec.set_posterior_scratch(0)
    assert np.array_equal(grad.view(np.uint32), one.view(np.uint32)) and np.array_equal(ll.view(np.uint32), ll_one.view(np.uint32)), "one slot"
    w100 = np.tile(np.asarray((1.0, 0.0, 0.0), np.float32), (len(c["lens"]), 1))
    three, _ = _grad(torch, dec, c, weights=w100)
    first, _ = _grad(torch, dec, c, tokens=c["tokens"][:, :1].copy(), lens=c["lens"][:, :1].copy(), weights=w100[:, :1].copy())
    assert first.any() and np.array_equal(three.view(np.uint32), first.view(np.uint32)), "weights (1, 0, 0)"


def test_edge_rows(torch_mod):
    """No frames, one frame, a row longer than its item, an empty row (the blank's column only), a repeated label, a whole frame of -inf;
    then an invalid row: ValueError, its item's word of status alone, and every bit of grad as with the row valid and its weight 0."""
    import ctcdecode_amd._native as native

    torch = torch_mod
    c = gu.edges_case()
    dec = _dec(6, c["blank"])
    grad, ll = _grad(torch, dec, c)
    _check(c, grad, ll, gu.BOUND["edges"], "edges")
    assert not grad[0].any() and not grad[5].any() and not np.isfinite(ll[2, 0])
    only_blank = np.delete(grad[3], c["blank"], axis=1)
    w0 = c["weights"].copy()
    w0[3, 1] = 0.0  # (the empty row alone)
    alone, _ = _grad(torch, dec, c, weights=w0)
    assert only_blank.any() and not np.delete(alone[3], c["blank"], axis=1).any() and np.all(np.abs(alone[3, :, c["blank"]] - 1.0) <= gu.BOUND["edges"])
    w0 = c["weights"].copy()
    w0[4, 0] = 0.0
    want, _ = _grad(torch, dec, c, weights=w0)
    bad = c["tokens"].copy()
    bad[4, 0, 1] = 6  # (a label == V)
    with pytest.raises(ValueError, match=r"items \[4\].*CTCD_ALIGN_BAD_ROW"):
        _grad(torch, dec, c, tokens=bad)
    # the same call through the C ABI, which leaves the outputs to look at
    lp, seq = torch.from_numpy(c["lp"]).cuda(), torch.from_numpy(c["seq_lens"]).cuda()
    tok, lens = torch.from_numpy(bad).cuda().permute(1, 0, 2).contiguous(), torch.from_numpy(c["lens"]).cuda().t().contiguous()
    w = torch.from_numpy(c["weights"]).cuda().t().contiguous()
    out, out_ll, status = torch.empty_like(lp), torch.empty((2, 6), device="cuda"), torch.zeros(6, dtype=torch.int32, device="cuda")
    native.check(native.lib.ctcd_ctc_loglik_grad(dec._handle, lp.data_ptr(), seq.data_ptr(), 6, 12, 6, c["blank"], 1, tok.data_ptr(), lens.data_ptr(), w.data_ptr(),
                                                 2, tok.shape[2], out.data_ptr(), out_ll.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream))
    assert status.tolist() == [0, 0, 0, 0, gu.BAD_ROW, 0]
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    after, _ = _grad(torch, dec, c)
    assert np.array_equal(after.view(np.uint32), grad.view(np.uint32)), "the decoder afterwards"


@pytest.mark.parametrize("mode", ("logp", "prob", "logits"))
@pytest.mark.parametrize("dtype", ("float32", "float16", "bfloat16"))
def test_modes_and_element_types_through_autograd(torch_mod, dtype, mode):
    """differentiable_log_likelihood(...).sum().backward() against the float64 reference on the widened input, chain rule included; in
    logits mode also against ctc_loss in float64 on the CPU.  The gradient arrives in the input's element type: one rounding, a unit
    roundoff u of 2^-24, 2^-11 or 2^-8 relative (and float16's subnormal spacing), is added to the bound."""
    torch = torch_mod
    dt, u = {"float32": (torch.float32, 2.0 ** -24), "float16": (torch.float16, 2.0 ** -11), "bfloat16": (torch.bfloat16, 2.0 ** -8)}[dtype]
    c = gu.modes_case()
    x = torch.from_numpy(gu.mode_input(c["x"], mode, lambda v: v)).to(dt).cuda().requires_grad_()
    seq, tok, lens = torch.from_numpy(c["seq_lens"]), torch.from_numpy(c["tokens"]).cuda(), torch.from_numpy(c["lens"]).cuda()
    dec = _dec(29, **{"logp": dict(log_probs_input=True), "prob": dict(log_probs_input=False), "logits": dict(logits_input=True)}[mode])
    ll = dec.differentiable_log_likelihood(x, seq, tok, lens)
    ll.sum().backward()
    assert x.grad.dtype == dt and tuple(x.grad.shape) == tuple(x.shape)
    wide = x.detach().double().cpu()
    ref = gu.mode_gradient(wide.numpy(), mode, c["seq_lens"], c["tokens"], c["lens"], np.ones(c["lens"].shape), c["blank"])
    got = x.grad.double().cpu().numpy()
    bound = gu.BOUND["modes_" + mode]
    dev = np.abs(got - ref["grad"])
    print("%s %s: max |device - float64| = %.3e (bound %.3e + rounding)" % (dtype, mode, dev.max(), bound))
    assert np.all(dev <= bound + u * (np.abs(ref["grad"]) + bound) + 2.0 ** -25)
    if mode == "logits":
        xs = wide.clone().requires_grad_()
        lp = torch.log_softmax(xs, -1).transpose(0, 1)
        sum(-torch.nn.functional.ctc_loss(lp, tok[:, r].cpu().long(), seq.long(), lens[:, r].cpu().long(), blank=c["blank"], reduction="sum")
            for r in range(2)).backward()
        assert np.all(np.abs(got - xs.grad.numpy()) <= bound + u * (np.abs(xs.grad.numpy()) + bound) + 2.0 ** -25)
