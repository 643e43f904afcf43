"""-m gpu tests of the edit distance (``CTCBeamDecoder.edit_distance`` / ``mbr_select`` / ``ctcd_edit_distance``): device output == the
numpy restatement of the header's definition (tests/editdist_util.py), exactly, at the lengths where the kernel can go wrong.  The
cases are those of tests/test_editdist_host.py; a reference is computed once per process.  Launches through the C entry point write
into outputs full of sentinel words, over rows whose positions at and beyond their lengths hold a token no case uses."""
import editdist_util as eu
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def dec():
    import ctcdecode_amd

    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(8)], blank_id=0, beam_width=16, log_probs_input=True)


def _entry(torch, dec, x, x_lens, y=None, y_lens=None, status=True):
    """ctcd_edit_distance on numpy arrays, the output preset to sentinel words.  -> (rc, out, status, pairs of the call)."""
    from ctcdecode_amd import _native

    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()  # noqa: E731
    tx, txl, ty, tyl = dev(x), dev(x_lens), dev(y), dev(y_lens)
    B, R, L = tx.shape
    Q, Lq = (R, L) if ty is None else ty.shape[1:]
    out = torch.full((B, R, Q), eu.SENTINEL, dtype=torch.int32, device="cuda")
    st = torch.zeros((max(B, 1),), dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else (t.data_ptr() if t.numel() else st.data_ptr())  # noqa: E731  (an empty tensor has no address)
    rc = _native.lib.ctcd_edit_distance(dec._handle, ptr(tx), ptr(txl), B, R, L, ptr(ty), ptr(tyl), Q, Lq, out.data_ptr(), st.data_ptr() if status else None,
                                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), st.cpu().numpy()[:B], dec.last_edit_pairs()


def _check(torch, dec, c, what):
    want, want_status = eu.cached(("ref", what), lambda: eu.case_reference(c))
    rc, out, status, pairs = _entry(torch, dec, c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0, what
    bad = np.argwhere(out != want)
    assert bad.size == 0, "%s: differs at %s: got %s, want %s" % (what, bad[:4].tolist(), out[tuple(bad[0])], want[tuple(bad[0])])
    assert (status == want_status).all(), what
    B, R, Q = want.shape
    assert pairs == (B * R * (R - 1) // 2 if c["y"] is None else B * R * Q), what
    return want


@pytest.mark.parametrize("C", eu.CLASSES)
def test_device_equals_the_restatement_over_the_length_grid(torch_mod, dec, C):
    """One launch per class and role: strips of 0, 1, C - 1, C, C + 1, 63 C, 64 C - 1, 64 C and 64 C + 1 tokens against streamed rows of
    n, n + 1, n + 62 .. n + 65 and 3 n."""
    for swap in (False, True):
        _check(torch_mod, dec, eu.grid_case(C, swap), "grid %d %s" % (C, swap))


@pytest.mark.parametrize("C", eu.CLASSES)
def test_closed_forms(torch_mod, dec, C):
    cases = eu.closed_form_cases(C)
    x, xl = eu.pack_rows([a for _, a, _, _ in cases])
    y, yl = eu.pack_rows([b for _, _, b, _ in cases])
    for s, sl, t, tl in ((x, xl, y, yl), (y, yl, x, xl)):
        rc, out, _, _ = _entry(torch_mod, dec, s[:, None], sl[:, None], t[:, None], tl[:, None])
        assert rc == 0 and out[:, 0, 0].tolist() == [d for _, _, _, d in cases], [n for n, _, _, _ in cases]


def test_token_values_are_compared_as_values(torch_mod, dec):
    _check(torch_mod, dec, eu.token_value_case(), "token values")


def test_a_launch_mixing_every_class_and_empty_rows(torch_mod, dec):
    """B = 3, R = 40, Q = 5: the 600 pairs of a call whose rows run from 0 to 2048 (x) and 3000 (y) tokens."""
    c = eu.mixed_case()
    want = _check(torch_mod, dec, c, "mixed")
    assert {eu.klass(min(int(a), int(q))) for a in c["x_lens"][0] for q in c["y_lens"][0] if a and q} == set(eu.CLASSES)
    assert (want[0][c["x_lens"][0] == 0] == c["y_lens"][0][None, :]).all()


def _check_against(torch, dec, c, want, what):
    rc, out, status, _ = _entry(torch, dec, c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0, what
    bad = np.argwhere(out != want[0])
    assert bad.size == 0, "%s: differs at %s: got %s, want %s" % (what, bad[:4].tolist(), out[tuple(bad[0])], want[0][tuple(bad[0])])
    assert (status == want[1]).all(), what


@pytest.mark.parametrize("grid", (1, 2))
def test_the_persistent_loop_at_a_capped_grid(torch_mod, dec, grid):
    """``set_edit_grid``: four or eight waves take the mixed launch's 600 pairs in turn -- 150 or 75 trips of the loop each, from class to
    class and item to item -- then the same launch with a bad length in the middle item (x, then y), so that a wave's validity answer
    goes from good to bad and back; then pairwise mode over 40 rows, with and without a bad item."""
    try:
        dec.set_edit_grid(grid)
        c = eu.mixed_case()
        _check(torch_mod, dec, c, "mixed")
        assert dec.last_edit_grid() == grid and dec.last_edit_pairs() == 600 > 4 * grid
        for side, bad in (("x", 2049), ("y", -1)):
            d, want = eu.with_bad_length(c, "mixed", 1, bad, side)
            assert want[1].tolist() == [0, eu.BAD_ROW, 0] and (want[0][0] != 0).any() and (want[0][2] != 0).any()
            _check_against(torch_mod, dec, d, want, "mixed, bad %s length, grid %d" % (side, grid))
        p = eu.pairwise_case(40, B=3)
        _check(torch_mod, dec, p, "pairwise 40 x 3")
        d, want = eu.with_bad_length(p, "pairwise 40 x 3", 1, 151)
        _check_against(torch_mod, dec, d, want, "pairwise, bad item, grid %d" % grid)
        assert dec.last_edit_grid() == grid
    finally:
        dec.set_edit_grid(0)
    with pytest.raises(ValueError):
        dec.set_edit_grid(-1)


def test_more_pairs_than_waves_at_the_default_grid(torch_mod, dec):
    """10080 short pairs, several per wave of the default grid (two workgroups of four waves per compute unit), exact; then with a bad
    item between good ones."""
    c = eu.many_short_case()
    want = _check(torch_mod, dec, c, "many short")
    pairs, waves = dec.last_edit_pairs(), 4 * dec.last_edit_grid()
    assert pairs == 5 * 64 * 63 // 2 and 0 < waves and pairs >= 2 * waves, (pairs, waves)
    d, bad_want = eu.with_bad_length(c, "many short", 2, 25)
    assert (bad_want[0][1] == want[1]).all() and (bad_want[0][2] == 0).all()
    _check_against(torch_mod, dec, d, bad_want, "many short, bad item")


@pytest.mark.parametrize("R", (1, 2, 7, 40))
def test_pairwise_mode(torch_mod, dec, R):
    c = eu.pairwise_case(R)
    want = _check(torch_mod, dec, c, "pairwise %d" % R)
    B = want.shape[0]
    assert dec.last_edit_pairs() == B * R * (R - 1) // 2
    assert (want == want.transpose(0, 2, 1)).all() and (np.diagonal(want, axis1=1, axis2=2) == 0).all()
    rc, out, _, pairs = _entry(torch_mod, dec, c["x"], c["x_lens"], c["x"].copy(), c["x_lens"].copy())
    assert rc == 0 and (out == want).all() and pairs == B * R * R
    x = torch_mod.from_numpy(c["x"]).cuda()
    D = dec.edit_distance(x, torch_mod.from_numpy(c["x_lens"]).cuda())
    assert D.is_cuda and D.dtype == torch_mod.int32 and (D.cpu().numpy() == want).all()
    assert (dec.edit_distance(x, torch_mod.from_numpy(c["x_lens"]), x.clone(), torch_mod.from_numpy(c["x_lens"])).cpu().numpy() == want).all()


def test_the_limit(torch_mod, dec):
    torch = torch_mod
    want = _check(torch, dec, eu.limit_case(), "limit")
    assert want[0, 0, 0] == 2048
    x = torch.zeros((1, 1, 2049), dtype=torch.int32, device="cuda")
    lens = torch.full((1, 1), 2049, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        dec.edit_distance(x, lens, x.clone(), lens)
    with pytest.raises(NotImplementedError):
        dec.edit_distance(x, lens)
    long = torch.arange(5000, dtype=torch.int32, device="cuda").reshape(1, 1, 5000)
    short = torch.tensor([[[0, 1, 2, 3, 9, 5, 6, 7]]], dtype=torch.int32, device="cuda")
    n5000, n8 = torch.tensor([[5000]]), torch.tensor([[8]])
    assert dec.edit_distance(long, n5000, short, n8).item() == 4993 and dec.edit_distance(short, n8, long, n5000).item() == 4993


def test_bad_lengths(torch_mod, dec):
    torch = torch_mod
    c = eu.pairwise_case(7, B=3, L=40)
    for bad in (-1, 41):
        xl = c["x_lens"].copy()
        xl[1, 3] = bad
        want, want_status = eu.reference(c["x"], xl)
        rc, out, status, _ = _entry(torch, dec, c["x"], xl)
        assert rc == 0 and (out == want).all() and status.tolist() == [0, eu.BAD_ROW, 0]
        rc, out, _, _ = _entry(torch, dec, c["x"], xl, status=False)  # (no status tensor: the outputs alone)
        assert rc == 0 and (out == want).all()
        with pytest.raises(ValueError, match=r"items \[1\]"):
            dec.edit_distance(torch.from_numpy(c["x"]), torch.from_numpy(xl))
        y, yl = c["x"][:, :2].copy(), c["x_lens"][:, :2].copy()
        yl[2, 1] = bad
        want, want_status = eu.reference(c["x"], c["x_lens"], y, yl)
        rc, out, status, _ = _entry(torch, dec, c["x"], c["x_lens"], y, yl)
        assert rc == 0 and (out == want).all() and status.tolist() == [0, 0, eu.BAD_ROW]
        with pytest.raises(ValueError, match=r"items \[2\]"):
            dec.edit_distance(torch.from_numpy(c["x"]), torch.from_numpy(c["x_lens"]), torch.from_numpy(y), torch.from_numpy(yl))
    one = c["x"][:, :1], c["x_lens"][:, :1].copy()  # pairwise items of one row: no pair, and still validated
    one[1][2, 0] = 41
    rc, out, status, pairs = _entry(torch, dec, one[0], one[1])
    assert rc == 0 and (out == 0).all() and status.tolist() == [0, 0, eu.BAD_ROW] and pairs == 0


def test_degenerate_shapes(torch_mod, dec):
    torch = torch_mod
    from ctcdecode_amd import _native

    z = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")  # noqa: E731
    for (B, R, L), (Q, Lq) in (((0, 3, 4), (2, 4)), ((2, 0, 4), (2, 4)), ((2, 3, 4), (0, 4))):
        D = dec.edit_distance(z(B, R, L), z(B, R), z(B, Q, Lq), z(B, Q))
        assert tuple(D.shape) == (B, R, Q) and dec.last_edit_pairs() == 0
    assert tuple(dec.edit_distance(z(0, 3, 4), z(0, 3)).shape) == (0, 3, 3) and tuple(dec.edit_distance(z(2, 0, 4), z(2, 0)).shape) == (2, 0, 0)
    yl = torch.tensor([[3, 0], [1, 4]], dtype=torch.int32)
    D = dec.edit_distance(z(2, 3, 0), z(2, 3), torch.ones((2, 2, 4), dtype=torch.int32), yl)
    assert (D.cpu() == yl[:, None, :].expand(2, 3, 2)).all()  # L == 0: the other side's lengths
    D = dec.edit_distance(torch.ones((2, 2, 4), dtype=torch.int32), yl, z(2, 3, 0), z(2, 3))
    assert (D.cpu() == yl[:, :, None].expand(2, 2, 3)).all()  # Lq == 0
    assert (dec.edit_distance(z(2, 3, 0), z(2, 3)).cpu() == 0).all()
    x, xl, out = z(2, 3, 4), z(2, 3), z(2, 3, 3)
    s = torch.cuda.current_stream().cuda_stream
    fn = _native.lib.ctcd_edit_distance
    p = lambda t: t.data_ptr()  # noqa: E731
    assert fn(dec._handle, p(x), p(xl), -1, 3, 4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, -3, 4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, -4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, 4, p(x), p(xl), -1, 4, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, 4, p(x), p(xl), 3, -4, p(out), None, s) == -1
    assert fn(dec._handle, None, p(xl), 2, 3, 4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), None, 2, 3, 4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, 4, None, None, 0, 0, None, None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, 4, p(x), None, 3, 4, p(out), None, s) == -1
    assert fn(None, p(x), p(xl), 2, 3, 4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, 4, None, None, 0, 0, p(out), None, s) == 0
    torch.cuda.synchronize()


def test_tensor_handling(torch_mod, dec):
    """CPU and int64 inputs, a [B, Lq] reference with [B] lengths, non-contiguous views."""
    torch = torch_mod
    c = eu.pairwise_case(7, B=3, L=40)
    y, yl = c["x"][:, 1].copy(), c["x_lens"][:, 1].copy()  # [B, Lq], [B]
    want, _ = eu.reference(c["x"], c["x_lens"], y[:, None], yl[:, None])
    x64, xl64 = torch.from_numpy(c["x"]).long(), torch.from_numpy(c["x_lens"]).long()
    D = dec.edit_distance(x64, xl64, torch.from_numpy(y).to(torch.int16), torch.from_numpy(yl))
    assert not D.is_cuda and D.dtype == torch.int32 and tuple(D.shape) == (3, 7, 1) and (D.numpy() == want).all()
    D = dec.edit_distance(x64.cuda(), xl64, torch.from_numpy(y), torch.from_numpy(yl).cuda())
    assert D.is_cuda and (D.cpu().numpy() == want).all()
    wide = torch.full((3, 7, 80), eu.GARBAGE, dtype=torch.int32, device="cuda")
    wide[:, :, ::2] = torch.from_numpy(c["x"]).cuda()
    view, lens_view = wide[:, :, ::2], torch.from_numpy(np.ascontiguousarray(c["x_lens"].T)).cuda().t()
    assert not view.is_contiguous() and not lens_view.is_contiguous()
    want_pw, _ = eu.reference(c["x"], c["x_lens"])
    assert (dec.edit_distance(view, lens_view).cpu().numpy() == want_pw).all()
    ref_view = wide[:, 1, ::2]
    assert (dec.edit_distance(view, lens_view, ref_view, torch.from_numpy(yl)).cpu().numpy() == want).all()
    import ctcdecode

    assert ctcdecode.CTCBeamDecoder.edit_distance is type(dec).edit_distance and ctcdecode.CTCBeamDecoder.mbr_select is type(dec).mbr_select


def test_end_to_end_on_a_decode(torch_mod):
    """decode_device(n_best=10) on a small random batch, then the rows against the greedy row and against each other."""
    torch = torch_mod
    import ctcdecode_amd

    V, B, T = 8, 4, 60
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=0, beam_width=16, log_probs_input=True)
    rng = np.random.default_rng(5)
    z = rng.standard_normal((B, T, V)) * 2.0
    lp = torch.from_numpy((z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)).cuda()
    seq = torch.tensor([60, 41, 17, 0], dtype=torch.int32)
    tokens, _, _, lens = dec.decode_device(lp, seq, n_best=10)
    g_tok, _, _, g_len = dec.greedy_decode_device(lp, seq)
    D = dec.edit_distance(tokens, lens, g_tok, g_len)
    P = dec.edit_distance(tokens, lens)
    tn, ln, gt, gl = tokens.cpu().numpy(), lens.cpu().numpy(), g_tok.cpu().numpy(), g_len.cpu().numpy()
    assert tuple(D.shape) == (B, 10, 1) and tuple(P.shape) == (B, 10, 10) and ln[:3].max() > 0
    assert (D.cpu().numpy() == eu.reference(tn, ln, gt, gl)[0]).all()
    assert (P.cpu().numpy() == eu.reference(tn, ln)[0]).all()


def _mbr_check(torch, dec, x, xl, lw):
    index, risk = dec.mbr_select(torch.from_numpy(x).cuda(), torch.from_numpy(xl).cuda(), torch.from_numpy(lw).cuda())
    assert index.is_cuda and index.dtype == torch.int64 and risk.dtype == torch.float64 and tuple(risk.shape) == lw.shape
    index, risk = index.cpu().numpy(), risk.cpu().numpy()
    D, _ = eu.reference(x, xl)
    want_index, want_risk = eu.mbr_reference(D, lw)
    R = lw.shape[1]
    for b in range(lw.shape[0]):
        live = np.isfinite(lw[b])
        assert (np.isinf(risk[b][~live]) & (risk[b][~live] > 0)).all()
        if not live.any():
            assert index[b] == -1 and want_index[b] == -1
            continue
        bound = R * 2.0 ** -52 * want_risk[b][live].max()  # the summation-order error of at most R non-negative terms
        err = np.abs(risk[b][live] - want_risk[b][live]).max()
        print("item %d: risk error %.3g, bound %.3g" % (b, err, bound))
        assert err <= bound
        assert live[index[b]] and want_risk[b][index[b]] <= want_risk[b][live].min() + bound
    return index, risk, want_index


def test_mbr_select(torch_mod, dec):
    torch = torch_mod
    c = eu.pairwise_case(40, B=3, L=150)
    rng = np.random.default_rng(9)
    lw = (-5.0 * rng.random((3, 40))).astype(np.float64)
    lw[0, ::3] = -np.inf
    lw[1, 0] = -np.inf
    lw[2] = -np.inf  # an item without a finite weight
    index, risk, _ = _mbr_check(torch, dec, c["x"], c["x_lens"], lw)
    assert index[2] == -1 and np.isinf(risk[2]).all() and index[0] % 3 != 0 and index[1] != 0
    # CPU tensors in, CPU tensors out
    i2, r2 = dec.mbr_select(torch.from_numpy(c["x"]), torch.from_numpy(c["x_lens"]), torch.from_numpy(lw))
    assert not i2.is_cuda and not r2.is_cuda and (i2.numpy() == index).all()


def test_mbr_prefers_the_consensus_to_the_top_weight_outlier(torch_mod, dec):
    """Three rows: two near-identical ones of weight 0.3 each and an outlier of weight 0.4.  The outlier has the top weight; its expected
    distance to the others is the greatest."""
    torch = torch_mod
    a = np.arange(1, 21, dtype=np.int32)
    b = a.copy()
    b[10] = 99  # one substitution away from a
    o = np.arange(101, 113, dtype=np.int32)  # shares nothing with them
    x, xl = eu.pack_rows([o, a, b])
    lw = np.log(np.asarray([[0.4, 0.3, 0.3]], np.float64))
    index, risk, want_index = _mbr_check(torch, dec, x[None], xl[None], lw)
    # 0.6 * 20 = 12 for the outlier against 0.4 * 20 + 0.3 = 8.3 for each of the other two; of equal risks the smaller index
    assert int(np.argmax(lw[0])) == 0 and risk[0, 0] > max(risk[0, 1], risk[0, 2])
    assert index[0] == (1 if risk[0, 1] <= risk[0, 2] else 2) and want_index[0] in (1, 2)
