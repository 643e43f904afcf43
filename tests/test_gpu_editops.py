"""-m gpu tests of the edit operations (``CTCBeamDecoder.edit_counts`` / ``edit_align``, ``ctcd_edit_counts`` / ``ctcd_edit_align``): device
output == the restatement of the header's definition (tests/editops_util.py), exactly, at the lengths where the kernels can go wrong.
The cases are those of tests/test_editops_host.py; a reference is computed once per process and shared.  Launches through the C entry
points write into outputs full of sentinel words, over rows whose positions at and beyond their lengths hold a token no case uses."""
import editdist_util as eu
import editops_util as ou
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


def _device(torch, x, x_lens, y, y_lens):
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()  # noqa: E731
    tx, txl, ty, tyl = dev(x), dev(x_lens), dev(y), dev(y_lens)
    B, R, L = tx.shape
    Q, Lq = (R, L) if ty is None else ty.shape[1:]
    st = torch.zeros((max(B, 1),), dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else (t.data_ptr() if t.numel() else st.data_ptr())  # noqa: E731  (an empty tensor has no address)
    return (tx, txl, ty, tyl), (ptr(tx), ptr(txl), B, R, L, ptr(ty), ptr(tyl), Q, Lq), st


def _counts_entry(torch, dec, x, x_lens, y=None, y_lens=None, status=True, fn="ctcd_edit_counts"):
    """ctcd_edit_counts (or ctcd_edit_distance) on numpy arrays, the output preset to sentinel words.  -> (rc, out, status, pairs)."""
    from ctcdecode_amd import _native

    keep, args, st = _device(torch, x, x_lens, y, y_lens)
    B, R, Q = args[2], args[3], args[7]
    out = torch.full((B, R, Q, 4) if fn == "ctcd_edit_counts" else (B, R, Q), eu.SENTINEL, dtype=torch.int32, device="cuda")
    rc = getattr(_native.lib, fn)(dec._handle, *args, out.data_ptr(), st.data_ptr() if status else None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), st.cpu().numpy()[:B], dec.last_edit_pairs()


def _align_entry(torch, dec, x, x_lens, y, y_lens, status=True, counts=True):
    """ctcd_edit_align on numpy arrays, every output preset to sentinel words.  -> (rc, x_to_y, y_to_x, counts, status)."""
    from ctcdecode_amd import _native

    keep, args, st = _device(torch, x, x_lens, y, y_lens)
    B, R, L, Q, Lq = args[2], args[3], args[4], args[7], args[8]
    xm = torch.full((B, R, Q, L), eu.SENTINEL, dtype=torch.int32, device="cuda")
    ym = torch.full((B, R, Q, Lq), eu.SENTINEL, dtype=torch.int32, device="cuda")
    cn = torch.full((B, R, Q, 4), eu.SENTINEL, dtype=torch.int32, device="cuda")
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    rc = _native.lib.ctcd_edit_align(dec._handle, *args, ptr(xm), ptr(ym), ptr(cn) if counts else None, st.data_ptr() if status else None,
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, xm.cpu().numpy(), ym.cpu().numpy(), cn.cpu().numpy(), st.cpu().numpy()[:B]


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: differs at %s: got %s, want %s" % (what, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _check_counts(torch, dec, c, what, want=None):
    if want is None:
        want = eu.cached(("ops counts", what), lambda: ou.case_reference(c))
    rc, out, status, pairs = _counts_entry(torch, dec, c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0, what
    _same(out, want[0], what)
    assert (status == want[-1]).all(), what
    B, R, Q = out.shape[:3]
    assert pairs == (B * R * (R - 1) // 2 if c["y"] is None else B * R * Q), what
    rc, dist, _, _ = _counts_entry(torch, dec, c["x"], c["x_lens"], c["y"], c["y_lens"], fn="ctcd_edit_distance")
    assert rc == 0 and (out[..., 1:].sum(-1) == dist).all(), "%s: S + Del + I == edit_distance" % what
    return out


def _check_maps(torch, dec, c, what, want=None):
    if want is None:
        want = eu.cached(("ops maps", what), lambda: ou.case_reference(c, True))
    rc, xm, ym, counts, status = _align_entry(torch, dec, c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0, what
    _same(xm, want[1], what + ": x_to_y")
    _same(ym, want[2], what + ": y_to_x")
    _same(counts, want[0], what + ": counts")
    assert (status == want[3]).all(), what
    return xm, ym, counts


def _mixed_reference():
    """The mixed launch's counts and maps from the restatement: the one long computation of this file, done once."""
    return eu.cached(("ops maps", "mixed"), lambda: ou.case_reference(eu.mixed_case(), True))


# ---- counts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", eu.CLASSES)
def test_counts_equal_the_restatement_over_the_length_grid(torch_mod, dec, C):
    """One launch per class and role over editdist's grid: strips of 0, 1, C - 1, C, C + 1, 63 C, 64 C - 1, 64 C and 64 C + 1 tokens
    against streamed rows of n, n + 1, n + 62 .. n + 65 and 3 n."""
    for swap in (False, True):
        _check_counts(torch_mod, dec, eu.grid_case(C, swap), "grid %d %s" % (C, swap))


def test_counts_of_a_launch_mixing_every_class_and_empty_rows(torch_mod, dec):
    c = eu.mixed_case()
    want = _mixed_reference()
    out = _check_counts(torch_mod, dec, c, "mixed", (want[0], want[3]))
    assert (out[..., 0] + out[..., 1] + out[..., 3] == c["x_lens"][:, :, None]).all() and (out[..., 0] + out[..., 1] + out[..., 2] == c["y_lens"][:, None, :]).all()


@pytest.mark.parametrize("R", (1, 2, 7, 40))
def test_pairwise_counts(torch_mod, dec, R):
    c = eu.pairwise_case(R)
    out = _check_counts(torch_mod, dec, c, "pairwise %d" % R)
    assert (out == out.transpose(0, 2, 1, 3)[..., [0, 1, 3, 2]]).all()  # [j][i] = [i][j] with Del and I exchanged
    assert (np.diagonal(out[..., 0], axis1=1, axis2=2) == c["x_lens"]).all() and (np.diagonal(out[..., 1:].sum(-1), axis1=1, axis2=2) == 0).all()
    rc, general, _, pairs = _counts_entry(torch_mod, dec, c["x"], c["x_lens"], c["x"].copy(), c["x_lens"].copy())
    assert rc == 0 and (general == out).all() and pairs == out.shape[0] * R * R
    got = dec.edit_counts(torch_mod.from_numpy(c["x"]).cuda(), torch_mod.from_numpy(c["x_lens"]).cuda())
    assert got.is_cuda and got.dtype == torch_mod.int32 and (got.cpu().numpy() == out).all()


def test_more_pairs_than_waves_at_the_default_grid(torch_mod, dec):
    """10080 short pairs in pairwise mode, several per wave of the default grid; then with a bad item between good ones."""
    c = eu.many_short_case()
    out = _check_counts(torch_mod, dec, c, "many short")
    pairs, waves = dec.last_edit_pairs(), 4 * dec.last_edit_grid()
    assert pairs == 5 * 64 * 63 // 2 and 0 < waves and pairs >= 2 * waves, (pairs, waves)
    xl = c["x_lens"].copy()
    xl[2, 32] = 25
    rc, bad, status, _ = _counts_entry(torch_mod, dec, c["x"], xl)
    assert rc == 0 and status.tolist() == [0, 0, eu.BAD_ROW, 0, 0] and (bad[2] == 0).all() and (bad[[0, 1, 3, 4]] == out[[0, 1, 3, 4]]).all()


# ---- maps ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", eu.CLASSES)
def test_maps_equal_the_restatement_over_the_length_grid(torch_mod, dec, C):
    """Per class and role: strips of 1, C, C + 1, 63 C + 1, 64 C - 1 and 64 C tokens against streamed rows of n, n + 1, n + 63, n + 64
    and n + 65; the maps' own properties on top."""
    for swap in (False, True):
        c = ou.map_grid_case(C, swap)
        xm, ym, counts = _check_maps(torch_mod, dec, c, "map grid %d %s" % (C, swap))
        assert dec.last_edit_slots() == len(c["pairs"]) == dec.last_edit_pairs()
        for k in range(len(c["pairs"])):
            lx, ly = int(c["x_lens"][k, 0]), int(c["y_lens"][k, 0])
            ou.check_maps(xm[k, 0, 0], ym[k, 0, 0], lx, ly)
            assert ou.counts_from_maps(xm[k, 0, 0], ym[k, 0, 0], c["x"][k, 0], c["y"][k, 0], lx, ly) == tuple(counts[k, 0, 0])


@pytest.mark.parametrize("C", eu.CLASSES)
def test_closed_forms_with_ties(torch_mod, dec, C):
    """[a, b] / [b, a] alone and in front of a common run, with a tail on either side (so that x is the strip, then the streamed row),
    equal and disjoint rows, a prefix, a suffix, a rotation: one launch, an item per case."""
    every = ou.tie_cases(C)
    # two launches, an item per case: the cases whose x is not the longer row, and the others (so that min(L, Lq) stays the strip's width)
    for cases in ([c for c in every if len(c[1]) <= len(c[2])], [c for c in every if len(c[1]) > len(c[2])]):
        x, xl = eu.pack_rows([c[1] for c in cases])
        y, yl = eu.pack_rows([c[2] for c in cases])
        assert len(cases) >= 2 and min(x.shape[1], y.shape[1]) <= eu.MAX_STRIP
        rc, xm, ym, counts, _ = _align_entry(torch_mod, dec, x[:, None], xl[:, None], y[:, None], yl[:, None])
        assert rc == 0
        for k, (name, a, b, cnt, want_x, want_y) in enumerate(cases):
            assert tuple(counts[k, 0, 0]) == cnt, "class %d %s" % (C, name)
            assert xm[k, 0, 0, :len(a)].tolist() == want_x and ym[k, 0, 0, :len(b)].tolist() == want_y, "class %d %s" % (C, name)
            assert (xm[k, 0, 0, len(a):] == -1).all() and (ym[k, 0, 0, len(b):] == -1).all()


# ---- the persistent loop and the slots -------------------------------------------------------------------------------------------------
def test_align_of_the_mixed_launch_at_capped_grids_and_one_slot(torch_mod, dec):
    """The 600 pairs of every class through edit_align: at the default grid against the restatement; then with four and eight waves
    taking them in turn (each wave's slot reused 150 or 75 times, from class to class), and through a scratch budget that holds exactly
    one slot, so that one wave takes all of them through it.  Identical results."""
    c = eu.mixed_case()
    want = _mixed_reference()
    _check_maps(torch_mod, dec, c, "mixed", want)
    slot = 3000 * 64 * 8
    assert dec.last_edit_pairs() == 600 and dec.last_edit_slots() == min(600, 4 * dec.last_edit_grid(), (1 << 30) // slot)
    try:
        for grid in (1, 2):
            dec.set_edit_grid(grid)
            _check_maps(torch_mod, dec, c, "mixed, grid %d" % grid, want)
            assert dec.last_edit_grid() == grid and dec.last_edit_slots() == 4 * grid
        dec.set_edit_grid(0)
        dec.set_edit_scratch(2 * slot - 1)
        _check_maps(torch_mod, dec, c, "mixed, one slot", want)
        assert dec.last_edit_slots() == 1 and dec.last_edit_grid() == 1
    finally:
        dec.set_edit_grid(0)
        dec.set_edit_scratch(0)
    with pytest.raises(ValueError):
        dec.set_edit_scratch(-1)


def test_slot_reuse_from_class_to_class(torch_mod, dec):
    """A long pair of class 16 followed on the same slot by a short one of class 1, and the reverse."""
    try:
        dec.set_edit_scratch(900 * 64 * 4)
        for k, c in enumerate(ou.slot_reuse_cases()):
            _check_maps(torch_mod, dec, c, "slot reuse %d" % k)
            assert dec.last_edit_slots() == 1
    finally:
        dec.set_edit_scratch(0)


# ---- limits ----------------------------------------------------------------------------------------------------------------------------
def test_the_limits(torch_mod, dec):
    torch = torch_mod
    c = ou.limit_case()
    D = ou.MAX_DIM
    rc, out, _, _ = _counts_entry(torch, dec, c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0 and out[0, 0, 0].tolist() == [0, 3, D - 3, 0]  # the greatest key: D = 262144, S = 3
    rc, out, _, _ = _counts_entry(torch, dec, c["y"], c["y_lens"], c["x"], c["x_lens"])
    assert rc == 0 and out[0, 0, 0].tolist() == [0, 3, 0, D - 3]
    rc, xm, ym, counts, _ = _align_entry(torch, dec, c["x"], c["x_lens"], c["y"], c["y_lens"])
    assert rc == 0 and counts[0, 0, 0].tolist() == [0, 3, D - 3, 0] and dec.last_edit_slots() == 1
    assert xm[0, 0, 0].tolist() == [D - 3, D - 2, D - 1] and (ym[0, 0, 0, :-3] == -1).all() and ym[0, 0, 0, -3:].tolist() == [0, 1, 2]
    over = ou.limit_case(D + 1)
    t = lambda k: torch.from_numpy(over[k]).cuda()  # noqa: E731
    with pytest.raises(NotImplementedError):
        dec.edit_counts(t("x"), t("x_lens"), t("y"), t("y_lens"))
    with pytest.raises(NotImplementedError):
        dec.edit_counts(t("y"), t("y_lens"))
    with pytest.raises(NotImplementedError):
        dec.edit_align(t("x"), t("x_lens"), t("y"), t("y_lens"))
    wide = torch.zeros((1, 1, 2049), dtype=torch.int32, device="cuda")
    lens = torch.full((1, 1), 2049, dtype=torch.int32, device="cuda")
    with pytest.raises(NotImplementedError):
        dec.edit_counts(wide, lens, wide.clone(), lens)
    with pytest.raises(NotImplementedError):
        dec.edit_align(wide, lens, wide.clone(), lens)
    with pytest.raises(ValueError):
        dec.edit_align(t("x"), t("x_lens"), None, None)
    assert dec.edit_counts(torch.tensor([[[1, 2]]]).cuda(), torch.tensor([[2]]), torch.tensor([[[2, 1]]]), torch.tensor([[2]])).tolist() == [[[[1, 0, 1, 1]]]]  # usable


def test_a_budget_below_one_slot(torch_mod, dec):
    from ctcdecode_amd import _native

    s = ou.slot_reuse_cases()[0]
    t = lambda k: torch_mod.from_numpy(s[k]).cuda()  # noqa: E731
    try:
        dec.set_edit_scratch(900 * 64 * 4 - 1)
        with pytest.raises(NotImplementedError, match="230400"):
            dec.edit_align(t("x"), t("x_lens"), t("y"), t("y_lens"))
        assert _align_entry(torch_mod, dec, s["x"], s["x_lens"], s["y"], s["y_lens"])[0] == -2 and b"230399" in _native.lib.ctcd_last_error()
        dec.set_edit_scratch(900 * 64 * 4)
        _check_maps(torch_mod, dec, s, "slot reuse 0")  # the decoder is usable, and one slot is enough
    finally:
        dec.set_edit_scratch(0)


def test_both_rows_full_at_the_strip_limit(torch_mod, dec):
    """min(L, Lq) = 2048 with both rows full: one pair, one slot of 2048 rows x 64 lanes x 8 bytes."""
    rng = np.random.default_rng(eu.hash_name("ops limit"))
    a, b = eu.related_rows(rng, 2048, 2048, 3)
    c = dict(x=a[None, None], x_lens=np.asarray([[2048]], np.int32), y=b[None, None], y_lens=np.asarray([[2048]], np.int32))
    assert ou.host_slot_bytes(2048, 2048) == 1 << 20
    xm, ym, counts = _check_maps(torch_mod, dec, c, "strip limit")
    assert dec.last_edit_slots() == 1 and 0 < counts[0, 0, 0, 1:].sum() < 2048
    ou.check_maps(xm[0, 0, 0], ym[0, 0, 0], 2048, 2048)
    _check_counts(torch_mod, dec, c, "strip limit", (eu.cached(("ops maps", "strip limit"), None)[0], np.zeros(1, np.int32)))


# ---- invalid and degenerate cases ------------------------------------------------------------------------------------------------------
def test_bad_lengths_in_a_middle_item(torch_mod, dec):
    torch = torch_mod
    c = eu.pairwise_case(7, B=3, L=40)
    y, yl = c["x"][:, :2].copy(), c["x_lens"][:, :2].copy()
    good = eu.cached(("ops maps", "bad lengths base"), lambda: ou.reference(c["x"], c["x_lens"], y, yl, True))
    for side, bad in (("x", -1), ("x", 41), ("y", 41)):
        xl, yl2 = c["x_lens"].copy(), yl.copy()
        (xl if side == "x" else yl2)[1, 1] = bad
        want = [a.copy() for a in good]
        want[0][1], want[1][1], want[2][1], want[3][1] = 0, -1, -1, eu.BAD_ROW
        d = dict(x=c["x"], x_lens=xl, y=y, y_lens=yl2)
        _check_maps(torch, dec, d, "bad %s" % side, want)  # maps -1, counts 0, status raised, neighbours intact
        _check_counts(torch, dec, d, "bad %s" % side, (want[0], want[3]))
        rc, xm, ym, counts, _ = _align_entry(torch, dec, c["x"], xl, y, yl2, status=False, counts=False)  # neither status nor counts
        assert rc == 0 and (xm == want[1]).all() and (ym == want[2]).all() and (counts == eu.SENTINEL).all()
        with pytest.raises(ValueError, match=r"items \[1\]"):
            dec.edit_align(torch.from_numpy(c["x"]), torch.from_numpy(xl), torch.from_numpy(y), torch.from_numpy(yl2))
        with pytest.raises(ValueError, match=r"items \[1\]"):
            dec.edit_counts(torch.from_numpy(c["x"]), torch.from_numpy(xl), torch.from_numpy(y), torch.from_numpy(yl2))
    xl = c["x_lens"].copy()
    xl[1, 3] = 41
    want = ou.reference(c["x"], xl)  # pairwise: the diagonal of the bad item is zero too
    rc, out, status, _ = _counts_entry(torch, dec, c["x"], xl)
    assert rc == 0 and (out == want[0]).all() and status.tolist() == [0, eu.BAD_ROW, 0] and (out[1] == 0).all()


def test_degenerate_shapes(torch_mod, dec):
    torch = torch_mod
    from ctcdecode_amd import _native

    z = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")  # noqa: E731
    for (B, R, L), (Q, Lq) in (((0, 3, 4), (2, 4)), ((2, 0, 4), (2, 4)), ((2, 3, 4), (0, 4))):
        assert tuple(dec.edit_counts(z(B, R, L), z(B, R), z(B, Q, Lq), z(B, Q)).shape) == (B, R, Q, 4) and dec.last_edit_pairs() == 0
        h2r, r2h, counts = dec.edit_align(z(B, R, L), z(B, R), z(B, Q, Lq), z(B, Q))
        assert tuple(h2r.shape) == (B, R, Q, L) and tuple(r2h.shape) == (B, R, Q, Lq) and tuple(counts.shape) == (B, R, Q, 4)
        assert dec.last_edit_pairs() == 0 and dec.last_edit_slots() == 0
    assert tuple(dec.edit_counts(z(0, 3, 4), z(0, 3)).shape) == (0, 3, 3, 4) and tuple(dec.edit_counts(z(2, 0, 4), z(2, 0)).shape) == (2, 0, 0, 4)
    yl = torch.tensor([[3, 0], [1, 4]], dtype=torch.int32)
    ones = torch.ones((2, 2, 4), dtype=torch.int32)
    h2r, r2h, counts = dec.edit_align(z(2, 3, 0), z(2, 3), ones, yl)  # L == 0: every reference token is a deletion
    assert tuple(h2r.shape) == (2, 3, 2, 0) and (r2h == -1).all() and (counts[..., 2].cpu() == yl[:, None, :]).all() and (counts[..., [0, 1, 3]] == 0).all()
    h2r, r2h, counts = dec.edit_align(ones, yl, z(2, 3, 0), z(2, 3))  # Lq == 0: every hypothesis token an insertion
    assert tuple(r2h.shape) == (2, 2, 3, 0) and (h2r == -1).all() and (counts[..., 3] == yl[:, :, None]).all() and (counts[..., :3] == 0).all()
    assert (dec.edit_counts(ones, yl, z(2, 3, 0), z(2, 3)) == counts).all()
    h2r, r2h, counts = dec.edit_align(ones, yl, ones[:, :1], z(2, 1))  # empty references in a tensor with columns
    assert (h2r == -1).all() and (r2h == -1).all() and (counts[..., 3] == yl[:, :, None]).all()
    x, xl, out, maps = z(2, 3, 4), z(2, 3), z(2, 3, 3, 4), z(2, 3, 3, 4)
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    fn = _native.lib.ctcd_edit_counts
    assert fn(dec._handle, p(x), p(xl), -1, 3, 4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, -4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, 4, p(x), p(xl), -1, 4, p(out), None, s) == -1
    assert fn(dec._handle, None, p(xl), 2, 3, 4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), None, 2, 3, 4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, 4, None, None, 0, 0, None, None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, 4, p(x), None, 3, 4, p(out), None, s) == -1
    assert fn(None, p(x), p(xl), 2, 3, 4, None, None, 0, 0, p(out), None, s) == -1
    assert fn(dec._handle, p(x), p(xl), 2, 3, 4, None, None, 0, 0, p(out), None, s) == 0
    fa = _native.lib.ctcd_edit_align
    assert fa(dec._handle, p(x), p(xl), 2, 3, 4, None, None, 3, 4, p(maps), p(maps), None, None, s) == -1  # pairwise
    assert fa(dec._handle, p(x), p(xl), 2, 3, 4, p(x), None, 3, 4, p(maps), p(maps), None, None, s) == -1
    assert fa(dec._handle, p(x), p(xl), 2, 3, 4, p(x), p(xl), 3, 4, None, p(maps), None, None, s) == -1
    assert fa(dec._handle, p(x), p(xl), 2, 3, 4, p(x), p(xl), 3, 4, p(maps), None, None, None, s) == -1
    assert fa(dec._handle, p(x), p(xl), 2, -3, 4, p(x), p(xl), 3, 4, p(maps), p(maps), None, None, s) == -1
    assert fa(None, p(x), p(xl), 2, 3, 4, p(x), p(xl), 3, 4, p(maps), p(maps), None, None, s) == -1
    m2 = z(2, 3, 3, 4)
    assert fa(dec._handle, p(x), p(xl), 2, 3, 4, p(x), p(xl), 3, 4, p(maps), p(m2), None, None, s) == 0
    torch.cuda.synchronize()
    assert (maps == -1).all() and (m2 == -1).all()  # rows of length 0


def test_tensor_handling(torch_mod, dec):
    """CPU and int64 inputs, a [B, Lq] reference with [B] lengths, non-contiguous views: what ``edit_distance`` accepts."""
    torch = torch_mod
    c = eu.pairwise_case(7, B=3, L=40)
    y, yl = c["x"][:, 1].copy(), c["x_lens"][:, 1].copy()  # [B, Lq], [B]
    want = ou.reference(c["x"], c["x_lens"], y[:, None], yl[:, None], True)
    x64, xl64 = torch.from_numpy(c["x"]).long(), torch.from_numpy(c["x_lens"]).long()
    outs = dec.edit_align(x64, xl64, torch.from_numpy(y).to(torch.int16), torch.from_numpy(yl))
    assert all(not o.is_cuda and o.dtype == torch.int32 for o in outs) and tuple(outs[0].shape) == (3, 7, 1, 40)
    assert (outs[0].numpy() == want[1]).all() and (outs[1].numpy() == want[2]).all() and (outs[2].numpy() == want[0]).all()
    cn = dec.edit_counts(x64.cuda(), xl64, torch.from_numpy(y), torch.from_numpy(yl).cuda())
    assert cn.is_cuda and (cn.cpu().numpy() == want[0]).all()
    wide = torch.full((3, 7, 80), eu.GARBAGE, dtype=torch.int32, device="cuda")
    wide[:, :, ::2] = torch.from_numpy(c["x"]).cuda()
    view, lens_view = wide[:, :, ::2], torch.from_numpy(np.ascontiguousarray(c["x_lens"].T)).cuda().t()
    assert not view.is_contiguous() and not lens_view.is_contiguous()
    outs = dec.edit_align(view, lens_view, wide[:, 1, ::2], torch.from_numpy(yl))
    assert all(o.is_cuda for o in outs) and (outs[0].cpu().numpy() == want[1]).all() and (outs[1].cpu().numpy() == want[2]).all()
    assert (dec.edit_counts(view, lens_view).cpu().numpy() == ou.reference(c["x"], c["x_lens"])[0]).all()
    import ctcdecode

    assert ctcdecode.CTCBeamDecoder.edit_counts is type(dec).edit_counts and ctcdecode.CTCBeamDecoder.edit_align is type(dec).edit_align


def test_end_to_end_on_a_decode(torch_mod):
    """Decode a small batch, make references by editing the best rows in known ways -- a token no label uses substituted at one place,
    another inserted, one label dropped, far enough apart that the breakdown is unique -- and align the rows against them: the counts
    are the edits', and ``ref_to_hyp`` carries the decode's time steps onto the reference."""
    torch = torch_mod
    import ctcdecode_amd

    V, B, T = 8, 3, 60
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], blank_id=0, beam_width=16, log_probs_input=True)
    rng = np.random.default_rng(5)
    z = rng.standard_normal((B, T, V)) * 2.0
    lp = torch.from_numpy((z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)).cuda()
    tokens, _, timesteps, lens = dec.decode_device(lp, torch.tensor([60, 50, 40], dtype=torch.int32))
    hyp, steps, n = tokens[:, :1].cpu().numpy(), timesteps[:, :1].cpu().numpy(), lens[:, :1].cpu().numpy()
    assert n.min() >= 12
    refs, keep, drops = [], [], []
    for b in range(B):
        row = hyp[b, 0, :n[b, 0]].tolist()
        # reference = the row with row[2] replaced by 100, 101 put in front of row[6], and row[p] left out: the first p >= 9 whose label
        # differs from the one before it (of two equal neighbours the walk, coming from the end, would pair the later one)
        p = next(q for q in range(9, len(row) - 1) if row[q] != row[q - 1])
        drops.append(p)
        refs.append(row[:2] + [100] + row[3:6] + [101] + row[6:p] + row[p + 1:])
        keep.append([0, 1, 2, 3, 4, 5, -1] + list(range(6, p)) + list(range(p + 1, len(row))))  # the hypothesis position under each reference token
    y, yl = eu.pack_rows(refs)
    h2r, r2h, counts = dec.edit_align(tokens[:, :1], lens[:, :1], torch.from_numpy(y[:, None]).cuda(), torch.from_numpy(yl[:, None]).cuda())
    assert h2r.is_cuda and tuple(h2r.shape) == (B, 1, 1, tokens.shape[2]) and tuple(r2h.shape) == (B, 1, 1, y.shape[1])
    for b in range(B):
        lx = int(n[b, 0])
        assert counts[b, 0, 0].tolist() == [lx - 2, 1, 1, 1]  # one substitution, one deletion (101), one insertion (row[p])
        assert r2h[b, 0, 0, :int(yl[b])].tolist() == keep[b] and h2r[b, 0, 0, drops[b]].item() == -1 and h2r[b, 0, 0, 2].item() == 2
    carried = torch.gather(timesteps[:, 0].to(torch.int64), 1, r2h[:, 0, 0].clamp_min(0).to(torch.int64)).cpu().numpy()
    for b in range(B):
        want = [int(steps[b, 0, p]) if p >= 0 else -1 for p in keep[b]]
        got = [int(carried[b, q]) if keep[b][q] >= 0 else -1 for q in range(int(yl[b]))]
        assert got == want and len(set(got)) > 10
    assert (dec.edit_counts(tokens[:, :1], lens[:, :1], torch.from_numpy(y[:, None]), torch.from_numpy(yl[:, None])) == counts).all()
