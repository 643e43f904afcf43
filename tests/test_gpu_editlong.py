"""-m gpu tests of the long edit pairs (``CTCBeamDecoder.set_edit_long``): ``edit_distance``, ``edit_counts`` and ``mbr_select`` on pairs
whose shorter row is beyond 2048 tokens == the references of tests/editlong_util.py, exactly, at the smallest shapes where the tiles,
the two-block lag, the LDS rings and the slot between rounds can go wrong."""
import editdist_util as eu
import editlong_util as lu
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dec():
    import ctcdecode_amd
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(8)], blank_id=0, beam_width=16, log_probs_input=True)


def _t(c, names=("x", "x_lens", "y", "y_lens")):
    import torch

    return tuple(torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in names)


@pytest.mark.parametrize("n", lu.STRIPS)
def test_strips_across_tiles_and_rounds_in_both_roles(dec, n):
    c = lu.strip_case(n)
    x, xl, y, yl = _t(c)  # (4097: the closed forms at the tile boundary among them; 6145: the ring across rounds)
    dec.set_edit_long(2)
    for swap in (False, True):
        a = (y, yl, x, xl) if swap else (x, xl, y, yl)
        dist, pairs = dec.edit_distance(*a).cpu().numpy()[:, 0, 0], dec.last_edit_long()
        counts = dec.edit_counts(*a).cpu().numpy()[:, 0, 0]
        assert pairs == dec.last_edit_long() == len(c["dist"])
        assert (dist == c["dist"]).all() and (counts == (c["counts"][:, [0, 1, 3, 2]] if swap else c["counts"])).all()
    assert n != lu.STRIPS[-1] or c["counts"][-1, 1] > 4095


def _raw(dec, name, c, words):
    """A C entry point over outputs of sentinel words.  -> (out, status)"""
    import torch
    from ctcdecode_amd import _native

    x, xl, y, yl = _t(c)
    (B, R, L), (Q, Lq) = x.shape, y.shape[1:]
    out = torch.full((B, R, Q) + words, eu.SENTINEL, dtype=torch.int32, device="cuda")
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    assert getattr(_native.lib, name)(dec._handle, x.data_ptr(), xl.data_ptr(), B, R, L, y.data_ptr(), yl.data_ptr(), Q, Lq, out.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    return out.cpu().numpy(), st.cpu().numpy()


def test_a_mixed_launch_is_the_same_at_every_width(dec):
    c = lu.mixed_case()
    for waves in (2, 4, 8, 16):  # against the reference: bit-identical across the widths
        dec.set_edit_long(waves)
        dist, st = _raw(dec, "ctcd_edit_distance", c, ())
        assert dec.last_edit_long() == c["long_pairs"] == 8
        counts, st2 = _raw(dec, "ctcd_edit_counts", c, (4,))
        assert dec.last_edit_long() == 8 and st.tolist() == st2.tolist() == [0, eu.BAD_ROW, 0], waves
        assert (dist == c["dist"]).all() and (counts == c["counts"]).all() and (dist[1] == 0).all() and (counts[1] == 0).all(), waves
    with pytest.raises(ValueError, match=r"items \[1\]"):
        dec.edit_distance(*_t(c))
    # the short rows through today's launch: tensors narrowed to 2048, the mode still on
    short = dict(c, x=c["x"][:, :4, :2048], x_lens=c["x_lens"][:, :4].copy())
    short["x_lens"][1, 2] = 300
    d2, _ = _raw(dec, "ctcd_edit_distance", short, ())
    assert dec.last_edit_long() == 0
    c2, _ = _raw(dec, "ctcd_edit_counts", short, (4,))
    assert (d2[[0, 2]] == dist[[0, 2], :4]).all() and (c2[[0, 2]] == counts[[0, 2], :4]).all()


def test_pairwise_mode_and_mbr(dec):
    rng = np.random.default_rng(eu.hash_name("long pairwise"))
    src = rng.integers(0, 4, 3000).astype(np.int32)
    rows = [np.where(rng.random(k) < 0.1, rng.integers(0, 4, k), src[:k]).astype(np.int32) for k in (2500, 2750, 3000, 2666)]
    x, xl = eu.pack_rows(rows)
    want = np.asarray([[eu.lev(a, b) for b in rows] for a in rows], np.int32)
    tx, txl, lw = _t(dict(x=x[None], xl=xl[None], lw=np.asarray([[-1.0, -2.5, -0.5, -1.5]])), ("x", "xl", "lw"))
    dec.set_edit_long(4)
    assert (dec.edit_distance(tx, txl)[0].cpu().numpy() == want).all() and dec.last_edit_long() == 6
    counts = dec.edit_counts(tx, txl)[0].cpu().numpy()
    assert (counts[..., 1:].sum(-1) == want).all() and (counts == counts.transpose(1, 0, 2)[..., [0, 1, 3, 2]]).all()
    assert tuple(counts[0, 1]) == lu.counts_ref(rows[0], rows[1]) and np.diagonal(counts[..., 0]).tolist() == xl.tolist()
    index, risk = dec.mbr_select(tx, txl, lw)
    ref_index, ref_risk = eu.mbr_reference(want[None], lw.cpu().numpy())
    assert index.tolist() == ref_index.tolist() and np.allclose(risk.cpu().numpy(), ref_risk, rtol=1e-12, atol=0)


def test_one_slot_one_workgroup_and_a_budget_too_small(dec):
    c = lu.strip_case(2049)  # six long pairs, a streamed row of 4103 tokens the longest
    a, want = _t(c), c["dist"][:, None, None]
    dec.set_edit_long(4)
    assert (dec.edit_distance(*a).cpu().numpy() == want).all() and dec.last_edit_long() == 6 and dec.last_edit_slots() == 6
    counts = dec.edit_counts(*a).cpu().numpy()
    slot = 33024  # 8 x (4103 + 1) bytes, rounded up to 256
    dec.set_edit_scratch(slot)  # one slot: six pairs through it in turn (a distance's slot is 16640 bytes: one fits as well)
    assert (dec.edit_distance(*a).cpu().numpy() == want).all() and dec.last_edit_slots() == 1
    assert (dec.edit_counts(*a).cpu().numpy() == counts).all() and dec.last_edit_slots() == 1 and dec.last_edit_long() == 6
    dec.set_edit_scratch(slot - 1)
    with pytest.raises(NotImplementedError, match=str(slot)):
        dec.edit_counts(*a)
    dec.set_edit_scratch(0)
    dec.set_edit_grid(1)  # one workgroup round the loop six times
    assert (dec.edit_counts(*a).cpu().numpy() == counts).all() and dec.last_edit_slots() == 1 and dec.last_edit_long() == 6
    dec.set_edit_long(0)  # off again: today's refusal
    with pytest.raises(NotImplementedError, match="2048"):
        dec.edit_distance(*a)
    assert dec.last_edit_long() == 0
    for bad in (1, 3, 32, -2):
        with pytest.raises(ValueError):
            dec.set_edit_long(bad)


def test_a_streamed_row_beyond_the_packed_key(dec):
    """One token against 262145 in tensors of 2049 and 262145 columns: the counts leave the packed key for the 64-bit one."""
    y = np.zeros((1, 1, 262145), np.int32)
    y[0, 0, 70000] = 3
    x, one, y, m = _t(dict(x=np.full((1, 1, 2049), 3, np.int32), x_lens=np.asarray([[1]], np.int32), y=y, y_lens=np.asarray([[262145]], np.int32)))
    dec.set_edit_long(2)
    assert dec.edit_counts(x, one, y, m)[0, 0, 0].tolist() == [1, 0, 262144, 0] and dec.edit_counts(y, m, x, one)[0, 0, 0].tolist() == [1, 0, 0, 262144] and dec.last_edit_long() == 1
    assert dec.edit_distance(x, one, y, m).item() == 262144 and dec.last_edit_long() == 0  # (a distance has no such limit)


def test_the_round_wrap_at_the_default_width(dec):
    """n = 32769 at sixteen waves: tile 16 is wave 0's second, its edges come through the slot.  1.07 G cells."""
    n = 32769
    rng = np.random.default_rng(eu.hash_name("long wrap"))
    a, b = eu.related_rows(rng, n, n + 70, 4)
    want = lu.counts_ref(a, b)
    x, xl, y, yl = _t(dict(x=a[None, None], x_lens=np.asarray([[n]], np.int32), y=b[None, None], y_lens=np.asarray([[n + 70]], np.int32)))
    dec.set_edit_long()
    assert dec.edit_distance(x, xl, y, yl).item() == sum(want[1:]) and dec.last_edit_long() == 1 and tuple(dec.edit_counts(x, xl, y, yl)[0, 0, 0].tolist()) == want
