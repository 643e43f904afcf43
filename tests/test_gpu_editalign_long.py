"""-m gpu tests of the long alignments (``edit_align`` with ``set_edit_long`` on): the maps of pairs whose shorter row is beyond 2048 tokens
== the references of tests/editalign_long_util.py, exactly; the counts == ``edit_counts`` of the same call; the maps' properties.  The
shapes are the smallest where the checkpoints, the blocks' corners and the slot can go wrong."""
import editalign_long_util as au
import editdist_util as eu
import editops_util as ou
import pytest
from test_gpu_editops import _align_entry, dec, torch_mod  # noqa: F401  (fixtures: torch, and a decoder of this module's own)

pytestmark = pytest.mark.gpu


def _align(torch, dec, rows):
    """One launch, an item per pair (R = Q = 1) in tensors beyond 2048 columns, checked three ways.  -> the long kernel's slots"""
    packed = [eu.pack_rows([r[k] for r in rows], max(2049, max(len(r[k]) for r in rows))) for k in (0, 1)]
    a = [torch.from_numpy(v[:, None]).cuda() for p in packed for v in p]
    xm, ym, counts = (o.cpu().numpy() for o in dec.edit_align(*a))
    assert dec.last_edit_long() == len(rows)
    slots = dec.last_edit_slots()
    assert (counts == dec.edit_counts(*a).cpu().numpy()).all()
    for k, (x, y, want_x, want_y) in enumerate(rows):
        assert (xm[k, 0, 0, :len(x)] == want_x).all() and (ym[k, 0, 0, :len(y)] == want_y).all(), k
        ou.check_maps(xm[k, 0, 0], ym[k, 0, 0], len(x), len(y))
    return slots


@pytest.mark.parametrize("name", au.CASES)
def test_the_maps_equal_the_references(torch_mod, dec, name):
    dec.set_edit_long(au.CASES[name])
    _align(torch_mod, dec, au.pairs(name))


def test_a_mixed_launch_is_the_same_at_every_width(torch_mod, dec):
    c = au.mixed_case()
    a = [c[k] for k in ("x", "x_lens", "y", "y_lens")]
    for waves in (2, 4, 8, 16):  # the C entry point over outputs of sentinel words: the bad item does not raise there
        dec.set_edit_long(waves)
        rc, xm, ym, counts, st = _align_entry(torch_mod, dec, *a)
        assert rc == 0 and dec.last_edit_long() == 4 and st.tolist() == [0, eu.BAD_ROW], waves
        assert (xm == c["xm"]).all() and (ym == c["ym"]).all() and (counts == c["counts"]).all(), waves
    assert (c["xm"][1] == -1).all() and (c["ym"][1] == -1).all() and (c["counts"][1] == 0).all()


def test_one_slot_one_workgroup_and_a_budget_too_small(torch_mod, dec):
    rows = au.limits_case()  # six long pairs in tensors of 2049 and 4103 columns
    short = 4103 * 64 * 8  # the per-wave kernel's slot, the larger of the two in this call: the long slot is 721152 bytes
    dec.set_edit_long(4)
    assert _align(torch_mod, dec, rows) == 6
    dec.set_edit_scratch(short)  # exactly one slot of the larger kind: six pairs through the two long slots that fit it
    assert _align(torch_mod, dec, rows) == 2
    dec.set_edit_scratch(short - 1)
    with pytest.raises(NotImplementedError, match=str(short)):
        _align(torch_mod, dec, rows)
    dec.set_edit_scratch(0)
    dec.set_edit_grid(1)  # one workgroup and one slot, round the loop six times
    assert _align(torch_mod, dec, rows) == 1
    dec.set_edit_grid(0)
