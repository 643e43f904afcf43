"""The certificate behind test_gpu_select_paths.py, on the CPU: select_path_inputs (tests/select_path_util.py) drive every scorer
instantiation of the decode kernel through the select's tie and replay paths.

The host twin (tests/native/core_host.cpp) counts which path a frame takes (beam_core.h enum Event, ctccore_event_counts).  For every
PROF 0, non-streamed scorer case of the kernel matrix it decodes select_path_inputs on one thread, instantiated as the case's own
class (select_path_util.host_env), and
  * equals the restated oracle and, where it was built, the compiled reference's own scorer, bit for bit;
  * reaches per case the floors of SCORER_FLOORS, and EV_EXACT >= B + 3: more replays than utterances end (a decode's last frame always
    replays), so std::nth_element is replayed mid-utterance, with the scorer's per-entry state behind it;
  * over the whole table takes the slow path's third way at least once (EV_SLOW_BELOW: the K-th key lies below the histogram's window)
    and settles a tie by character, without the replay (EV_TIE_FRAMES > EV_EXACT).
The floors are conditions on the INPUTS, not measurements of the product: each lies under the smallest value measured when the recipe
was chosen (profiles/select_path_coverage.json).  A case that falls short needs another recipe, not another floor.

Callback cases.  The scorer hook's twin (decode_core_host_lm_cb) decodes unpruned batches in the run-time layout; every unpruned
callback case goes through it as well (same results, the floors hold there too: a frame that parked on a miss is counted again when
it is run again, so those counts are no smaller).  A PRUNED callback case is certified by the built-in-scorer twin of the same layout
class alone: the select reads keys and slot layout, neither depends on CB -- what CB changes is where a conditional probability comes
from and that a frame can be abandoned in front of the select.

What km.inputs already gives the scorer-free cases is pinned the same way (SCORER_FREE_FLOORS, and the four outcomes of the speculative
select for the cases with a compile-time layout in LDS, whose device policy has it: beam_core.h kSpec), so that a later change of seeds or recipes cannot
lose it unnoticed.

Two counters are left out: EV_HOT_LIST and EV_WIDE_LIST count paths behind experiment switches that are off in the product
(CTC_EXP_HOT_PRELIST, CTC_EXP_WIDE_LIST); no kernel of CTC_KERNEL_LIST contains them, so there is nothing on the device to certify."""
import json
import os

import pytest

import kernel_matrix_util as km
import oracle_util as ou
import select_path_util as sp
import stream_matrix_util as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCORER_FLOORS = dict(EV_TIE_FRAMES=8, EV_TIE_BIG=5, EV_SLOW_CROWDED=10, EV_SLOW_SINGLE=5, EV_REVIVED=5)  # and EV_EXACT >= B + 3
SCORER_FREE_FLOORS = dict(EV_TIE_FRAMES=15, EV_TIE_BIG=10, EV_SLOW_CROWDED=40, EV_SLOW_SINGLE=10, EV_EXACT=15)
SPEC_FLOOR = 3  # each of EV_SPEC_OK / UNDER / OVER / OTHER, scorer-free cases whose kernel has the speculative select

SCORER = sp.scorer_cases()
SCORER_FREE = sp.scorer_free_cases()


@pytest.fixture(scope="module")
def wide99(tmp_path_factory):
    from test_lm import make_wide_label_lm

    return make_wide_label_lm(tmp_path_factory.mktemp("select_paths_lm"))


def _env(monkeypatch, c):
    sp.set_host_env(c, monkeypatch.setenv, lambda name: monkeypatch.delenv(name, raising=False))  # (the twin reads them on each call)


_MEASURED = {}


def _scorer_counts(monkeypatch, wide99, c, hook=False):
    """-> (the twin's result, its counters) of a scorer case, decoded once per module."""
    key = (km.case_id(c), hook)
    if key not in _MEASURED:
        lm = km.lm_spec(c, *wide99)
        lp, sl = sp.select_path_inputs(c, lm[1])
        with monkeypatch.context() as m:
            _env(m, c)
            _MEASURED[key] = sp.counted(lambda: sp.host_decode(c, lp, sl, lm, callback=hook))
    return _MEASURED[key]


def _scorer_free_counts(monkeypatch, c):
    key = (km.case_id(c), None)
    if key not in _MEASURED:
        lp, sl = km.inputs(c)
        with monkeypatch.context() as m:
            _env(m, c)
            _MEASURED[key] = sp.counted(lambda: sp.host_decode(c, lp, sl, None))
    return _MEASURED[key]


def _assert_floors(cnt, floors, what):
    print(what, cnt)
    for name, floor in floors.items():
        assert cnt[name] >= floor, "%s: %s = %d, the inputs must give at least %d" % (what, name, cnt[name], floor)


def test_the_tables_cover_the_matrix():
    assert len(SCORER) == 26 and len(SCORER_FREE) == 20
    assert sum(1 for c in SCORER if c["callback"]) == 10 and sum(1 for c in SCORER if c["callback"] and not sp.is_pruned(c)) == 5
    rest = [c for c in km.CASES if c not in SCORER and c not in SCORER_FREE]
    assert all(c["streamed"] or c["profile"] for c in rest)  # (PROF 1, 2, 4, 5: the same select behind timers or streamed rows)
    for name in sp.COUNTERS + sp.LEFT_OUT:
        sm.event_index(name)
    # the twin's scorer classes are all named by some case: HBM levels 0-3, the run-time layout at a fixed-layout shape, general / word model
    envs = [sp.host_env(c) for c in SCORER]
    assert set(e.get("CTC_HOST_BIG", "0") for e in envs) == {"0", "1", "2", "3"}
    assert any("CTC_HOST_LM_RUNTIME_LAYOUT" in e for e in envs) and any("CTC_HOST_GENERAL_LM" in e for e in envs) and any(not e for e in envs)


@pytest.mark.parametrize("c", SCORER, ids=km.case_id)
def test_scorer_case_reaches_the_select_paths(monkeypatch, wide99, c):
    lm = km.lm_spec(c, *wide99)
    lp, sl = sp.select_path_inputs(c, lm[1])
    what = "%s %s" % (km.case_id(c), sp.host_env(c))
    wants = [ou.decode(lp, sl, scorer=ou.Scorer(lm[2], lm[3], lm[0], lm[1], "restated"), **sm.oracle_args(c))]
    if ou.have_reference():
        wants.append(ou.decode(lp, sl, which="reference", scorer=ou.Scorer(lm[2], lm[3], lm[0], lm[1], "reference"), **sm.oracle_args(c)))
    runs = [(False, what)] + ([(True, what + " (through the scorer hook)")] if c["callback"] and not sp.is_pruned(c) else [])
    for hook, name in runs:
        got, cnt = _scorer_counts(monkeypatch, wide99, c, hook)
        for want in wants:
            ou.assert_same(got, want, name)
        _assert_floors(cnt, SCORER_FLOORS, name)
        assert cnt["EV_EXACT"] >= c["B"] + 3, "%s: %d replays, %d utterances" % (name, cnt["EV_EXACT"], c["B"])
        assert cnt["EV_SPEC_OK"] + cnt["EV_SPEC_UNDER"] + cnt["EV_SPEC_OVER"] + cnt["EV_SPEC_OTHER"] == 0  # (as on the device: no kSpec behind a scorer)
        if hook:
            assert got["callback_calls"] > 0 and got["resumptions"] > 0


def test_scorer_table_reaches_the_rare_paths(monkeypatch, wide99):
    counts = dict((km.case_id(c), _scorer_counts(monkeypatch, wide99, c)[1]) for c in SCORER)
    below = [i for i, n in counts.items() if n["EV_SLOW_BELOW"] >= 1]
    by_character = [i for i, n in counts.items() if n["EV_TIE_FRAMES"] > n["EV_EXACT"]]
    print("K-th key below the window:", below, "ties settled by character:", by_character)
    assert below and by_character


def test_select_path_inputs_are_the_matrix_inputs_plus_the_frames(wide99):
    import numpy as np

    for c in SCORER:
        lm = km.lm_spec(c, *wide99)
        lp, sl = sp.select_path_inputs(c, lm[1])
        lp0, sl0 = km.inputs(c, lm[1])
        T = c["T"]
        assert np.array_equal(sl, sl0) and lp.dtype == np.float32 and lp.shape == lp0.shape
        same = np.ones(lp.shape[:2], bool)
        f0, f1 = sp.flat_frames(c)
        same[0, [2, 3, (2 * T) // 3] + list(range(f0, f1))] = False
        same[2, 5:8] = False
        assert np.array_equal(lp[same].view(np.uint32), lp0[same].view(np.uint32))
        assert (lp[0, 2:4] == np.float32(-3.0e38)).all() and np.isneginf(lp[0, (2 * T) // 3]).all() and (lp[2, 5:8] == sp.FLAT_2).all()
        flat = [f for f in range(f0, f1) if f > 3]
        assert len(flat) >= 2 and (lp[0, flat] == sp.FLAT_0).all()
        assert sl[0] == T and sl[2] > 5  # (the frames lie inside their items)


@pytest.mark.parametrize("c", SCORER_FREE, ids=km.case_id)
def test_scorer_free_case_keeps_its_select_paths(monkeypatch, c):
    """(Counters alone: the twin's results on these inputs are held against the oracles by test_core_host.py and, on the device,
    by test_gpu_kernel_matrix.py.)"""
    what = "%s %s" % (km.case_id(c), sp.host_env(c))
    _, cnt = _scorer_free_counts(monkeypatch, c)
    _assert_floors(cnt, SCORER_FREE_FLOORS, what)
    spec = [cnt[n] for n in ("EV_SPEC_OK", "EV_SPEC_UNDER", "EV_SPEC_OVER", "EV_SPEC_OTHER")]
    if sp.has_spec_select(c):
        assert min(spec) >= SPEC_FLOOR, "%s: the speculative select's outcomes (settled, too few, too many, handed back): %s" % (what, spec)
    else:
        assert sum(spec) == 0, spec


def test_stored_table_is_what_the_twin_measures(monkeypatch, wide99):
    """profiles/select_path_coverage.json (tools/select_path_coverage.py --write) is the table measured here, and every case in it
    stands at or above its floors."""
    table = json.load(open(os.path.join(ROOT, "profiles", "select_path_coverage.json")))
    assert table["left_out"] == sp.LEFT_OUT
    assert sorted(table["scorer"]) == sorted(km.case_id(c) for c in SCORER)
    assert sorted(table["hook"]) == sorted(km.case_id(c) for c in SCORER if c["callback"] and not sp.is_pruned(c))
    assert sorted(table["scorer_free"]) == sorted(km.case_id(c) for c in SCORER_FREE)
    for c in SCORER:
        i = km.case_id(c)
        assert table["scorer"][i] == _scorer_counts(monkeypatch, wide99, c)[1], i
        if i in table["hook"]:
            assert table["hook"][i] == _scorer_counts(monkeypatch, wide99, c, True)[1], i
        for cnt in [table["scorer"][i]] + ([table["hook"][i]] if i in table["hook"] else []):
            assert all(cnt[n] >= f for n, f in SCORER_FLOORS.items()) and cnt["EV_EXACT"] >= c["B"] + 3, i
    for c in SCORER_FREE:
        i = km.case_id(c)
        assert table["scorer_free"][i] == _scorer_free_counts(monkeypatch, c)[1], i
        assert all(table["scorer_free"][i][n] >= f for n, f in SCORER_FREE_FLOORS.items()), i
