"""The exact-shape policy of the decoder core (beam_core.h ShapeExact<100, 29, 0>) on the CPU: stage 1 (beam width, label count,
blank rank as constants) and stage 2 (the live beam size as well, once the beam is full) against the run-time policy and the oracle,
bit for bit, with every assumption the policy hands the optimiser checked (tests/native/exact_shape_host.cpp, -DCTC_ASSUME_CHECKED).
The inputs are the ones the GPU test sends through the twin kernel (exact_shape_util.cases, and the kernel matrix's recipe at the
twin's shape: exact_shape_util.matrix_inputs); the event counters certify that they reach the select's paths, and the header's
list of shapes is held to the table the tests cover."""
import numpy as np
import pytest

import exact_shape_util as xs
import kernel_matrix_util as km
import oracle_util as ou
import stream_matrix_util as sm

CASES = xs.cases()


def _same_everywhere(a, b, what):
    for k in ("tokens", "timesteps", "scores", "lens", "nres"):
        x, y = a[k], b[k]
        if k == "scores":
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), "%s: %s differ" % (what, k)


@pytest.mark.parametrize("name,lp,sl", CASES, ids=[c[0] for c in CASES])
def test_exact_policy_matches_runtime_policy_and_oracle(name, lp, sl):
    base, ev0 = xs.decode_host(lp, sl, 0)
    want = xs.oracle(name, lp, sl)
    ou.assert_same(base, want, name + " run-time policy vs oracle:")
    for stage in (1, 2):
        got, ev = xs.decode_host(lp, sl, stage)
        _same_everywhere(got, base, "%s stage %d vs run-time policy" % (name, stage))
        ou.assert_same(got, want, "%s stage %d vs oracle:" % (name, stage))
        assert ev == ev0, (name, stage, ev, ev0)  # the same frames take the same paths


def test_inputs_reach_the_select_paths():
    """Over the chosen inputs, under the exact policy (stage 2): the speculative select settles frames, falls back for a short hot
    list and for an overfull one, and the exact std::nth_element replay runs -- also in frames that are not an utterance's last
    (equal scores across the beam boundary: the quantised rows)."""
    total = dict((e, 0) for e in xs.EVENTS)
    ties = 0
    for name, lp, sl in CASES:
        if not name.endswith("_ragged"):
            continue
        _, ev = xs.decode_host(lp, sl, 2)
        for e in xs.EVENTS:
            total[e] += ev[e]
        if name.startswith("quant"):
            ties = ev["EV_TIE_FRAMES"]
            # (every utterance of three or more frames replays in its last frame: anything beyond that is a tie or danger mode)
            assert ev["EV_EXACT"] > int((sl >= 3).sum()), ev
    print(total)
    assert total["EV_SPEC_OK"] > 0, total
    assert total["EV_SPEC_UNDER"] > 0, total
    assert total["EV_SPEC_OVER"] > 0, total
    assert total["EV_EXACT"] > 0, total
    assert ties > 0, total


# ---- the kernel matrix's recipe at the twin's shape: the select-path certificate of the twin ------------------------------------------
_MATRIX = {}


def _matrix(stage):
    """The host twin's decode of exact_shape_util.matrix_inputs() at a stage, once per module -> (result, counters)."""
    if stage not in _MATRIX:
        lp, sl = xs.matrix_inputs()
        _MATRIX[stage] = xs.decode_host(lp, sl, stage)
    return _MATRIX[stage]


def test_matrix_inputs_exact_policy_matches_runtime_policy_and_oracle():
    """The recipe every kernel of CTC_KERNEL_LIST is checked with (kernel_matrix_util.inputs), at beam 100 / 29 labels / blank 0: a
    one-frame item, an item quantised to 0.5, and the item whose two -3e38 frames overflow every score to -inf (danger mode with
    finite inputs), which none of exact_shape_util.cases() has."""
    lp, sl = xs.matrix_inputs()
    c = xs.matrix_case()
    assert lp.shape == (4, 40, xs.LABELS) and sl.tolist() == [40, 1, 26, 38] and km.degenerate_item(c) == 3
    assert (lp[3, 2:4] == np.float32(-3.0e38)).all() and np.isneginf(lp[3, 26]).all()
    assert np.array_equal(lp[2], np.round(lp[2] / np.float32(0.5)) * np.float32(0.5))
    which = "reference" if ou.have_reference() else "restated"
    want = ou.decode(lp, sl, which=which, **sm.oracle_args(c))
    base, ev0 = _matrix(0)
    ou.assert_same(base, want, "matrix inputs, run-time policy vs the %s oracle:" % which)
    for stage in (1, 2):
        got, ev = _matrix(stage)
        _same_everywhere(got, base, "matrix inputs, stage %d vs run-time policy" % stage)
        ou.assert_same(got, want, "matrix inputs, stage %d vs the %s oracle:" % (stage, which))
        assert ev == ev0, (stage, ev, ev0)
    # the overflow is what the degenerate item exercises: with -inf in place of -3e38 the oracle's result for that item changes
    lp_inf, sl_inf = xs.matrix_inputs(overflow_as_inf=True)
    d = km.degenerate_item(c)
    other = ou.decode(lp_inf[d:d + 1], sl_inf[d:d + 1], which=which, **sm.oracle_args(c))
    assert np.array_equal(sl_inf, sl)
    assert not (np.array_equal(other["scores"][0].view(np.uint32), want["scores"][d].view(np.uint32))
                and np.array_equal(other["tokens"][0], want["tokens"][d]) and np.array_equal(other["lens"][0], want["lens"][d])), \
        "-inf frames decode like the -3e38 frames: the overflow is not exercised"


def test_matrix_inputs_reach_the_select_paths():
    """Floors on the stage-2 counters of the matrix inputs: the ones every scorer-free kernel of the matrix is held to
    (test_select_paths.SCORER_FREE_FLOORS, SPEC_FLOOR -- imported, not restated), the slow path's third way and a revived slot at
    least as often as the scorer cases must, and more replays than utterances end.  Conditions on the INPUTS: if a change of the
    recipe misses one, the recipe changes, not the floor."""
    from test_select_paths import SCORER_FREE_FLOORS, SPEC_FLOOR

    lp, sl = xs.matrix_inputs()
    _, ev = _matrix(2)
    print("matrix inputs, stage 2:", ev)
    floors = dict(SCORER_FREE_FLOORS, EV_SLOW_BELOW=1, EV_REVIVED=5)
    for name in ("EV_SPEC_OK", "EV_SPEC_UNDER", "EV_SPEC_OVER", "EV_SPEC_OTHER"):
        floors[name] = SPEC_FLOOR
    for name, floor in floors.items():
        assert ev[name] >= floor, "matrix inputs: %s = %d, the inputs must give at least %d" % (name, ev[name], floor)
    # (every utterance of three or more frames replays in its last frame: anything beyond that is a tie or danger mode)
    assert ev["EV_EXACT"] > int((sl >= 3).sum()), ev
    assert ev["EV_FRAMES"] == int(np.clip(sl, 0, lp.shape[1]).sum())


def test_shape_list_and_tests_agree():
    """decode_kernel.h CTC_EXACT_SHAPES (product branch) is the table these tests cover: a second line there fails here until the
    tests -- exact_shape_util.SHAPES, the host twin, the GPU tests -- have been taught about it."""
    import os

    header = open(os.path.join(ou.ROOT, "ctcdecode_amd", "csrc", "decode_kernel.h")).read()
    assert xs.parse_exact_shapes(header) == xs.SHAPES
    assert len(xs.SHAPES) == 1 and xs.SHAPES[0][1:4] == (xs.BEAM, xs.LABELS, xs.BLANK)
    c = xs.matrix_case()
    assert c["kernel"] == xs.PARENT_KERNEL and (c["K"], c["V"], c["blank"]) == xs.SHAPES[0][1:4] and c["top_n"] >= c["V"] and c["cutoff_prob"] == 1.0
    # (the parser reads the product branch, not the measurement build's)
    two = header.replace("X(6, 100, 29, 0, true)", "X(6, 100, 29, 0, true) X(7, 64, 29, 0, true)")
    assert two != header and xs.parse_exact_shapes(two) == xs.SHAPES + [(7, 64, 29, 0, True)]
