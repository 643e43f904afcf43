"""The exact-shape policy of the decoder core (beam_core.h ShapeExact<100, 29, 0>) on the CPU: stage 1 (beam width, label count,
blank rank as constants) and stage 2 (the live beam size as well, once the beam is full) against the run-time policy and the oracle,
bit for bit, with every assumption the policy hands the optimiser checked (tests/native/exact_shape_host.cpp, -DCTC_ASSUME_CHECKED).
The inputs are the ones the GPU test sends through the twin kernel (exact_shape_util.cases); the event counters certify that they
reach the select's paths."""
import numpy as np
import pytest

import exact_shape_util as xs
import oracle_util as ou

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
