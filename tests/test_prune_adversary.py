"""The certificates of the adversarial prune rows (tests/prune_adversary_util.py): every case's killer frames really drive the std::sort
replay where the case says -- the heap sort on one range longer than big_cut, the heap sort on a range up to big_cut, a long right side
that must be left alone, rows at the introsort threshold -- so that test_gpu_prune_adversary.py runs those branches of
sort_prefix_parallel / sort_parallel on the device for the first time.  The certificate walks the recursion with stl_emul.h's serial
primitives (tests/native/prune_adversary.cpp) and checks its own result against the live std::sort.  The same rows go through the
per-frame prune oracles: the reference's get_pruned_log_probs (or its restatement) and the host twin of the product's core agree."""
import numpy as np
import pytest

import oracle_util as ou
import prune_adversary_util as pa


def _frames(c):
    certs = pa.certificates(c)
    return [(b, t, pa.frame_kind(b, t), certs[b][t]) for b in range(pa.B) for t in range(pa.T)]


@pytest.mark.parametrize("c", pa.CASES, ids=pa.case_id)
def test_certificate(c):
    what = pa.case_id(c)
    n_adv = 0
    for b, t, kind, q in _frames(c):
        at = "%s frame (%d, %d) %s: %s" % (what, b, t, kind, q)
        assert q["walk_ok"] == 1, at  # (the walk's kept places are std::sort's: the certificate describes the real recursion)
        assert q["max_pending"] < pa.BSTACK_SLOTS, at
        assert q["max_tasks"] <= c["V"] // 17 + 2, at  # (prune_resolve_task_cap)
        if kind == "benign":
            # the baseline next to the killer: the same values in random order never come near the depth limit
            assert q["long_heaps"] == 0 and q["short_heaps"] == 0, at
            continue
        n_adv += 1
        assert pa.in_cell(c, q), at
        # fold > 1: equal values straddle the cut, so nothing but the replay can settle the frame.  fold 1 cannot tie there.
        if c["top_n"] < c["V"]:
            assert q["tie_at_cut"] == (1 if c["fold"] > 1 else 0), at
    assert n_adv >= pa.B * pa.T // 2


def test_every_cell_is_certified():
    """>= 1 certified, flagged frame per named cell and per layout of the replay's arrays; the figures of the issue's table."""
    seen = {}
    for c in pa.CASES:
        for b, t, kind, q in _frames(c):
            if kind == "adversarial" and pa.in_cell(c, q) and (q["tie_at_cut"] or c["tie_top"] or c["cell"] == "boundary"):
                key = (c["cell"], c["resolve_global"])
                seen[key] = seen.get(key, 0) + 1
    print("certified frames per (cell, arrays in global memory):", seen)
    for key in [("long", False), ("short", False), ("right", False), ("boundary", False), ("long", True), ("short", True)]:
        assert seen.get(key, 0) >= 1, key
    # (V, top_n) -> workgroup rounds and the one heap-sorted range of the descending killer, fold 1 and fold 2 alike
    for V, top_n, rounds, heap in [(300, 7, 16, 269), (1000, 39, 18, 965), (1026, 39, 20, 987), (4096, 63, 24, 4049)]:
        for fold in (1, 2):
            q = pa.certificate(pa.values_of_ranks(pa.killer(V, True, fold), "f32", 1), top_n)
            assert (q["wg_rounds"], q["long_heaps"], q["long_heap_max"], q["short_heaps"]) == (rounds, 1, heap, 0), (V, fold, q)
    for V, wg, th in [(16, 0, 0), (17, 0, 1), (18, 0, 2), (256, 0, None), (257, 1, None), (258, 2, None), (272, 9, None)]:
        q = pa.certificate(pa.values_of_ranks(pa.killer(V, True, 2), "f32", 1), 7)
        assert q["wg_rounds"] == wg and (th is None or q["thread_rounds"] == th), (V, q)
        assert q["short_heaps"] == (1 if V > 18 else 0) and q["long_heaps"] == 0, (V, q)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("li", [0, 1])
def test_values_carry_the_rank_order(dt, li):
    """Consecutive representable values: distinct ranks give distinct values in the same order, in every dtype, at the longest row."""
    r = pa.killer(5000, True, 1)
    v = pa.values_of_ranks(r, dt, li, offset=5)
    assert np.array_equal(np.argsort(r, kind="stable"), np.argsort(v, kind="stable")) and len(np.unique(v)) == 5000
    import prepass_matrix_util as pm

    assert np.array_equal(pm.round_to(v, dt).view(np.uint32), v.view(np.uint32))  # representable in dt
    assert np.all(np.isfinite(v)) and (np.all(v < 0) if li else np.all((v > 0) & (v < 1)))


def _oracle_name():
    return "reference" if ou.have_reference_prune() else "restated"


@pytest.mark.parametrize("c", [c for c in pa.CASES if not c["resolve_global"]], ids=pa.case_id)
def test_prune_oracles_agree(c):
    """The case's rows through the per-frame prune: the reference (its restatement where oracle/_ref is not built) against the host twin of
    the product's core -- log-probability rows; the twin does not prune probabilities -- and against the restatement."""
    x, xo, shift = pa.inputs(c)
    li = c["li"]
    want = ou.pruned_rows(xo, c["cp"], c["top_n"], li != 0, which=_oracle_name())
    ou.assert_same_pruned(ou.pruned_rows(xo, c["cp"], c["top_n"], li != 0, which="restated"), want, pa.case_id(c) + " restated")
    if li != 0:
        ou.assert_same_pruned(ou.pruned_rows(xo, c["cp"], c["top_n"], True, which="host"), want, pa.case_id(c) + " host twin")
    if c["cp"] >= 1.0:
        assert np.all(want[0] == min(c["top_n"], c["V"]))
    else:
        assert np.all(want[0] < min(c["top_n"], c["V"])) and np.all(want[0] >= 2)  # the cumulative cut stops inside the sorted prefix


def test_logits_case_certifies_what_it_claims():
    """Raw logits: normalising could merge neighbouring values and break the killer.  The spacing inputs() settled on keeps it whole: the
    log-softmax rows certify the long-range heap and still tie across the cut."""
    (c,) = [c for c in pa.CASES if c["li"] == 2 and not c["resolve_global"]]
    x, xo, shift = pa.inputs(c)
    assert shift in pa.LOGIT_SHIFTS
    for b, t, kind, q in _frames(c):
        if kind == "adversarial":
            assert q["long_heaps"] == 1 and q["long_heap_max"] == 965 and q["tie_at_cut"] == 1, (shift, q)


@pytest.mark.parametrize("c", pa.CARRY, ids=lambda c: "frames%d_%s" % (c["frames"], "far" if c["resolve_global"] else "lds"))
def test_carry_batch(c):
    """More flagged frames than the replay has workgroups; every killer frame among them reaches the long-range heap."""
    x, kinds = pa.carry_inputs(c)
    n_flagged = n_adv = 0
    for b in range(2):
        for t in range(x.shape[1]):
            q = pa.certificate(x[b, t], c["top_n"])
            assert q["walk_ok"] == 1 and q["tie_at_cut"] == 1 and q["max_pending"] < pa.BSTACK_SLOTS
            n_flagged += 1
            if kinds[b][t] == "adversarial":
                assert q["long_heaps"] == 1 and q["long_heap_max"] == 269
                n_adv += 1
            else:
                assert q["long_heaps"] == 0 and q["short_heaps"] == 0
    assert n_flagged == c["frames"] > (64 if c["resolve_global"] else 256) and n_adv >= c["frames"] // 3
    want = ou.pruned_rows(x, 1.0, c["top_n"], True, which=_oracle_name())
    ou.assert_same_pruned(ou.pruned_rows(x, 1.0, c["top_n"], True, which="host"), want, "carry batch, host twin")
