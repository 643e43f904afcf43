"""The streamed kernel matrix on the CPU (tests/stream_matrix_util.py): its table covers exactly the keys of CTC_KERNEL_LIST a stream
can launch, the host's planner (launch_plan.h plan_launch, through the core's host build) plans each entry's kernel from the entry's
arguments, switches and batch size, and the chunk bounds put at least two boundaries of every scorer-free entry directly behind a
frame in which item 2 replayed std::nth_element (a condition of the inputs, checked on the host twin)."""
import os

import pytest

import kernel_matrix_util as km
import stream_matrix_util as sm
from test_launch_plan import CU_COUNT, plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_table_covers_the_stream_reachable_keys_exactly():
    listed = km.parse_kernel_list(open(os.path.join(ROOT, "ctcdecode_amd", "csrc", "decode_kernel.h")).read())
    reachable = [k for k in listed if sm.stream_reachable(k)]
    assert len(reachable) == len(set(reachable)) == 46
    plain = [e["kernel"] for e in sm.STREAM_CASES if not e["production"]]
    assert sorted(plain) == sorted(reachable), "the table and the stream-reachable keys of CTC_KERNEL_LIST differ"
    # one more entry per OCC2 key, reached through the batch size alone
    serving = [e["kernel"] for e in sm.STREAM_CASES if e["production"]]
    assert sorted(serving) == sorted(k for k in reachable if k[6])
    for e in sm.STREAM_CASES:
        c = e["case"]
        assert not c["profile"] and not c["streamed"]
        if e["production"]:
            assert c["cu_sharing"] == -1 and (c["K"], c["T"]) == (sm.PRODUCTION_K, sm.PRODUCTION_T) and c["V"] <= 29
    ids = [sm.entry_id(e) for e in sm.STREAM_CASES]
    assert len(set(ids)) == len(ids)
    assert set(sm.MID_BOUND) | set(sm.EXTRA_BOUND) <= set(ids)


@pytest.mark.parametrize("e", sm.STREAM_CASES, ids=sm.entry_id)
def test_plan_matches_stream_matrix(e):
    """What configure() sets on the streaming decoder plans the entry's kernel; a stream never passes frames_ready (streamed=False)."""
    c = sm.sized_case(e, CU_COUNT)
    rc, key, layout = plan(c["V"], c["K"], c["top_n"], c["cutoff_prob"], B=c["B"], threads=c["threads"] or 0, fixed=c["fixed"],
                           cu_sharing=c["cu_sharing"], subtree=c["subtree"], scorer=km.scorer_kind(c), streamed=False)
    assert rc == 0, rc
    assert key == e["kernel"]
    assert layout == km.expected_layout(e["kernel"])
    if e["production"]:  # the same streams, fewer than the CUs: the plain build (what the hand-over test relies on)
        _, few, _ = plan(c["V"], c["K"], c["top_n"], c["cutoff_prob"], B=3, threads=c["threads"] or 0, fixed=c["fixed"],
                         cu_sharing=c["cu_sharing"], subtree=c["subtree"], scorer=km.scorer_kind(c), streamed=False)
        assert few == e["kernel"][:6] + (0,)


@pytest.mark.parametrize("e", sm.STREAM_CASES, ids=sm.entry_id)
def test_bounds_keep_their_properties(e):
    c = e["case"]
    T, b = c["T"], sm.bounds(e)
    assert b[:4] == [0, 1, 3, 3] and b[-1] == T and b[-2] == (2 * T) // 3 + 1  # one-frame chunk, between the overflow frames, empty chunk
    assert sorted(b) == b and len(set(b)) == len(b) - 1  # (the empty chunk alone repeats a bound)
    assert (2 * T) // 3 >= 4, "the -inf frame lies behind the overflow frames"
    _, sl = km.inputs(dict(c, B=c["B"] or 4))
    assert sl[0] == T and sl[1] == 1 and sl[2] == max(2, (2 * T) // 3)
    lens = [sm.chunk_lens(sl, lo, hi) for lo, hi in zip(b, b[1:])]
    assert (sum(lens) == sl).all()  # every item's frames are fed exactly once


@pytest.mark.parametrize("e", [e for e in sm.STREAM_CASES if not e["case"]["lm"]], ids=sm.entry_id)
def test_two_boundaries_follow_a_replay(e):
    got = sm.tie_boundaries(e)
    print(sm.entry_id(e), "bounds", sm.bounds(e), "behind a replay frame of item 2:", got)
    assert len(got) >= 2, "bounds %s: only %s directly follow a frame in which item 2 replayed nth_element" % (sm.bounds(e), got)


@pytest.mark.parametrize("h", sm.HAND_OVERS, ids=sm.hand_over_id)
def test_plan_of_both_sides_of_a_hand_over(h):
    """Each side's switches (and batch size: all CU count + 8 streams, or three of them) plan that side's kernel, and the two differ."""
    assert h["kernel_x"] != h["kernel_y"] and h["cause"] in ("serving", "hook")
    for side, kernel in ((h["x"], h["kernel_x"]), (h["y"], h["kernel_y"])):
        c = dict(h["case"], **{k: v for k, v in side.items() if k != "few"})
        B = c["B"] if c["B"] else (3 if side.get("few") else CU_COUNT + sm.PRODUCTION_EXTRA)
        rc, key, _ = plan(c["V"], c["K"], c["top_n"], c["cutoff_prob"], B=B, threads=c["threads"] or 0, fixed=c["fixed"],
                          cu_sharing=c["cu_sharing"], subtree=c["subtree"], scorer=km.scorer_kind(c), streamed=False)
        assert rc == 0 and key == kernel, (side, key, kernel)


def test_plan_of_the_automatic_subtree_switch():
    a = sm.AUTO_SUBTREE
    for on, prof in ((False, 0), (True, 3)):
        assert plan(a["V"], a["K"], a["V"], B=a["B"], threads=a["threads"], subtree=-1, subtree_on=on)[1] == (prof, 0, 1, 0, 1024, 0, 0)
    assert a["bounds"][0] == 0 and a["blank_frames"] in a["bounds"]
