"""The streamed kernel matrix on the CPU (tests/stream_matrix_util.py): its table covers exactly the keys of CTC_KERNEL_LIST a stream
can launch, the host's planner (launch_plan.h plan_launch, through the core's host build) plans each entry's kernel from the entry's
arguments, switches and batch size, and the chunk bounds put at least two boundaries of every scorer-free entry directly behind a
frame in which item 2 replayed std::nth_element (a condition of the inputs, checked on the host twin).

The commit walks of test_gpu_stream_matrix.py rest on conditions of their inputs as well, proved here on the oracle alone: over
commit_inputs at commit_bounds at least two commits hand the fading item labels (the second one re-roots a re-rooted state) and row
0 keeps labels to the end, for all 20 scorer-free entries; the commit in front of every hand-over hands the fading item labels; every
deep walk ends between two express levels with more than one level's labels uncommitted.  And the host twin (stream_commit.h on the
host build of the core) walks the same inputs -- the overflowed, the one-frame and the tie item among them -- before any GPU does.

The scorer entries are streamed over select_path_inputs (tests/select_path_util.py, test_gpu_select_paths.py): their bounds keep the
list's properties, at least two of them directly follow a frame in which item 0 or item 2 replayed std::nth_element although it was no
decode's last frame, and one lies between the two overflow frames of item 0."""
import os

import pytest

import kernel_matrix_util as km
import numpy as np
import peek_util as pu
import select_path_util as sp
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


@pytest.fixture(scope="module")
def wide99(tmp_path_factory):
    from test_lm import make_wide_label_lm

    return make_wide_label_lm(tmp_path_factory.mktemp("stream_matrix_plan_lm"))


def test_select_path_tables_cover_the_scorer_entries():
    entries = sp.stream_entries()
    assert len(entries) == 26 and sorted(e["kernel"] for e in entries) == sorted(c["kernel"] for c in sp.scorer_cases())
    ids = [sm.entry_id(e) for e in entries]
    assert set(sm.SELECT_PATH_EXTRA) <= set(ids) and set(sm.ITEM2_AT_MID) <= set(ids) and not set(sm.SELECT_PATH_EXTRA) & set(sm.ITEM2_AT_MID)
    assert len(sm.SELECT_PATH_EXTRA) + len(sm.ITEM2_AT_MID) >= 12  # (every HBM level and both layouts among them)
    assert set(e["kernel"][1] for e in entries if sm.entry_id(e) in sm.SELECT_PATH_EXTRA) == {0, 1, 2}


@pytest.mark.parametrize("e", sp.stream_entries(), ids=sm.entry_id)
def test_select_path_bounds_follow_replays(monkeypatch, wide99, e):
    """On the host twin, instantiated as the entry's own class: the replays of item 0 and item 2 that are no decode's last frame."""
    c = e["case"]
    T, eid = c["T"], sm.entry_id(e)
    b = sp.select_path_bounds(e)
    assert b[:4] == [0, 1, 3, 3] and b[-1] == T and b[-2] == (2 * T) // 3 + 1 and T // 2 in b
    assert sorted(b) == b and len(set(b)) == len(b) - 1  # (the empty chunk alone repeats a bound)
    lm = km.lm_spec(c, *wide99)
    lp, sl = sp.select_path_inputs(c, lm[1])
    assert sl[0] == T and (lp[0, 2:4] == np.float32(-3.0e38)).all() and 3 in b  # the bound 3 parts the two overflow frames of item 0
    assert (sum(sm.chunk_lens(sl, lo, hi) for lo, hi in zip(b, b[1:])) == sl).all()  # every item's frames are fed exactly once
    sp.set_host_env(c, monkeypatch.setenv, lambda name: monkeypatch.delenv(name, raising=False))
    got = sp.replay_boundaries(e, lm)
    print(eid, "bounds", b, "behind a replay frame of item 0:", got[0], "of item 2:", got[2])
    assert len(set(got[0]) | set(got[2])) >= 2, "bounds %s: only %s directly follow a replay of item 0 or item 2" % (b, got)
    assert got[0], "item 0 is in danger mode behind its overflow frames: %s" % (got,)
    if eid in sm.SELECT_PATH_EXTRA:
        assert sm.SELECT_PATH_EXTRA[eid] in got[2], (b, got)
    if eid in sm.ITEM2_AT_MID:
        assert T // 2 in got[2], (b, got)


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


# ---- the commit walks: what their inputs must give, on the oracle alone -------------------------------------------------------------
SCORER_FREE = [e for e in sm.STREAM_CASES if not e["production"] and not e["case"]["lm"]]
SCORER_FREE_HAND_OVERS = [h for h in sm.HAND_OVERS if not h["case"]["lm"]]


def test_commit_tables_cover_the_scorer_free_entries():
    assert len(SCORER_FREE) == 20 and len(SCORER_FREE_HAND_OVERS) == 8
    ids = [sm.entry_id(e) for e in SCORER_FREE]
    assert set(sm.COMMIT_BOUND) <= set(ids)
    assert set(sm.HAND_OVER_COMMIT_MID) <= set(h["name"] for h in SCORER_FREE_HAND_OVERS)
    for e in SCORER_FREE:
        c = e["case"]
        b, plain = sm.commit_bounds(e), sm.bounds(e)
        assert set(plain) <= set(b) and 0 <= len(b) - len(plain) <= 2 and all(3 < x < c["T"] for x in set(b) - set(plain))
        lp, sl = sm.commit_inputs(c)
        lp0, sl0 = km.inputs(c)
        f = sm.fading_index(c)
        assert lp.shape == (c["B"] + 1, c["T"], c["V"]) and lp.dtype == np.float32 and f == c["B"] and sl[f] == c["T"]
        assert np.array_equal(lp[:f].view(np.uint32), lp0.view(np.uint32)) and np.array_equal(sl[:f], sl0)
        # the fading item: even frames peak on a label, odd frames on the blank (where the margin still exceeds the noise), and the margin falls
        top = lp[f].argmax(axis=-1)
        assert (top[1:c["T"] // 2:2] == c["blank"]).all() and (top[0:c["T"] // 2:2] != c["blank"]).all()
        part = np.sort(lp[f], axis=-1)
        margin = part[:, -1] - part[:, -2]
        assert margin[0] > 35 and margin[-1] < 3 and margin[c["T"] // 2] < margin[0] - 10
    keys = [d["kernel"] for d in sm.DEEP_WALKS]
    assert sorted(keys) == sorted([(0, 0, 1, 0, 1024, 0, 1), (3, 0, 1, 0, 1024, 0, 0), (0, 0, 2, 1, 1024, 0, 0), (0, 2, 0, 0, 0, 0, 0)])
    assert 96 <= sm.DEEP_T <= 128 and sm.DEEP_CHUNK == 16


@pytest.mark.parametrize("e", SCORER_FREE, ids=sm.entry_id)
def test_commit_walk_commits_twice(e):
    """The GPU walk's rule -- a commit after every chunk that is not the last -- on the oracle: at least two commits hand the fading
    item a label, the second of them at committed_len > 0 (a re-rooted state is re-rooted again), and at the stream's end row 0 keeps
    at least 2 uncommitted labels.  Every scorer-free entry, none left out."""
    c = e["case"]
    lp, sl = sm.commit_inputs(c)
    f = sm.fading_index(c)
    kw = sm.oracle_args(c)
    b = sm.commit_bounds(e)
    ev = sm.commit_events(lp, f, b[1:-1], **kw)
    hits = [x for x in ev if x[1] > 0]
    final = pu.oracle_prefix(lp[f:f + 1], c["T"], "restated", **kw)
    left = int(final["lens"][0, 0]) - (ev[-1][1] + ev[-1][2])
    print(sm.entry_id(e), "bounds", b, "(frame, labels handed out, committed before):", ev, "left at the end:", left)
    assert len(hits) >= 2, "bounds %s: %s" % (b, ev)
    assert hits[1][2] > 0
    assert left >= 2, left


@pytest.mark.parametrize("e", [e for e in SCORER_FREE if sm.host_twin_builds(e["case"])], ids=sm.entry_id)
def test_commit_host_walk_over_the_matrix_inputs(e):
    """commit_inputs at commit_bounds through the host twin (test_stream_commit_host._walk: a commit after every chunk but the last,
    twice; counts, labels, time steps, kept nodes, peeks and the end against the oracle), every item at its own length, with the
    entry's beam, cutoff_top_n, cutoff_prob and blank."""
    from test_stream_commit_host import _walk

    c = e["case"]
    lp, sl = sm.commit_inputs(c)
    f = sm.fading_index(c)
    kw = sm.oracle_args(c)
    b = sm.commit_bounds(e)
    for i in range(lp.shape[0]):
        n = int(sl[i])
        stats = _walk(np.ascontiguousarray(lp[i:i + 1, :n]), kw, [min(x, n) for x in b], 1)
        print(sm.entry_id(e), "item", i, "length", n, "(commits that handed out labels, committed, left):", stats)
        if i == f:
            assert stats[0][0] >= 2 and stats[0][2] >= 2, stats


def test_host_twin_builds_all_but_the_widest_layout():
    skipped = [e["kernel"] for e in SCORER_FREE if not sm.host_twin_builds(e["case"])]
    assert sorted(skipped) == [(0, 3, 0, 0, 0, 0, 0), (0, 3, 0, 1, 0, 0, 0)], skipped


@pytest.mark.parametrize("h", SCORER_FREE_HAND_OVERS, ids=sm.hand_over_id)
def test_commit_in_front_of_a_hand_over_commits(h):
    """The commit at the hand-over's bound hands the fading item a label; the streams of a `few` side (the fading item among them) still
    plan that side's kernel."""
    c = dict(h["case"], B=h["case"]["B"] or CU_COUNT + sm.PRODUCTION_EXTRA)
    lp, sl = sm.commit_inputs(c)
    f = sm.fading_index(c)
    mid = sm.hand_over_commit_mid(h)
    b = sm.hand_over_commit_bounds(h)
    assert mid in b and b[:4] == [0, 1, 3, 3] and b[-1] == c["T"]
    ev = sm.commit_events(lp, f, [mid], **sm.oracle_args(c))
    print(h["name"], "bounds", b, "the commit at frame %d hands the fading item %d labels" % (mid, ev[0][1]))
    assert ev[0][1] > 0, ev
    few = sm.hand_over_few(c)
    assert f in few and len(few) == len(set(few)) <= 4
    for side, kernel in ((h["x"], h["kernel_x"]), (h["y"], h["kernel_y"])):
        cs = dict(c, **{k: v for k, v in side.items() if k != "few"})
        B = len(few) if side.get("few") else c["B"] + 1
        rc, key, _ = plan(cs["V"], cs["K"], cs["top_n"], cs["cutoff_prob"], B=B, threads=cs["threads"] or 0, fixed=cs["fixed"],
                          cu_sharing=cs["cu_sharing"], subtree=cs["subtree"], scorer=km.scorer_kind(cs), streamed=False)
        assert rc == 0 and key == kernel, (side, key, kernel)


def _deep_stats(d):
    """Per stream of a deep walk, on the oracle: [(frame, labels handed out, committed before, labels of row 0 left behind the
    commit)] and the labels left at the end."""
    c, lp, b = sm.deep_inputs(d)
    kw = sm.oracle_args(c)
    out = []
    for i in range(lp.shape[0]):
        ev = sm.commit_events(lp, i, b[1:-1], **kw)
        left = [int(pu.oracle_prefix(lp[i:i + 1], F, "restated", **kw)["lens"][0, 0]) - (m + C) for F, m, C in ev]
        final = int(pu.oracle_prefix(lp[i:i + 1], sm.DEEP_T, "restated", **kw)["lens"][0, 0])
        out.append(([x + (l,) for x, l in zip(ev, left)], ev[-1][1] + ev[-1][2], final - (ev[-1][1] + ev[-1][2])))
    return out


@pytest.mark.parametrize("d", sm.DEEP_WALKS, ids=sm.deep_walk_id)
def test_deep_walks_end_between_express_levels(d):
    """Some stream of the deep walk ends with a committed length that is no multiple of 32 and at least 33 labels of row 0
    uncommitted: the express levels of the re-rooted coordinates are written (by the commit's layout and by later chunks) and read
    back by finish().  deep_commit: a commit itself hands out labels and leaves such a state."""
    stats = _deep_stats(d)
    for i, (ev, C, left) in enumerate(stats):
        print(sm.deep_walk_id(d), "stream", i, "(frame, handed out, committed before, left):", ev, "committed", C, "left at the end", left)
    assert any(C % 32 != 0 and left >= 33 for _, C, left in stats), stats
    assert all(sum(1 for x in ev if x[1] > 0) >= 2 for ev, _, _ in stats), stats
    if d["deep_commit"]:
        assert any(m > 0 and (C + m) % 32 != 0 and l >= 33 for ev, _, _ in stats for _, m, C, l in ev), stats


@pytest.mark.parametrize("d", sm.DEEP_WALKS, ids=sm.deep_walk_id)
def test_commit_host_walk_over_the_deep_inputs(d):
    from test_stream_commit_host import _walk

    c, lp, b = sm.deep_inputs(d)
    assert sm.host_twin_builds(c)
    stats = _walk(lp, sm.oracle_args(c), b, 1)
    print(sm.deep_walk_id(d), stats)
    assert any(C % 32 != 0 and left >= 33 for _, C, left in stats), stats
