"""The stream commit on the CPU: ctcdecode_amd/csrc/stream_commit.h (host build, sequential policy) run on the parked state of the
host build of the core between chunks.  The contract: a commit hands out the oracle's row 0 at the newly final positions (all of the
common prefix but its last label), re-roots the stream there and keeps exactly the oracle's live trie below the new root; from then on
every peek and the final result are the oracle's with the committed labels removed from the front of every row -- scores, result
counts and row order bit for bit; a second commit changes no byte."""
import os

import commit_util as mu
import compact_util as cu
import numpy as np
import oracle_util as ou
import peek_util as pu
import pytest

_WANTS = {}  # (input id, F, kw) -> the oracle's one-shot decode of the first F frames: computed once, shared, never written to


def _want_at(lp, kw, F, which):
    key = (id(lp), F, tuple(sorted(kw.items())), which)
    if key not in _WANTS:
        _WANTS[key] = (lp, pu.oracle_prefix(lp, F, which, **kw))  # (lp kept alive: its id stays its own)
    return _WANTS[key][1]


def _walk(lp, kw, bounds, every, frames_hint=None, order="commit", min_nodes=0):
    """Feed every item of lp chunk by chunk (bounds: frame boundaries, repeats = empty chunks); after every `every`-th chunk commit
    TWICE (count, labels, pool against the oracle; the second one commits nothing and changes no byte) -- order: "commit" alone,
    "commit+compact" or "compact+commit"; after every chunk peek with n_best in {1, K} and since in {0, stable'} against the oracle
    with the offset applied; the final result: committed ++ rows == the one-shot decode.  kw: the oracle's arguments, and the
    stream's (beam, cutoff_top_n, cutoff_prob, blank_id).  -> per item (commits that committed something, committed length, labels
    of row 0 left uncommitted)."""
    which = pu.which_oracle()
    B, T, V = lp.shape
    K = kw["beam"]
    final = _want_at(lp, kw, T, which)
    stats = []
    for b in range(B):
        st = mu.HostStream(V, K, frames_hint or T + 1, cutoff_prob=kw.get("cutoff_prob", 1.0), cutoff_top_n=kw.get("cutoff_top_n", 40),
                           blank_id=kw.get("blank_id", 0), min_nodes=min_nodes)
        frames = 0
        hits = 0

        def commit_twice(tag):
            what = "%s item %d F=%d" % (tag, b, frames)
            want = _want_at(lp, kw, frames, which)
            C = st.committed_len
            m = max(0, pu.common_prefix_len(want, b) - 1 - C)
            want_live = cu.oracle_live_count(want, b) - (C + m)  # (the root now stands for the dropped trunk)
            if order == "compact+commit":
                assert st.compact() == cu.oracle_live_count(want, b) - C, what
            tok, ts = st.commit()
            assert len(tok) == m, "%s: %d labels committed, want %d" % (what, len(tok), m)
            assert np.array_equal(tok, want["tokens"][b, 0, C:C + m]), "%s: committed tokens differ from the oracle's row 0" % what
            assert np.array_equal(ts, want["timesteps"][b, 0, C:C + m]), "%s: committed time steps differ from the oracle's row 0" % what
            assert st.live == want_live, "%s: %d nodes kept, want %d" % (what, st.live, want_live)
            if frames > 0:
                assert st.pool_count == want_live, "%s: pool count %d, want %d" % (what, st.pool_count, want_live)
                assert st.parents_below(), "%s: a parent index is not below its child's" % what
                assert st.bound == want_live, "%s: bound %d, live %d" % (what, st.bound, want_live)
            d0 = st.digest
            if order == "commit+compact":
                assert st.compact() == want_live and st.digest == d0, "%s: a compaction after the commit changed the block" % what
            tok2, _ = st.commit()
            assert len(tok2) == 0 and st.digest == d0, "%s: a second commit changed the block" % what
            return m

        def peek_all(tag):
            sh = mu.shifted(_want_at(lp, kw, frames, which), b, st.committed_len)
            stable = pu.common_prefix_len(sh, 0)
            for nb in sorted({1, K}):
                for since in sorted({0, stable}):
                    got, fits, _ = st.peek(nb, since)
                    assert fits
                    pu.assert_peek_equals(got, sh, 0, nb, since, "%s item %d F=%d C=%d n_best=%d since=%d" % (tag, b, frames, st.committed_len, nb, since))

        if bounds[0] == 0 and len(bounds) > 1 and bounds[1] == 0:
            commit_twice("zeroed state")  # before anything was fed: the block is zeroed memory
            peek_all("zeroed state")
        last = None
        for c in range(len(bounds) - 1):
            lo, hi = bounds[c], bounds[c + 1]
            end = c == len(bounds) - 2
            last = st.feed(lp[b, lo:hi], finish=end)
            frames = hi
            if not end:
                if c % every == every - 1:
                    hits += 1 if commit_twice("chunk %d" % c) > 0 else 0
                peek_all("chunk %d" % c)
        C = st.committed_len
        mu.assert_committed_prefix(final, b, st.tokens, st.timesteps, "item %d: committed" % b)
        mu.assert_final(last, final, b, C, "item %d: the final result after the commits" % b)
        stats.append((hits, C, int(final["lens"][b, 0]) - C))
    return stats


def _every(T, step=10):
    return list(range(0, T, step)) + [T]


CLASSES = pu.five_classes() + [pu.pruned_class()]


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("case", CLASSES, ids=lambda c: c["name"])
def test_commit_host_walk(case, every):
    T = case["lp"].shape[1]
    stats = _walk(case["lp"], case["kw"], _every(T), every)
    print(case["name"], every, stats)
    assert sum(1 for h, _, _ in stats if h > 0) >= 2, stats


def test_commits_are_long_and_fall_between_express_levels():
    """Non-vacuity, stated on the oracle alone (a commit after every 10 frames): at least two of the three items of every class
    commit; in randn, quantised, peaky_k100, peaky_k20 and pruned some item ends with a committed length that is no multiple of 32
    and at least 65 labels of row 0 uncommitted -- new express levels are written by the commit and by later chunks, and finish()
    reads them back; randn item 0 commits 195 of 212 labels."""
    which = pu.which_oracle()
    found = {}
    for case in CLASSES:
        lp, kw = case["lp"], case["kw"]
        B, T, V = lp.shape
        final = _want_at(lp, kw, T, which)
        per = []
        for b in range(B):
            C, hits = 0, 0
            for F in range(10, T, 10):
                m = max(0, pu.common_prefix_len(_want_at(lp, kw, F, which), b) - 1 - C)
                C += m
                hits += 1 if m else 0
            per.append((hits, C, int(final["lens"][b, 0]) - C))
        print(case["name"], per)
        found[case["name"]] = per
        assert sum(1 for h, _, _ in per if h > 0) >= 2, (case["name"], per)
        if case["name"] != "blank_dominated":
            assert any(C % 32 != 0 and left >= 65 for _, C, left in per), (case["name"], per)
    assert found["randn"][0][1:] == (195, 212 - 195), found["randn"]
    assert found["peaky_k100"][1][0] == 0 and found["pruned"][1][0] == 0  # (the only items that never commit)
    assert sum(1 for per in found.values() for h, _, _ in per if h == 0) == 2, found


def test_commit_host_ragged_chunks_empty_chunks_no_frames_and_one_entry():
    lp = ou.synth_logprobs(3, 100, 29, 66)
    bounds = [0, 0, 7, 7, 7, 30, 31, 64, 64, 100]
    # from a small frames_hint: the pool doubles between the commits
    stats = _walk(lp, dict(beam=30), bounds, 1, frames_hint=4)
    assert any(h > 0 for h, _, _ in stats), stats
    _walk(lp, dict(beam=30), bounds, 3, frames_hint=4)
    # a stream that is only ever fed empty chunks, committed in between, then ended: the root alone
    assert _walk(lp[:, :0], dict(beam=30), [0, 0, 0, 0], 1) == [(0, 0, 0)] * 3
    # a beam of one entry (n = 1): the stable length is its depth, and the commit leaves its last label
    stats = _walk(lp, dict(beam=1), bounds, 1, frames_hint=4)
    assert all(h > 0 for h, _, _ in stats), stats


@pytest.mark.parametrize("order", ["commit+compact", "compact+commit"])
def test_commit_host_interleaved_with_compact(order):
    case = CLASSES[0]
    stats = _walk(case["lp"], case["kw"], _every(case["lp"].shape[1]), 1, order=order)
    assert sum(1 for h, _, _ in stats if h > 0) >= 2, stats


def test_commit_host_with_the_compaction_policy_on():
    """min_nodes policy on, a small frames_hint: feed() compacts on its own between the commits; bound == live after every commit."""
    case = CLASSES[4]
    stats = _walk(case["lp"], case["kw"], _every(case["lp"].shape[1]), 3, frames_hint=4, min_nodes=1)
    assert sum(1 for h, _, _ in stats if h > 0) >= 2, stats


@pytest.mark.parametrize("beam", [4, 1])
def test_commit_host_timesteps_beyond_16_bits(beam):
    """Across frame 65535 with a commit on each side (65000 and 65600): the committed time steps are the oracle's absolute ones, and
    the kept nodes keep the high parts of theirs.  Beam 4: the common prefix ends before frame 65535, everything behind it is kept;
    beam 1 (one entry: all but its last label is final): labels past frame 65535 are committed."""
    T = 65536 + 300
    lp = ou.synth_logprobs(1, T, 5, 7, blank_bias=2.0)
    which = pu.which_oracle()
    st = mu.HostStream(5, beam, T + 1)
    for lo, hi in ((0, 65000), (65000, 65600)):
        st.feed(lp[0, lo:hi])
        want = pu.oracle_prefix(lp, hi, which, beam=beam)
        C = st.committed_len
        m = max(0, pu.common_prefix_len(want, 0) - 1 - C)
        tok, ts = st.commit()
        assert len(tok) == m > 0, (hi, len(tok), m)
        assert np.array_equal(tok, want["tokens"][0, 0, C:C + m]) and np.array_equal(ts, want["timesteps"][0, 0, C:C + m]), hi
        assert st.pool_count == cu.oracle_live_count(want, 0) - (C + m) and st.parents_below(), hi
        sh = mu.shifted(want, 0, C + m)
        got, fits, _ = st.peek(beam, 0)
        assert fits
        pu.assert_peek_equals(got, sh, 0, beam, 0, "F=%d" % hi)
        if hi > 65536:
            assert int(got["timesteps"].max()) > 65535
            assert max(st.node_thi(i) for i in range(st.pool_count)) == 1, "the kept nodes lost the high parts of their time steps"
    if beam == 1:
        assert int(st.timesteps.max()) > 65535, "no committed time step lies past frame 65535"
    last = st.feed(lp[0, 65600:], finish=True)
    final = pu.oracle_prefix(lp, T, which, beam=beam)
    mu.assert_committed_prefix(final, 0, st.tokens, st.timesteps, "T > 65536: committed")
    mu.assert_final(last, final, 0, st.committed_len, "T > 65536 after commits")
    assert int(last["timesteps"].max()) > 65535


def test_commit_host_refuses_a_stream_with_a_scorer():
    c = pu.LM_PEEK_CASES[0]
    lp, kw = pu.lm_case_inputs(c)
    path = os.path.join(pu.DATA, c["arpa"])
    st = mu.HostStream(len(c["labels"]), c["K"], c["T"] + 1, cutoff_top_n=kw["cutoff_top_n"], lm=(c["alpha"], c["beta"], path, c["labels"]))
    st.feed(lp[0, :60])
    d0 = st.digest
    with pytest.raises(NotImplementedError):
        st.commit()
    assert st.digest == d0 and st.committed_len == 0
    which = pu.which_oracle()
    sc = ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which)
    last = st.feed(lp[0, 60:], finish=True)
    want = ou.decode(lp, which=which, scorer=sc, **kw)
    ou.assert_same(last, dict((k, v[0:1]) for k, v in want.items()), "the refused stream decodes on")
