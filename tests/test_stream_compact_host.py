"""The stream compaction on the CPU: ctcdecode_amd/csrc/stream_compact.h (host build, sequential policy) run on the parked state of
the host build of the core between chunks.  The contract: nothing a later call computes changes -- every peek and the final result
equal the oracle's one-shot decode bit for bit, compacted or not, however often and wherever; what is kept is exactly the trie the
oracle's own result rows span; a second compaction changes no byte; and with the policy on a stream's capacity follows its live set."""
import os

import compact_util as cu
import numpy as np
import oracle_util as ou
import peek_util as pu
import pytest


def _walk(lp, kw, bounds, every, lm=None, scorer=None, which=None, frames_hint=None):
    """Feed every item of lp chunk by chunk (bounds: frame boundaries, repeats = empty chunks); after every `every`-th chunk compact
    TWICE (count and pool against the oracle's live set, parents below children, the second run changes no byte); after every chunk
    peek with n_best in {1, K} and since in {0, stable} against the oracle; the final result against the one-shot decode."""
    which = which or pu.which_oracle()
    B, T, V = lp.shape
    K = kw["beam"]
    wants = {}

    def want_at(F):
        if F not in wants:
            wants[F] = pu.oracle_prefix(lp, F, which, scorer=scorer, **kw)
        return wants[F]

    final = want_at(T)
    compacted = 0
    for b in range(B):
        st = cu.HostStream(V, K, frames_hint or T + 1, cutoff_top_n=kw.get("cutoff_top_n", 40), lm=lm)
        frames = 0

        def compact_twice(tag):
            want_live = cu.oracle_live_count(want_at(frames), b)
            live = st.compact()
            assert live == want_live, "%s item %d F=%d: %d nodes kept, the oracle's rows span %d" % (tag, b, frames, live, want_live)
            if frames > 0:
                assert st.pool_count == want_live, "%s item %d F=%d: pool count %d, want %d" % (tag, b, frames, st.pool_count, want_live)
                assert st.parents_below(), "%s item %d F=%d: a parent index is not below its child's" % (tag, b, frames)
                assert st.bound == want_live
            d0 = st.digest
            assert st.compact() == live and st.digest == d0, "%s item %d F=%d: a second compaction changed the block" % (tag, b, frames)

        def peek_all(tag):
            want = want_at(frames)
            stable = pu.common_prefix_len(want, b)
            for nb in sorted({1, K}):
                for since in sorted({0, stable}):
                    got, fits, _ = st.peek(nb, since)
                    assert fits
                    pu.assert_peek_equals(got, want, b, nb, since, "%s item %d F=%d n_best=%d since=%d" % (tag, b, frames, nb, since))

        if bounds[0] == 0 and len(bounds) > 1 and bounds[1] == 0:
            compact_twice("zeroed state")  # before anything was fed: the block is zeroed memory
            peek_all("zeroed state")
        last = None
        for c in range(len(bounds) - 1):
            lo, hi = bounds[c], bounds[c + 1]
            end = c == len(bounds) - 2
            last = st.feed(lp[b, lo:hi], finish=end)
            frames = hi
            if not end:
                if c % every == every - 1:
                    compact_twice("chunk %d" % c)
                    compacted += 1
                peek_all("chunk %d" % c)
        one = dict((k, v[b:b + 1]) for k, v in final.items())
        ou.assert_same(last, one, "item %d: the final result after the compactions" % b)
    return compacted


def _every(T, step=10):
    return list(range(0, T, step)) + [T]


CLASSES = pu.five_classes() + [pu.pruned_class()]


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("case", CLASSES, ids=lambda c: c["name"])
def test_compact_host_changes_nothing_and_keeps_the_oracles_trie(case, every):
    T = case["lp"].shape[1]
    assert _walk(case["lp"], case["kw"], _every(T), every) > 0


def test_compact_host_ragged_chunks_empty_chunks_and_no_frames():
    lp = ou.synth_logprobs(3, 100, 29, 66)
    assert _walk(lp, dict(beam=30), [0, 0, 7, 7, 7, 30, 31, 64, 64, 100], 1) > 0
    # a stream that is only ever fed empty chunks, compacted in between, then ended: the root alone
    _walk(lp[:, :0], dict(beam=30), [0, 0, 0, 0], 1)
    # ... and from a small frames_hint: the pool doubles between the compactions
    assert _walk(lp, dict(beam=30), [0, 0, 7, 7, 7, 30, 31, 64, 64, 100], 3, frames_hint=4) > 0


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("c", pu.LM_PEEK_CASES, ids=lambda c: c["name"])
def test_compact_host_with_the_built_in_scorer(c, every):
    lp, kw = pu.lm_case_inputs(c)
    path = os.path.join(pu.DATA, c["arpa"])
    which = pu.which_oracle()
    sc = ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which)
    assert _walk(lp, kw, [0, 0] + _every(c["T"])[1:], every, lm=(c["alpha"], c["beta"], path, c["labels"]), scorer=sc, which=which) > 0


def test_live_set_is_a_small_part_of_the_pool():
    """Non-vacuity, stated on the oracle alone: at F in {T/4, T/2, T} the trie the oracle's rows span has at most 0.6 * (F * K + 1)
    nodes in every item of all six classes, and at most 0.05 * (F * K + 1) on the blank-dominated rows."""
    which = pu.which_oracle()
    worst = {}
    for case in CLASSES:
        lp = case["lp"]
        B, T, V = lp.shape
        K = case["kw"]["beam"]
        for F in (T // 4, T // 2, T):
            want = pu.oracle_prefix(lp, F, which, **case["kw"])
            for b in range(B):
                live = cu.oracle_live_count(want, b)
                ratio = live / float(F * K + 1)
                worst[case["name"]] = max(worst.get(case["name"], 0.0), ratio)
                print("%s item %d F=%d: live %d of %d (%.3f)" % (case["name"], b, F, live, F * K + 1, ratio))
                assert live <= 0.6 * (F * K + 1), (case["name"], b, F, live)
                if case["name"] == "blank_dominated":
                    assert live <= 0.05 * (F * K + 1), (b, F, live)
    print("worst live / capacity per class:", worst)


def test_compact_host_timesteps_beyond_16_bits():
    """A small beam across frame 65535, compacted at 65000 and at 65600: the kept nodes keep the high parts of their time steps."""
    T = 65536 + 300
    lp = ou.synth_logprobs(1, T, 5, 7, blank_bias=2.0)
    which = pu.which_oracle()
    st = cu.HostStream(5, 4, T + 1)
    got = None
    for lo, hi, tag in ((0, 65000, "before"), (65000, 65600, "after")):
        st.feed(lp[0, lo:hi])
        want = pu.oracle_prefix(lp, hi, which, beam=4)
        live = st.compact()
        assert live == cu.oracle_live_count(want, 0) == st.pool_count and st.parents_below(), tag
        got, fits, _ = st.peek(4, 0)
        assert fits
        pu.assert_peek_equals(got, want, 0, 4, 0, tag)
    assert int(got["timesteps"].max()) > 65535
    last = st.feed(lp[0, 65600:], finish=True)
    final = pu.oracle_prefix(lp, T, which, beam=4)
    ou.assert_same(last, final, "T > 65536 after compactions")
    assert int(last["timesteps"].max()) > 65535


def test_compact_host_policy_bounds_the_capacity():
    """A blank-dominated stream of 3000 frames in 100-frame chunks from frames_hint = 200, beam 10.  Policy on: the capacity never
    exceeds max(initial, 2 * (L_max + 100 * beam)) nodes, L_max = the largest oracle live count at the chunk boundaries.  Policy off:
    the same stream's capacity reaches 3000 * beam (today's behaviour).  Both end with the oracle's result."""
    T, V, K, chunk, hint = 3000, 29, 10, 100, 200
    lp = cu.blank_dominated_long(T, V)
    which = pu.which_oracle()
    final = pu.oracle_prefix(lp, T, which, beam=K)
    l_max = max(cu.oracle_live_count(pu.oracle_prefix(lp, F, which, beam=K), 0) for F in range(chunk, T, chunk))
    caps = {}
    for min_nodes in (1, 0):
        st = cu.HostStream(V, K, hint, min_nodes=min_nodes)
        initial = st.capacity
        assert initial == hint * K + 1
        peak = initial
        for lo in range(0, T, chunk):
            last = st.feed(lp[0, lo:lo + chunk], finish=lo + chunk == T)
            peak = max(peak, st.capacity)
            assert st.bound <= st.capacity
        ou.assert_same(last, final, "policy %s: the final result" % ("on" if min_nodes else "off"))
        caps[min_nodes] = (initial, peak, st.compactions)
    print("L_max %d; policy on: initial %d peak %d (%d compactions); off: peak %d" % (l_max, caps[1][0], caps[1][1], caps[1][2], caps[0][1]))
    assert caps[1][2] > 0, "the policy never compacted"
    assert caps[1][1] <= max(caps[1][0], 2 * (l_max + chunk * K)), (caps[1], l_max)
    assert caps[0][1] >= T * K and caps[0][2] == 0, caps[0]
