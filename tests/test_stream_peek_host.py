"""The streaming peek on the CPU: ctcdecode_amd/csrc/stream_peek.h (host build, sequential policy) run on the parked state of the
host build of the core between chunks, against the oracle's one-shot decode of the frames fed so far -- the contract of a peek:
rows, scores, lengths, n_results bit for bit, stable_len = the common prefix of ALL oracle beams; peeks disturb nothing."""
import os

import numpy as np
import oracle_util as ou
import peek_util as pu
import pytest


def _walk(lp, kw, bounds, lm=None, scorer=None, which=None, n_bests=None, stats=None):
    """Feed every item of lp chunk by chunk (bounds: frame boundaries, repeats = empty chunks), peek after every chunk with n_best in
    n_bests and since in {0, the previous stable_len}, compare with the oracle; check the stable prefix's properties along the way and
    the final result against the one-shot decode.  stats (a list) collects (frames, oracle common prefix) per item and peek."""
    which = which or pu.which_oracle()
    B, T, V = lp.shape
    K = kw["beam"]
    n_bests = n_bests or sorted({1, min(3, K), K})
    okw = dict(kw)
    wants = {}

    def want_at(F):
        if F not in wants:
            wants[F] = pu.oracle_prefix(lp, F, which, scorer=scorer, **okw)
        return wants[F]

    final = want_at(T)
    for b in range(B):
        st = pu.HostStream(V, K, T + 1, cutoff_top_n=kw.get("cutoff_top_n", 40), lm=lm)
        prev_stable, pre_tok, pre_ts = 0, np.zeros((0,), np.int32), np.zeros((0,), np.int32)
        frames = 0

        def peek_all(tag):
            nonlocal prev_stable, pre_tok, pre_ts
            want = want_at(frames)
            stable = None
            for nb in n_bests:
                for since in sorted({0, prev_stable}):
                    got, fits, d0 = st.peek(nb, since)
                    _, _, d1 = st.peek(nb, since)
                    assert fits and d0 == d1, "%s: a peek changed the parked state" % tag
                    pu.assert_peek_equals(got, want, b, nb, since, "%s item %d F=%d n_best=%d since=%d" % (tag, b, frames, nb, since))
                    stable = got["stable"]
            # the properties: never shorter, and every beam of this peek begins with the earlier stable prefix
            assert stable >= prev_stable, "%s item %d F=%d: stable_len fell from %d to %d" % (tag, b, frames, prev_stable, stable)
            full, _, _ = st.peek(K, 0)
            res = dict(tokens=full["tokens"][None], timesteps=full["timesteps"][None], lens=full["lens"][None], nres=np.array([full["nres"]]))
            pu.assert_starts_with(res, 0, pre_tok, pre_ts, "%s item %d F=%d" % (tag, b, frames))
            if stats is not None:
                stats.append((b, frames, pu.common_prefix_len(want, b)))
            prev_stable = stable
            pre_tok, pre_ts = full["tokens"][0, :stable].copy(), full["timesteps"][0, :stable].copy()

        if bounds[0] == 0 and len(bounds) > 1 and bounds[1] == 0:
            peek_all("zeroed state")  # before anything was fed: the block is zeroed memory
        last = None
        for c in range(len(bounds) - 1):
            lo, hi = bounds[c], bounds[c + 1]
            end = c == len(bounds) - 2
            last = st.feed(lp[b, lo:hi], finish=end)
            frames = hi
            if not end:
                peek_all("chunk %d" % c)
        one = dict((k, v[b:b + 1]) for k, v in final.items())
        ou.assert_same(last, one, "item %d: the final result after the peeks" % b)
        pu.assert_starts_with(final, b, pre_tok, pre_ts, "item %d: final result" % b)


def _every(T, step=10):
    return list(range(0, T, step)) + [T]


@pytest.mark.parametrize("case", pu.five_classes() + [pu.pruned_class()], ids=lambda c: c["name"])
def test_peek_host_equals_one_shot_of_the_frames_so_far(case):
    _walk(case["lp"], case["kw"], _every(case["lp"].shape[1]))


def test_peek_host_ragged_chunks_empty_chunks_and_no_frames():
    lp = ou.synth_logprobs(3, 100, 29, 66)
    _walk(lp, dict(beam=30), [0, 0, 7, 7, 7, 30, 31, 64, 64, 100])
    # a stream that is only ever fed empty chunks, then ended: the root alone, peeked and final
    _walk(lp[:, :0], dict(beam=30), [0, 0, 0, 0])


def test_peek_host_timesteps_beyond_16_bits():
    """A small beam across frame 65535: the reported time steps come from the pool's high-part array as well."""
    T = 65536 + 300
    lp = ou.synth_logprobs(1, T, 5, 7, blank_bias=2.0)
    which = pu.which_oracle()
    st = pu.HostStream(5, 4, T + 1)
    for lo, hi, tag in ((0, 65000, "before"), (65000, 65600, "after")):
        st.feed(lp[0, lo:hi])
        want = pu.oracle_prefix(lp, hi, which, beam=4)
        got, fits, _ = st.peek(4, 0)
        assert fits
        pu.assert_peek_equals(got, want, 0, 4, 0, tag)
        tail, fits, _ = st.peek(1, got["stable"])
        pu.assert_peek_equals(tail, want, 0, 1, got["stable"], tag + " since=stable")
    assert int(got["timesteps"].max()) > 65535
    last = st.feed(lp[0, 65600:], finish=True)
    ou.assert_same(last, pu.oracle_prefix(lp, T, which, beam=4), "T > 65536 after peeks")


def test_stable_prefix_is_not_vacuous():
    """The condition on the inputs, stated on the oracle alone: over the five classes, peeked every 10 frames from frame 10 on, the
    oracle's own common prefix is longer than zero in at least 80 % of the peeks, and one stream ends with more than 20 stable labels."""
    which = pu.which_oracle()
    total = nonzero = 0
    longest = 0
    for case in pu.five_classes():
        lp = case["lp"]
        B, T, V = lp.shape
        for F in range(10, T + 1, 10):
            want = pu.oracle_prefix(lp, F, which, **case["kw"])
            for b in range(B):
                m = pu.common_prefix_len(want, b)
                total += 1
                nonzero += 1 if m > 0 else 0
                if F == T:
                    longest = max(longest, m)
    print("oracle common prefix > 0 in %d of %d peeks; longest final stable prefix %d" % (nonzero, total, longest))
    assert nonzero >= 0.8 * total, (nonzero, total)
    assert longest > 20, longest


@pytest.mark.parametrize("c", pu.LM_PEEK_CASES, ids=lambda c: c["name"])
def test_peek_host_with_the_built_in_scorer(c):
    lp, kw = pu.lm_case_inputs(c)
    path = os.path.join(pu.DATA, c["arpa"])
    which = pu.which_oracle()
    sc = ou.Scorer(c["alpha"], c["beta"], path, c["labels"], which)
    _walk(lp, kw, [0, 0] + _every(c["T"])[1:], lm=(c["alpha"], c["beta"], path, c["labels"]), scorer=sc, which=which)


def test_peek_host_row_overflow_is_reported_not_cut():
    lp = ou.synth_logprobs(1, 60, 29, 67)
    st = pu.HostStream(29, 10, 61)
    st.feed(lp[0])
    full, fits, _ = st.peek(3, 0)
    assert fits and int(full["lens"].max()) > 4
    got, fits, _ = st.peek(3, 0, L_cap=int(full["lens"][:3].max()) - 1)
    assert not fits
    assert not got["tokens"].any() and not got["timesteps"].any(), "an overflowing stream writes no labels"
    got, fits, _ = st.peek(3, 0, L_cap=int(full["lens"][:3].max()))
    assert fits and np.array_equal(got["tokens"], full["tokens"][:, :got["tokens"].shape[1]])
