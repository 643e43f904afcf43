"""Keyword search of live streams on the CPU (include/ctcdecode_amd.h "Keyword search of live streams"): the host twin of
keyword_stream.h, fed chunk by chunk, against the one-shot restatement of tests/keyword_util.py on the concatenation, bit for bit."""
import numpy as np
import pytest

import greedy_util as gu
import keyword_stream_util as su
import keyword_util as ku

T, V = 70, 29
CUTS = ([70], [1] * 70, [31, 1, 32, 6], [0, 33, 0, 37])


def _play(stored, x, dtype, cuts, kws, blank, mode, first, pad=2):
    """Feeds the cuts of item 0 (each call's tensor ``pad`` frames longer than its chunk), then ends the stream on an empty call; every
    call is checked on the way.  -> the last call's results."""
    st, lo = su.HostStream(kws, first), 0
    want = su.want_of(x, x.shape[0], blank, mode, kws, first)  # (the one-shot result of the concatenation, computed once)
    for n in list(cuts) + [0]:
        eos = lo == x.shape[0] and n == 0
        chunk = np.concatenate([stored[lo:lo + n], stored[:pad]])  # (the rows behind a chunk's length are never read into a result)
        got, status = st.feed(chunk, dtype, n, x.shape[1], blank, mode, eos)
        su.check_call(got, want, lo, n, first, "call at frame %d" % lo)
        # the running result: the header's walk over the one-shot traces of the frames so far
        ku.assert_same(got, dict(zip(su.KEYS[:3], su.chunk_walk(want, 0, lo + n, first).values())), "running result after %d frames" % (lo + n))
        assert not status.any() and st.frames == lo + n
        lo += n
    assert st.ended
    ku.assert_same(got, {k: want[k] for k in su.KEYS[:3]}, "the last call against the one-shot result")
    return got


@pytest.mark.parametrize("first", (0, 1000))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("L", (1, 8, 9, 16, 17, 33, 64))
@pytest.mark.parametrize("cuts", CUTS, ids=lambda c: "cut%d" % len(c))
def test_cuts_equal_the_one_shot_result(cuts, L, mode, first):
    c = ku.case("stream L%d" % L, dtype=L % 3, mode=mode, V=V, T=T, B=1, L=(L, max(1, L - 2)))
    _play(c["stored"][0], c["x"][0], c["dtype"], cuts, c["kws"], c["blank"], mode, first)


@pytest.mark.parametrize("mode", (0, 1))
def test_a_cut_inside_an_occurrence_keeps_the_start_an_earlier_call_saw(mode):
    path = [0, 0, 1, 1, 0, 2, 2, 3, 0, 0, 4, 0]  # blank 0: the occurrence 1 2 3 spans frames 2 .. 7
    x = gu.path_rows(np.random.default_rng(11 + mode), [path], 6, mode)[0]
    got = _play(x, x, 0, [4, 2, 6], [[1, 2, 3], [2, 3]], 0, mode, 500)
    assert gu.bits1(got["scores"][0]) == 0 and (got["starts"][0], got["ends"][0]) == (502, 507)
    assert (got["starts"][1], got["ends"][1]) == (505, 507)


def test_invalid_keywords_every_call_and_the_record_size():
    lib = su.host_lib()
    assert [lib.ctckws_host_state_bytes(Q, L) for Q, L in ((1, 1), (3, 8), (3, 9), (2, 64))] == [32 + 16 + 128, 32 + 48 + 384, 32 + 48 + 768, 32 + 32 + 2048]
    assert not lib.ctckws_host_new(1, 65, 0) and not lib.ctckws_host_new(1, 8, 2 ** 31)
    x = gu.random_rows(np.random.default_rng(2), 1, 6, 9, 1)[0]  # blank 8
    st = su.HostStream([[3], [8], [9], [3, -1], []], Lk=2)
    for n in (4, 2):
        got, status = st.feed(x[:n], 0, n, 9, 8, 1)
        assert status.tolist() == [0, 8, 8, 8, 8]
        assert (got["scores"][1:] == 0).all() and (got["starts"][1:] == -1).all() and (got["ends"][1:] == -1).all() and not got["end_scores"][1:].any()
        assert (got["chunk_scores"][1:] == 0).all() and (got["chunk_ends"][1:] == -1).all()
