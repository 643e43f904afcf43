"""-m gpu tests of the greedy decode of live streams (``GreedyState``, ``OnlineCTCBeamDecoder.greedy_decode`` / ``greedy_decode_device``,
``ctcd_greedy_stream_*``): every call's device output == the slicing rule of the header applied to ``greedy_util.reference`` of all of
the stream's frames (tests/greedy_stream_util.py), bit for bit -- scores and label scores as uint32, labels and frames exactly.  The
scenarios are those of tests/test_greedy_stream_host.py; a reference is computed once per process.  Through the raw ABI the outputs
are pre-filled with a sentinel: every position is written."""
import greedy_stream_util as su
import greedy_util as gu
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch


_DECS = {}


def _dec(V, blank, mode):
    """One decoder per (V, blank, mode) and process."""
    import ctcdecode_amd

    key = (V, blank, mode)
    if key not in _DECS:
        _DECS[key] = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], blank_id=blank, beam_width=8, log_probs_input=mode == 1, logits_input=mode == 2)
    return _DECS[key]


def _numpy(outs):
    tok, sc, st, lens, en, ls, closed = (o.cpu().numpy() for o in outs)
    return dict(tokens=tok[:, 0], scores=sc[:, 0], starts=st[:, 0], lens=lens[:, 0], ends=en[:, 0], label_scores=ls[:, 0], closed_lens=closed[:, 0])


def _raw_call(torch, details=True):
    """A chunk call through the raw ABI: output tensors pre-filled with a sentinel."""
    import ctypes

    import ctcdecode_amd
    from ctcdecode_amd import _native

    def call(streams, eos, stored, seq_lens, sc):
        dec = _dec(sc["V"], sc["blank"], sc["mode"])
        B, Tc, V = stored.shape
        x = gu.to_torch(torch, stored, sc["dtype"])
        seq = None if seq_lens is None else torch.from_numpy(np.asarray(seq_lens, np.int32)).cuda()
        tok, st = (torch.full((B, Tc), gu.SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2))
        en, ls_bits = (torch.full((B, Tc + 1), gu.SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2))
        closed, lens = (torch.full((B,), gu.SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2))
        ls = ls_bits.view(torch.float32)
        score = torch.full((B,), -123.0, dtype=torch.float32, device="cuda")
        ctcdecode_amd._set_input_dtype(dec, sc["dtype"])
        ptrs = (ctypes.c_void_p * B)(*[s._handle.value for s in streams])
        flags = (ctypes.c_ubyte * B)(*[1 if e else 0 for e in eos])
        _native.check(_native.lib.ctcd_greedy_stream_decode(
            dec._handle, ptrs, flags, x.data_ptr() if x.numel() else None, seq.data_ptr() if seq is not None else None, B, Tc, V, sc["blank"], sc["mode"],
            tok.data_ptr() if Tc else None, st.data_ptr() if Tc else None, en.data_ptr() if details else None, ls.data_ptr() if details else None,
            closed.data_ptr() if details else None, score.data_ptr(), lens.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        for s, e in zip(streams, eos):
            s._ended = s._ended or bool(e)
        got = dict(tokens=tok, starts=st, ends=en, label_scores=ls, closed_lens=closed, scores=score, lens=lens)
        got = dict((k, v.cpu().numpy()) for k, v in got.items())
        if not details:
            assert (got["ends"] == gu.SENTINEL).all() and (got["label_scores"].view(np.int32) == gu.SENTINEL).all() and (got["closed_lens"] == gu.SENTINEL).all()
            got.update(ends=None, label_scores=None, closed_lens=None)
        return got

    return call


def _player(torch, raw=None):
    import ctcdecode_amd

    def call(streams, eos, stored, seq_lens, sc):
        dec = _dec(sc["V"], sc["blank"], sc["mode"])
        B, Tc, V = stored.shape
        x = gu.to_torch(torch, stored, sc["dtype"])
        outs = dec.greedy_decode_device(x, streams, eos, None if seq_lens is None else torch.from_numpy(np.asarray(seq_lens, np.int32)), details=True)
        assert [tuple(o.shape) for o in outs] == [(B, 1, Tc), (B, 1), (B, 1, Tc), (B, 1), (B, 1, Tc + 1), (B, 1, Tc + 1), (B, 1)] and all(o.is_cuda for o in outs)
        assert [o.dtype for o in outs] == [torch.int32, torch.float32, torch.int32, torch.int32, torch.int32, torch.float32, torch.int32]
        return _numpy(outs)

    def make(sc):
        return lambda first: ctcdecode_amd.GreedyState(_dec(sc["V"], sc["blank"], sc["mode"]), first)

    return lambda sc: su.play(sc, make(sc), raw or call)


def test_every_output_position_is_written(torch_mod):
    """The raw ABI over outputs pre-filled with a sentinel, with and without the detail outputs (which then stay untouched): streams of
    different ages and ragged lengths, Tc == 0 with and without eos, the Tc + 1 column, a workgroup-per-frame label count."""
    for details in (True, False):
        play = _player(torch_mod, _raw_call(torch_mod, details))
        for sc in (su.ages_scenario(1, 0), su.ages_scenario(2, 2), su.emission_scenario("a | b eos"), su.emission_scenario("a | eos"), su.emission_scenario("a | | a"),
                   su.emission_scenario("eos alone", 0), su.family_scenario(1024, 2, 1), su.batch_scenario(gu.long_run_case(1), [1023], key="long 1 1023")):
            play(sc)


@pytest.mark.parametrize("mode", gu.MODES)
def test_one_call_with_eos_equals_the_one_shot_call(torch_mod, mode):
    """gu.long_run_case fed in one call with eos: the one-shot call's six tensors in their first T columns."""
    import ctcdecode_amd

    torch = torch_mod
    c = gu.long_run_case(mode)
    _, _, outs = _player(torch)(su.batch_scenario(c, [], key="long %d whole" % mode))
    one_dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(4)], blank_id=0, beam_width=8, log_probs_input=mode == 1, logits_input=mode == 2)
    tok, sc, st, lens, en, ls = (o.cpu().numpy()[:, 0] for o in one_dec.greedy_decode_device(gu.to_torch(torch, c["stored"], 0), torch.from_numpy(c["seq_lens"]), details=True))
    got, T = outs[0], 1200
    assert np.array_equal(got["tokens"], tok) and np.array_equal(got["starts"], st) and np.array_equal(got["lens"], lens) and np.array_equal(got["closed_lens"], lens)
    assert np.array_equal(got["ends"][:, :T], en) and np.array_equal(gu.bits(got["label_scores"][:, :T]), gu.bits(ls)) and not got["ends"][:, T].any()
    assert np.array_equal(gu.bits(got["scores"]), gu.bits(sc))


@pytest.mark.parametrize("mode", gu.MODES)
@pytest.mark.parametrize("chunk", [1, 7, 64])
def test_long_runs_in_even_chunks(torch_mod, mode, chunk):
    c = gu.long_run_case(mode)
    _player(torch_mod)(su.batch_scenario(c, list(range(chunk, c["x"].shape[1], chunk)), key="long %d by %d" % (mode, chunk)))


@pytest.mark.parametrize("mode", gu.MODES)
def test_long_runs_cut_around_the_kernel_chunk_and_the_runs(torch_mod, mode):
    """1023 | rest, 1024 | rest, 1025 | rest; a cut inside each long run; a cut exactly behind a run's last frame; 8 | 1100 | rest: a call
    that itself spans the kernel's internal chunk of 1024 frames, inside a run, with a carried open run."""
    c = gu.long_run_case(mode)
    play = _player(torch_mod)
    for name, cuts in (("1023", [1023]), ("1024", [1024]), ("1025", [1025]), ("inside", [62, 600, 1015, 1050]), ("behind", [64, 71, 1024, 1041, 1101, 1196]),
                       ("8 then 1100", [8, 1108])):
        play(su.batch_scenario(c, cuts, key="long %d %s" % (mode, name)))


@pytest.mark.parametrize("name", sorted(su.EMISSION_CASES))
def test_emission_across_a_cut(torch_mod, name):
    for mode in gu.MODES:
        streams, _, outs = _player(torch_mod)(su.emission_scenario(name, mode))
        if name == "a | b eos":
            assert outs[1]["closed_lens"][0] == 2 and outs[1]["ends"][0].tolist() == [0, 1], "two closed runs in a call of one frame: the Tc + 1 column"
        if name == "eos alone":
            assert outs[0]["lens"][0] == 0 and gu.bits1(outs[0]["scores"][0]) == 0 and streams[0].ended
        if name == "a a | a":
            assert streams[0].info() == dict(frames=3, emitted=1, closed=0, open_run=True)


def test_signed_zeros_across_calls(torch_mod):
    play = _player(torch_mod)
    for first, second, bits_ in ((0.0, -0.0, 0), (-0.0, 0.0, 0x80000000)):
        _, _, outs = play(su.scenario(4, su.BL, 1, 0, [0], su.zero_calls(first, second), key="zeros %r %r" % (first, second)))
        assert gu.bits1(outs[1]["label_scores"][0, 0]) == bits_, "the earlier call's zero wins the tie"
    raw = np.full((1, 1, 4), -5.0, np.float32)
    raw[0, 0, su.A] = -0.0
    _, _, outs = play(su.scenario(4, su.BL, 1, 0, [0], [dict(raw=raw, streams=[0], eos=[False], seq_lens=None)], key="first -0.0"))
    assert gu.bits1(outs[0]["scores"][0]) == 0x80000000, "the first frame sets the score to its lp, not 0 + lp"


def test_a_frame_of_minus_infinity_in_the_second_call(torch_mod):
    rng = np.random.default_rng(5)
    raws = [gu.random_rows(rng, 1, 4, 6, 1) for _ in range(3)]
    raws[1][0, 2] = -np.inf
    calls = [dict(raw=r, streams=[0], eos=[i == 2], seq_lens=None) for i, r in enumerate(raws)]
    _, _, outs = _player(torch_mod)(su.scenario(6, 0, 1, 0, [0], calls, key="neg inf"))
    assert np.isfinite(outs[0]["scores"][0]) and np.isneginf(outs[1]["scores"][0]) and np.isneginf(outs[2]["scores"][0])


def test_streams_of_different_ages_in_one_batch(torch_mod):
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            streams, books, _ = _player(torch_mod)(su.ages_scenario(mode, dtype))
            assert [s.ended for s in streams] == [False, True, True, True, True] and [s.info()["frames"] for s in streams] == [bk.frames for bk in books]


@pytest.mark.parametrize("V", [29, 65, 1024])
def test_one_case_per_argmax_kernel_family(torch_mod, V):
    """29 labels: lanes of a wave per frame; 65: a wave; 1024: a workgroup (logits: the row in registers); three calls each."""
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            _player(torch_mod)(su.family_scenario(V, mode, dtype))


def test_first_frame_near_the_limit(torch_mod):
    torch = torch_mod
    F0 = 2**31 - 40
    rng = np.random.default_rng(3)
    c = gu._case(gu.path_rows(rng, [[1, 1, 0, 2] * 9 + [3, 3, 3]], 4, 1), 1, 0, 0)  # 39 frames
    streams, _, outs = _player(torch)(su.batch_scenario(c, [20], eos_last=False, first_frames=[F0], key="limit"))
    assert outs[1]["starts"][0, outs[1]["lens"][0] - 1] == 2**31 - 4
    st, dec = streams[0], _dec(4, 0, 1)
    before = st.info()
    assert before == dict(frames=39, emitted=19, closed=18, open_run=True)
    with pytest.raises(NotImplementedError):
        dec.greedy_decode_device(torch.zeros((1, 1, 4), device="cuda"), [st], [False])
    assert st.info() == before and not st.ended, "the refused call left the stream intact"
    out = _numpy(dec.greedy_decode_device(torch.zeros((1, 0, 4), device="cuda"), [st], [True], details=True))
    assert out["closed_lens"][0] == 1 and out["ends"][0, 0] == 2**31 - 2 and st.info() == dict(frames=39, emitted=19, closed=19, open_run=False)


def test_reset_gives_a_fresh_stream(torch_mod):
    import ctcdecode_amd

    sc = su.family_scenario(29, 1, 0)
    dec = _dec(sc["V"], sc["blank"], 1)
    used = [ctcdecode_amd.GreedyState(dec, 3) for _ in sc["first_frames"]]
    dec.greedy_decode_device(gu.to_torch(torch_mod, gu.shape_case(29, 1, 0, T=5, B=2)["stored"], 0), used, [False, True])
    assert used[1].ended and used[0].info()["frames"] == 5

    def again(first):
        st = used.pop(0)
        st.reset(first)
        assert not st.ended and st.info() == dict(frames=0, emitted=0, closed=0, open_run=False)
        return st

    su.play(dict(sc, first_frames=[0, 17]), again, lambda streams, eos, stored, seq_lens, s: _numpy(
        dec.greedy_decode_device(gu.to_torch(torch_mod, stored, 0), streams, eos, details=True)))


def test_refused_calls_run_nothing(torch_mod):
    import ctcdecode_amd

    torch = torch_mod
    dec = _dec(6, 0, 1)
    a, b = ctcdecode_amd.GreedyState(dec), ctcdecode_amd.GreedyState(dec)
    x = gu.to_torch(torch, gu.shape_case(6, 1, 0, T=4, B=2)["stored"], 0)
    dec.greedy_decode_device(x, [a, b], [True, False])
    assert a.ended and not b.ended
    seen = b.info()
    for states, eos, rows in (([a, b], [False, False], x), ([b, b], [False, False], x), ([b], [False], x), ([b, b, b], [False] * 3, x), ([b, b], [False], x),
                              ([b, ctcdecode_amd.GreedyState(dec)], [False, False], x[:, :, :5]), ([b, object()], [False, False], x)):
        with pytest.raises(ValueError):
            dec.greedy_decode_device(rows, states, eos)
    assert b.info() == seen, "an ended state, a duplicate state, wrong list lengths and a wrong V: nothing ran"
    # the C ABI refuses an ended and a duplicate stream itself
    from ctcdecode_amd import _native
    import ctypes

    out = torch.empty((2, 8), dtype=torch.int32, device="cuda")
    for pair in ((a, b), (b, b)):
        ptrs = (ctypes.c_void_p * 2)(pair[0]._handle.value, pair[1]._handle.value)
        rc = _native.lib.ctcd_greedy_stream_decode(dec._handle, ptrs, (ctypes.c_ubyte * 2)(0, 0), x.data_ptr(), None, 2, 4, 6, 0, 1, out.data_ptr(), out.data_ptr(),
                                                   None, None, None, out.data_ptr(), out.data_ptr(), None)
        assert rc == -1
    assert b.info() == seen


def test_align_of_the_streams_labels_returns_its_score(torch_mod):
    """Mode 1: the labels of all calls concatenated, given to ``CTCBeamDecoder.align`` on the concatenated rows, return the stream's
    final score with equal bits."""
    import ctcdecode_amd

    torch = torch_mod
    c = gu.shape_case(29, 1, 0, T=40, B=1)
    _, _, outs = _player(torch)(su.batch_scenario(c, [9, 10, 31], key="align"))
    tok = su.joined(outs)[0]
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(29)], blank_id=c["blank"], beam_width=8, log_probs_input=True)
    rows = torch.zeros((1, 1, 40), dtype=torch.int32)
    rows[0, 0, : len(tok)] = torch.from_numpy(tok)
    _, _, score = dec.align(gu.to_torch(torch, c["stored"], 0), torch.tensor([40]), rows.cuda(), torch.tensor([[len(tok)]], dtype=torch.int32).cuda())
    assert len(tok) > 0 and gu.bits1(score.cpu().numpy()[0, 0]) == gu.bits1(outs[-1]["scores"][0])


def test_cpu_tensors_and_the_plain_call(torch_mod):
    """``greedy_decode``: the same tensors on the CPU, with and without details; CPU input rows."""
    import ctcdecode_amd

    sc = su.family_scenario(29, 1, 0)
    dec = _dec(29, sc["blank"], 1)

    def call(streams, eos, stored, seq_lens, s):
        outs = dec.greedy_decode(torch_mod.from_numpy(stored), streams, eos, details=True)
        assert not any(o.is_cuda for o in outs)
        return _numpy(outs)

    su.play(sc, lambda first: ctcdecode_amd.GreedyState(dec, first), call)
    st = ctcdecode_amd.GreedyState(dec)
    assert len(dec.greedy_decode(torch_mod.from_numpy(sc["calls"][0]["raw"][:1].copy()), [st], [False])) == 4
