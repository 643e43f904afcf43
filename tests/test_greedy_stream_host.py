"""Greedy decode of live streams on the CPU: the rules of ctcdecode_amd/csrc/greedy.h "live streams" run sequentially (host twin,
tests/native/greedy_stream_host.cpp) against the slicing rule of the header applied to ``greedy_util.reference`` of all of a stream's
frames (tests/greedy_stream_util.py), bit for bit -- scores and label scores as uint32, labels and frames exactly -- over a few
hundred random small scenarios and the named cases the GPU tests run too; the stand-alone sanitizer driver on a handful of them."""
import os
import struct
import subprocess

import greedy_stream_util as su
import greedy_util as gu
import numpy as np
import pytest


def _play(sc):
    return su.play(sc, su.HostStream, su.host_call)


def test_one_shot_twin_is_unchanged_by_the_shared_argmax_routine():
    """greedy_item_host now shares frame_recs_host with the stream twin: a stream fed a whole batch with eos returns the one-shot
    twin's six tensors in their first T columns."""
    for mode in gu.MODES:
        c = gu.shape_case(5, mode, mode, T=12, B=3)
        one = gu.host_decode(c["stored"], c["dtype"], None, c["blank"], mode)
        _, _, outs = _play(su.batch_scenario(c, [], key="whole %d" % mode))
        got = outs[0]
        for k in ("tokens", "starts"):
            assert np.array_equal(got[k], one[k])
        assert np.array_equal(got["ends"][:, :12], one["ends"]) and np.array_equal(gu.bits(got["label_scores"][:, :12]), gu.bits(one["label_scores"]))
        assert np.array_equal(gu.bits(got["scores"]), gu.bits(one["scores"])) and np.array_equal(got["lens"], one["lens"])
        assert np.array_equal(got["closed_lens"], one["lens"]) and not got["ends"][:, 12].any()


def test_random_small_scenarios():
    """B 1..3 streams, 1..5 calls, Tc 0..20, V 1..8, the three modes and element types, ragged seq_lens (0, negative, above Tc), eos on
    a random call, coarse values for ties."""
    rng = np.random.default_rng(11)
    for i in range(300):
        S, n_calls, V = int(rng.integers(1, 4)), int(rng.integers(1, 6)), int(rng.integers(1, 9))
        mode, dtype = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        alive = list(range(S))
        calls = []
        for j in range(n_calls):
            if not alive:
                break
            Tc = int(rng.integers(0, 21))
            who = [s for s in alive if rng.random() < 0.8] or alive[:1]
            raw = gu.random_rows(rng, len(who), Tc, V, mode, scale=3.0)
            if i % 3 == 0:
                raw = np.round(raw * 2) / 2 if mode else np.round(raw * 4) / 4
            eos = [bool(rng.random() < 0.25) for _ in who]
            calls.append(dict(raw=raw.astype(np.float32), streams=who, eos=eos, seq_lens=rng.integers(-2, Tc + 3, len(who)).astype(np.int32) if i % 2 else None))
            alive = [s for s in alive if not (s in who and eos[who.index(s)])]
        sc = su.scenario(V, int(rng.integers(0, V)), mode, dtype, [int(rng.integers(0, 50)) * (i % 4 == 0) for _ in range(S)], calls, key=None)
        sc["key"] = "random %d" % i
        books, wants, stored = su.expected(dict(sc, key=None))
        streams = [su.HostStream(f) for f in sc["first_frames"]]
        for j, (c, rows, want) in enumerate(zip(calls, stored, wants)):
            details = bool((i + j) % 5)
            rc, got = su.host_call_rc([streams[s] for s in c["streams"]], c["eos"], rows, dtype, c["seq_lens"], sc["blank"], mode, details=details)
            assert rc == 0
            gu.assert_same(got, want, "random %d call %d" % (i, j))
            if details:
                assert np.array_equal(got["closed_lens"], want["closed_lens"])
        for s, bk in enumerate(books):
            inf = streams[s].info()
            assert inf["frames"] == bk.frames and inf["ended"] == any(e for _, _, e in bk.calls)
            assert inf["emitted"] - inf["closed"] == int(inf["open_run"])


@pytest.mark.parametrize("mode", gu.MODES)
def test_long_runs_in_every_chunking(mode):
    """gu.long_run_case (T = 1200, runs across frames 64 and 1024): one call; chunks of 7 and 64; cuts around 1024; a cut inside each
    long run and one exactly behind a run's last frame."""
    c = gu.long_run_case(mode)
    for name, cuts in (("whole", []), ("7", range(7, 1200, 7)), ("64", range(64, 1200, 64)), ("1023", [1023]), ("1024", [1024]), ("1025", [1025]),
                       ("inside", [62, 600, 1015, 1050]), ("behind", [64, 71, 1024, 1041, 1101, 1196])):
        _, books, outs = _play(su.batch_scenario(c, list(cuts), key="long %d %s" % (mode, name)))
        assert [bk.frames for bk in books] == [1200, 1200, 1199]
    one = gu.cached(("ref", "long runs mode %d" % mode), lambda: gu.case_reference(c))
    for b in range(3):
        tok, st, en, ls = su.joined(outs, b)
        L = one["lens"][b]
        assert np.array_equal(tok, one["tokens"][b, :L]) and np.array_equal(st, one["starts"][b, :L]) and np.array_equal(en, one["ends"][b, :L])
        assert np.array_equal(gu.bits(ls), gu.bits(one["label_scores"][b, :L])) and gu.bits1(outs[-1]["scores"][b]) == gu.bits1(one["scores"][b])


@pytest.mark.parametrize("name", sorted(su.EMISSION_CASES))
def test_emission_across_a_cut(name):
    for mode in gu.MODES:
        streams, books, outs = _play(su.emission_scenario(name, mode))
        lens, closed = [int(o["lens"][0]) for o in outs], [int(o["closed_lens"][0]) for o in outs]
        want = {"a a | a": ([1, 0], [0, 0]), "a | _ a": ([1, 1], [0, 1]), "a | b": ([1, 1], [0, 1]), "a _ | a": ([1, 1], [1, 0]), "_ | _": ([0, 0], [0, 0]),
                "a | | a": ([1, 0, 0], [0, 0, 0]), "a | eos": ([1, 0], [0, 1]), "eos alone": ([0], [0]), "a | b eos": ([1, 1], [0, 2])}[name]
        assert (lens, closed) == want, (name, lens, closed)
        if name == "a | _ a":
            assert outs[1]["ends"][0, 0] == 0, "the first run closes in call 2 with end = the last frame of call 1"
        if name == "a | b eos":
            assert outs[1]["ends"][0].tolist() == [0, 1], "two closed runs in a call of one frame: the Tc + 1 column"
        if name == "eos alone":
            assert gu.bits1(outs[0]["scores"][0]) == 0 and streams[0].info()["ended"]


def test_signed_zeros_across_calls():
    for first, second, bits_ in ((0.0, -0.0, 0), (-0.0, 0.0, 0x80000000)):
        _, _, outs = _play(su.scenario(4, su.BL, 1, 0, [0], su.zero_calls(first, second), key="zeros %r %r" % (first, second)))
        assert outs[1]["closed_lens"][0] == 1 and gu.bits1(outs[1]["label_scores"][0, 0]) == bits_, "the earlier call's zero wins the tie"
    raw = np.full((1, 1, 4), -5.0, np.float32)
    raw[0, 0, su.A] = -0.0
    _, _, outs = _play(su.scenario(4, su.BL, 1, 0, [0], [dict(raw=raw, streams=[0], eos=[False], seq_lens=None)], key="first -0.0"))
    assert gu.bits1(outs[0]["scores"][0]) == 0x80000000, "the first frame sets the score to its lp, not 0 + lp"


def test_a_frame_of_minus_infinity_in_the_second_call():
    rng = np.random.default_rng(5)
    raws = [gu.random_rows(rng, 1, 4, 6, 1) for _ in range(3)]
    raws[1][0, 2] = -np.inf
    calls = [dict(raw=r, streams=[0], eos=[i == 2], seq_lens=None) for i, r in enumerate(raws)]
    _, _, outs = _play(su.scenario(6, 0, 1, 0, [0], calls, key="neg inf"))
    assert np.isfinite(outs[0]["scores"][0]) and np.isneginf(outs[1]["scores"][0]) and np.isneginf(outs[2]["scores"][0])


def test_streams_of_different_ages_in_one_batch():
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            streams, books, _ = _play(su.ages_scenario(mode, dtype))
            assert [s.info()["ended"] for s in streams] == [False, True, True, True, True]


@pytest.mark.parametrize("V", [29, 65, 1024])
def test_label_counts_of_the_argmax_families(V):
    for mode in gu.MODES:
        for dtype in gu.DTYPES:
            _play(su.family_scenario(V, mode, dtype))


def test_first_frame_near_the_limit_and_refusals():
    F0 = 2**31 - 40
    rng = np.random.default_rng(3)
    c = gu._case(gu.path_rows(rng, [[1, 1, 0, 2] * 9 + [3, 3, 3]], 4, 1), 1, 0, 0)  # 39 frames
    streams, _, outs = _play(su.batch_scenario(c, [20], eos_last=False, first_frames=[F0], key="limit"))
    assert outs[1]["starts"][0, outs[1]["lens"][0] - 1] == 2**31 - 4 and streams[0].info() == dict(frames=39, emitted=19, closed=18, open_run=True, ended=False)
    before = streams[0].rec.copy()
    rc, _ = su.host_call_rc(streams, [True], np.zeros((1, 1, 4), np.float32), 0, None, 0, 1)
    assert rc == -2 and np.array_equal(streams[0].rec, before), "a frame number of 2^31 - 1 is refused, and the stream is intact"
    rc, out = su.host_call_rc(streams, [True], np.zeros((1, 0, 4), np.float32), 0, None, 0, 1)
    assert rc == 0 and out["ends"][0, 0] == 2**31 - 2 and out["closed_lens"][0] == 1
    rc, _ = su.host_call_rc(streams, [False], np.zeros((1, 0, 4), np.float32), 0, None, 0, 1)
    assert rc == -1, "an ended stream is refused"


def _write_scenario(path, sc):
    _, wants, stored = su.expected(sc)
    with open(path, "wb") as f:
        f.write(struct.pack("<6i", sc["V"], sc["blank"], sc["mode"], sc["dtype"], len(sc["first_frames"]), len(sc["calls"])))
        f.write(np.asarray(sc["first_frames"], np.int64).tobytes())
        for c, rows, want in zip(sc["calls"], stored, wants):
            B, Tc = rows.shape[:2]
            f.write(struct.pack("<3i", B, Tc, 0 if c["seq_lens"] is None else 1))
            f.write(np.asarray(c["streams"], np.int32).tobytes())
            f.write(np.asarray([1 if e else 0 for e in c["eos"]], np.uint8).tobytes())
            f.write(np.ascontiguousarray(rows).tobytes())
            if c["seq_lens"] is not None:
                f.write(np.ascontiguousarray(c["seq_lens"], np.int32).tobytes())
            for k, dt in (("tokens", np.int32), ("starts", np.int32), ("ends", np.int32), ("label_scores", np.float32), ("closed_lens", np.int32),
                          ("scores", np.float32), ("lens", np.int32)):
                f.write(np.ascontiguousarray(want[k], dt).tobytes())


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/greedy_stream_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own: scenarios of
    every mode and element type against the slicing rule's outputs, and the rows the driver makes and cuts itself."""
    scs = [su.batch_scenario(gu.long_run_case(1), [1023], key="long 1 1023"), su.batch_scenario(gu.long_run_case(2), list(range(64, 1200, 64)), key="long 2 64"),
           su.ages_scenario(0, 2), su.ages_scenario(2, 1), su.family_scenario(65, 2, 1), su.family_scenario(29, 0, 2), su.emission_scenario("a | b eos"),
           su.emission_scenario("a | eos", 2), su.emission_scenario("eos alone", 0)]
    files = []
    for i, sc in enumerate(scs):
        files.append(str(tmp_path / ("scenario%02d.bin" % i)))
        _write_scenario(files[-1], sc)
    exe = str(tmp_path / "greedy_stream_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(gu.NATIVE, "greedy_stream_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failures" in r.stdout
