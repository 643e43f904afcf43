"""Forced alignment on the CPU: the routines of ctcdecode_amd/csrc/align.h run sequentially (host twin, tests/native/align_host.cpp)
against the numpy restatement of the header's definition (tests/align_util.py), bit for bit -- scores as uint32, spans exactly; the
tie cases shown to have more than one optimal path by the restatement alone; the slot and grid arithmetic; the stand-alone sanitizer
driver on the same cases."""
import os
import struct
import subprocess

import align_util as au
import numpy as np
import pytest


@pytest.mark.parametrize("name", au.CASES)
def test_twin_equals_the_restatement(name):
    c, want = au.case(name)
    got = au.host_align(c["lp"], c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    assert got["invalid_rows"] == 0
    assert not (got["start"] == 0x5A5A5A5A).any() and not (got["end"] == 0x5A5A5A5A).any(), "a position of the outputs was not written"
    au.assert_same(got, want, name)


def test_the_cases_cover_what_they_are_named_for():
    c, want = au.case("edges")
    sc, al, lens = want["scores"], want["aligned"], c["lens"]
    assert sc[0, 0] == 0 and np.isneginf(sc[0, 1]) and np.isneginf(sc[0, 2]), "n = 0: L = 0 scores 0, L > 0 is not aligned"
    assert sc[1, 0] == c["lp"][1, 0, 0] and sc[1, 1] == c["lp"][1, 0, 4] and np.isneginf(sc[1, 2]), "n = 1: L = 0, L = 1, L = 2"
    assert al[2, 0] and want["start"][2, 0, :2].tolist() == [0, 2] and want["end"][2, 0, :2].tolist() == [0, 2], "'a a' at n = 3"
    assert al[2, 1] and want["start"][2, 1, :3].tolist() == [0, 1, 2], "L = n, distinct"
    assert not al[2, 2] and np.isneginf(sc[2, 2]), "L = n with a repeat"
    assert al[3, 0] and not al[3, 1] and al[4, 1]
    # L = 0, n >= 1: the blank's column added up in frame order
    acc = c["lp"][2, 0, 0]
    for t in range(1, 3):
        acc = np.float32(c["lp"][2, t, 0]) + acc
    assert sc[2, 3] == acc and lens[2, 3] == 0
    c, want = au.case("neg_inf")
    assert want["aligned"][0, 0] and not want["aligned"][1, 0] and not want["aligned"][1, 2] and np.isneginf(want["scores"][1, 1])
    assert want["aligned"][0, 2] and not (3 <= want["start"][0, 2, 0] <= 9), "label 2 sits outside the stretch it cannot have"
    c, want = au.case("wave_edge")
    assert [2 * int(v) + 1 for v in c["lens"].max(1)] == [63, 65] and want["aligned"][:, :3].all()
    c, want = au.case("workgroup_edge")
    assert [2 * int(v) + 1 for v in c["lens"][0, :3]] == [255, 257, 259] and want["aligned"].all()
    c, want = au.case("many_per_lane")
    assert [au.host_npl(2 * int(v) + 1) for v in c["lens"][0]] == [16, 4, 1, 1] and want["aligned"].all()
    c, want = au.case("mixed_group")
    rows, n = c["lens"].reshape(-1), np.repeat(c["seq_lens"], c["lens"].shape[1])
    assert [2 * int(v) + 1 for v in rows] == [259, 7, 201, 129, 79, 1], "a full group of four that straddles the items, then a partial one: both hold a row beyond a wave"
    assert (rows > n).tolist() == [False, False, False, True, False, False] and np.isneginf(want["scores"][1, 0]), "the first group holds a row without a path"
    assert want["aligned"].reshape(-1).tolist() == [True, True, True, False, True, True]


@pytest.mark.parametrize("name", ["ties_half", "ties_constant"])
def test_tie_cases_have_more_than_one_optimal_path(name):
    """Vacuity: by the restatement alone, most aligned rows of the tie cases have a cell on their path where two predecessors are equal
    (or an end-state tie): another path scores the same, so spans that match were decided by the tie rules."""
    c, want = au.case(name)
    rows = want["aligned"] & (c["lens"] > 0)
    tied = rows & (want["ties"] > 0)
    assert rows.sum() >= 8 and tied.sum() * 2 >= rows.sum(), (int(rows.sum()), int(tied.sum()))
    if name == "ties_constant":  # every row with room to spare has ties
        n = 19
        assert all(want["ties"][b, r] > 0 for b in range(2) for r in range(8) if rows[b, r] and 2 * c["lens"][b, r] + 1 < n)


def test_probability_mode_equals_math_log_per_element():
    c, _ = au.case("ties_half")
    rng = np.random.default_rng(5)
    p = rng.random(c["lp"].shape).astype(np.float32)
    p /= p.sum(-1, keepdims=True)
    p[0, 3, 1] = 0.0  # log(FLT_MIN): finite
    p[1, 2, :] = 0.0
    want = au.reference(au.prob_to_lp(p), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    got = au.host_align(p, c["seq_lens"], c["tokens"], c["lens"], c["blank"], log_input=0)
    au.assert_same(got, want, "probabilities")
    # (a zero probability is log(FLT_MIN), not -inf: only a row longer than its item stays without a path)
    assert want["aligned"].sum() >= 20 and want["aligned"][:2].all() and np.isfinite(want["scores"][want["aligned"]]).all()


def test_half_rows_are_read_as_their_float_copies():
    c, _ = au.case("blank_last")
    h = c["lp"].astype(np.float16)
    want = au.reference(h.astype(np.float32), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    au.assert_same(au.host_align(h.view(np.uint16), c["seq_lens"], c["tokens"], c["lens"], c["blank"], dtype=1), want, "f16")
    bits = au.to_bf16_bits(c["lp"])
    want = au.reference(au.bf16_bits_to_f32(bits), c["seq_lens"], c["tokens"], c["lens"], c["blank"])
    au.assert_same(au.host_align(bits, c["seq_lens"], c["tokens"], c["lens"], c["blank"], dtype=2), want, "bf16")


def test_invalid_rows_raise_their_item_alone():
    c, want = au.case("blank_mid")
    V, blank = c["lp"].shape[2], c["blank"]
    r0 = int(np.argmax(c["lens"][0] > 1))
    for what, edit in (("label = V", lambda t, l: t.__setitem__((0, r0, 1), V)), ("label = blank", lambda t, l: t.__setitem__((0, r0, 0), blank)),
                       ("label < 0", lambda t, l: t.__setitem__((0, r0, 0), -7)), ("length < 0", lambda t, l: l.__setitem__((0, r0), -1)),
                       ("length > L_stride", lambda t, l: l.__setitem__((0, r0), t.shape[2] + 1))):
        tok, lens = c["tokens"].copy(), c["lens"].copy()
        edit(tok, lens)
        got = au.host_align(c["lp"], c["seq_lens"], tok, lens, blank)
        ref = au.reference(c["lp"], c["seq_lens"], tok, lens, blank)
        assert got["invalid_rows"] == 1 and got["status"].tolist() == [au.BAD_ROW, 0], what
        assert not got["start"][0, r0].any() and not got["end"][0, r0].any() and got["scores"][0, r0] == 0, what
        au.assert_same(got, ref, what)
        keep = np.ones(c["lens"].shape, bool)
        keep[0, r0] = False
        assert np.array_equal(got["start"][keep], want["start"][keep]) and np.array_equal(got["scores"][keep].view(np.uint32), want["scores"][keep].view(np.uint32)), what


def test_slot_and_grid_arithmetic():
    """A slot holds T rows of the longest extended sequence the shape allows, or four one-wave hypotheses; the grid is the rows or the
    slots the budget pays for, at least one."""
    assert au.host_row_words(1) == 1 and au.host_row_words(16) == 1 and au.host_row_words(17) == 2 and au.host_row_words(2001) == 126
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731  (slots are whole 256-byte lines)
    assert au.host_slot_bytes(1000, 1000) == up(1000 * 126 * 4)  # (100 KB of back-pointers at T 1000, L 200: they do not fit LDS)
    assert au.host_slot_bytes(1000, 10) == up(1000 * 16 * 4) and au.host_slot_bytes(45, 45) == up(45 * 16 * 4)
    assert au.host_slot_bytes(100, 1000) == au.host_slot_bytes(100, 100), "a row longer than T runs no recurrence"
    slot = au.host_slot_bytes(45, 45)
    assert au.host_grid(40, 3 * slot, 45, 45) == 3 and au.host_grid(40, 3 * slot + slot - 1, 45, 45) == 3 and au.host_grid(40, 1, 45, 45) == 1
    assert au.host_grid(40, 0, 45, 45) == 40 and au.host_grid(41, 0, 45, 45) == 41 and au.host_grid(1, 0, 45, 45) == 1
    assert au.host_grid(6400, 0, 1000, 1000) == au.host_default_scratch() // au.host_slot_bytes(1000, 1000)
    assert [au.host_npl(s) for s in (1, 256, 257, 1024, 1025, 4096)] == [1, 1, 4, 4, 16, 16] and au.host_max_labels() == 2047


def _write_case(path, c, want, log_input=1):
    B, T, V = c["lp"].shape
    R, Ls = c["tokens"].shape[1:]
    with open(path, "wb") as f:
        f.write(struct.pack("<9i", B, T, V, R, Ls, c["blank"], log_input, 0, 0 if c["seq_lens"] is None else 1))
        f.write(np.ascontiguousarray(c["lp"], np.float32).tobytes())
        if c["seq_lens"] is not None:
            f.write(np.ascontiguousarray(c["seq_lens"], np.int32).tobytes())
        for a, dt in ((c["tokens"], np.int32), (c["lens"], np.int32), (want["start"], np.int32), (want["end"], np.int32), (want["scores"], np.float32),
                      (want["status"], np.int32)):
            f.write(np.ascontiguousarray(a, dt).tobytes())


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/align_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own: the cases above against
    the restatement's outputs, one of them with out-of-range labels and lengths, and the rows the driver makes itself."""
    files = []
    for name in au.CASES:
        c, want = au.case(name)
        files.append(str(tmp_path / (name + ".bin")))
        _write_case(files[-1], c, want)
    c, _ = au.case("blank_mid")
    tok, lens = c["tokens"].copy(), c["lens"].copy()
    tok[0, 0, 0], tok[1, 1, 0], lens[0, 2], lens[1, 3] = c["lp"].shape[2], c["blank"], -3, tok.shape[2] + 5
    lens[0, 0], lens[1, 1] = max(lens[0, 0], 1), max(lens[1, 1], 1)
    bad = dict(c, tokens=tok, lens=lens)
    want = au.reference(bad["lp"], bad["seq_lens"], tok, lens, bad["blank"])
    assert want["status"].tolist() == [au.BAD_ROW, au.BAD_ROW]
    files.append(str(tmp_path / "invalid.bin"))
    _write_case(files[-1], bad, want)
    exe = str(tmp_path / "align_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(au.NATIVE, "align_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failures" in r.stdout
