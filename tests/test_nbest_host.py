"""The n-best expansion on the CPU: the routines of ctcdecode_amd/csrc/nbest.h (host twin, tests/native/nbest_host.cpp) -- the
product's host expansion of the rows below n, and the kernel's segment walk run sequentially -- against the slices of the full host
expansion and the zeros the contract defines, on records built from the oracle's rows and on hand-made tries; malformed records; the
launch geometry; the stand-alone sanitizer driver."""
import os
import subprocess

import nbest_util as nb
import numpy as np
import oracle_util as ou
import pytest

METHODS = [0, 1]  # 0: expand_item_nbest_host (the product's host route), 1: rows_by_segments_host (the kernel's method)


def _check(hdr, ent, lab, T, n, what, want_full=None):
    """Both methods at ``n`` against rows [:, :n] of the full host expansion (and of ``want_full``: the rows the records were made of)."""
    ftok, fts = nb.host_full(hdr, ent, lab, T)
    if want_full is not None:
        assert np.array_equal(ftok, want_full["tokens"]) and np.array_equal(fts, want_full["timesteps"]), "%s: the full host expansion differs from the rows" % what
    nres = hdr[:, 0]
    for method in METHODS:
        tok, ts, ok, st = nb.host_nbest(hdr, ent, lab, T, n, method)
        assert not st.any(), "%s method %d: status %s for well-formed records" % (what, method, st)
        assert np.array_equal(tok, ftok[:, :n]), "%s method %d n=%d: tokens differ from the full expansion's rows" % (what, method, n)
        assert np.array_equal(ts, fts[:, :n]), "%s method %d n=%d: time steps differ from the full expansion's rows" % (what, method, n)
        for b in range(hdr.shape[0]):
            have = min(int(nres[b]), n)
            assert ok[b, :have].all() and not ok[b, have:].any(), "%s method %d: rows with a result %s, want the first %d" % (what, method, ok[b], have)
            assert not tok[b, have:].any() and not ts[b, have:].any(), "%s method %d: a row without a result is not zero" % (what, method)
    return ftok, fts


@pytest.mark.parametrize("T", [1, 3, 67])
@pytest.mark.parametrize("order,share", [("trie", "all"), ("reverse", "all"), ("row", "all"), ("trie", "half")])
def test_twin_on_oracle_rows(T, order, share):
    """Records built in Python from the oracle's rows, in every valid order; n = 1, beam - 1, beam; ragged lengths, one of them 0."""
    beam = 16
    sl = np.asarray([T, max(T - 4, 0), 0, T // 2, T], np.int32)
    res = nb.cached(("rows", T), lambda: ou.decode(ou.synth_logprobs(5, T, 29, 31 + T), sl, beam=beam, which=nb.which_oracle()))
    hdr, ent, lab = nb.records_of(res, order=order, share=share, pad=3 if order == "row" else 0)
    for n in (1, beam - 1, beam):
        ftok, fts = _check(hdr, ent, lab, T, n, "T=%d %s/%s" % (T, order, share), want_full=res)
        # ... and the contract restated on the oracle's tensors
        want = nb.want_nbest(res, n)
        tok, ts, ok, st = nb.host_nbest(hdr, ent, lab, T, n, 0)
        assert np.array_equal(tok, want["tokens"]) and np.array_equal(ts, want["timesteps"])


def test_fewer_results_than_n():
    """T 2, V 3, beam 8: fewer than eight prefixes exist (seven: the empty one, two of one label, four of two).  The rows beyond them
    come out zero, without a result."""
    res = ou.decode(ou.synth_logprobs(2, 2, 3, 4), None, beam=8, which=nb.which_oracle())
    assert (res["nres"] < 8).all() and (res["nres"] > 1).all(), res["nres"]
    hdr, ent, lab = nb.records_of(res)
    for n in (1, 7, 8):
        _check(hdr, ent, lab, 2, n, "nres < n", want_full=res)


def test_no_results_at_all():
    hdr = np.zeros((2, 4), np.int32)
    ent = np.full((2, 8, 4), 0x7FFFFFF0, np.int32)  # (entries at or beyond the result count are never looked at)
    for n in (1, 7, 8):
        _check(hdr, ent, np.zeros((0,), np.uint32), 5, n, "nres = 0")


def _labels(seq, t0=0):
    return [(c, t0 + 2 * i) for i, c in enumerate(seq)]


def test_prefix_owned_by_entries_that_are_not_selected():
    """Row 0 is the last entry in trie order; it owns two labels, its first four belong to two entries whose rows are not asked for."""
    T = 8
    entries = [(1, 0, _labels([5, 6, 7])), (2, 3, _labels([8, 9], 6)), (0, 4, _labels([3, 4], 8))]
    hdr, ent, lab = nb.trie(entries)
    want = nb.expand_py(hdr, ent, lab, T)
    assert want["tokens"][0, 0, :6].tolist() == [5, 6, 7, 8, 3, 4]
    for n in (1, 2, 3):
        _check(hdr, ent, lab, T, n, "prefix of others", want_full=want)


@pytest.mark.parametrize("K,T", [(3, 3), (66, 67)])
def test_owner_chain_crosses_every_entry(K, T):
    """Entry j shares j labels with its predecessor and adds one: every entry owns exactly one label of the last entry's row (66 entries:
    the walk goes beyond one wave's 64)."""
    entries = [(K - 1 - j, j, [(j + 1, 3 * j)]) for j in range(K)]
    hdr, ent, lab = nb.trie(entries)
    want = nb.expand_py(hdr, ent, lab, T)
    assert want["tokens"][0, 0, :K].tolist() == list(range(1, K + 1))
    for n in (1, K - 1, K):
        _check(hdr, ent, lab, T, n, "chain K=%d" % K, want_full=want)


def test_empty_sequence_as_row_zero_and_the_ends_of_the_trie():
    T = 3
    # the empty sequence is the best result and the first entry; the second-best is the last entry
    entries = [(0, 0, []), (2, 0, _labels([4])), (3, 1, _labels([5], 2)), (1, 0, _labels([6, 7]))]
    hdr, ent, lab = nb.trie(entries, K=6)
    want = nb.expand_py(hdr, ent, lab, T)
    assert want["lens"][0].tolist() == [0, 2, 1, 2, 0, 0]
    for n in (1, 2, 5, 6):
        _check(hdr, ent, lab, T, n, "empty row 0", want_full=want)
    # row 0 as the last entry, row 1 as the first
    entries = [(1, 0, _labels([4, 5])), (2, 1, _labels([6], 2)), (0, 2, _labels([7], 4))]
    hdr, ent, lab = nb.trie(entries)
    want = nb.expand_py(hdr, ent, lab, T)
    assert want["tokens"][0, 0].tolist() == [4, 6, 7]
    for n in (1, 2, 3):
        _check(hdr, ent, lab, T, n, "row 0 last", want_full=want)


def _assert_malformed(hdr, ent, lab, T, n, zero_rows, good_rows, what, want=None):
    for method in METHODS:
        tok, ts, ok, st = nb.host_nbest(hdr, ent, lab, T, n, method)
        assert st.tolist() == [nb.BAD_RECORD], "%s method %d: status %s" % (what, method, st)
        assert not (tok == 0x5A5A5A5A).any() and not (ts == 0x5A5A5A5A).any(), "%s method %d: a row was not written" % (what, method)
        for p in zero_rows:
            assert not ok[0, p] and not tok[0, p].any() and not ts[0, p].any(), "%s method %d: row %d is not zero" % (what, method, p)
        for p in good_rows:
            assert ok[0, p], "%s method %d: row %d lost its result" % (what, method, p)
            assert np.array_equal(tok[0, p], want["tokens"][0, p]) and np.array_equal(ts[0, p], want["timesteps"][0, p]), (what, method, p)


def test_malformed_records_zero_the_row_and_report():
    T = 8
    entries = [(1, 0, _labels([5, 6, 7])), (2, 3, _labels([8, 9], 6)), (0, 4, _labels([3, 4], 8)), (3, 0, _labels([2], 1))]
    hdr, ent, lab = nb.trie(entries)
    want = nb.expand_py(hdr, ent, lab, T)
    # an offset beyond the label buffer on the entry that holds position 3 of rows 2 and 0: those rows are zero, rows 1 and 3 stand
    e = ent.copy()
    e[0, 1, 3] = lab.size + 100
    _assert_malformed(hdr, e, lab, T, 4, zero_rows=[0, 2], good_rows=[1, 3], what="offset beyond the buffer", want=want)
    _assert_malformed(hdr, e, lab, T, 1, zero_rows=[0], good_rows=[], what="offset beyond the buffer, n = 1")
    # ... below the item's first label (records of two items in one buffer: item 1's entry points into item 0's labels)
    hdr2 = np.concatenate([hdr, hdr]).astype(np.int32)
    hdr2[1, 2] = lab.size
    ent2 = np.concatenate([ent, ent]).astype(np.int32)
    ent2[1, :, 3] += lab.size
    ent2[1, 0, 3] = 0
    for method in METHODS:
        tok, ts, ok, st = nb.host_nbest(hdr2, ent2, np.concatenate([lab, lab]), T, 4, method)
        assert st.tolist() == [0, nb.BAD_RECORD]
        assert np.array_equal(tok[0], want["tokens"][0]) and not tok[1, :3].any() and ok[1].tolist() == [False, False, False, True]
    # a row index at the beam width, and below zero: the entry is dropped, the row it should have named is zero
    for bad in (4, -1, 1 << 30):
        e = ent.copy()
        e[0, 2, 0] = bad
        _assert_malformed(hdr, e, lab, T, 4, zero_rows=[0], good_rows=[1, 2, 3], what="row index %d" % bad, want=want)
    # longer than a row; sharing more than it has; sharing more than its predecessor has
    e = ent.copy()
    e[0, 2, 2] = T + 1
    _assert_malformed(hdr, e, lab, T, 4, zero_rows=[0], good_rows=[1, 2, 3], what="length beyond T", want=want)
    e = ent.copy()
    e[0, 3, 1] = 2
    _assert_malformed(hdr, e, lab, T, 4, zero_rows=[3], good_rows=[1, 2, 0], what="lcp beyond the length", want=want)
    e = ent.copy()
    e[0, 2, 1], e[0, 2, 2], e[0, 2, 3] = 6, 7, 5  # (its own label is in range; positions 5 .. 6 are nobody's)
    _assert_malformed(hdr, e, lab, T, 4, zero_rows=[0], good_rows=[1, 2, 3], what="lcp beyond the predecessor", want=want)
    # a result count beyond the entries, and an item whose range leaves the buffer: no row has a result
    h = hdr.copy()
    h[0, 0] = 5
    _assert_malformed(h, ent, lab, T, 4, zero_rows=[0, 1, 2, 3], good_rows=[], what="result count beyond beam")
    h = hdr.copy()
    h[0, 1] = lab.size + 1
    _assert_malformed(h, ent, lab, T, 4, zero_rows=[0, 1, 2, 3], good_rows=[], what="range beyond the buffer")
    # a row claimed twice: the first claimant in trie order stays
    e = ent.copy()
    e[0, 3, 0] = 1
    _assert_malformed(hdr, e, lab, T, 4, zero_rows=[3], good_rows=[0, 1, 2], what="row claimed twice", want=want)


def test_launch_geometry():
    """A wave per selected row, at most four: n = 1 is one wave.  The tables of the widest beam fit a gfx950 workgroup's LDS.  16-byte
    stores need whole rows of 16-byte words."""
    assert [nb.host_threads(n) for n in (1, 2, 3, 4, 100, 4096)] == [64, 128, 192, 256, 256, 256]
    assert nb.host_lds_bytes(4096, 4096) + 1024 <= 160 * 1024
    assert nb.host_lds_bytes(100, 1) == (3 * 100 + 1) * 4 + 100 * 2
    assert nb.host_vec16(64, 4096, 8192) and not nb.host_vec16(67, 4096, 8192) and not nb.host_vec16(64, 4100, 8192) and not nb.host_vec16(64, 4096, 8)


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/nbest_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / "nbest_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(nb.NATIVE, "nbest_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failures" in r.stdout
