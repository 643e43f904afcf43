"""The blank-frame filter on the CPU: the routines of ctcdecode_amd/csrc/blank_skip.h (host twin, tests/native/blank_skip_host.cpp)
against the definition restated in numpy (tests/blank_skip_util.py) for every input mode and dtype, the edge cases of the definition,
both remaps on the oracle's results, the certificate that the anchor case of the GPU tests is not vacuous, and the stand-alone
sanitizer driver."""
import math
import os
import subprocess

import blank_skip_util as bs
import numpy as np
import oracle_util as ou
import pytest


def _check_filter(x32, dtype, seq_lens, blank_id, thr, mode, what):
    """x32: values exactly representable in dtype.  The twin on their storage against filter_frames / gather_rows."""
    kept, n2 = bs.filter_frames(x32, seq_lens, blank_id, thr, mode if mode != "logits" else "log")
    bits = bs.to_dtype_bits(x32, dtype)
    rows, gn, gk, word = bs.host_filter(bits, dtype, seq_lens, blank_id, bs.bound(thr, mode))
    assert np.array_equal(gn, n2), "%s: n' %s want %s" % (what, gn, n2)
    assert np.array_equal(gk, kept), "%s: kept differs" % what
    want = bs.gather_rows(bits, kept, n2)
    for b in range(bits.shape[0]):
        assert np.array_equal(rows[b, :n2[b]].view(np.uint8), want[b, :n2[b]].view(np.uint8)), "%s: kept rows of item %d differ" % (what, b)
        assert (rows[b, n2[b]:].view(np.uint8) == 0x5A).all(), "%s: item %d: rows at or beyond n' were written" % (what, b)
    row_bytes = bits.shape[2] * bits.dtype.itemsize
    assert word == (16 if row_bytes % 16 == 0 else bits.dtype.itemsize), (what, word)
    return kept, n2


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("V", [29, 31, 32])
@pytest.mark.parametrize("mode", ["log", "prob", "logits"])
def test_twin_filters_as_the_definition_says(dtype, V, mode):
    """Every input mode, dtype and row alignment (half rows at 2, 2 and 16 bytes, float32 rows at 4 and 16), ragged lengths, both ends
    of the vocabulary as blank.  Raw logits are filtered on the float32 log-softmax, whatever the input's dtype."""
    T = 150
    for blank_id in (0, V - 1):
        x = bs.to_dtype_values(bs.synth(3, T, V, 5 + V, blank_id=blank_id, mode=mode), dtype)
        if mode == "logits":
            x, dt = ou.log_softmax_rows(x), "f32"
        else:
            dt = dtype
        sl = np.asarray([T, 97, 31], np.int32)
        kept, n2 = _check_filter(x, dt, sl, blank_id, 0.6, mode, "%s %s V=%d blank=%d" % (mode, dtype, V, blank_id))
        assert 0 < n2.sum() < sl.sum(), "the case filters nothing or everything: %s of %s" % (n2, sl)
        _check_filter(x, dt, None, blank_id, 0.6, mode, "%s %s V=%d blank=%d, no seq_lens" % (mode, dtype, V, blank_id))


def test_twin_scan_crosses_chunks():
    T = 2 * 1024 + 37
    x = bs.synth(2, T, 29, 3)
    kept, n2 = _check_filter(x, "f32", np.asarray([T, 2 * 1024 - 1], np.int32), 0, 0.6, "log", "two chunks and a bit")
    assert n2[0] > 1024 and kept[0, n2[0] - 1] > 2 * 1024, "the kept frames do not cross two chunk boundaries"


def test_twin_edges():
    T, V = 40, 7
    lp = bs.synth(3, T, V, 9)
    # thr = 1.0 on normalised log-probabilities skips nothing
    kept, n2 = _check_filter(lp, "f32", np.asarray([T, 17, 0], np.int32), 0, 1.0, "log", "thr 1.0")
    assert n2.tolist() == [T, 17, 0] and np.array_equal(kept[0], np.arange(T)) and np.array_equal(kept[1, :17], np.arange(17))
    # every frame skipped; an item without frames
    x = lp.copy()
    x[:, :, 0] = np.float32(-1e-3)
    kept, n2 = _check_filter(x, "f32", np.asarray([T, 17, 0], np.int32), 0, 0.6, "log", "all skipped")
    assert not n2.any() and not kept.any()
    # equal to the bound, NaN and +inf are kept; -inf is kept; a blank-dominated frame directly at seq_lens[b] is not counted
    c = bs.bound(0.6, "log")
    x = lp.copy()
    x[0, :, 0] = np.float32(-1e-3)
    x[0, 3, 0] = c
    x[0, 5, 0] = np.float32("nan")
    x[0, 7, 0] = np.float32("inf")
    x[0, 9, 0] = np.float32("-inf")
    x[0, 11, 0] = np.nextafter(c, np.float32(0))  # the next float above the bound: skipped
    kept, n2 = _check_filter(x, "f32", np.asarray([T, 17, 0], np.int32), 0, 0.6, "log", "specials")
    assert kept[0, :n2[0]].tolist() == [3, 5, 9], kept[0, :n2[0]]  # (+inf > c is true: skipped; NaN, -inf and the bound itself are kept)
    x[1, 17, 0] = np.float32(-1e-3)
    x[1, :17, 0] = np.float32(-5)
    kept, n2 = _check_filter(x, "f32", np.asarray([T, 17, 0], np.int32), 0, 0.6, "log", "a blank frame at seq_lens")
    assert n2[1] == 17
    # the same specials as half patterns
    for dt in ("f16", "bf16"):
        xh = bs.to_dtype_values(x, dt)
        xh[0, 3, 0] = np.float32(-0.5)
        _check_filter(xh, dt, np.asarray([T, 17, 0], np.int32), 0, math.exp(-0.5), "log", "specials " + dt)


def test_twin_widens_every_half_pattern_exactly():
    lib = bs._lib()
    u = np.arange(65536, dtype=np.uint32)
    want16 = u.astype(np.uint16).view(np.float16).astype(np.float32).view(np.uint32)
    got16 = np.asarray([lib.ctcskip_host_widen_bits(1, int(v)) for v in u], np.uint32)
    nan = np.isnan(want16.view(np.float32))
    assert np.array_equal(got16[~nan], want16[~nan]) and np.isnan(got16[nan].view(np.float32)).all()
    gotb = np.asarray([lib.ctcskip_host_widen_bits(2, int(v)) for v in u[::7]], np.uint32)
    assert np.array_equal(gotb, u[::7] << 16)


def test_nan_and_inf_definition_note():
    """The compare is ordered and strict: NaN is kept, the bound is kept -- and +inf, being greater than any finite bound, is
    skipped (the definition has no special case for it)."""
    with np.errstate(invalid="ignore"):
        v = np.asarray([np.nan, np.inf, -np.inf, bs.bound(0.6, "log")], np.float32)
        assert (~(v > bs.bound(0.6, "log"))).tolist() == [True, False, True, True]


def test_twin_remaps_the_oracles_results():
    """Both remaps of the twin on the oracle's decode of the anchor case's kept rows: the padded one equals the numpy restatement
    and leaves everything beyond the valid prefixes alone; the compact one, expanded, equals it too."""
    lp, sl = bs.anchor_input()
    want, kept, n2 = bs.anchor_want()
    raw = ou.decode(bs.gather_rows(lp, kept, n2), n2, beam=bs.ANCHOR["beam"], which=bs.which_oracle())
    ts = raw["timesteps"].copy()
    B, K, T = ts.shape
    for b in range(B):
        for p in range(K):
            ts[b, p, int(raw["lens"][b, p]):] = 7_000_000  # no index of a kept frame, and not to be read
    got = bs.host_remap_timesteps(ts, raw["lens"], kept, n2)
    for b in range(B):
        for p in range(K):
            L = int(raw["lens"][b, p])
            assert np.array_equal(got[b, p, :L], want["timesteps"][b, p, :L]), (b, p)
            assert (got[b, p, L:] == 7_000_000).all(), "words beyond a valid prefix were touched"
    hdr, ent, lab = bs.compact_of(raw)
    lab2 = bs.host_remap_compact(hdr, ent, lab, kept, n2, T)
    wh, we, wl = bs.compact_of(want)
    assert np.array_equal(lab2, wl), "the compact remap differs from the restatement"


def test_anchor_case_is_not_vacuous():
    """The certificate, on the oracle alone: every non-empty utterance keeps 25-75 % of its frames, at least 100 reported time steps
    change under the map, and at least one top row differs from the unfiltered decode."""
    lp, sl = bs.anchor_input()
    want, kept, n2 = bs.anchor_want()
    for b, n in enumerate(sl):
        if n:
            assert 0.25 * n <= n2[b] <= 0.75 * n, "item %d keeps %d of %d frames" % (b, n2[b], n)
    assert n2[2] == 0
    raw = ou.decode(bs.gather_rows(lp, kept, n2), n2, beam=bs.ANCHOR["beam"], which=bs.which_oracle())
    moved = sum(int((raw["timesteps"][b, p, :L] != want["timesteps"][b, p, :L]).sum())
                for b in range(len(sl)) for p in range(bs.ANCHOR["beam"]) for L in [int(raw["lens"][b, p])])
    assert moved >= 100, "only %d time steps move under the map" % moved
    full = bs.plain(lp, sl, beam=bs.ANCHOR["beam"])
    differ = [b for b in range(len(sl)) if int(full["lens"][b, 0]) != int(want["lens"][b, 0])
              or not np.array_equal(full["tokens"][b, 0], want["tokens"][b, 0]) or not np.array_equal(full["timesteps"][b, 0], want["timesteps"][b, 0])]
    assert differ, "the filtered decode's top rows equal the unfiltered decode's"
    print("anchor: kept %s of %s frames, %d time steps move, top rows differ in items %s" % (n2.tolist(), sl.tolist(), moved, differ))


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/blank_skip_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / "blank_skip_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(bs.NATIVE, "blank_skip_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert " 0 failures" in r.stdout
