"""The blank-frame filter of live streams on the CPU: the host twin (tests/native/stream_blank_skip_host.cpp) compiles the routines of
ctcdecode_amd/csrc/stream_blank_skip.h the kernels compile.  The scan with carry over a concatenation cut into chunks must give the
map and the counts of ``blank_skip_util.filter_frames`` on the whole, for every cut and element width; both remaps must equal
``blank_skip_util.remap``, on padded rows and on ``compact_of`` records; the guard leaves alone what is no index of a decoded frame;
the stand-alone sanitizer driver."""
import os
import subprocess

import numpy as np
import pytest

import blank_skip_util as bu
import oracle_util as ou
import stream_blank_skip_util as su

N, V, THR = 2200, 5, 0.6
_CACHE = {}


def _whole(dtype):
    """(storage [2, N, V], kept, n') of the scan-carry case: V 5, 2200 frames, seed 7, blank bias 4, thr 0.6 -- computed once per dtype."""
    if dtype not in _CACHE:
        lp = bu.to_dtype_values(ou.synth_logprobs(2, N, V, 7, blank_bias=4.0), dtype)
        kept, n2 = bu.filter_frames(lp, None, 0, THR, "log")
        assert dtype != "f32" or n2.tolist() == [102, 108], "the case is not the one the scan-carry tests were written for"
        _CACHE[dtype] = (bu.to_dtype_bits(lp, dtype), kept, n2)
    return _CACHE[dtype]


def _values(bits, dtype):
    """The float32 values of a storage array (the inverse of blank_skip_util.to_dtype_bits)."""
    if dtype == "f32":
        return bits
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32) if dtype == "bf16" else bits.view(np.float16).astype(np.float32)


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("size", [1, 3, 63, 64, 65, 1023, 1024, 1025])
def test_scan_with_carry_equals_the_filter_of_the_whole(size, dtype):
    bits, kept, n2 = _whole(dtype)
    st = su.HostStreams(2, dtype, 0, bu.bound(THR, "log"))
    for a, z in su.cuts(N, size):
        ck, cn = st.feed(bits[:, a:z])
        for b in range(2):  # the chunk-local list the gather reads: the kept frames of [a, z), counted from a
            want = kept[b, :n2[b]][(kept[b, :n2[b]] >= a) & (kept[b, :n2[b]] < z)] - a
            assert cn[b] == len(want) and np.array_equal(ck[b, :cn[b]], want) and (ck[b, cn[b]:] == -1).all(), (a, z, b)
    assert st.seen.tolist() == [N, N] and st.frames.tolist() == n2.tolist()
    for b, m in enumerate(st.maps()):
        assert np.array_equal(m, kept[b, :n2[b]]), b


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_zero_length_chunks_and_ragged_lengths(dtype):
    """Chunks of changing sizes with zero-length chunks between them; item 1 sees a ragged part of every chunk, so its seen frames are
    a concatenation of its own."""
    bits, _, _ = _whole(dtype)
    rng = np.random.default_rng(3)
    st = su.HostStreams(2, dtype, 0, bu.bound(THR, "log"))
    seen1, at, call = [], 0, 0
    while at < N:
        size = 0 if call % 3 == 1 else int(rng.integers(1, 1400))
        z = min(at + size, N)
        l1 = int(rng.integers(0, z - at + 1))
        st.feed(bits[:, at:z], np.asarray([z - at + 5, l1], np.int32))  # (item 0: a length beyond T is clamped)
        seen1.append(bits[1, at:at + l1])
        at, call = z, call + 1
    whole1 = np.concatenate(seen1)[None]
    _, k0, n0 = _whole(dtype)
    k1, n1 = bu.filter_frames(_values(whole1, dtype), None, 0, THR, "log")
    assert st.seen.tolist() == [N, whole1.shape[1]] and st.frames.tolist() == [int(n0[0]), int(n1[0])]
    m = st.maps()
    assert np.array_equal(m[0], k0[0, :n0[0]]) and np.array_equal(m[1], k1[0, :n1[0]])


def test_a_threshold_that_skips_everything_and_one_that_skips_nothing():
    bits, _, _ = _whole("f32")
    for c, want in ((-np.inf, 0), (np.inf, 100)):  # v > -inf for every finite v: all skipped; v > +inf never: all kept
        st = su.HostStreams(2, "f32", 0, c)
        for a, z in su.cuts(100, 37):
            st.feed(bits[:, a:z])
        assert st.frames.tolist() == [want, want] and st.seen.tolist() == [100, 100]
        if want:
            assert all(np.array_equal(m, np.arange(100)) for m in st.maps())


def _fake_result(rng, B, K, T, n2):
    """A result dict of the oracle's shape with time steps that index kept frames (what a decode of the kept rows reports)."""
    res = dict(tokens=np.zeros((B, K, T), np.int32), timesteps=np.zeros((B, K, T), np.int32), lens=np.zeros((B, K), np.int32), nres=np.zeros((B,), np.int32))
    for b in range(B):
        res["nres"][b] = K if n2[b] else 1
        for p in range(int(res["nres"][b])):
            L = int(rng.integers(0, n2[b] + 1))
            res["lens"][b, p] = L
            res["tokens"][b, p, :L] = rng.integers(1, 29, L)
            res["timesteps"][b, p, :L] = np.sort(rng.choice(n2[b], L, replace=False)) if L else []
    return res


def test_both_remaps_equal_the_numpy_remap():
    lp, sl = bu.anchor_input()
    kept, n2 = bu.filter_frames(lp, sl, 0, bu.ANCHOR["thr"], "log")
    assert n2.tolist() == [77, 57, 0, 40]
    B, T = lp.shape[:2]
    res = _fake_result(np.random.default_rng(1), B, 8, T, n2)
    want = bu.remap(res, kept)
    maps = [kept[b, :n2[b]] for b in range(B)]
    got = su.host_remap_rows(res["timesteps"], res["lens"], maps, n2)
    assert np.array_equal(got, want["timesteps"])
    hdr, ent, lab = bu.compact_of(res)
    whdr, went, wlab = bu.compact_of(want)
    assert np.array_equal(su.host_remap_compact(hdr, ent, lab, maps, n2), wlab) and np.array_equal(hdr, whdr) and np.array_equal(ent, went)
    # a peek's rows: reported from depth since[b] on, the lengths are the full ones
    since = np.asarray([3, 0, 0, 50], np.int32)
    cut = np.zeros_like(res["timesteps"])
    wcut = np.zeros_like(cut)
    for b in range(B):
        for p in range(8):
            n = max(0, int(res["lens"][b, p]) - int(since[b]))
            cut[b, p, :n] = res["timesteps"][b, p, since[b]:since[b] + n]
            wcut[b, p, :n] = want["timesteps"][b, p, since[b]:since[b] + n]
    assert np.array_equal(su.host_remap_rows(cut, res["lens"], maps, n2, since=since), wcut)
    # a commit's rows: one row per stream, each at a place of its own
    rows = [res["timesteps"][b, 0, :res["lens"][b, 0]].copy() for b in range(B)]
    su.host_remap_rows(None, res["lens"][:, 0], maps, n2, rows=rows)
    for b in range(B):
        assert np.array_equal(rows[b], want["timesteps"][b, 0, :res["lens"][b, 0]]), b


def test_the_guard_leaves_alone_what_is_no_index_of_a_decoded_frame():
    maps = [np.asarray([4, 9, 70000], np.int32), np.zeros((0,), np.int32)]
    frames = np.asarray([3, 0], np.int32)
    ts = np.asarray([[[0, 1, 2, 3, -1, 2]], [[0, 1, 2, 3, 4, 5]]], np.int32)
    lens = np.asarray([[5], [9]], np.int32)  # (a length beyond the row's stride is clamped to it)
    got = su.host_remap_rows(ts, lens, maps, frames)
    assert got.tolist() == [[[4, 9, 70000, 3, -1, 2]], [[0, 1, 2, 3, 4, 5]]]
    # compact records: an index at or beyond the stream's frames, and an image that does not fit 16 bits, stay
    hdr = np.asarray([[1, 4, 0, 0], [0, 0, 4, 0]], np.int32)
    ent = np.zeros((2, 1, 4), np.int32)
    ent[0, 0] = (0, 0, 4, 0)
    lab = np.asarray([7 | 0 << 16, 8 | 1 << 16, 9 | 2 << 16, 10 | 3 << 16, 11 | 0 << 16], np.uint32)
    got = su.host_remap_compact(hdr, ent, lab, maps, frames)
    assert got.tolist() == [7 | 4 << 16, 8 | 9 << 16, 9 | 2 << 16, 10 | 3 << 16, 11 | 0 << 16]
    assert su.lib().ctcsskip_host_compact_route_ok(65536 - 6000, 6000) == 1 and su.lib().ctcsskip_host_compact_route_ok(60000, 6000) == 0
    assert [su.lib().ctcsskip_host_map_grown_cap(c, n) for c, n in ((0, 37), (256, 257), (1024, 1025), (512, 5000))] == [256, 512, 2048, 8192]


def test_sanitizer_driver_runs_clean(tmp_path):
    """tests/native/stream_blank_skip_host_main.cpp, built with -fsanitize=address,undefined and run as a program of its own."""
    exe = str(tmp_path / "stream_blank_skip_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(su.NATIVE, "stream_blank_skip_host_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert "stream_blank_skip_host_main: ok" in r.stdout
