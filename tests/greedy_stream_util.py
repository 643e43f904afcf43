"""Helpers of the tests of the greedy decode of live streams (TEST INFRASTRUCTURE ONLY).  What a chunked stream must return is derived
from ``greedy_util.reference`` of ALL its frames together by the slicing rule of include/ctcdecode_amd.h "Greedy decode of live
streams" alone -- a label belongs to the call its emitting frame lies in; a run is reported by the first call that knows its last
frame; a call's score is the score of the frames so far -- and not by a carry mechanism of its own.  Plus the scenarios the CPU and
the GPU tests share, and the ctypes front-end of the host twin (tests/native/greedy_stream_host.cpp)."""
import ctypes
import os
import subprocess

import greedy_util as gu
import numpy as np

F32 = np.float32
GREEDY_STREAM_HOST_SO = os.path.join(gu.ROOT, "oracle", "_build", "libctcgreedy_stream_host.so")
_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)
_u8p = ctypes.POINTER(ctypes.c_ubyte)


def clamp(n, T):
    return min(max(int(n), 0), int(T))


# ---- the slicing rule --------------------------------------------------------------------------------------------------------------
class StreamBook(object):
    """The test's book-keeping of one stream: the frames it was fed (their float32 copies) and the calls that fed them.  Nothing is
    decoded here."""

    def __init__(self, first_frame=0):
        self.first = int(first_frame)
        self.rows = []   # float32 [n, V] pieces
        self.calls = []  # (frames before the call, frames of the call, eos)
        self.frames = 0

    def feed(self, rows, eos):
        rows = np.ascontiguousarray(rows, np.float32)
        self.calls.append((self.frames, len(rows), bool(eos)))
        if len(rows):
            self.rows.append(rows)
        self.frames += len(rows)

    def all_rows(self, V):
        return np.concatenate(self.rows, 0) if self.rows else np.zeros((0, V), np.float32)


def item_reference(x, blank, mode, key=None):
    """``greedy_util.reference`` of one item of all the frames ``x`` [N, V], and the score of every prefix: by the definition, lp of
    frame 0 and then one float32 addition per frame.  ``key``: computed once per process and shared."""
    def make():
        N = len(x)
        ref = gu.reference(x[None] if N else np.zeros((1, 0, x.shape[1]), np.float32), None, blank, mode)
        lps = ref["lps"][0]
        prefix = np.zeros(N + 1, np.float32)
        for t in range(N):
            prefix[t + 1] = lps[t] if t == 0 else F32(prefix[t] + lps[t])
        assert N == 0 or gu.bits1(prefix[N]) == gu.bits1(ref["scores"][0])
        L = int(ref["lens"][0])
        return dict(tokens=ref["tokens"][0, :L].copy(), starts=ref["starts"][0, :L].copy(), ends=ref["ends"][0, :L].copy(),
                    label_scores=ref["label_scores"][0, :L].copy(), prefix=prefix, L=L)
    return make() if key is None else gu.cached(("stream item", key), make)


def slice_call(ref, first, N0, n, eos, Tc):
    """What the call that feeds frames [N0, N0 + n) returns, cut out of the reference of all frames: dict of rows [Tc] / [Tc + 1]."""
    out = dict(tokens=np.zeros(Tc, np.int32), starts=np.zeros(Tc, np.int32), ends=np.zeros(Tc + 1, np.int32), label_scores=np.zeros(Tc + 1, np.float32))
    # labels whose emitting frame lies in the chunk
    lo, hi = np.searchsorted(ref["starts"], N0, "left"), np.searchsorted(ref["starts"], N0 + n, "left")
    E = int(hi - lo)
    out["tokens"][:E] = ref["tokens"][lo:hi]
    out["starts"][:E] = ref["starts"][lo:hi].astype(np.int64) + first
    # runs with last frame e: reported by the first call with N0 + n > e + 1, or eos and N0 + n == e + 1.  No earlier call had eos, so
    # the earlier calls reported e + 1 < N0: this one reports N0 <= e + 1 < N0 + n, and e + 1 == N0 + n with eos
    lo = np.searchsorted(ref["ends"], N0 - 1, "left")
    hi = np.searchsorted(ref["ends"], N0 + n - 1, "right" if eos else "left")
    C = int(max(hi - lo, 0))
    out["ends"][:C] = ref["ends"][lo:lo + C].astype(np.int64) + first
    out["label_scores"][:C] = ref["label_scores"][lo:lo + C]
    out["lens"], out["closed_lens"] = E, C
    out["scores"] = ref["prefix"][N0 + n]  # (a stream that never had a frame: 0.0f)
    return out


# ---- scenarios -----------------------------------------------------------------------------------------------------------------------
def scenario(V, blank, mode, dtype, first_frames, calls, key=None):
    """first_frames: per stream.  calls: list of dict(raw float32 [B, Tc, V], streams [B] indices, eos [B], seq_lens None or [B])."""
    return dict(V=V, blank=blank, mode=mode, dtype=dtype, first_frames=list(first_frames), calls=calls, key=key)


def batch_scenario(case, cuts, eos_last=True, first_frames=None, key=None):
    """The items of a ``greedy_util`` case as streams of one batch, fed the frames [cuts[i], cuts[i + 1]) call by call; an item's
    ``seq_lens`` entry reaches every call shifted by the cut (negative and above Tc are clamped by the callee)."""
    x = case["x"]
    B, T, V = x.shape
    lens = np.full(B, T, np.int64) if case["seq_lens"] is None else np.asarray(case["seq_lens"], np.int64)
    cuts = [0] + [c for c in cuts if 0 < c < T] + [T]
    calls = []
    for i in range(len(cuts) - 1):
        a, b = cuts[i], cuts[i + 1]
        calls.append(dict(raw=x[:, a:b], streams=list(range(B)), eos=[eos_last and i == len(cuts) - 2] * B,
                          seq_lens=None if case["seq_lens"] is None else (lens - a).astype(np.int32)))
    return scenario(V, case["blank"], case["mode"], case["dtype"], first_frames or [0] * B, calls, key)


def expected(sc):
    """-> (the streams' books, per call the dict of expected arrays, per call the stored rows of the scenario's element type)."""
    books = [StreamBook(f) for f in sc["first_frames"]]
    stored_rows = []
    for c in sc["calls"]:
        raw = np.ascontiguousarray(c["raw"], np.float32)
        Tc = raw.shape[1]
        stored, x = gu.as_dtype(raw, sc["dtype"])
        stored_rows.append(stored)
        for b, s in enumerate(c["streams"]):
            books[s].feed(x[b, :Tc if c["seq_lens"] is None else clamp(c["seq_lens"][b], Tc)], c["eos"][b])
    refs = [item_reference(bk.all_rows(sc["V"]), sc["blank"], sc["mode"], None if sc["key"] is None else (sc["key"], s)) for s, bk in enumerate(books)]
    turn = [0] * len(books)
    wants = []
    for c in sc["calls"]:
        B, Tc, V = c["raw"].shape
        want = dict(tokens=np.zeros((B, Tc), np.int32), starts=np.zeros((B, Tc), np.int32), ends=np.zeros((B, Tc + 1), np.int32),
                    label_scores=np.zeros((B, Tc + 1), np.float32), scores=np.zeros(B, np.float32), lens=np.zeros(B, np.int32), closed_lens=np.zeros(B, np.int32))
        for b, s in enumerate(c["streams"]):
            N0, n, eos = books[s].calls[turn[s]]
            turn[s] += 1
            w = slice_call(refs[s], books[s].first, N0, n, eos, Tc)
            for k in want:
                want[k][b] = w[k]
        wants.append(want)
    return books, wants, stored_rows


def play(sc, make_stream, call):
    """Runs the scenario.  ``make_stream(first_frame)`` -> a stream object; ``call(streams, eos, stored, seq_lens, sc)`` -> dict of
    numpy arrays tokens / starts [B, Tc], ends / label_scores [B, Tc + 1], closed_lens / scores / lens [B].  Every call's output is
    compared, bit for bit, with the slices of the references of the streams' whole inputs.  -> (stream objects, books, outputs)."""
    books, wants, stored = expected(sc)
    streams = [make_stream(f) for f in sc["first_frames"]]
    outs = [call([streams[s] for s in c["streams"]], c["eos"], rows, c["seq_lens"], sc) for c, rows in zip(sc["calls"], stored)]
    for j, (c, got, want) in enumerate(zip(sc["calls"], outs, wants)):
        B = len(c["streams"])
        what = "%s call %d" % (sc["key"], j)
        for k in ("tokens", "starts", "ends", "lens", "closed_lens"):
            if got.get(k) is not None:
                assert not (np.asarray(got[k]) == gu.SENTINEL).any(), "%s: a position of %s was not written" % (what, k)
        if got.get("label_scores") is not None:
            assert not (np.asarray(got["label_scores"]).view(np.int32) == gu.SENTINEL).any(), "%s: a position of label_scores was not written" % what
        gu.assert_same(got, want, what)
        if got.get("closed_lens") is not None:
            assert np.array_equal(np.asarray(got["closed_lens"]).reshape(B), want["closed_lens"]), "%s: closed_lens %s, want %s" % (what, got["closed_lens"], want["closed_lens"])
    return streams, books, outs


def joined(outs, b=0):
    """The calls' outputs for batch position b concatenated over the calls: (tokens, starts, ends, label_scores)."""
    tok = np.concatenate([o["tokens"][b, : o["lens"][b]] for o in outs])
    st = np.concatenate([o["starts"][b, : o["lens"][b]] for o in outs])
    en = np.concatenate([o["ends"][b, : o["closed_lens"][b]] for o in outs])
    ls = np.concatenate([o["label_scores"][b, : o["closed_lens"][b]] for o in outs])
    return tok, st, en, ls


# ---- named cases -----------------------------------------------------------------------------------------------------------------------
A, Bb, BL = 1, 2, 0  # labels a, b and the blank of the emission cases (V = 4)


def path_calls(paths, eos, mode=1, seed=0):
    """One stream; call i feeds the frames whose labels are ``paths[i]`` (a list, possibly empty); ``eos[i]`` per call."""
    rng = np.random.default_rng(gu.hash_name("stream paths %s %d %d" % (paths, mode, seed)))
    calls = []
    for p, e in zip(paths, eos):
        raw = gu.path_rows(rng, [list(p)], 4, mode) if len(p) else np.zeros((1, 0, 4), np.float32)
        calls.append(dict(raw=raw, streams=[0], eos=[e], seq_lens=None))
    return calls


EMISSION_CASES = {
    "a a | a": ([[A, A], [A]], [False, False]),
    "a | _ a": ([[A], [BL, A]], [False, False]),
    "a | b": ([[A], [Bb]], [False, False]),
    "a _ | a": ([[A, BL], [A]], [False, False]),
    "_ | _": ([[BL], [BL]], [False, False]),
    "a | | a": ([[A], [], [A]], [False, False, False]),
    "a | eos": ([[A], []], [False, True]),
    "eos alone": ([[]], [True]),
    "a | b eos": ([[A], [Bb]], [False, True]),
}


def emission_scenario(name, mode=1, dtype=0):
    paths, eos = EMISSION_CASES[name]
    return scenario(4, BL, mode, dtype, [0], path_calls(paths, eos, mode), key="emission %s %d %d" % (name, mode, dtype))


def zero_calls(first, second, eos_second=True):
    """Mode 1, one stream, one run of label 1 over two calls of one frame each whose lp are ``first`` and ``second``."""
    calls = []
    for v, e in ((first, False), (second, eos_second)):
        raw = np.full((1, 1, 4), -5.0, np.float32)
        raw[0, 0, A] = v
        calls.append(dict(raw=raw, streams=[0], eos=[e], seq_lens=None))
    return calls


def ages_scenario(mode, dtype=0, Tc=6, V=5):
    """Five streams of different ages in one call: ragged seq_lens [0, 1, Tc, Tc + 9, -3], eos for two; the others go on in a second call."""
    rng = np.random.default_rng(gu.hash_name("ages %d %d" % (mode, dtype)))
    calls = []
    for s, k in enumerate((0, 1, 2, 3, 1)):  # stream s has had k calls of its own before the batch
        for _ in range(k):
            calls.append(dict(raw=np.round(gu.random_rows(rng, 1, 3, V, mode, 3.0) * 2) / 2 if mode else gu.random_rows(rng, 1, 3, V, mode, 3.0),
                              streams=[s], eos=[False], seq_lens=None))
    calls.append(dict(raw=gu.random_rows(rng, 5, Tc, V, mode, 3.0), streams=[0, 1, 2, 3, 4], eos=[False, True, False, True, False],
                      seq_lens=np.asarray([0, 1, Tc, Tc + 9, -3], np.int32)))
    calls.append(dict(raw=gu.random_rows(rng, 3, 4, V, mode, 3.0), streams=[4, 0, 2], eos=[True, False, True], seq_lens=np.asarray([4, 2, 0], np.int32)))
    return scenario(V, 1, mode, dtype, [0, 5, 0, 100, 7], calls, key="ages %d %d" % (mode, dtype))


def family_scenario(V, mode, dtype):
    """Random rows of V labels (29: lanes, 65: a wave, 1024: a workgroup per frame) in three calls of 3, 1 and 4 frames, two streams."""
    c = gu.shape_case(V, mode, dtype, T=8, B=2)
    return batch_scenario(c, [3, 4], key="family %d %d %d" % (V, mode, dtype))


# ---- the host twin -----------------------------------------------------------------------------------------------------------------
def build_greedy_stream_host():
    src = os.path.join(gu.NATIVE, "greedy_stream_host.cpp")
    csrc = os.path.join(gu.ROOT, "ctcdecode_amd", "csrc")
    deps = [src] + [os.path.join(csrc, f) for f in ("greedy.h", "align.h", "blank_skip.h", "exact_math_f64.h", "exact_math_f64_tables.h", "exact_math.h")]
    so = GREEDY_STREAM_HOST_SO
    if os.path.exists(so) and all(os.path.getmtime(so) >= os.path.getmtime(p) for p in deps):
        return so
    os.makedirs(os.path.dirname(so), exist_ok=True)
    tmp = "%s.%d.tmp" % (so, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", src, "-o", tmp], check=True)
    os.replace(tmp, so)
    return so


def _lib():
    def make():
        lib = ctypes.CDLL(build_greedy_stream_host())
        lib.ctcgreedy_stream_host_init.argtypes = [_i32p, ctypes.c_longlong]
        lib.ctcgreedy_stream_host_info.argtypes = [_i32p, ctypes.POINTER(ctypes.c_longlong)]
        lib.ctcgreedy_stream_host_info.restype = None
        lib.ctcgreedy_stream_host_decode.argtypes = [_i32p, _u8p, ctypes.c_void_p, ctypes.c_int, _i32p] + [ctypes.c_int] * 5 + [_i32p, _i32p, _i32p, _f32p, _i32p, _f32p, _i32p]
        assert lib.ctcgreedy_stream_host_record_bytes() == 32
        return lib
    return gu.cached("stream lib", make)


class HostStream(object):
    """A stream of the twin: its record, 8 words."""

    def __init__(self, first_frame=0):
        self.rec = np.zeros(8, np.int32)
        assert _lib().ctcgreedy_stream_host_init(self.rec.ctypes.data_as(_i32p), int(first_frame)) == 0

    def info(self):
        out = (ctypes.c_longlong * 5)()
        _lib().ctcgreedy_stream_host_info(self.rec.ctypes.data_as(_i32p), out)
        return dict(frames=int(out[0]), emitted=int(out[1]), closed=int(out[2]), open_run=bool(out[3]), ended=bool(out[4]))


def host_call_rc(streams, eos, stored, dtype, seq_lens, blank, mode, details=True):
    """The twin's chunk call over output buffers of sentinel words -> (return code, outputs).  The streams' records are updated."""
    stored = np.ascontiguousarray(stored)
    B, Tc, V = stored.shape
    recs = np.ascontiguousarray(np.stack([s.rec for s in streams]) if B else np.zeros((0, 8), np.int32))
    tok, st = (np.full((B, Tc), gu.SENTINEL, np.int32) for _ in range(2))
    en = np.full((B, Tc + 1), gu.SENTINEL, np.int32)
    ls = np.full((B, Tc + 1), gu.SENTINEL, np.int32).view(np.float32)
    closed, lens = (np.full((B,), gu.SENTINEL, np.int32) for _ in range(2))
    sc = np.full((B,), np.float32(-123.0), np.float32)
    sl = None if seq_lens is None else np.ascontiguousarray(seq_lens, np.int32)
    flags = np.ascontiguousarray([1 if e else 0 for e in eos], np.uint8)
    p = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    rc = _lib().ctcgreedy_stream_host_decode(p(recs, _i32p), p(flags, _u8p), stored.ctypes.data, dtype, None if sl is None else p(sl, _i32p), B, Tc, V, blank, mode,
                                             p(tok, _i32p), p(st, _i32p), p(en, _i32p) if details else None, p(ls, _f32p) if details else None,
                                             p(closed, _i32p) if details else None, p(sc, _f32p), p(lens, _i32p))
    for s, r in zip(streams, recs):
        s.rec[:] = r
    return rc, dict(tokens=tok, starts=st, ends=en if details else None, label_scores=ls if details else None, closed_lens=closed if details else None,
                    scores=sc, lens=lens)


def host_call(streams, eos, stored, seq_lens, sc):
    rc, out = host_call_rc(streams, eos, stored, sc["dtype"], seq_lens, sc["blank"], sc["mode"])
    assert rc == 0, "the twin refused its arguments (%d)" % rc
    return out
