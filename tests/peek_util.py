"""Helpers of the streaming-peek tests (TEST INFRASTRUCTURE ONLY): the host twin of the peek (tests/native/peek_host.cpp: the host
build of the core fed chunk by chunk, ctcdecode_amd/csrc/stream_peek.h run on the parked state between chunks), the inputs both test
files use, and the comparisons against the oracle's one-shot decode of the frames fed so far."""
import ctypes
import os

import numpy as np
import oracle_util as ou

ROOT = ou.ROOT
DATA = os.path.join(ROOT, "tests", "data")
PEEK_HOST_SO = os.path.join(ROOT, "oracle", "_build", "libctcpeek_host.so")

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)


def build_peek_host():
    import subprocess

    src = os.path.join(ROOT, "tests", "native", "peek_host.cpp")
    csrc = os.path.join(ROOT, "ctcdecode_amd", "csrc")
    deps = [src, os.path.join(ROOT, "tests", "native", "core_host.cpp")] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")]
    if os.path.exists(PEEK_HOST_SO) and all(os.path.getmtime(PEEK_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return PEEK_HOST_SO
    os.makedirs(os.path.dirname(PEEK_HOST_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (PEEK_HOST_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-DCTC_ASSUME_CHECKED", src, "-o", tmp, "-lpthread"], check=True)
    os.replace(tmp, PEEK_HOST_SO)
    return PEEK_HOST_SO


def which_oracle():
    return "reference" if ou.have_reference() else "restated"


class HostStream(object):
    """One stream of the host twin."""

    def __init__(self, V, beam, cap_frames, cutoff_prob=1.0, cutoff_top_n=40, blank_id=0, lm=None):
        self.lib = ctypes.CDLL(build_peek_host())
        self.lib.ctcpeek_host_create.restype = ctypes.c_void_p
        self.lib.ctcpeek_host_create.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                                 ctypes.c_char_p, ctypes.c_char_p]
        self.lib.ctcpeek_host_destroy.argtypes = [ctypes.c_void_p]
        self.lib.ctcpeek_host_destroy.restype = None
        self.lib.ctcpeek_host_feed.argtypes = [ctypes.c_void_p, _f32p, ctypes.c_int, ctypes.c_int, _i32p, _i32p, _f32p, _i32p, _i32p, ctypes.c_int]
        self.lib.ctcpeek_host_peek.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, _i32p, _i32p, ctypes.c_int, _f32p, _i32p, _i32p, _i32p,
                                               ctypes.POINTER(ctypes.c_ulonglong)]
        self.V, self.beam, self.frames = V, beam, 0
        if lm is not None:
            alpha, beta, path, labels = lm
            self.h = self.lib.ctcpeek_host_create(V, beam, cap_frames, cutoff_prob, cutoff_top_n, blank_id, alpha, beta, os.fsencode(path), ou._pack(labels))
        else:
            self.h = self.lib.ctcpeek_host_create(V, beam, cap_frames, cutoff_prob, cutoff_top_n, blank_id, 0.0, 0.0, None, None)
        if not self.h:
            raise RuntimeError("could not create the host stream")

    def feed(self, rows, finish=False):
        """rows [len, V]; finish: ends the stream and returns its result dict (one item)."""
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.V)
        T = self.frames + rows.shape[0]
        K = self.beam
        out = dict(tokens=np.zeros((1, K, T), np.int32), timesteps=np.zeros((1, K, T), np.int32), scores=np.zeros((1, K), np.float32),
                   lens=np.zeros((1, K), np.int32), nres=np.zeros((1,), np.int32))
        rc = self.lib.ctcpeek_host_feed(self.h, ou._ptr(rows, _f32p), rows.shape[0], 1 if finish else 0, ou._ptr(out["tokens"], _i32p),
                                        ou._ptr(out["timesteps"], _i32p), ou._ptr(out["scores"], _f32p), ou._ptr(out["lens"], _i32p),
                                        ou._ptr(out["nres"], _i32p), T)
        if rc != 1:
            raise RuntimeError("host stream: feed returned %d" % rc)
        self.frames = T
        return out if finish else None

    def peek(self, n_best=1, since=0, L_cap=None):
        """-> (dict(tokens[n_best, L_cap], timesteps, scores[n_best], lens[n_best], nres, stable), fits, digest of the state)."""
        L_cap = max(0, self.frames - since) if L_cap is None else L_cap
        tok = np.full((n_best, L_cap), -7, np.int32)
        ts = np.full((n_best, L_cap), -7, np.int32)
        sc = np.full((n_best,), np.nan, np.float32)
        ln = np.full((n_best,), -7, np.int32)
        nres = np.full((1,), -7, np.int32)
        stable = np.full((1,), -7, np.int32)
        dig = ctypes.c_ulonglong(0)
        rc = self.lib.ctcpeek_host_peek(self.h, n_best, since, ou._ptr(tok, _i32p), ou._ptr(ts, _i32p), L_cap, ou._ptr(sc, _f32p), ou._ptr(ln, _i32p),
                                        ou._ptr(nres, _i32p), ou._ptr(stable, _i32p), ctypes.byref(dig))
        return dict(tokens=tok, timesteps=ts, scores=sc, lens=ln, nres=int(nres[0]), stable=int(stable[0])), rc == 1, int(dig.value)

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.ctcpeek_host_destroy(self.h)
            self.h = None


# ---- inputs ----------------------------------------------------------------------------------------------------------
def peaky_logprobs(B, T, V, seed, hold=5, strong=20.0, weak=1.0, p_weak=0.4, blank_id=0):
    """Transcript-like rows: a label (or the blank) dominates for a few frames, then the next one -- most stretches with a sharp peak
    (the model is sure), some with a faint one (it is not): the beam's alternatives gather at the unsure stretches, and what lies
    before the oldest of them is common to all of them."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    for b in range(B):
        t = 0
        while t < T:
            n = int(rng.integers(1, hold + 1))
            c = blank_id if rng.random() < 0.5 else int(rng.integers(0, V))
            x[b, t:t + n, c] += np.float32(weak if rng.random() < p_weak else strong)
            t += n
    m = x.max(axis=-1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=np.float32), dtype=np.float32)
    return (x - lse).astype(np.float32)


# the five input classes whose oracle common prefix must be long enough for the properties to mean something (B = 3 each)
def five_classes():
    return [
        dict(name="randn", lp=ou.synth_logprobs(3, 240, 29, 61), kw=dict(beam=50)),
        dict(name="blank_dominated", lp=ou.synth_logprobs(3, 300, 29, 63, blank_bias=4), kw=dict(beam=20)),
        dict(name="quantised", lp=ou.synth_logprobs(3, 150, 9, 62, quant=0.5), kw=dict(beam=100)),
        dict(name="peaky_k100", lp=peaky_logprobs(3, 300, 29, 64), kw=dict(beam=100)),
        dict(name="peaky_k20", lp=peaky_logprobs(3, 300, 29, 65), kw=dict(beam=20)),
    ]


def pruned_class():
    return dict(name="pruned", lp=ou.synth_logprobs(3, 120, 64, 64), kw=dict(beam=16, cutoff_top_n=8))


LABELS29 = ["_", "'", " "] + [chr(ord("a") + i) for i in range(26)]  # blank first
ABCD = ["_", "a", "b", "c", "d", "'", " "]
# (tests/test_lm.py's LM_CASES generator, restated: words of the model must actually complete)
LM_PEEK_CASES = [
    dict(name="testarpa", arpa="test.arpa", labels=LABELS29, alpha=1.5, beta=0.8, B=3, T=120, K=40, seed=101, bias={" ": 1.5, "a": 1.0}),
    dict(name="testarpa_quant", arpa="test.arpa", labels=LABELS29, alpha=1.5, beta=0.8, B=3, T=100, K=40, seed=111, bias={" ": 1.5, "a": 1.0}, quant=0.5),
    dict(name="abcd_words_full", arpa="abcd_words.arpa", labels=ABCD, alpha=0.4, beta=2.0, B=3, T=100, K=3, seed=105, quant=0.5),
    dict(name="chars", arpa="chars.arpa", labels=["_", "a", "b", "c", "d", "'", "é", " "], alpha=0.6, beta=0.2, B=3, T=100, K=24, seed=106),
    dict(name="chars_quant", arpa="chars.arpa", labels=["_", "a", "b", "c", "d", "'", "é", " "], alpha=0.6, beta=0.2, B=3, T=80, K=24, seed=116, quant=0.5),
    dict(name="abcd_topn", arpa="abcd_words.arpa", labels=ABCD, alpha=0.7, beta=0.9, B=3, T=100, K=20, seed=108, top_n=4),
]


def lm_case_inputs(c):
    V = len(c["labels"])
    lp = ou.synth_logprobs(c["B"], c["T"], V, c["seed"])
    if c.get("bias"):
        x = lp.copy()
        for ch, v in c["bias"].items():
            x[:, :, c["labels"].index(ch)] += np.float32(v)
        m = x.max(-1, keepdims=True)
        lp = (x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))).astype(np.float32)
    if c.get("quant"):  # (after the bias: equal scores are the point)
        lp = (np.round(lp / np.float32(c["quant"])) * np.float32(c["quant"])).astype(np.float32)
    return np.ascontiguousarray(lp), dict(beam=c["K"], cutoff_top_n=c.get("top_n", 40))


# ---- the oracle's side -----------------------------------------------------------------------------------------------
def oracle_prefix(lp, F, which, scorer=None, **kw):
    """The one-shot decode of the first F frames of every item: the contract of a peek after F frames."""
    return ou.decode(np.ascontiguousarray(lp[:, :F]), which=which, scorer=scorer, **kw)


def common_prefix_len(res, b):
    """Length of the longest common prefix of ALL result rows of item b (tokens; computed from the oracle's output)."""
    n = int(res["nres"][b])
    lens = [int(v) for v in res["lens"][b, :n]]
    m = min(lens)
    first = res["tokens"][b, 0, :m]
    for p in range(1, n):
        d = np.nonzero(res["tokens"][b, p, :m] != first)[0]
        if len(d):
            m = int(d[0])
            first = first[:m]
    return m


def assert_peek_equals(got, want, b, n_best, since, what):
    """got: one stream's peek (tokens [n, L] from depth `since` on, ...); want: the oracle's result dict, item b."""
    n = min(n_best, int(want["nres"][b]))
    assert got["nres"] == n, "%s: n_results %d, want %d" % (what, got["nres"], n)
    assert np.array_equal(np.asarray(got["lens"][:n]), want["lens"][b, :n]), "%s: lens differ" % what
    sa = np.ascontiguousarray(got["scores"][:n], dtype=np.float32).view(np.uint32)
    sb = np.ascontiguousarray(want["scores"][b, :n]).view(np.uint32)
    assert np.array_equal(sa, sb), "%s: scores differ bitwise: %s vs %s" % (what, got["scores"][:n], want["scores"][b, :n])
    L = got["tokens"].shape[1]
    for p in range(n):
        ln = int(want["lens"][b, p])
        r = max(0, ln - since)
        assert r <= L, "%s: row %d reports %d labels, width %d" % (what, p, r, L)
        assert np.array_equal(got["tokens"][p, :r], want["tokens"][b, p, since:since + r]), "%s: tokens differ (row %d)" % (what, p)
        assert np.array_equal(got["timesteps"][p, :r], want["timesteps"][b, p, since:since + r]), "%s: timesteps differ (row %d)" % (what, p)
        assert not got["tokens"][p, r:].any() and not got["timesteps"][p, r:].any(), "%s: positions behind row %d's end are not zero" % (what, p)
    for p in range(n, got["tokens"].shape[0]):
        assert not got["tokens"][p].any() and not got["timesteps"][p].any(), "%s: row %d beyond n_results is not zero" % (what, p)
    assert got["stable"] == common_prefix_len(want, b), "%s: stable_len %d, want %d" % (what, got["stable"], common_prefix_len(want, b))


def assert_starts_with(res, b, pre_tok, pre_ts, what):
    """Every result row of item b begins with the stable prefix, tokens and timesteps."""
    m = len(pre_tok)
    for p in range(int(res["nres"][b])):
        assert int(res["lens"][b, p]) >= m, "%s: row %d is shorter than the stable prefix" % (what, p)
        assert np.array_equal(res["tokens"][b, p, :m], pre_tok), "%s: row %d leaves the stable prefix (tokens)" % (what, p)
        assert np.array_equal(res["timesteps"][b, p, :m], pre_ts), "%s: row %d leaves the stable prefix (timesteps)" % (what, p)
