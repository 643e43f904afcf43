"""Helpers of the lattice matrix tests (TEST INFRASTRUCTURE ONLY): the cases that drive every instantiation <DT, PROB, CLS> of the
align, log-likelihood and posterior kernels -- three element types x two input modes x the row classes 0 / 1 / 4 / 16 -- and the walk
of lattice_device.h at its limits, with their references: the restatements of align_util / loglik_util / posterior_util, or a closed
form where a row has exactly one alignment.

  matrix       one launch that holds rows of all four classes; values exact in float32, float16 and bfloat16, so one reference per
               feature and mode serves every element type
  max_states   L = n = 2047 without adjacent repeats, S = 4095: the most states a workgroup holds; one alignment, exact sums
  third_wave   L = 1030 in 1040 frames, S = 2061: many alignments, states in the workgroup's third wave
  big_vocab    V = 70001, labels on both sides of 2^8 and 2^16, the blank near the end of a frame's row

The class census is computed here from the documented rule (S = 2L + 1 against 64 / 256 / 1024; groups of four consecutive rows; a
group whose rows all fit a wave goes to class 0) and not read from the library."""
import time

import align_util as au
import loglik_util as lu
import numpy as np
import posterior_util as pu

F32 = np.float32
FEATURES = ("align", "loglik", "posteriors")
DTYPES = ("float32", "float16", "bfloat16")  # (their index is the twins' dtype code)
MODES = ("log", "prob")
REFERENCE = dict(align=au.reference, loglik=lu.reference, posteriors=pu.reference)
ASSERT_SAME = dict(align=au.assert_same, loglik=lu.assert_same, posteriors=pu.assert_same)
TIMES = {}  # what each reference took to compute, in seconds: (case, feature, variant) -> float


# ---- cases -------------------------------------------------------------------------------------------------------------------------
MATRIX_SEQ = [518, 204, 74, 36]


def _matrix_rows(V):
    def c(L, first=0):
        return au.cycle(L, V, first=first)

    return [[c(513), [1, 1, 2], c(510, 2), []],
            [c(200), c(196, 1), [3], c(31, 3)],
            [c(70), c(32, 2), c(66, 1), c(5)],
            [c(31, 1), c(30), [2, 2], c(28, 3)]]


def single_path_case(L, V=4):
    """B = 1, R = 2, T = L_stride = L: two rows of L labels without adjacent repeats in L frames -- one alignment each -- over
    log-probabilities that are multiples of 0.25 in [-4, 0]: every sum is exact (the largest is 4 L), in all three element types."""
    rng = np.random.default_rng(au.hash_name("single_path_%d" % L))
    lp = (-0.25 * rng.integers(0, 17, (1, L, V))).astype(F32)
    tok, lens = au.pack_rows([[au.cycle(L, V), au.cycle(L, V, first=2)]], R=2, Ls=L)
    return dict(lp=lp, seq_lens=None, tokens=tok, lens=lens, blank=0)


BIG_VOCAB_LABELS = [1, 2, 255, 256, 65535, 65536, 65537, 70000]


def make_case(name):
    """-> dict(lp float32 [B, T, V], seq_lens, tokens, lens, blank), and for the cases with a probability mode p float32 [B, T, V]."""
    rng = np.random.default_rng(au.hash_name("lattice_" + name))
    if name == "matrix":
        B, T, V = 4, 518, 5
        tok, lens = au.pack_rows(_matrix_rows(V), R=4, Ls=T)
        lp = (-0.125 * rng.integers(0, 49, (B, T, V))).astype(F32)
        p = (rng.integers(0, 256, (B, T, V)) / 256.0).astype(F32)
        p[rng.random((B, T, V)) < 0.002] = 0.0
        return dict(lp=lp, p=p, seq_lens=np.asarray(MATRIX_SEQ, np.int32), tokens=tok, lens=lens, blank=0)
    if name == "max_states":
        return single_path_case(au.host_max_labels())
    if name == "third_wave":
        T, V, L = 1040, 5, 1030
        tok, lens = au.pack_rows([[au.cycle(L, V)]], R=1, Ls=T)
        return dict(lp=au.log_softmax_rows(rng, 1, T, V, scale=1.0), seq_lens=None, tokens=tok, lens=lens, blank=0)
    if name == "big_vocab":
        B, T, V, R, blank = 2, 12, 70001, 6, 69999
        rows = [[[BIG_VOCAB_LABELS[int(i)] for i in rng.integers(0, len(BIG_VOCAB_LABELS), int(rng.integers(0, 9)))] for _ in range(R)] for _ in range(B)]
        rows[0][0] = BIG_VOCAB_LABELS  # (every label at least once, in a row that has alignments)
        tok, lens = au.pack_rows(rows, R=R, Ls=T)
        lp = au.log_softmax_rows(rng, B, T, V)
        return dict(lp=lp, p=np.exp(lp), seq_lens=None, tokens=tok, lens=lens, blank=blank)
    raise KeyError(name)


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case(name):
    """The case, made once per process and left unchanged."""
    return _cached(("case", name), lambda: make_case(name))


def release():
    """Drops the cached cases and references: a test module that is done with them leaves the process as it found it."""
    _CACHE.clear()


# ---- inputs as the library and the twins take them ------------------------------------------------------------------------------------
def half_bits(x, dtype):
    """float32 -> the uint16 bit patterns of its float16 / bfloat16 copy (numpy's rounding; bfloat16 by truncation, for values it holds)."""
    if dtype == "float16":
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(x, F32).astype(np.float16).view(np.uint16)
    assert dtype == "bfloat16"
    return au.to_bf16_bits(x)


def widen(bits, dtype):
    return bits.view(np.float16).astype(F32) if dtype == "float16" else au.bf16_bits_to_f32(bits)


def exact_in(x, dtype):
    """Every value of x survives the trip through the element type."""
    return dtype == "float32" or bool(np.array_equal(widen(half_bits(x, dtype), dtype).view(np.uint32), np.ascontiguousarray(x, F32).view(np.uint32)))


def twin_rows(x, dtype):
    """-> (rows, dtype code) for the host twins: float32 as it is, the half types as uint16 bit patterns."""
    return (np.ascontiguousarray(x, F32), 0) if dtype == "float32" else (half_bits(x, dtype), DTYPES.index(dtype))


def host(feature, c, x, dtype="float32", mode="log"):
    """The feature's host twin on the case's labels over the rows x (log-probabilities, or probabilities for mode "prob")."""
    rows, code = twin_rows(x, dtype)
    fn = dict(align=au.host_align, loglik=lu.host_loglik, posteriors=pu.host_posteriors)[feature]
    got = fn(rows, c["seq_lens"], c["tokens"], c["lens"], c["blank"], log_input=0 if mode == "prob" else 1, dtype=code)
    assert got["invalid_rows"] == 0
    return got


# ---- references ------------------------------------------------------------------------------------------------------------------------
def used_columns(c):
    cols = {int(c["blank"])}
    for (b, r), L in np.ndenumerate(c["lens"]):
        cols.update(int(v) for v in c["tokens"][b, r, :L])
    return sorted(cols)


def prob_lp(name):
    """The log-probabilities the definition reads in the case's probability mode: align_util.prob_to_lp per element.  Only the columns
    of the blank and of the case's labels are formed; the others hold NaN, so a reference that read one would show it."""
    def make():
        c = case(name)
        cols = used_columns(c)
        lp = np.full(c["p"].shape, np.nan, F32)
        lp[:, :, cols] = au.prob_to_lp(c["p"][:, :, cols])
        return lp
    return _cached(("prob lp", name), make)


def reference_on(name, feature, variant, lp):
    """The feature's restatement on the case's labels over the log-probabilities lp, computed once per (case, feature, variant)."""
    def make():
        c = case(name)
        t0 = time.perf_counter()
        want = REFERENCE[feature](lp, c["seq_lens"], c["tokens"], c["lens"], c["blank"])
        TIMES[(name, feature, variant)] = time.perf_counter() - t0
        assert not want["status"].any(), "the case has no invalid row"
        return want
    return _cached(("reference", name, feature, variant), make)


def want(name, feature, mode="log"):
    """The reference of a case whose values every element type holds exactly: one per feature and mode.  The matrix's must not be
    degenerate: every row has alignments, every label is occupied, and the posterior restatement clamps at least one cell."""
    c = case(name)
    w = reference_on(name, feature, mode, c["lp"] if mode == "log" else prob_lp(name))
    if name == "matrix":
        if feature == "align":
            assert w["aligned"].all() and np.isfinite(w["scores"]).all()
        else:
            assert np.isfinite(w["loglik"]).all(), "every row has a finite log-likelihood"
        if feature == "posteriors":
            for (b, r), L in np.ndenumerate(c["lens"]):
                assert (w["occupancy"][b, r, :L] > 0).all(), ("a label without occupancy", mode, b, r)
            assert w["diag"]["clamped"] >= 1, "the restatement forms x > 0 at least once"
    return w


def single_path_expected(c):
    """The closed form of a case whose rows all have L == n without adjacent repeats, over values whose sums are exact: the label i
    sits on frame i alone -- starts = ends = peaks = i, occupancy 1.0f, confidence e80(lp[i, y_i]) -- and the score and the
    log-likelihood are the float32 sum in frame order.  -> {feature: the dict its assert_same takes}."""
    B, T, _ = c["lp"].shape
    R, Ls = c["tokens"].shape[1:]
    i32 = lambda: np.zeros((B, R, Ls), np.int32)
    f32 = lambda: np.zeros((B, R, Ls), F32)
    st, pk, occ, conf, sc = i32(), i32(), f32(), f32(), np.zeros((B, R), F32)
    rows = lu.single_path_rows(c)
    assert len(rows) == B * R, "every row has one alignment"
    for b, r, n in rows:
        L = int(c["lens"][b, r])
        assert L == n >= 1
        st[b, r, :L] = pk[b, r, :L] = np.arange(L)
        occ[b, r, :L] = 1.0
        conf[b, r, :L] = [pu.e80(v) for v in c["lp"][b, np.arange(L), c["tokens"][b, r, :L]]]
        sc[b, r] = lu.path_sum(c, b, r, n)
    status = np.zeros((B,), np.int32)
    return dict(align=dict(start=st, end=st.copy(), scores=sc, status=status), loglik=dict(loglik=sc, status=status),
                posteriors=dict(peaks=pk, occupancy=occ, confidence=conf, loglik=sc, status=status))


def max_states_expected():
    return _cached(("expected", "max_states"), lambda: single_path_expected(case("max_states")))


# ---- the class census ----------------------------------------------------------------------------------------------------------------
def census(c):
    """Which kernel class runs each row's recurrence, from the documented rule.  -> (rows, groups): rows = {cls: [(b, r, S), ...]} of
    the rows that run the recurrence (valid, n >= 1, L <= n); groups = [(first row, all_short, [S or None, ...]), ...]."""
    B, T, _ = c["lp"].shape
    R = c["tokens"].shape[1]
    lens = c["lens"].reshape(-1)
    rows, groups = {0: [], 1: [], 4: [], 16: []}, []
    for g0 in range(0, B * R, 4):
        states = []
        for h in range(g0, min(g0 + 4, B * R)):
            b = h // R
            n = T if c["seq_lens"] is None else min(max(int(c["seq_lens"][b]), 0), T)
            L = int(lens[h])
            states.append(2 * L + 1 if n >= 1 and 0 <= L <= n else None)
        all_short = all(S is None or S <= 64 for S in states)
        groups.append((g0, all_short, states))
        for h, S in zip(range(g0, g0 + 4), states):
            if S is not None:
                cls = 0 if all_short else (1 if S <= 256 else (4 if S <= 1024 else 16))
                rows[cls].append((h // R, h % R, S))
    return rows, groups
