"""Inputs and the host twin of the exact-shape kernel (beam 100 over 29 labels, blank 0: decode_kernel.h CTC_EXACT_SHAPES).

Shared by test_exact_shape_host.py (the exact policy of beam_core.h on the CPU, against the run-time policy and the oracle) and
test_gpu_exact_shape.py (the twin kernel against the planned kernel and the oracle, over the same inputs).  No torch here: the CPU
suite imports this module.  Every shape is the twin's own at T <= 64, B <= 8.  matrix_case() / matrix_inputs() are the kernel
matrix's recipe at the twin's shape (the select-path certificate, with overflow frames); SHAPES / parse_exact_shapes() tie the
tests to the header's list of shapes."""
import ctypes
import os
import subprocess

import numpy as np

import kernel_matrix_util as km
import oracle_util as ou
import select_path_util as sp
import stream_matrix_util as sm

BEAM, LABELS, BLANK = 100, 29, 0
# The table the tests cover, as decode_kernel.h CTC_EXACT_SHAPES lists it: (PROF code, beam, labels, blank, fold the live beam size).
# test_exact_shape_host.py holds the header to it: a further shape fails there until the tests have been taught about it.
SHAPES = [(6, 100, 29, 0, True)]
PARENT_KERNEL = (0, 0, 1, 0, 1024, 0, 0)  # the planned kernel a twin replaces (ctcdecode_amd.hip kExactParent)
KINDS = ["randn", "blank", "peaky", "quant", "minus_inf"]
LENGTHS = [0, 1, 2, 3, 5, 40]
RAGGED_T = 40
RAGGED_LENS = np.array([40, 0, 1, 2, 3, 5, 17, 33], np.int32)

EXACT_HOST_SO = os.path.join(ou.ROOT, "oracle", "_build", "libctcexact_host.so")


def rows(kind, B, T, seed):
    """[B, T, 29] float32 log-probabilities of one kind:
      randn      log-softmax of N(0, 1) logits;
      blank      ... with +6 on the blank logit (blank-dominated: chain-shaped beams);
      peaky      ... with +8 on one label per frame, in runs of 5-15 frames;
      quant      log-probabilities rounded to multiples of 1/4: equal scores cross the beam boundary (tie frames, exact replays);
      minus_inf  randn with -inf entries: single labels in every third frame, one whole frame (danger mode)."""
    if kind == "randn":
        return ou.synth_logprobs(B, T, LABELS, seed)
    if kind == "blank":
        return ou.synth_logprobs(B, T, LABELS, seed, blank_bias=6.0, blank_id=BLANK)
    if kind == "quant":
        return ou.synth_logprobs(B, T, LABELS, seed, quant=0.25)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, LABELS)).astype(np.float32)
    if kind == "peaky":
        for b in range(B):
            t = 0
            while t < T:
                run, c = int(rng.integers(5, 16)), int(rng.integers(0, LABELS))
                x[b, t:t + run, c] += np.float32(8.0)
                t += run
    m = x.max(axis=-1, keepdims=True)
    lp = (x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=np.float32), dtype=np.float32))).astype(np.float32)
    if kind == "minus_inf":
        lp[:, ::3, 2] = -np.inf
        lp[:, 1::4, 7] = -np.inf
        if T > 6:
            lp[:, 6, :] = -np.inf
    elif kind != "peaky":
        raise ValueError(kind)
    return np.ascontiguousarray(lp, dtype=np.float32)


def cases():
    """(name, rows [B, T, 29], seq_lens or None): every kind at every length (B = 2), and every kind as a ragged batch of eight
    whose lengths include 0."""
    out = []
    for ki, kind in enumerate(KINDS):
        for T in LENGTHS:
            out.append(("%s_T%d" % (kind, T), rows(kind, 2, T, 100 + 10 * ki + T), None))
        out.append(("%s_ragged" % kind, rows(kind, len(RAGGED_LENS), RAGGED_T, 900 + ki), RAGGED_LENS.copy()))
    return out


def parse_exact_shapes(header_text):
    """The X(code, beam, labels, blank, fold) items of the product branch of CTC_EXACT_SHAPES (the #else branch, not the
    CTC_EXACT_STAGE1 measurement build) -> list of (int, int, int, int, bool), in the order of the list."""
    import re

    m = re.search(r"#if defined\(CTC_EXACT_STAGE1\).*?\n#else\s*\n#define CTC_EXACT_SHAPES\(X\)(.*?)\n#endif", header_text, flags=re.S)
    assert m, "the product branch of CTC_EXACT_SHAPES was not found"
    words = {"true": True, "false": False}
    out = []
    for it in re.findall(r"\bX\(([^)]*)\)", m.group(1)):
        args = [a.strip() for a in it.split(",")]
        assert len(args) == 5 and args[4] in words, it
        out.append(tuple(int(a) for a in args[:4]) + (words[args[4]],))
    return out


def matrix_case():
    """The kernel matrix's recipe (kernel_matrix_util.inputs) at the twin's shape: the planned kernel's case with 29 labels, beam 100,
    blank 0.  The twin is outside CTC_KERNEL_LIST and so outside kernel_matrix_util.CASES; this is the case it would have there."""
    c = km._case(PARENT_KERNEL, V=LABELS, K=BEAM, T=40, B=4, threads=1024, blank=BLANK)
    c["seed"] = 9100
    return c


def matrix_inputs(overflow_as_inf=False):
    """km.inputs of matrix_case(): item 0 the full length, item 1 one frame, item 2 quantised to 0.5 (ties across the beam boundary),
    item 3 with -3e38 in frames 2 and 3 (adding the second overflows every score to -inf: danger mode from finite inputs) and -inf at
    frame 26 -> (lp [4, 40, 29], seq_lens [4])."""
    return km.inputs(matrix_case(), overflow_as_inf=overflow_as_inf)


def build_exact_host():
    """tests/native/exact_shape_host.cpp, compiled the way oracle_util.build_core_host compiles core_host.cpp (checked assumptions)."""
    src = os.path.join(ou.ROOT, "tests", "native", "exact_shape_host.cpp")
    deps = [src, os.path.join(ou.ROOT, "tests", "native", "core_host.cpp")] + [os.path.join(ou.ROOT, "ctcdecode_amd", "csrc", f) for f in (
        "beam_core.h", "launch_plan.h", "stl_emul.h", "exact_math.h", "exact_math_f64.h", "exact_math_f64_tables.h", "lm_tables.h", "lm_build.h",
        "lm_callback.h", "compact_results.h")]
    if os.path.exists(EXACT_HOST_SO) and all(os.path.getmtime(EXACT_HOST_SO) >= os.path.getmtime(p) for p in deps):
        return EXACT_HOST_SO
    os.makedirs(os.path.dirname(EXACT_HOST_SO), exist_ok=True)
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-mfma", "-DCTC_ASSUME_CHECKED"]
                   + os.environ.get("CTC_HOST_EXTRA_FLAGS", "").split() + [src, "-o", EXACT_HOST_SO, "-lpthread"], check=True)
    return EXACT_HOST_SO


EVENTS = list(sp.COUNTERS)  # the counters of the select-path certificate (select_path_util.COUNTERS), by their place in enum Event


def decode_host(lp, seq_lens, stage):
    """The host twin's decode with the run-time policy (stage 0), the exact policy (1), or the exact policy that folds the live beam
    size (2) -> (result dict as oracle_util.decode gives it, {event: count during this decode})."""
    lp = np.ascontiguousarray(lp, dtype=np.float32)
    B, T, V = lp.shape
    assert V == LABELS
    if seq_lens is not None:
        seq_lens = np.ascontiguousarray(seq_lens, dtype=np.int32)
    tok = np.zeros((B, BEAM, T), np.int32)
    ts = np.zeros((B, BEAM, T), np.int32)
    sc = np.zeros((B, BEAM), np.float32)
    ln = np.zeros((B, BEAM), np.int32)
    nres = np.zeros((B,), np.int32)
    lib = ctypes.CDLL(build_exact_host())
    ids = (ctypes.c_int32 * 8)()
    lib.ctcexact_event_ids(ids)
    ev = (ctypes.c_longlong * int(ids[7]))()
    p = ou._ptr
    rc = lib.ctcexact_decode_f32(p(lp, ou._f32p), p(seq_lens, ou._i32p), B, T, int(stage), p(tok, ou._i32p), p(ts, ou._i32p), p(sc, ou._f32p),
                                 p(ln, ou._i32p), p(nres, ou._i32p), ev)
    if rc != 1:
        raise RuntimeError("exact-shape host twin returned %d" % rc)
    idx = dict((name, sm.event_index(name)) for name in EVENTS)
    assert all(0 <= i < len(ev) for i in idx.values())
    return dict(tokens=tok, timesteps=ts, scores=sc, lens=ln, nres=nres), dict((name, int(ev[i])) for name, i in idx.items())


_ORACLE = {}


def oracle(name, lp, seq_lens):
    """The CPU oracle's decode of a case, computed once per process."""
    if name not in _ORACLE:
        which = "reference" if ou.have_reference() else "restated"
        _ORACLE[name] = ou.decode(lp, seq_lens, beam=BEAM, cutoff_prob=1.0, cutoff_top_n=40, blank_id=BLANK, which=which)
    return _ORACLE[name]
