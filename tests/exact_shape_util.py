"""Inputs and the host twin of the exact-shape kernel (beam 100 over 29 labels, blank 0: decode_kernel.h CTC_EXACT_SHAPES).

Shared by test_exact_shape_host.py (the exact policy of beam_core.h on the CPU, against the run-time policy and the oracle) and
test_gpu_exact_shape.py (the twin kernel against the planned kernel and the oracle, over the same inputs).  No torch here: the CPU
suite imports this module.  Every shape is the twin's own at T <= 64, B <= 8."""
import ctypes
import os
import subprocess

import numpy as np

import oracle_util as ou

BEAM, LABELS, BLANK = 100, 29, 0
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


EVENTS = ["EV_FRAMES", "EV_EXACT", "EV_SPEC_OK", "EV_SPEC_UNDER", "EV_SPEC_OVER", "EV_SPEC_OTHER", "EV_TIE_FRAMES"]


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
    return dict(tokens=tok, timesteps=ts, scores=sc, lens=ln, nres=nres), dict((name, int(ev[ids[i]])) for i, name in enumerate(EVENTS))


_ORACLE = {}


def oracle(name, lp, seq_lens):
    """The CPU oracle's decode of a case, computed once per process."""
    if name not in _ORACLE:
        which = "reference" if ou.have_reference() else "restated"
        _ORACLE[name] = ou.decode(lp, seq_lens, beam=BEAM, cutoff_prob=1.0, cutoff_top_n=40, blank_id=BLANK, which=which)
    return _ORACLE[name]
