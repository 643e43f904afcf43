"""Inputs that take the rank table of the pruned default's compile-time layout (ctcdecode_amd/csrc/beam_core.h kRankEpoch) across
frame 1023 mod 1024.  Its entries are tagged (t mod 1024) << 6 | rank; a never-written or wiped entry (0xFFFF) carries frame 1023's tag
with rank 63, and a tag written 1024 frames ago matches again unless the table is wiped.  Shared by the host-build tests
(test_core_host.py) and the GPU tests (test_gpu_rank_epoch.py)."""
import numpy as np

import oracle_util as ou

# a shape of the class (beam <= 112, cutoff_top_n <= 40, more than 32 labels); on the GPU it needs set_threads(1024), the automatic
# choice gives it 512 threads and the run-time layout (K * (top_n + 2) <= 1300)
V, TOP_N, K = 300, 20, 30
KINDS = ["blank_pruned", "blank_pruned_at_wraps", "stale_tag"]




def prune_blank(lp, top_n, frames=slice(None), blank=0):
    """Push the blank out of the candidates of the given frames: 1e-3 below the (top_n + 5)-th largest value of its row."""
    rows = lp[:, frames]
    rows[..., blank] = np.sort(rows, axis=-1)[..., -(top_n + 5)] - np.float32(1e-3)
    lp[:, frames] = rows
    return lp


def strong_wrap_frames(lp, top_n, seed):
    """At every frame t = 1023 mod 1024, top_n non-blank labels close together at the top of the row: a miscounted candidate list
    (the blank read as rank 63) drops the last of them, whose children would have entered the beam."""
    rng = np.random.default_rng(seed)
    for t in range(1023, lp.shape[1], 1024):
        lp[:, t, 1 + rng.permutation(lp.shape[2] - 1)[:top_n]] = (-3.0 - 0.01 * np.arange(top_n)).astype(np.float32)
    return lp


def wrap_frames(T, w=3):
    return np.array([t for t in range(T) if t % 1024 >= 1024 - w or (t >= 1024 and t % 1024 < w)], np.int64)


def epoch_case(kind, T, top_n=TOP_N, V=V):
    if kind == "blank_pruned":  # the blank is a candidate in no frame
        return prune_blank(strong_wrap_frames(ou.synth_logprobs(1, T, V, 600 + T), top_n, T), top_n)
    if kind == "blank_pruned_at_wraps":  # ... only in the frames around every wrap; a candidate (blank-heavy rows) elsewhere
        return prune_blank(strong_wrap_frames(ou.synth_logprobs(1, T, V, 700 + T, blank_bias=2.0), top_n, T), top_n, wrap_frames(T))
    assert kind == "stale_tag"
    # labels that are candidates in one frame each (then the likely last label of the beam's prefixes: blank-dominated rows) and never
    # again: 1024 frames later their entry still holds that frame's tag -- unless the table was wiped in between
    lp = ou.synth_logprobs(1, T, V, 800 + T, blank_bias=8.0)
    for i, f in enumerate(f for f in (0, 3, 17, 500, 1000, 1030, 1500, 2040) if f < T):
        c = 1 + i
        lp[0, :, c] = np.sort(lp[0], axis=-1)[:, -(top_n + 5)] - np.float32(1e-3)
        lp[0, f, c] = -0.05
    return lp
