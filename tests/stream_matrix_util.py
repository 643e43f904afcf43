"""The kernel matrix, streamed: one entry per instantiation of ctc_beam_decode_kernel that a stream can launch, with the chunking
that puts a parked state (beam_core.h save_state / load_state) in front of it.  Shared by the CPU checks
(test_stream_matrix_plan.py) and the GPU tests (test_gpu_stream_matrix.py).  No torch here: the CPU suite imports this module.

Which kernels a stream reaches.  ctcd_stream_decode and ctcd_stream_decode_to_host (ctcdecode_amd.hip) both go through
decode_common -> plan_launch with the decoder's own switches, and neither passes frames_ready.  So a stream reaches every key of
the product branch of CTC_KERNEL_LIST with PROF 0 or PROF 3, in every BIG / LAYOUT / PRUNED / NT / LM / OCC2 combination of the list
(46 keys), and no other:
  * PROF 1 and 2 need the profile switch (ctcd_debug_set_profile), which no serving path sets;
  * PROF 4 and 5 are planned only for a call that passes frames_ready, and only the host-tensor one-shot entry does.

Every entry reuses its matrix case (kernel_matrix_util.CASES): shape, decoder arguments, switches and km.inputs(c, labels) -- item 0
at full length, item 1 with one frame, item 2 with coarse rows that tie, and without a scorer the degenerate item (-3e38 at frames 2
and 3, -inf at frame 2T/3).  The switches OnlineCTCBeamDecoder does not expose go through _native.lib on dec._handle (configure()).
Each OCC2 key has one more entry that reaches it the way serving does: more streams than the device has CUs, cu_sharing left
automatic (`production`: B is the CU count + 8, known only where the test runs -- sized_case()).

Chunk bounds [0, 1, 3, 3, T // 2, 2 * T // 3 + 1, T]: a one-frame chunk, a boundary between the two overflow frames (SH_DANGER and the
overflowed scores cross it), an empty chunk, a boundary right behind the -inf frame.  Item b's chunk lengths are
clip(len_b - lo, 0, hi - lo); every stream ends at the last chunk.  For every scorer-free entry at least two boundaries directly
follow a frame in which item 2 replayed std::nth_element (the `fin` order of that replay is what the parked state carries):
test_stream_matrix_plan.py checks this on the host twin.  Where an entry's seed does not give it, MID_BOUND moves the entry's T // 2
bound to the nearest frame that does; where neither frame 0 nor frame 2 of item 2 replays, so that moving one bound can only ever
give one such boundary, EXTRA_BOUND adds one more boundary at the next nearest such frame (the entry keeps every bound of the
list above).

The commit walks (OnlineCTCBeamDecoder.commit behind every scorer-free entry) need inputs on which a commit hands labels out:
commit_inputs() appends an item whose confidence fades to km.inputs(c), commit_bounds() adds the boundaries of COMMIT_BOUND, the
hand-over walks commit at hand_over_commit_mid(), and DEEP_WALKS are the walks whose paths grow past an express level.  What these
inputs must give is proved on the oracle in test_stream_matrix_plan.py."""
import numpy as np

import kernel_matrix_util as km

# the production-route entries: T, K of the issue's shape; more streams than CUs
PRODUCTION_T, PRODUCTION_K, PRODUCTION_EXTRA = 24, 16, 8

# entry_id -> the bound that replaces T // 2, and the bound that is added (see the module docstring; found with replay_frames(), held
# by test_stream_matrix_plan.py::test_two_boundaries_follow_a_replay)
MID_BOUND = {"k0011_1024_lm0_occ1": 23, "k0011_0_lm0_occ0": 22, "k3010_1024_lm0_occ0": 21, "k0000_0_lm0_occ0": 19, "k0001_0_lm0_occ0": 18,
             "k0021_1024_lm0_occ0": 23, "k0130_1024_lm0_occ0": 13, "k0101_1024_lm0_occ0": 13, "k0010_1024_lm0_occ1_serving": 6,
             "k0011_1024_lm0_occ1_serving": 8}
EXTRA_BOUND = {"k0010_1024_lm0_occ0": 22, "k0010_1024_lm0_occ1": 21, "k3010_1024_lm0_occ0": 25, "k0001_0_lm0_occ0": 17,
               "k0130_1024_lm0_occ0": 17, "k0100_1024_lm0_occ0": 14, "k0101_0_lm0_occ0": 14}

# The scorer entries over select_path_util.select_path_inputs (test_gpu_select_paths.py), bounds of select_path_util.select_path_bounds.
# Item 0 is in danger mode from its overflow frames on and replays in every frame behind them, so the bounds T // 2 and 2T/3 + 1 of
# every entry directly follow a replay of item 0.  Item 2's replays are the ones a tie forces (the boundary splits a group of equivalent
# prefixes): where it has one mid-utterance, the entry gets one more bound directly behind it.  entry_id -> that bound (found with
# select_path_util.replay_frames_lm(); held by test_stream_matrix_plan.py::test_select_path_bounds_follow_replays).  The unpruned fixed-layout entries
# have none: every tie of their item 2 is settled by character.
SELECT_PATH_EXTRA = {"k0011_1024_lm2_occ0": 12, "k0011_1024_lm2_occ1": 10, "k0011_1024_lm1_occ0": 10, "k0011_1024_lm1_occ1": 7,
                     "k0100_0_lm1_occ0": 5, "k0200_0_lm1_occ0": 6, "k0201_0_lm1_occ0": 7, "k0011_1024_lm3_occ0": 10, "k0100_0_lm3_occ0": 5,
                     "k0101_0_lm3_occ0": 7}
# ... and the entries whose T // 2 bound already follows a replay of item 2
ITEM2_AT_MID = ["k0001_0_lm1_occ0", "k0301_0_lm3_occ0"]


def stream_reachable(key):
    """A key of CTC_KERNEL_LIST that ctcd_stream_decode / ctcd_stream_decode_to_host can plan."""
    return key[0] in (0, 3)


def _production_case(c, seed):
    """The matrix case of an OCC2 key, reshaped to the serving route: K = 16, T = 24, cu_sharing automatic, B left to sized_case()."""
    p = dict(c, K=PRODUCTION_K, T=PRODUCTION_T, B=None, cu_sharing=-1, seed=seed)
    if not c["lm"]:
        p["V"] = 29
    p["top_n"] = min(c["top_n"], 10) if c["top_n"] < c["V"] else p["V"]
    return p


def _entries():
    out = []
    for c in km.CASES:
        if stream_reachable(c["kernel"]):
            out.append(dict(case=c, kernel=c["kernel"], production=False))
    n = 0
    for c in km.CASES:
        if stream_reachable(c["kernel"]) and c["kernel"][6]:
            out.append(dict(case=_production_case(c, 9900 + 13 * n), kernel=c["kernel"], production=True))
            n += 1
    return out


STREAM_CASES = _entries()


def entry_id(e):
    return km.case_id(e["case"]) + ("_serving" if e["production"] else "")


def sized_case(e, cu_count):
    """The entry's case with its batch size: the matrix's own, or CU count + 8 streams for a production-route entry."""
    c = e["case"]
    return dict(c, B=cu_count + PRODUCTION_EXTRA) if e["production"] else c


def bounds(e):
    """Chunk bounds of an entry."""
    T, eid = e["case"]["T"], entry_id(e)
    mid = MID_BOUND.get(eid, T // 2)
    inner = sorted([mid] + ([EXTRA_BOUND[eid]] if eid in EXTRA_BOUND else []))
    b = [0, 1, 3, 3] + inner + [(2 * T) // 3 + 1, T]
    assert all(x <= y for x, y in zip(b, b[1:])) and 3 < inner[0] and inner[-1] < (2 * T) // 3 + 1 < T, b
    return b


def plain_bounds(T):
    """The bounds of a stream that is no entry of the table (the hand-over tests)."""
    return [0, 1, 3, 3, T // 2, (2 * T) // 3 + 1, T]


def chunk_lens(seq_lens, lo, hi):
    """Per-item lengths of the chunk [lo, hi) of a ragged batch."""
    return np.clip(np.asarray(seq_lens, np.int64) - lo, 0, hi - lo).astype(np.int32)


def configure(dec, c, lib, check):
    """Set the switches of case c on an OnlineCTCBeamDecoder (lib = ctcdecode_amd._native.lib, check = _native.check).  A
    production-route case (cu_sharing -1) leaves the two-workgroups-per-CU choice automatic."""
    if c["threads"]:
        dec.set_threads(c["threads"])
    check(lib.ctcd_set_subtree_search(dec._handle, int(c["subtree"])))
    check(lib.ctcd_set_cu_sharing(dec._handle, int(c["cu_sharing"])))
    check(lib.ctcd_debug_set_fixed_layout(dec._handle, 1 if c["fixed"] else 0))


def oracle_args(c):
    return dict(beam=c["K"], cutoff_prob=c["cutoff_prob"], cutoff_top_n=c["top_n"], blank_id=c["blank"])


def event_index(name):
    """Position of an event counter in ctccore_event_counts' output (beam_core.h enum Event)."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "ctcdecode_amd", "csrc", "beam_core.h")).read()
    m = re.search(r"enum Event \{(.*?)\}", text, flags=re.S)
    assert m, "enum Event was not found in beam_core.h"
    return [w.strip() for w in m.group(1).split(",")].index(name)


def replay_frames(c):
    """The frames (0-based) in which item 2 of a scorer-free case replays std::nth_element: EV_EXACT of the host twin, one thread,
    item 2 decoded to f + 1 frames against f frames."""
    import ctypes

    import oracle_util as ou

    assert not c["lm"]
    c = dict(c, B=c["B"] or 4)  # (item 2's rows do not depend on the batch size)
    lib = ctypes.CDLL(ou.build_core_host())
    ev = event_index("EV_EXACT")
    cnt = (ctypes.c_longlong * 64)()
    lp, sl = km.inputs(c)
    rows = np.ascontiguousarray(lp[2:3])
    total = []
    for f in range(int(sl[2]) + 1):
        lib.ctccore_event_counts(cnt, 1)
        ou.decode_core_host(rows, np.array([f], np.int32), threads=1, **oracle_args(c))
        n = lib.ctccore_event_counts(cnt, 0)
        assert ev < n
        total.append(int(cnt[ev]))
    return [f for f in range(int(sl[2])) if total[f + 1] - total[f] == 1]


def tie_boundaries(e):
    """The bounds of the entry that directly follow a frame in which item 2 replayed std::nth_element (bounds inside item 2's
    length: its state is parked there with frames still to come or just consumed)."""
    c = e["case"]
    len2 = max(2, (2 * c["T"]) // 3)  # (km.inputs)
    rep = set(replay_frames(c))
    return sorted(b for b in set(bounds(e)) if 0 < b <= len2 and (b - 1) in rep)


# ---- hand-overs: one stream, kernel X for the chunks up to the T // 2 bound, kernel Y after it -----------------------------------
def _matrix_case(kernel):
    return next(c for c in km.CASES if c["kernel"] == tuple(kernel))


def _serving_entry(kernel):
    return next(e for e in STREAM_CASES if e["production"] and e["kernel"] == tuple(kernel))


def _hand_over(name, cause, case, x, y, kernel_x, kernel_y):
    """x, y: what differs between the two sides -- fields of the case that configure() sets (threads, subtree, fixed), or few=True:
    only three of the CU count + 8 streams are fed (the batch no longer outnumbers the CUs)."""
    return dict(name=name, cause=cause, case=case, x=x, y=y, kernel_x=tuple(kernel_x), kernel_y=tuple(kernel_y))


HAND_OVERS = [
    # what serving does by itself: the batch size crosses the CU count (OCC2 <-> plain), the subtree search is switched
    _hand_over("occ2_plain", "serving", _serving_entry((0, 0, 1, 0, 1024, 0, 1))["case"], dict(few=False), dict(few=True),
               (0, 0, 1, 0, 1024, 0, 1), (0, 0, 1, 0, 1024, 0, 0)),
    _hand_over("occ2_plain_pruned", "serving", _serving_entry((0, 0, 1, 1, 1024, 0, 1))["case"], dict(few=False), dict(few=True),
               (0, 0, 1, 1, 1024, 0, 1), (0, 0, 1, 1, 1024, 0, 0)),
    _hand_over("occ2_plain_word_model", "serving", _serving_entry((0, 0, 1, 0, 1024, 2, 1))["case"], dict(few=False), dict(few=True),
               (0, 0, 1, 0, 1024, 2, 1), (0, 0, 1, 0, 1024, 2, 0)),
    _hand_over("subtree_forced", "serving", _matrix_case((3, 0, 1, 0, 1024, 0, 0)), dict(subtree=1), dict(subtree=0),
               (3, 0, 1, 0, 1024, 0, 0), (0, 0, 1, 0, 1024, 0, 0)),
    _hand_over("subtree_forced_pruned", "serving", _matrix_case((3, 0, 1, 1, 1024, 0, 0)), dict(subtree=1), dict(subtree=0),
               (3, 0, 1, 1, 1024, 0, 0), (0, 0, 1, 1, 1024, 0, 0)),
    # a switch changed between two chunks: the workgroup size, the fixed layout
    _hand_over("threads_fixed_layout", "hook", _matrix_case((0, 0, 1, 0, 1024, 0, 0)), dict(threads=1024), dict(threads=512),
               (0, 0, 1, 0, 1024, 0, 0), (0, 0, 1, 0, 0, 0, 0)),
    _hand_over("threads_pruned_default", "hook", _matrix_case((0, 0, 2, 1, 1024, 0, 0)), dict(threads=1024), dict(threads=512),
               (0, 0, 2, 1, 1024, 0, 0), (0, 0, 0, 1, 0, 0, 0)),
    _hand_over("threads_wide_beam", "hook", _matrix_case((0, 1, 3, 0, 1024, 0, 0)), dict(threads=1024), dict(threads=512),
               (0, 1, 3, 0, 1024, 0, 0), (0, 1, 0, 0, 0, 0, 0)),
    _hand_over("threads_word_model", "hook", _matrix_case((0, 0, 0, 0, 0, 1, 0)), dict(threads=1024), dict(threads=512),
               (0, 0, 1, 0, 1024, 2, 0), (0, 0, 0, 0, 0, 1, 0)),
    _hand_over("fixed_layout_switch", "hook", _matrix_case((0, 0, 1, 0, 0, 0, 0)), dict(fixed=True), dict(fixed=False),
               (0, 0, 1, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0)),
]


def hand_over_id(h):
    return h["name"]


# The automatic PROF 0 <-> 3 switch: the shape statistic of a checked chunk chooses the next chunk's build (ctcd_check_status:
# chains, >= 8 entries with descendants per item -> the subtree search; <= 4 -> the plain build).  Blank-dominated rows first,
# random rows behind them.
AUTO_SUBTREE = dict(V=29, K=100, B=4, threads=1024, blank_bias=8.0, bounds=[0, 12, 24, 36, 48, 60], blank_frames=24, seed=9990)

# The hand-overs the host twin can express (oracle_util.decode_core_host_chunked_mixed: instantiation ids 0 run-time layout, 1 fixed
# layout, 2 its far-replay build = what OCC2 runs, 3 the pruned default's class), by the matrix entry whose inputs and bounds they use.
HOST_HAND_OVERS = [
    ((0, 0, 1, 0, 1024, 0, 1), 2, 1), ((0, 0, 1, 1, 1024, 0, 1), 2, 1),  # OCC2 <-> plain
    ((0, 0, 1, 0, 1024, 0, 0), 2, 1), ((0, 0, 1, 1, 1024, 0, 0), 2, 1),
    ((0, 0, 1, 0, 0, 0, 0), 1, 0), ((0, 0, 1, 1, 0, 0, 0), 1, 0),        # fixed <-> run-time layout
    ((0, 0, 1, 0, 1024, 0, 0), 2, 0),
    ((0, 0, 2, 1, 1024, 0, 0), 3, 0),                                    # the pruned default's class <-> run-time layout
]


def mid_index(e):
    """Index of the first chunk behind the T // 2 bound (the moved one, where MID_BOUND moves it) in bounds(e)."""
    mid = MID_BOUND.get(entry_id(e), e["case"]["T"] // 2)
    return bounds(e).index(mid)


# ---- commits: inputs whose common prefix grows with every chunk -------------------------------------------------------------------
# On km.inputs(c) at bounds(e) a commit hands out next to nothing (random rows: the stable prefix stays below 2 at most boundaries), so
# the commit walks append one item whose confidence fades: the cheapest alternatives always lie in its newest frames, and what is
# common to all beam entries grows chunk by chunk.
FADE_FROM, FADE_TO, FADE_NOISE = 40.0, 0.5, 0.3


def fading_item(T, V, blank, seed, fade_to=FADE_TO):
    """[T, V] float32 log-probabilities: even frames peak on a random non-blank label, odd frames on the blank; the margin of the peak
    over the other labels falls linearly from FADE_FROM at frame 0 to fade_to at frame T - 1 (never below 0: a steeper fade ends in
    rows of noise alone); Gaussian noise of FADE_NOISE, then a float32 log-softmax."""
    rng = np.random.default_rng(seed)
    x = (np.float32(FADE_NOISE) * rng.standard_normal((T, V))).astype(np.float32)
    others = [v for v in range(V) if v != blank]
    for t in range(T):
        margin = FADE_FROM + (fade_to - FADE_FROM) * t / max(1, T - 1)
        peak = blank if t % 2 else others[int(rng.integers(0, len(others)))]
        x[t, peak] += np.float32(max(0.0, margin))
    m = x.max(axis=-1, keepdims=True)
    lse = m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True, dtype=np.float32), dtype=np.float32)
    return (x - lse).astype(np.float32)


def commit_inputs(c, labels=None):
    """km.inputs(c) with the fading item appended at full length: (lp [B + 1, T, V], seq_lens [B + 1]).  The tie item, the degenerate
    item and the one-frame item stay in the batch and are committed along with it."""
    lp, sl = km.inputs(c, labels)
    fade = fading_item(c["T"], c["V"], c["blank"], c["seed"] + 7)
    return np.ascontiguousarray(np.concatenate([lp, fade[None]]), dtype=np.float32), np.concatenate([sl, [c["T"]]]).astype(np.int32)


def fading_index(c):
    """Where commit_inputs(c) puts the fading item."""
    return c["B"]


# entry_id -> boundaries added to bounds(e) for the commit walk, so that at least two commits (one after every chunk but the last) hand
# the fading item a label and row 0 still keeps two at the end (held by test_stream_matrix_plan.py::test_commit_walk_commits_twice)
COMMIT_BOUND = {"k0101_1024_lm0_occ0": (19,), "k0101_0_lm0_occ0": (19,), "k0200_0_lm0_occ0": (16,), "k0201_0_lm0_occ0": (16,)}


def commit_bounds(e):
    """Chunk bounds of an entry's commit walk: bounds(e) and the entry's COMMIT_BOUND."""
    b = sorted(bounds(e) + list(COMMIT_BOUND.get(entry_id(e), ())))
    assert len(set(b)) == len(b) - 1 and b[-1] == e["case"]["T"], b  # (the empty chunk alone repeats a bound)
    return b


def host_twin_builds(c):
    """The shapes the streaming host twin decodes (tests/native/peek_host.cpp: the fixed and the run-time layout, 16-bit slot indices --
    at most 65535 candidate slots; the build for more exists on the device alone)."""
    return not c["lm"] and c["K"] * (min(c["V"], c["top_n"]) + 2) <= 65535


def commit_events(lp, b, F_list, which="restated", **kw):
    """The oracle's side of a commit walk of item b: a commit after F frames, for every F of F_list in turn, hands out
    max(0, stable - 1 - committed) labels.  -> [(F, labels handed out, committed before)]."""
    import peek_util as pu

    out, C = [], 0
    for F in F_list:
        m = 0
        if F > 0:
            m = max(0, pu.common_prefix_len(pu.oracle_prefix(lp[b:b + 1], F, which, **kw), 0) - 1 - C)
        out.append((F, m, C))
        C += m
    return out


# A committed state across a hand-over: the streams that cross are committed at the T // 2 bound, directly before the switch.
# hand-over name -> the bound that replaces T // 2 where the oracle commits nothing to the fading item there (none needs it: held by
# test_stream_matrix_plan.py::test_commit_in_front_of_a_hand_over_commits)
HAND_OVER_COMMIT_MID = {}


def hand_over_commit_mid(h):
    return HAND_OVER_COMMIT_MID.get(h["name"], h["case"]["T"] // 2)


def hand_over_commit_bounds(h):
    T = h["case"]["T"]
    b = plain_bounds(T)
    b[b.index(T // 2)] = hand_over_commit_mid(h)
    assert sorted(b) == b and 3 < hand_over_commit_mid(h) < (2 * T) // 3 + 1, b
    return b


def hand_over_few(c):
    """The streams of a CU count + 8 batch of commit_inputs that cross a `few` hand-over: item 0, the tie item, the degenerate item
    and the fading item."""
    return sorted({0, 2, km.degenerate_item(c), fading_index(c)})


# Depth past an express level (beam_core.h kExpress = 32): at T <= 40 no path is deeper than about 20 labels, so the walks above never
# lay a path out across an express level of the new coordinates.  One walk per key the long commit tests do not reach: two fading
# items of DEEP_T frames whose fade is steeper (the margin reaches 0 at two fifths of the item, rows of noise alone follow: the
# common prefix stalls there while row 0 grows on), a commit every DEEP_CHUNK frames.  seeds: offsets to the matrix case's seed, chosen
# so that an item ends with a committed length that is no multiple of 32 and at least 33 labels of row 0 uncommitted; `deep_commit`:
# one of its commits itself hands out labels at such a place (held by test_stream_matrix_plan.py::test_deep_walks_end_between_express_levels)
DEEP_T, DEEP_CHUNK, DEEP_FADE_TO = 128, 16, -60.0
DEEP_WALKS = [
    dict(kernel=(0, 0, 1, 0, 1024, 0, 1), seeds=(15, 16), deep_commit=False),
    dict(kernel=(3, 0, 1, 0, 1024, 0, 0), seeds=(14, 15), deep_commit=False),
    dict(kernel=(0, 0, 2, 1, 1024, 0, 0), seeds=(12, 13), deep_commit=True),
    dict(kernel=(0, 2, 0, 0, 0, 0, 0), seeds=(11, 15), deep_commit=False),
]


def deep_walk_id(d):
    return "k%d%d%d%d_%d_lm%d_occ%d" % d["kernel"]


def deep_inputs(d):
    """-> (the key's matrix case, lp [2, DEEP_T, V], the chunk bounds)."""
    c = _matrix_case(d["kernel"])
    lp = np.stack([fading_item(DEEP_T, c["V"], c["blank"], c["seed"] + s, fade_to=DEEP_FADE_TO) for s in d["seeds"]])
    return c, np.ascontiguousarray(lp), list(range(0, DEEP_T + 1, DEEP_CHUNK))
