"""Inputs that drive a scorer kernel's select through its tie and replay paths, and the host twin's certificate that they do.

Every frame of the decode ends in a select of the K best candidates (beam_core.h steps C and D): the fast path over one histogram
bucket, the slow path's further rounds (a bucket with more than 128 keys, a single-valued bucket, a K-th key below the window), a
boundary tie settled by resolve_by_character, an exact replay of std::nth_element, danger mode.  On the device each is a
wave-parallel routine of its own that the host twin (tests/native/core_host.cpp HostX) replaces with a sequential stand-in, so only a
GPU run that reaches a path proves that path's device code.  km.inputs(c, labels) reaches them for scorer-free cases (the degenerate
item, the coarse item); for scorer cases it leaves the degenerate frames out, and the scorer's contributions break most of the
coarse item's ties.  select_path_inputs() puts them back; counted() reads from the host twin, instantiated as the case's own
class, how often a decode took each path (beam_core.h enum Event).  No torch here: the CPU suite imports this module.

Shared by test_select_paths.py (the certificate: floors on the counters, the twin against the oracles), test_gpu_select_paths.py (the
same inputs through every scorer kernel, one-shot and behind a parked state), test_stream_matrix_plan.py (the chunk bounds of the
streamed form) and tools/select_path_coverage.py (the measured table, profiles/select_path_coverage.json)."""
import ctypes

import numpy as np

import kernel_matrix_util as km
import oracle_util as ou
import stream_matrix_util as sm

# The counters of the certificate.  Two counters of enum Event are left out on purpose: EV_WIDE_LIST and EV_HOT_LIST belong to
# experiment switches that are off in the product (CTC_EXP_WIDE_LIST, CTC_EXP_HOT_PRELIST): no product kernel can count them.
COUNTERS = ["EV_FRAMES", "EV_CANDIDATES", "EV_EXACT", "EV_REVIVED", "EV_SPEC_OK", "EV_SPEC_UNDER", "EV_SPEC_OVER", "EV_SPEC_OTHER", "EV_SLOW_BELOW", "EV_SLOW_CROWDED",
            "EV_SLOW_SINGLE", "EV_SLOW_ROUNDS", "EV_TIE_FRAMES", "EV_TIE_KEYS", "EV_TIE_BIG"]
LEFT_OUT = ["EV_WIDE_LIST", "EV_HOT_LIST"]

FLAT_0, FLAT_2 = np.float32(-3.0), np.float32(-2.5)


def scorer_cases():
    """The PROF 0, non-streamed scorer cases of the kernel matrix: the 26 scorer instantiations a plain decode launches."""
    return [c for c in km.CASES if c["lm"] and c["kernel"][0] == 0 and not c["streamed"] and not c["profile"]]


def scorer_free_cases():
    """The PROF 0 / PROF 3, non-streamed scorer-free cases of the kernel matrix."""
    return [c for c in km.CASES if not c["lm"] and c["kernel"][0] in (0, 3) and not c["streamed"] and not c["profile"]]


def flat_frames(c):
    """(first, last + 1) of item 0's flat frames."""
    return c["T"] // 3, c["T"] // 3 + 3


def select_path_inputs(c, labels):
    """km.inputs(c, labels) of a scorer case with the frames that km.inputs gives scorer-free cases alone, and flat frames:
      * item 0 (full length): frames T//3 .. T//3+2 a flat -3.0 (every label ties with every other: buckets of one value, ties
        of more than 128 keys), frames 2 and 3 at -3e38 (adding the second overflows every score to -inf: danger mode from there
        on, with the scorer's per-entry state in it) and frame 2T/3 at -inf;
      * item 2 (the coarse item, 2T/3 frames): frames 5-7 a flat -2.5.
    Where T is small (T = 10: T//3 = 3) the flat frames would cover the second overflow frame; the overflow frames are written last,
    so that both stay and a chunk boundary between them parks overflowed scores."""
    assert c["lm"]
    lp, sl = km.inputs(c, labels)
    T = c["T"]
    f0, f1 = flat_frames(c)
    assert 3 <= f0 and f1 <= (2 * T) // 3 and sl[0] == T and 6 <= sl[2]  # (T = 10: item 2 ends with its first flat frame)
    lp[0, f0:f1, :] = FLAT_0
    lp[0, 2:4, :] = np.float32(-3.0e38)
    lp[0, (2 * T) // 3, :] = -np.inf
    lp[2, 5:8, :] = FLAT_2
    return np.ascontiguousarray(lp, dtype=np.float32), sl


def host_env(c):
    """The switches of tests/native/core_host.cpp that make decode_impl instantiate decode_utterance as the device does for the
    case's kernel (decode_kernel.h: <!PRUNED, LAYOUT, LM != 0, BIG != 0, BIG != 0 || OCC2, BIG == 3, LM == 2, LM == 3>), as far as the
    twin has a switch: name -> value, every other switch of the list must be unset.
      * CTC_HOST_BIG: the case's BIG;
      * scorer cases: CTC_HOST_GENERAL_LM for a kernel without the word-model branches (LM 1 or 3) over the word model,
        CTC_HOST_LM_RUNTIME_LAYOUT for LAYOUT 0 at a shape of the fixed-layout class;
      * scorer-free cases: CTC_HOST_NO_CLASS2 for a pruned LAYOUT 0 kernel at a shape of the pruned default's class; the
        two-workgroups-per-CU builds (the fixed layout with the replay scratch in HBM) have no switch: host_decode() takes them
        through ctccore_decode_chunked_mixed_f32's instantiation 2, fed in one chunk.
    What the twin cannot express: OCC2 of a scorer kernel (the replay scratch alone in HBM), CB of a pruned or fixed-layout kernel
    (decode_core_host_lm_cb is unpruned, run-time layout) -- the select does not depend on either."""
    _, big, layout, _, _, lm, occ2 = c["kernel"]
    env = {}
    if big:
        env["CTC_HOST_BIG"] = str(big)
    if lm:
        if lm in (1, 3) and c["lm"] == "word":
            env["CTC_HOST_GENERAL_LM"] = "1"
        if layout == 0 and not big:
            env["CTC_HOST_LM_RUNTIME_LAYOUT"] = "1"
    else:
        if layout == 0 and not big and c["top_n"] < c["V"]:
            env["CTC_HOST_NO_CLASS2"] = "1"
    return env


HOST_SWITCHES = ["CTC_HOST_BIG", "CTC_HOST_GENERAL_LM", "CTC_HOST_LM_RUNTIME_LAYOUT", "CTC_HOST_FARREP", "CTC_HOST_NO_CLASS2", "CTC_HOST_NO_SPEC"]


def set_host_env(c, setenv, delenv):
    """Apply host_env(c) with a pair of functions (monkeypatch.setenv / monkeypatch.delenv(name, raising=False), or os.environ's)."""
    env = host_env(c)
    for name in HOST_SWITCHES:
        if name in env:
            setenv(name, env[name])
        else:
            delenv(name)


def has_spec_select(c):
    """beam_core.h kSpec on the device: a compile-time layout in LDS (the fixed layout, the pruned default's) without a scorer."""
    _, big, layout, _, _, lm, _ = c["kernel"]
    return layout in (1, 2) and not big and not lm


_LIB = []


def _lib():
    if not _LIB:
        _LIB.append(ctypes.CDLL(ou.build_core_host()))
    return _LIB[0]


def counted(fn):
    """fn() on the host twin -> (its result, {counter: events during the call}).  The twin's counters are per process and add up
    racily over host threads: fn must decode on one thread."""
    cnt = (ctypes.c_longlong * 64)()
    _lib().ctccore_event_counts(cnt, 1)
    res = fn()
    n = _lib().ctccore_event_counts(cnt, 0)
    idx = dict((name, sm.event_index(name)) for name in COUNTERS)
    assert all(i < n for i in idx.values())
    return res, dict((name, int(cnt[i])) for name, i in idx.items())


def host_decode(c, lp, sl, lm, callback=False):
    """The host twin's decode of a case's inputs on one thread (the caller has applied host_env(c)): lm = km.lm_spec of a scorer case
    or None; callback: through the scorer hook's twin (unpruned cases)."""
    args = sm.oracle_args(c)
    if lm is None:
        if c["kernel"][6]:  # (OCC2: decode_utterance<IDENT, 1, false, false, true>)
            return ou.decode_core_host_chunked_mixed(lp, [0, c["T"]], [2], seq_lens=sl, **args)
        return ou.decode_core_host(lp, sl, threads=1, **args)
    if callback:
        assert c["top_n"] >= c["V"] and c["cutoff_prob"] >= 1.0
        return ou.decode_core_host_lm_cb(lp, lm[2], lm[3], lm[0], lm[1], sl, beam=c["K"], blank_id=c["blank"])
    return ou.decode_core_host_lm(lp, lm[2], lm[3], lm[0], lm[1], sl, threads=1, **args)


def is_pruned(c):
    return c["top_n"] < c["V"] or c["cutoff_prob"] < 1.0


# ---- the same behind a parked state ---------------------------------------------------------------------------------------------------
def stream_entries():
    """The scorer entries of the streamed matrix that reuse their matrix case (not the serving-route ones)."""
    return [e for e in sm.STREAM_CASES if e["case"]["lm"] and not e["production"]]


def replay_frames_lm(c, lm, item, lp=None, sl=None):
    """stream_matrix_util.replay_frames for a scorer case and any item: the frames (0-based) in which `item` of
    select_path_inputs(c) replays std::nth_element -- EV_EXACT of the host twin (built-in scorer, one thread, the caller has applied
    host_env(c)) over prefixes of the item.  The decode of a prefix replays in its LAST frame whenever that frame has more than K
    candidates (beam_core.h step C: `last`), so the counts of two prefixes differ by more than the frame between them:
        exact(p + 1) - exact(p) = replays(p - 1) + forced(p) - forced(p - 1),   forced(f) = [frame f has more than K candidates],
    with exact(p) the count of the prefix of p frames and the candidates of frame f = EV_CANDIDATES(f + 1) - EV_CANDIDATES(f).  The
    frames returned are those that replay although they are NOT a decode's last frame -- what a stream's chunk does in front of a
    boundary; the item's own last frame is not among them.  (stream_matrix_util.replay_frames takes the plain difference of two
    prefixes, exact(f + 1) - exact(f): once the beam is full that is replays(f - 1), so the frame it names lies one behind the replay.
    Its tables stay as they were found; this function is not built on it.)"""
    if lp is None:
        lp, sl = select_path_inputs(c, lm[1])
    rows = np.ascontiguousarray(lp[item:item + 1])
    n = int(sl[item])
    exact, cand = [], []
    for p in range(n + 1):
        _, cnt = counted(lambda: host_decode(c, rows, np.array([p], np.int32), lm))
        exact.append(cnt["EV_EXACT"])
        cand.append(cnt["EV_CANDIDATES"])
    forced = [int(cand[f + 1] - cand[f] > c["K"]) for f in range(n)]
    out = []
    for f in range(n - 1):
        r = exact[f + 2] - exact[f + 1] - forced[f + 1] + forced[f]
        assert r in (0, 1), (f, exact, forced)
        if r:
            out.append(f)
    return out


def select_path_bounds(e):
    """Chunk bounds of a streamed scorer entry over select_path_inputs, chosen as stream_matrix_util.bounds chooses:
    [0, 1, 3, 3, ..., 2T/3 + 1, T] -- a one-frame chunk, a boundary between the two overflow frames (the danger flag, the overflowed
    scores and the scorer's per-entry state cross it together), an empty chunk, a boundary right behind the -inf frame -- with the
    T // 2 and the entry's stream_matrix_util.SELECT_PATH_EXTRA bound in between."""
    T, eid = e["case"]["T"], sm.entry_id(e)
    inner = sorted([T // 2] + ([sm.SELECT_PATH_EXTRA[eid]] if eid in sm.SELECT_PATH_EXTRA else []))
    b = [0, 1, 3, 3] + inner + [(2 * T) // 3 + 1, T]
    assert all(x <= y for x, y in zip(b, b[1:])) and 3 < inner[0] and inner[-1] < (2 * T) // 3 + 1 < T and len(set(inner)) == len(inner), b
    return b


def replay_boundaries(e, lm):
    """The bounds of the entry that directly follow a frame in which item 0 or item 2 replayed std::nth_element, inside that item's
    length: {item: [bounds]}."""
    c = e["case"]
    lp, sl = select_path_inputs(c, lm[1])
    out = {}
    for item in (0, 2):
        rep = set(replay_frames_lm(c, lm, item, lp, sl))
        out[item] = sorted(b for b in set(select_path_bounds(e)) if 0 < b <= int(sl[item]) and (b - 1) in rep)
    return out
