"""Adversarial rows for the vocabulary prune's std::sort replay (prune_resolve_kernel -> stl_emul.h sort_prefix_parallel): the case list,
their inputs and, per frame, the certificate of what the replay has to do for it (tests/native/prune_adversary.cpp).  Shared by the CPU
certificate test (test_prune_adversary.py), the GPU test (test_gpu_prune_adversary.py) and tools/prune_adversary_probe.py.  No torch.

A row is a list of integer ranks, one per label (larger = better): McIlroy's killer of the live std::sort, folded (``fold``: ranks // fold,
ties in groups of fold) -- or, in the benign frames next to it, a random permutation of the same ranks.  Ranks become CONSECUTIVE
representable values of the case's dtype, by bit pattern, so that float32, bf16 and fp16 rows carry exactly the rank order (bf16 has no
5000 evenly spaced values any other way): log-probabilities downward from -1.0, probabilities downward from the largest value below 1.0
(all positive normal numbers).  Logits are ranks * 2^-k (float32; k: ``logit_shift``), and what the sort compares is their log-softmax.

Case fields are those of prepass_matrix_util (so that its expected_prepass says which kernels a case must launch) plus ``cell`` (what the
certificate of its adversarial frames must show), ``big_left`` (the killer's long side starts at place 0) and ``fold``."""
import ctypes
import os
import subprocess

import numpy as np

import oracle_util as ou

B, T, K = 2, 6, 8
BIG_CUT = 256       # prepass.hip kResolveBigCut
BSTACK_SLOTS = 64   # stl_emul.h sort_prefix_parallel: bstack holds 3 * 64 ints
SEQ_LENS = np.array([T, T - 1], np.int32)
LOGIT_SHIFTS = (4, 5, 6, 7, 8)

ADV_SO = os.path.join(ou.ROOT, "oracle", "_build", "libctcprune_adversary.so")
_i32p = ctypes.POINTER(ctypes.c_int32)
_f32p = ctypes.POINTER(ctypes.c_float)
CERT_FIELDS = ("wg_rounds", "thread_rounds", "long_heaps", "long_heap_max", "short_heaps", "short_heap_max", "max_pending", "tie_at_cut",
               "skipped", "skipped_max", "max_tasks", "walk_ok")


def build_adversary():
    """Compile tests/native/prune_adversary.cpp for the host -- test infrastructure only."""
    src = os.path.join(ou.ROOT, "tests", "native", "prune_adversary.cpp")
    deps = [src, os.path.join(ou.ROOT, "ctcdecode_amd", "csrc", "stl_emul.h")]
    if os.path.exists(ADV_SO) and all(os.path.getmtime(ADV_SO) >= os.path.getmtime(p) for p in deps):
        return ADV_SO
    os.makedirs(os.path.dirname(ADV_SO), exist_ok=True)
    tmp = "%s.%d.tmp" % (ADV_SO, os.getpid())
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", src, "-o", tmp], check=True)
    os.replace(tmp, ADV_SO)
    return ADV_SO


_killers = {}


def killer(n, big_left=True, fold=1):
    """int32 [n]: the ranks of McIlroy's adversary against std::sort (descending) on n labels in label order, // fold."""
    key = (n, bool(big_left), fold)
    if key not in _killers:
        r = np.zeros((n,), np.int32)
        assert ctypes.CDLL(build_adversary()).ctcadv_killer(n, int(bool(big_left)), fold, r.ctypes.data_as(_i32p)) == 1
        r.setflags(write=False)
        _killers[key] = r
    return _killers[key]


def certificate(row, top_n, big_cut=BIG_CUT):
    """What the replay of one row (float32: the values the sort compares) goes through, as a dict over CERT_FIELDS."""
    row = np.ascontiguousarray(row, dtype=np.float32)
    out = np.zeros((12,), np.int32)
    assert ctypes.CDLL(build_adversary()).ctcadv_certificate(row.ctypes.data_as(_f32p), row.size, int(top_n), int(big_cut), out.ctypes.data_as(_i32p)) == 1
    return dict(zip(CERT_FIELDS, (int(v) for v in out)))


def values_of_ranks(ranks, dt, li, offset=0):
    """ranks (int, larger = better) -> float32 values exactly representable in dtype dt that carry the same order: the best rank the
    value `offset` places below -1.0 (log-probabilities, li 1) / below the largest value under 1.0 (probabilities, li 0), every next
    rank the next representable value further down."""
    ranks = np.asarray(ranks, dtype=np.int64)
    down = (ranks.max() - ranks) + int(offset)
    if li == 1:  # negative values: a larger bit pattern lies further down
        base = {"f32": 0xBF800000, "bf16": 0xBF80, "f16": 0xBC00}[dt]
        bits = base + down
        assert bits.max() < {"f32": 0xFF800000, "bf16": 0xFF80, "f16": 0xFC00}[dt]  # finite
    else:
        base = {"f32": 0x3F7FFFFF, "bf16": 0x3F7F, "f16": 0x3BFF}[dt]
        bits = base - down
        assert bits.min() >= {"f32": 0x00800000, "bf16": 0x0080, "f16": 0x0400}[dt]  # positive and normal
    if dt == "f32":
        return bits.astype(np.uint32).view(np.float32)
    if dt == "bf16":
        return (bits.astype(np.uint32) << 16).view(np.float32)
    return bits.astype(np.uint16).view(np.float16).astype(np.float32)


def _case(cell, V, top_n, fold=2, dt="f32", li=1, cp=1.0, big_left=True, reg=True, misaligned=False, resolve_global=False, tie_top=False):
    return dict(cell=cell, V=V, top_n=top_n, fold=fold, dt=dt, li=li, cp=cp, big_left=big_left, reg=reg, misaligned=misaligned,
                resolve_global=resolve_global, tie_top=tie_top, fused=True, K=K)


def _cases():
    C = []
    # ---- the depth budget spent on ONE long range that starts at place 0: heap_select + heap_sort_down by one thread on a range
    # > big_cut.  fold 2 with V even and top_n odd: a pair of equal values straddles the cut, the frame is flagged and the kept labels
    # depend on every decision of the replay.  fold 1: distinct values, the kept set is unique -- and the fast pass settles the frame
    # itself, unless the two best labels are made equal (tie_top): then the frame is flagged for a tie INSIDE the kept labels, the replay
    # runs, and the kept set behind the heap sort has to be the unique right one.
    C.append(_case("long", 300, 7))                                     # (prune_wg, F4 1)
    C.append(_case("long", 300, 7, misaligned=True))                    # (prune_rows: rows off the workgroup kernel's alignment)
    C.append(_case("long", 300, 7, fold=1, tie_top=True))
    C.append(_case("long", 300, 7, dt="f16", reg=False))
    C.append(_case("long", 1000, 7, dt="bf16"))
    C.append(_case("long", 1000, 39, dt="f16", reg=False))
    C.append(_case("long", 1000, 39, fold=1, tie_top=True, dt="bf16"))
    C.append(_case("long", 1000, 39, cp=0.9))                           # the exact cumulative chain behind a heap-sorted prefix
    C.append(_case("long", 1000, 39, li=0))                             # probabilities
    C.append(_case("long", 1000, 39, li=2))                             # raw logits: the fused pass
    C.append(_case("long", 1026, 39))                                   # (V % 4 != 0: prune_rows)
    C.append(_case("long", 4096, 63))
    C.append(_case("long", 4096, 63, dt="bf16", reg=False))
    C.append(_case("long", 4096, 63, fold=1, dt="f16"))
    C.append(_case("long", 300, 300, cp=0.9))                           # top_n >= V: every place of the row is wanted
    # ---- the depth budget spent on a range <= big_cut: the heap sort inside sort_parallel, lengths on both sides of big_cut.  (V odd:
    # fold 2 leaves the best rank alone, pairs straddle an EVEN cut; fold 3 at V = 260 / 1000: a cut of 64 / 39 lies inside a group)
    C.append(_case("short", 40, 7, dt="bf16"))
    C.append(_case("short", 256, 39))
    C.append(_case("short", 257, 40, dt="f16"))
    C.append(_case("short", 258, 39, li=0))
    C.append(_case("short", 260, 64, fold=3))
    C.append(_case("short", 272, 39, dt="bf16", reg=False))
    C.append(_case("short", 272, 39, fold=1, tie_top=True))
    C.append(_case("short", 1000, 39, fold=3))
    # ---- the ascending killer: the long side of every partition starts beyond top_n and must be left alone
    C.append(_case("right", 1000, 39, big_left=False))
    C.append(_case("right", 4096, 63, big_left=False, dt="bf16"))
    # ---- rows at the introsort threshold (16: the serial sort; 17: one thread round; 18: two), and top_n >= V (pruned by cutoff_prob)
    C.append(_case("boundary", 16, 7))
    C.append(_case("boundary", 17, 7, fold=3, dt="f16"))
    C.append(_case("boundary", 18, 7, dt="bf16"))
    C.append(_case("boundary", 18, 40, cp=0.9))
    # ---- the long- and short-range cases up to 1026 labels again with the sort's arrays in global memory (the layout of rows beyond
    # ~11 000 labels).  No larger V: one thread's heap sort of n elements is about 2 n lg n dependent accesses.
    for c in list(C):
        if c["cell"] in ("long", "short") and c["V"] <= 1026:
            C.append(dict(c, resolve_global=True))
    return C


CASES = _cases()
for _i, _c in enumerate(CASES):
    _c["seed"] = 9100 + 7 * _i


def case_id(c):
    return "%s_V%d_n%d_fold%d_%s_%s%s%s%s%s%s" % (c["cell"], c["V"], c["top_n"], c["fold"], c["dt"], ("prob", "log", "logits")[c["li"]],
                                                 "" if c["cp"] >= 1.0 else "_cp%g" % c["cp"], "" if c["big_left"] else "_asc",
                                                 "" if c["reg"] else "_noreg", "_misaligned" if c["misaligned"] else "",
                                                 ("_tietop" if c["tie_top"] else "") + ("_far" if c["resolve_global"] else ""))


def frame_kind(b, t):
    """Even frames carry the killer (each a few representable values further down than the last), odd frames a benign permutation of the
    same ranks: a workgroup that settles both goes from a heap-sorted row into an ordinary one."""
    return "adversarial" if t % 2 == 0 else "benign"


def _rank_rows(c, rng):
    k = killer(c["V"], c["big_left"], c["fold"])
    if c["tie_top"]:
        k = np.minimum(k, k.max() - 1)
    return [[k if frame_kind(b, t) == "adversarial" else rng.permutation(k) for t in range(T)] for b in range(B)]


def _from_ranks(c, ranks, shift):
    x = np.empty((B, T, c["V"]), np.float32)
    for b in range(B):
        for t in range(T):
            if c["li"] == 2:
                x[b, t] = (ranks[b][t].astype(np.float32) + np.float32(t)) * np.float32(2.0 ** -shift)
            else:
                x[b, t] = values_of_ranks(ranks[b][t], c["dt"], c["li"], offset=t)
    return x


_inputs = {}


def inputs(c):
    """-> (x [B, T, V] float32 in the case's domain, every value representable in its dtype; xo: the float32 rows the sort compares
    and the oracle reads -- for raw logits their log-softmax by the host twin, else x itself; logit_shift or None).

    Raw logits: normalising may merge neighbouring values and break the killer, so the spacings 2^-k of LOGIT_SHIFTS are tried in turn
    and the first whose adversarial frames all certify the case's cell is kept (none: the one with the most heap-sorted elements)."""
    key = case_id(c)
    if key in _inputs:
        return _inputs[key]
    ranks = _rank_rows(c, np.random.default_rng(c["seed"]))
    if c["li"] != 2:
        x = _from_ranks(c, ranks, 0)
        res = (x, x, None)
    else:
        best = None
        for shift in LOGIT_SHIFTS:
            x = _from_ranks(c, ranks, shift)
            xo = ou.log_softmax_rows(x)
            certs = [certificate(xo[b, t], c["top_n"]) for b in range(B) for t in range(T) if frame_kind(b, t) == "adversarial"]
            score = min(q["long_heap_max"] for q in certs)
            if best is None or score > best[0]:
                best = (score, (x, xo, shift))
            if all(in_cell(c, q) for q in certs):
                break
        res = best[1]
    for a in res[:2]:
        a.setflags(write=False)
    _inputs[key] = res
    return res


def in_cell(c, q):
    """Does certificate q show what case c's cell is named for?"""
    if c["cell"] == "long":
        return q["long_heaps"] >= 1 and q["long_heap_max"] > BIG_CUT
    if c["cell"] == "short":
        return q["short_heaps"] >= 1 and 16 < q["short_heap_max"] <= BIG_CUT
    if c["cell"] == "right":
        return q["long_heaps"] == 0 and q["short_heaps"] == 0 and q["skipped"] >= 1 and q["skipped_max"] > BIG_CUT
    return q["long_heaps"] == 0 and q["short_heaps"] == 0 and q["wg_rounds"] <= 1  # boundary


def certificates(c):
    """[B][T] certificates of the case's frames, on the float32 values the sort really compares."""
    xo = inputs(c)[1]
    return [[certificate(xo[b, t], c["top_n"]) for t in range(T)] for b in range(B)]


def live_rows(seq_lens=SEQ_LENS, frames=T):
    return [b * frames + t for b in range(len(seq_lens)) for t in range(int(seq_lens[b]))]


# ---- state carried from row to row: one call with more flagged frames than the replay has workgroups (256 with its arrays in LDS, 64
# with them in global memory), so that a workgroup settles several rows in turn -- killer, benign-tie and constant frames interleaved.
CARRY = [dict(V=300, top_n=7, frames=300, resolve_global=False), dict(V=300, top_n=7, frames=80, resolve_global=True)]
CARRY_KINDS = ("adversarial", "benign", "constant")


def carry_inputs(c):
    """-> (x [2, frames / 2, V] float32 log-probabilities, the kind of every frame [2][frames / 2]).  Every frame ties across the cut."""
    V, Tc = c["V"], c["frames"] // 2
    rng = np.random.default_rng(977 + c["frames"])
    k = killer(V, True, 2)
    x = np.empty((2, Tc, V), np.float32)
    kinds = [[CARRY_KINDS[(b + t) % 3] for t in range(Tc)] for b in range(2)]
    for b in range(2):
        for t in range(Tc):
            if kinds[b][t] == "constant":
                x[b, t] = np.float32(-1.0 - 0.25 * (t % 5))
            else:
                x[b, t] = values_of_ranks(k if kinds[b][t] == "adversarial" else rng.permutation(k), "f32", 1, offset=t % 7)
    return x, kinds
