"""One case per instantiation of ctc_beam_decode_kernel (ctcdecode_amd/csrc/decode_kernel.h CTC_KERNEL_LIST, product branch): the
template arguments the case must launch, the decoder arguments and switches that select it, and an input recipe.  Shared by the CPU
checks (test_abi.py: the table covers the list exactly; test_launch_plan.py: the host's choice plans each case's kernel) and the GPU
tests (test_gpu_kernel_matrix.py: the hook reports the expected kernel, which decodes like the oracle).  No torch here: the CPU suite
imports this module.

A kernel is the tuple (PROF, BIG, LAYOUT, PRUNED, NT, LM, OCC2), LM as 0 / 1 / 2 / 3 (no scorer / general scorer / word model over
<= 64 labels / callback scorer).  Shapes were chosen with the workspace sizes of beam_core.h carve() against 160 KB of LDS:
  * fixed layout (LAYOUT 1): beam <= 128, <= 32 labels;  pruned default (LAYOUT 2): beam <= 112, <= 40 of <= 10240 labels, 1024 threads;
  * beam 300 over 29 labels: HBM level 1 (BIG 1), LAYOUT 3 when unpruned, without a scorer, at 1024 threads;
  * beam 700 over 29 labels: level 2;  more than 65535 candidate slots (beam * (candidates + 2)): level 3."""
import numpy as np

import oracle_util as ou

LABELS29 = ["_", "'", " "] + [chr(ord("a") + i) for i in range(26)]  # (= test_lm.LABELS29)
CHARS8 = ["_", "a", "b", "c", "d", "'", "é", " "]

# the scorers a case can name: (ARPA file under tests/data or "wide99" = test_lm.make_wide_label_lm, labels, alpha, beta)
LMS = {
    "word": ("test.arpa", LABELS29, 0.5, 1.0),
    "chars": ("chars.arpa", CHARS8, 0.6, 0.2),
    "wide99": ("wide99", None, 0.4, 0.7),
}


def _case(kernel, V, K, T=40, B=4, top_n=None, cutoff_prob=1.0, threads=None, blank=0, subtree=0, cu_sharing=0, fixed=True,
          lm=None, general=False, callback=False, profile=0, streamed=False, seed=0):
    assert len(kernel) == 7
    return dict(kernel=tuple(int(x) for x in kernel), V=V, K=K, T=T, B=B, top_n=V if top_n is None else top_n, cutoff_prob=cutoff_prob,
                threads=threads, blank=blank, subtree=subtree, cu_sharing=cu_sharing, fixed=fixed, lm=lm, general=general,
                callback=callback, profile=profile, streamed=streamed, seed=seed)


CASES = [
    # fixed layout at 1024 threads, and its two-workgroups-per-CU build
    _case((0, 0, 1, 0, 1024, 0, 0), V=32, K=100, threads=1024, blank=5),
    _case((0, 0, 1, 1, 1024, 0, 0), V=29, K=64, top_n=12, cutoff_prob=0.95, threads=1024, blank=28),
    _case((0, 0, 1, 0, 1024, 0, 1), V=29, K=100, threads=1024, cu_sharing=1, blank=13),
    _case((0, 0, 1, 1, 1024, 0, 1), V=32, K=48, top_n=10, threads=1024, cu_sharing=1),
    # fixed layout, other workgroup sizes
    _case((0, 0, 1, 0, 0, 0, 0), V=29, K=50, threads=256, blank=3),
    _case((0, 0, 1, 1, 0, 0, 0), V=32, K=40, top_n=10, threads=512),
    # subtree search
    _case((3, 0, 1, 0, 1024, 0, 0), V=29, K=80, threads=1024, subtree=1, blank=20),
    _case((3, 0, 1, 1, 1024, 0, 0), V=29, K=64, top_n=14, cutoff_prob=0.99, threads=1024, subtree=1),
    # run-time layout (> 32 labels; pruned below 1024 threads, where the pruned default's layout does not apply)
    _case((0, 0, 0, 0, 0, 0, 0), V=64, K=40, blank=63),
    _case((0, 0, 0, 1, 0, 0, 0), V=300, K=30, top_n=20, blank=150),
    # the pruned default
    _case((0, 0, 2, 1, 1024, 0, 0), V=300, K=30, top_n=20, threads=1024, blank=299),
    # wide beams: compile-time, HBM level 1 at 1024 threads and below, level 2
    _case((0, 1, 3, 0, 1024, 0, 0), V=29, K=300, T=30, B=3, blank=1),
    _case((0, 1, 0, 0, 1024, 0, 0), V=29, K=300, T=30, B=3, fixed=False),
    _case((0, 1, 0, 1, 1024, 0, 0), V=29, K=300, T=30, B=3, top_n=20, blank=9),
    _case((0, 1, 0, 0, 0, 0, 0), V=29, K=300, T=30, B=3, threads=512, blank=7),
    _case((0, 1, 0, 1, 0, 0, 0), V=29, K=300, T=30, B=3, top_n=20, cutoff_prob=0.99, threads=512),
    _case((0, 2, 0, 0, 0, 0, 0), V=29, K=700, T=20, B=3, blank=28),
    _case((0, 2, 0, 1, 0, 0, 0), V=29, K=700, T=20, B=3, top_n=25),
    # more than 65535 candidate slots
    _case((0, 3, 0, 0, 0, 0, 0), V=700, K=100, T=16, B=3, blank=350),
    _case((0, 3, 0, 1, 0, 0, 0), V=1500, K=60, T=16, B=3, top_n=1200),
    # word model over <= 64 labels, with and without two workgroups per CU
    _case((0, 0, 1, 0, 1024, 2, 0), V=29, K=64, lm="word"),
    _case((0, 0, 1, 1, 1024, 2, 0), V=29, K=48, cutoff_prob=0.95, lm="word"),
    _case((0, 0, 1, 0, 1024, 2, 1), V=29, K=64, lm="word", cu_sharing=1),
    _case((0, 0, 1, 1, 1024, 2, 1), V=29, K=48, top_n=12, lm="word", cu_sharing=1),
    # general scorer: a character model, or a word model with CTCD_GENERAL_LM_KERNEL=1; run-time layout at 512 threads
    _case((0, 0, 1, 0, 1024, 1, 0), V=8, K=32, lm="chars"),
    _case((0, 0, 1, 1, 1024, 1, 0), V=29, K=48, top_n=15, lm="word", general=True),
    _case((0, 0, 1, 0, 1024, 1, 1), V=8, K=40, lm="chars", cu_sharing=1),
    _case((0, 0, 1, 1, 1024, 1, 1), V=29, K=48, cutoff_prob=0.95, lm="word", general=True, cu_sharing=1),
    _case((0, 0, 0, 0, 0, 1, 0), V=29, K=40, lm="word", threads=512),
    _case((0, 0, 0, 1, 0, 1, 0), V=29, K=40, top_n=10, lm="word", threads=512),
    # scorer, wide beams: level 1 / 2 over 29 labels, level 3 with the 99-label model
    _case((0, 1, 0, 0, 0, 1, 0), V=29, K=300, T=24, B=3, lm="word"),
    _case((0, 1, 0, 1, 0, 1, 0), V=29, K=300, T=24, B=3, cutoff_prob=0.95, lm="word"),
    _case((0, 2, 0, 0, 0, 1, 0), V=29, K=700, T=16, B=3, lm="word"),
    _case((0, 2, 0, 1, 0, 1, 0), V=29, K=700, T=16, B=3, top_n=20, lm="word"),
    _case((0, 3, 0, 0, 0, 1, 0), V=99, K=700, T=10, B=3, lm="wide99"),
    _case((0, 3, 0, 1, 0, 1, 0), V=99, K=700, T=10, B=3, cutoff_prob=0.95, lm="wide99"),
    # callback scorer (the built-in tables behind the callback): the same shapes
    _case((0, 0, 1, 0, 1024, 3, 0), V=29, K=48, lm="word", callback=True),
    _case((0, 0, 1, 1, 1024, 3, 0), V=29, K=48, top_n=12, lm="word", callback=True),
    _case((0, 0, 0, 0, 0, 3, 0), V=29, K=40, lm="word", callback=True, threads=512),
    _case((0, 0, 0, 1, 0, 3, 0), V=29, K=40, cutoff_prob=0.95, lm="word", callback=True, threads=512),
    _case((0, 1, 0, 0, 0, 3, 0), V=29, K=300, T=24, B=3, lm="word", callback=True),
    _case((0, 1, 0, 1, 0, 3, 0), V=29, K=300, T=24, B=3, top_n=20, lm="word", callback=True),
    _case((0, 2, 0, 0, 0, 3, 0), V=29, K=700, T=16, B=3, lm="word", callback=True),
    _case((0, 2, 0, 1, 0, 3, 0), V=29, K=700, T=16, B=3, cutoff_prob=0.95, lm="word", callback=True),
    _case((0, 3, 0, 0, 0, 3, 0), V=99, K=700, T=10, B=3, lm="wide99", callback=True),
    _case((0, 3, 0, 1, 0, 3, 0), V=99, K=700, T=10, B=3, cutoff_prob=0.95, lm="wide99", callback=True),
    # streamed host input (decode() of a CPU tensor: T >= 128 and at least 1 MiB of rows)
    _case((4, 0, 1, 0, 1024, 0, 0), V=32, K=16, T=128, B=64, threads=1024, streamed=True, blank=31),
    _case((5, 0, 1, 0, 1024, 0, 0), V=32, K=16, T=128, B=64, threads=1024, subtree=1, streamed=True),
    _case((4, 0, 1, 0, 1024, 0, 1), V=32, K=16, T=128, B=64, threads=1024, cu_sharing=1, streamed=True, blank=2),
    _case((4, 0, 1, 0, 1024, 2, 0), V=29, K=16, T=128, B=72, lm="word", streamed=True),
    # phase timers (tools/phase_profile.py)
    _case((1, 0, 1, 0, 0, 0, 0), V=32, K=64, profile=1, blank=31),
    _case((1, 0, 1, 1, 0, 0, 0), V=29, K=64, top_n=12, profile=1),
    _case((1, 0, 0, 0, 0, 0, 0), V=64, K=40, profile=1, blank=10),
    _case((1, 0, 0, 1, 0, 0, 0), V=300, K=30, top_n=20, threads=1024, profile=1),
    _case((1, 1, 0, 0, 0, 0, 0), V=29, K=300, T=30, B=3, profile=1, blank=4),
    _case((1, 1, 0, 1, 0, 0, 0), V=29, K=300, T=30, B=3, top_n=20, profile=1),
    # barrier timeline (tools/barrier_timeline.py)
    _case((2, 0, 1, 0, 1024, 0, 0), V=29, K=64, profile=2, threads=1024, blank=17),
    _case((2, 1, 0, 0, 1024, 0, 0), V=29, K=300, T=30, B=3, profile=2),
    _case((2, 0, 1, 0, 1024, 1, 0), V=8, K=32, lm="chars", profile=2),
    _case((2, 0, 1, 0, 1024, 2, 0), V=29, K=48, lm="word", profile=2),
]
for _i, _c in enumerate(CASES):
    _c["seed"] = 9100 + 17 * _i


def case_id(c):
    return "k%d%d%d%d_%d_lm%d_occ%d" % c["kernel"]


def expected_layout(kernel):
    """ctcd_debug_last_layout of a kernel: LAYOUT 3 -> 3, BIG b at LAYOUT 0 -> 3 + b, LAYOUT 2 -> 2, LAYOUT 1 -> 1, else 0."""
    _, big, layout = kernel[:3]
    if layout == 3:
        return 3
    if big and layout == 0:
        return 3 + big
    return layout if layout in (1, 2) else 0


def scorer_kind(c):
    """The scorer of a case as launch_plan.h ScorerKind: 0 none, 1 one the general builds serve (a character model, a word model over
    more than 64 labels, or any with CTCD_GENERAL_LM_KERNEL=1), 2 a word model over <= 64 labels, 3 a callback."""
    if not c["lm"]:
        return 0
    if c["callback"]:
        return 3
    return 2 if c["lm"] == "word" and not c["general"] else 1


def parse_kernel_list(header_text):
    """The X(PROF, BIG, LAYOUT, PRUNED, NT, LM, OCC2, group) items of the product branch of CTC_KERNEL_LIST (the #else branch) ->
    list of 7-tuples of ints, in the order of the list."""
    import re

    m = re.search(r"#else\s*\n#define CTC_KERNEL_LIST\(X\)(.*?)\n#endif", header_text, flags=re.S)
    assert m, "the product branch of CTC_KERNEL_LIST was not found"
    words = {"true": 1, "false": 0}
    items = re.findall(r"\bX\(([^)]*)\)", m.group(1))
    out = []
    for it in items:
        args = [a.strip() for a in it.split(",")]
        assert len(args) == 8, it
        out.append(tuple(words[a] if a in words else int(a) for a in args[:7]))
    return out


def lm_spec(c, wide99_path=None, wide99_labels=None):
    """-> (lm_path, labels, alpha, beta) of a scorer case."""
    import os

    name, labels, alpha, beta = LMS[c["lm"]]
    if name == "wide99":
        return wide99_path, wide99_labels, alpha, beta
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", name), labels, alpha, beta


def degenerate_item(c):
    """The utterance of a scorer-free case that carries the degenerate frames."""
    return 3 if c["B"] > 3 else 0


def inputs(c, labels=None, overflow_as_inf=False):
    """-> (lp [B, T, V] float32 log-probabilities, seq_lens [B] int32).

    Utterance 0 runs the full length; 1 has one frame; 2 has coarse rows (multiples of 0.5: exact ties, the nth_element replay, and
    ties at the prune cut); without a scorer, 3 (0 if B == 3) carries two frames of -3e38 (frames 2 and 3: adding the second overflows
    every score to -inf) and a frame of -inf at 2T/3 (overflow_as_inf: the two frames are -inf as well -- the CPU suite checks that
    this changes the oracle's result, i.e. that the overflow is exercised); any further
    utterances (the streamed cases) are random at random lengths.  Scorer cases favour the space label."""
    B, T, V, blank, seed = c["B"], c["T"], c["V"], c["blank"], c["seed"]
    rng = np.random.default_rng(seed)
    lp = ou.synth_logprobs(B, T, V, seed, blank_id=blank, blank_bias=0.5 if c["lm"] else 0.0)
    lp[2] = ou.synth_logprobs(1, T, V, seed + 1, quant=0.5, blank_id=blank)[0]
    lens = rng.integers(1, T + 1, size=B)
    lens[0], lens[1], lens[2] = T, 1, max(2, (2 * T) // 3)
    if B > 3:
        lens[3] = T - 2
    if not c["lm"]:
        d = degenerate_item(c)
        lp[d, 2:4, :] = -np.inf if overflow_as_inf else np.float32(-3.0e38)  # (two frames: every sum of scores overflows to -inf)
        lp[d, (2 * T) // 3, :] = -np.inf
    if c["lm"] and labels is not None and " " in labels:
        lp[:, :, labels.index(" ")] += np.float32(1.0)  # (after the rounding: the coarse rows keep their ties)
    return np.ascontiguousarray(lp, dtype=np.float32), lens.astype(np.int32)
