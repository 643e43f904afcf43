#!/usr/bin/env python3
"""What an adversarial row costs the prune's std::sort replay: per shape of tests/prune_adversary_util.py, the certificate of its killer
row (rounds, heap-sorted ranges) and ctcd_last_resolve_ms of a call whose 8 frames all carry the killer, next to the same call with benign
permutations of the same values (8 flagged frames either way, one workgroup each, so the figure is one frame's replay plus the launch).
Median of --reps calls, the two kinds alternating.    python tools/prune_adversary_probe.py --out profiles/prune_adversary.json"""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import ctcdecode_amd
import ctcdecode_amd._native as n
import oracle_util as ou
import prune_adversary_util as pa

ap = argparse.ArgumentParser()
ap.add_argument("--out", required=True)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--frames", type=int, default=8)
a = ap.parse_args()
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
res = []
for c in pa.CASES:
    if c["misaligned"]:  # (the same replay as the aligned case)
        continue
    V, top_n = c["V"], c["top_n"]
    k = pa.killer(V, c["big_left"], c["fold"])
    if c["tie_top"]:
        k = np.minimum(k, k.max() - 1)
    rng = np.random.default_rng(c["seed"])
    shift = pa.inputs(c)[2]  # (raw logits: the spacing 2^-shift whose log-softmax rows keep the killer whole)
    value = (lambda r, t: (r.astype(np.float32) + np.float32(t)) * np.float32(2.0 ** -shift)) if c["li"] == 2 else (lambda r, t: pa.values_of_ranks(r, c["dt"], c["li"], offset=t))
    rows = {"adversarial": np.stack([value(k, t) for t in range(a.frames)])[None], "benign": np.stack([value(rng.permutation(k), t) for t in range(a.frames)])[None]}
    compared = {kind: ou.log_softmax_rows(x) if c["li"] == 2 else x for kind, x in rows.items()}  # (what the sort compares and the oracle reads)
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=pa.K, cutoff_top_n=top_n, cutoff_prob=c["cp"], log_probs_input=c["li"] == 1,
                                       logits_input=c["li"] == 2, device="cuda:0")
    dec.set_timing(True)
    dec.set_prune_registers(c["reg"])
    n.check(n.lib.ctcd_debug_set_prune_resolve(dec._handle, 0 if c["resolve_global"] else 1))
    xs = {kind: torch.from_numpy(x).to(device="cuda:0", dtype=DT[c["dt"]]) for kind, x in rows.items()}
    ms = {kind: [] for kind in rows}
    flagged = {}
    for rep in range(a.reps + 1):  # (the first call of each kind warms up)
        for kind in ("adversarial", "benign"):
            dec.decode_device(xs[kind], None)
            torch.cuda.synchronize()
            if rep:
                ms[kind].append(dec.last_resolve_ms())
            flagged[kind] = int(n.lib.ctcd_last_prune_flagged_rows(dec._handle))
    # (the timed calls computed the right thing)
    which = "reference" if ou.have_reference_prune() else "restated"
    ou.assert_same_pruned(dec.last_prune_rows(a.frames, min(top_n, V)), ou.pruned_rows(compared["benign"], c["cp"], top_n, c["li"] != 0, which=which), pa.case_id(c))
    r = dict(case=pa.case_id(c), V=V, top_n=top_n, fold=c["fold"], dtype=c["dt"], logit_shift=shift, arrays="global memory" if c["resolve_global"] else "LDS",
             frames_per_call=a.frames, flagged_frames=flagged,
             certificate={kind: pa.certificate(compared[kind][0, 0], top_n) for kind in rows},
             last_resolve_ms={kind: round(statistics.median(v), 4) for kind, v in ms.items()},
             last_resolve_ms_min_max={kind: [round(min(v), 4), round(max(v), 4)] for kind, v in ms.items()})
    res.append(r)
    print(json.dumps(r), flush=True)
with open(a.out, "w") as f:
    json.dump(dict(what="prune_resolve_kernel on adversarial rows: ctcd_last_resolve_ms (end of the prune pass to the start of the decode kernel) of a call "
                        "of %d flagged frames, median of %d calls, killer rows against benign permutations of the same values" % (a.frames, a.reps),
                   raw_logits="normalising could merge neighbouring logits and break the killer; the spacing 2^-logit_shift is the first of %s whose "
                              "log-softmax rows certify the case's cell in full: %s" % (list(pa.LOGIT_SHIFTS), {r["case"]: bool(pa.in_cell(c, r["certificate"]["adversarial"]))
                                                                                         for c in pa.CASES for r in res if c["li"] == 2 and r["case"] == pa.case_id(c)}),
                   device=torch.cuda.get_device_name(0), cases=res), f, indent=1)
    f.write("\n")
