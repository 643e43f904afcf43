#!/usr/bin/env python3
"""What one step of a label-synchronous decode costs with ``prefix_scores`` / ``prefix_advance``, next to what a caller had to do
before them, in one process, medians of 7.

    python tools/prefix_probe.py [--reps N] [--only NAME[,NAME]] [--out profiles/prefix.json]

Workloads: the north-star tensor (B 256, T 1000, V 29) with R = 10 prefixes per item and all labels as candidates, and configs[3]'s
tensor (B 64, T 500, V 10000) with R = 10 and C = 40 listed candidates, and with all labels.  The prefixes have two labels (init and
two advances with random parents and labels).  Per workload, between two HIP events after one untimed pass: one ``prefix_scores``
call, one ``prefix_advance`` call (R new prefixes), each as it comes -- the status words read back -- and with ``status=``, where
nothing is read, and -- the comparison -- one ``log_likelihood`` call on the B x (R x C) rows
"prefix + candidate", which recomputes every lattice and returns the whole-sequence probability, not the prefix's.  Also the rates
the scores call reaches: (prefix, candidate, frame) steps -- one expf each -- per second, and the bytes of rows it must read at least
(every row once per tile of 8 prefixes with all labels, once per prefix and candidate with lists) per second."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctcdecode_amd  # noqa: E402

WORKLOADS = [dict(name="north_star_all_labels", B=256, T=1000, V=29, R=10, C=None),
             dict(name="cfg3_listed_40", B=64, T=500, V=10000, R=10, C=40),
             dict(name="cfg3_all_labels", B=64, T=500, V=10000, R=10, C=None, loglik_reps=2)]


def timed(fn, reps):
    ms = []
    for i in range(reps + 1):  # (the first pass is not counted)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    ms.sort()
    return dict(median=round(statistics.median(ms), 4), min=round(ms[0], 4), max=round(ms[-1], 4), n=len(ms))


def probe(w, reps):
    B, T, V, R = w["B"], w["T"], w["V"], w["R"]
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.empty((B, T, V), device="cuda")
    for b in range(B):  # (row by row: the logits of configs[3] are 1.28 GB)
        x[b] = torch.randn((T, V), generator=g, device="cuda").log_softmax(-1)
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=8, log_probs_input=True, device="cuda:0")
    rnd = lambda hi, shape, lo=0: torch.randint(lo, hi, shape, generator=g, device="cuda", dtype=torch.int32)
    st = dec.prefix_init(x, None, R)
    l1, p2, l2 = rnd(V, (B, R), 1), rnd(R, (B, R)), rnd(V, (B, R), 1)
    st = dec.prefix_advance(x, None, st, torch.zeros((B, R), dtype=torch.int32), l1)
    st = dec.prefix_advance(x, None, st, p2, l2)
    cands = None if w["C"] is None else rnd(V, (B, R, w["C"]), 1)
    C = V if cands is None else w["C"]
    rec = dict(B=B, T=T, V=V, R=R, C=C, listed=cands is not None)
    # (the plain calls read their status words back and wait for the device; with the caller's status tensor nothing is read)
    status = torch.zeros((B,), dtype=torch.int32, device="cuda")
    rec["prefix_scores_ms"] = timed(lambda: dec.prefix_scores(x, None, st, cands), reps)
    rec["prefix_scores_unchecked_ms"] = timed(lambda: dec.prefix_scores(x, None, st, cands, status=status), reps)
    rec["scores_kernel_code"] = dec.last_prefix_kernel()
    rec["prefix_advance_ms"] = timed(lambda: dec.prefix_advance(x, None, st, p2, l2), reps)
    rec["prefix_advance_unchecked_ms"] = timed(lambda: dec.prefix_advance(x, None, st, p2, l2, status=status), reps)
    s = rec["prefix_scores_unchecked_ms"]["median"] * 1e-3
    rec["steps_per_s"] = round(B * R * C * T / s, 1)
    rec["row_bytes_per_s_at_least"] = round((B * T * V * 4 * -(-R // 8) if cands is None else B * R * C * T * 4) / s, 1)
    # the comparison: the rows prefix + candidate, three labels each (the blank column's rows take label 1 instead)
    cc = (torch.arange(V, device="cuda", dtype=torch.int32).clamp(min=1).expand(B, R, V) if cands is None else cands).reshape(B, R * C, 1)
    pre = torch.stack((torch.gather(l1, 1, p2.long()), l2), -1).repeat_interleave(C, 1)
    tok = torch.cat((pre, cc), -1).contiguous()
    lens = torch.full((B, R * C), 3, dtype=torch.int32, device="cuda")
    rec["log_likelihood_rows"] = B * R * C
    rec["log_likelihood_ms"] = timed(lambda: dec.log_likelihood(x, None, tok, lens), w.get("loglik_reps", reps))
    rec["log_likelihood_over_prefix_scores"] = round(rec["log_likelihood_ms"]["median"] / rec["prefix_scores_ms"]["median"], 2)  # (both read their status)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix.json"))
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "method": " ".join(__doc__.split("\n\n")[2].split())}
    for w in WORKLOADS:
        if only and w["name"] not in only:
            continue
        res[w["name"]] = probe(w, a.reps)
        print(w["name"], json.dumps(res[w["name"]]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
