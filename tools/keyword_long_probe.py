#!/usr/bin/env python3
"""What ``find_keywords`` costs on keywords of 65 .. 2048 labels (``set_long_keywords``), in one process on one device, medians.

    python tools/keyword_long_probe.py [--reps N] [--only NAME[,NAME]] [--out profiles/keywords_long.json]

Workloads: the north-star shape (B 256, T 1000, V 29: the staged route) and configs[3]'s shape (B 64, T 500, V 10000: the gathered
route), float32 log-probabilities, random rows; Q = 1 and 16 keywords of L labels each, L = 64 on the one-label-per-lane kernel (the
baseline) and L = 65, 512, 513, 1024, 2048 on the long kernel.  Per (workload, L, Q): ctcd_ctc_keywords (the argmax pass and the
keyword kernel) into tensors allocated beforehand between two HIP events, without the traces; next to it, alternated in one loop after
one untimed pass, ctcd_ctc_align on B x Q rows of the same lengths (through align() with set_long_rows on: the call's wall time between
synchronisations).  Medians of 7.  us_per_frame is the keywords' median over T: what one frame of one item's walk costs while the
device is as full as B x Q makes it.  Before anything is timed the first item's first keyword is compared bit for bit with the
vectorised restatement of tests/test_gpu_keyword_long.py."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import keyword_util as ku  # noqa: E402
import test_gpu_keyword_long as kl  # noqa: E402
from greedy_probe import med, timed, wall  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

WORKLOADS = [dict(name="north_star", B=256, T=1000, V=29), dict(name="cfg3", B=64, T=500, V=10000)]
LS = (64, 65, 512, 513, 1024, 2048)
QS = (1, 16)
KEYS = ("scores", "starts", "ends", "end_scores", "end_starts")


def probe(w, x, L, Q, reps):
    B, T, V = w["B"], w["T"], w["V"]
    rng = np.random.default_rng(L * 31 + Q)
    kws = [ku._keyword(rng, L, V, 0) for _ in range(Q)]
    k, lens = (torch.from_numpy(a).cuda() for a in ku.kw_tensors(kws, L))
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], log_probs_input=True, device="cuda:0")
    dec.set_long_keywords()
    dec.set_long_rows()
    stream = torch.cuda.current_stream().cuda_stream
    outs = dec.find_keywords(x, None, k, lens, details=True)
    x0 = x[:1].cpu().numpy()
    want = kl.reference(dict(x=x0, seq_lens=None, blank=0, mode=1, kws=kws[:1]))
    try:
        ku.assert_same({n: o[:1, :1].cpu().numpy() for n, o in zip(KEYS, outs)}, want, "item 0")
        same = True
    except AssertionError as e:
        print("MISMATCH", e, flush=True)
        same = False

    def keywords():
        p = [o.data_ptr() for o in outs[:3]] + [None, None]
        _native.check(_native.lib.ctcd_ctc_keywords(dec._handle, x.data_ptr(), None, B, T, V, 0, 1, k.data_ptr(), lens.data_ptr(), Q, L, *p, None, stream))

    rows, rlens = k.unsqueeze(0).expand(B, Q, L).contiguous(), lens.unsqueeze(0).expand(B, Q).contiguous()
    t_kw, t_al = [], []
    for i in range(reps + 1):  # (the first pass is not counted)
        t = timed(keywords), wall(lambda: dec.align(x, None, rows, rlens))
        if i:
            t_kw.append(t[0]), t_al.append(t[1])
    rec = dict(equals_restatement_on_item_0=same, kernel=dec.last_keyword_kernel(), keywords_ms=med(t_kw), align_call_ms=med(t_al))
    rec["us_per_frame"] = round(rec["keywords_ms"]["median"] * 1e3 / T, 4)
    rec["keywords_over_align_call"] = round(rec["keywords_ms"]["median"] / rec["align_call_ms"]["median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keywords_long.json"))
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "method": " ".join(__doc__.split("\n\n")[2].split())}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for w in WORKLOADS:
        if only and w["name"] not in only:
            continue
        res[w["name"]] = {}
        x = torch.randn((w["B"], w["T"], w["V"]), device="cuda").log_softmax(-1)
        for L in LS:
            for Q in QS:
                key = "L%d_Q%d" % (L, Q)
                res[w["name"]][key] = probe(w, x, L, Q, a.reps)
                print(w["name"], key, json.dumps(res[w["name"]][key]), flush=True)
                with open(a.out, "w") as f:  # (after every record: a run that is cut short leaves what it measured)
                    json.dump(res, f, indent=1, sort_keys=True)
                    f.write("\n")


if __name__ == "__main__":
    main()
