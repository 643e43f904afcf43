#!/usr/bin/env python3
"""What ``CTCBeamDecoder.find_keywords`` costs next to ``align`` and ``greedy_decode_device`` on the same rows, in one process, medians.

    python tools/keyword_probe.py [--reps N] [--only NAME[,NAME]] [--out profiles/keywords.json]

Workloads: the north-star shape (B 256, T 1000, V 29) and configs[3]'s shape (B 64, T 500, V 10000), float32 log-probabilities,
transcript-like rows (three frames in four dominated by the blank) and random rows; Q = 1, 16 and 256 keywords of 4 - 12 labels.
Per (workload, rows, Q): ctcd_ctc_keywords (the argmax pass and the keyword kernel) into tensors allocated beforehand between two HIP
events, with and without the traces; the bytes of the input over that time; next to it, alternated in one loop after one untimed
pass, ctcd_ctc_align on B x Q rows of the same lengths (through align(): the call's wall time between synchronisations) and the
greedy decode's two kernels on the same tensor.  Medians of 7.  Before anything is timed the first item's results are compared bit for
bit with the host twin (tests/native/keyword_host.cpp)."""
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
from greedy_probe import med, rows_of, timed, wall  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

WORKLOADS = [dict(name="north_star", B=256, T=1000, V=29), dict(name="cfg3", B=64, T=500, V=10000)]
QS = (1, 16, 256)


def probe(w, kind, Q, reps):
    B, T, V = w["B"], w["T"], w["V"]
    x = rows_of(w, 1, torch.float32) if kind == "transcript" else torch.randn((B, T, V), device="cuda").log_softmax(-1)
    rng = np.random.default_rng(Q)
    kws = [ku._keyword(rng, int(rng.integers(4, 13)), V, 0) for _ in range(Q)]
    k, lens = (torch.from_numpy(a).cuda() for a in ku.kw_tensors(kws, 12))
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], log_probs_input=True, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    outs = dec.find_keywords(x, None, k, lens, details=True)
    c = dict(stored=x[:1].cpu().numpy(), dtype=0, seq_lens=None, blank=0, mode=1, kws=kws[:16])
    want, _ = ku.host_find(c, 12)
    try:
        ku.assert_same({n: o[:1, :16].cpu().numpy() for n, o in zip(("scores", "starts", "ends", "end_scores", "end_starts"), outs)}, want, "item 0")
        same = True
    except AssertionError as e:
        print("MISMATCH", e, flush=True)
        same = False
    g = [t.clone() for t in dec.greedy_decode_device(x, details=True)]

    def keywords(details):
        p = [o.data_ptr() for o in outs[:3]] + ([o.data_ptr() for o in outs[3:]] if details else [None, None])
        _native.check(_native.lib.ctcd_ctc_keywords(dec._handle, x.data_ptr(), None, B, T, V, 0, 1, k.data_ptr(), lens.data_ptr(), Q, 12, *p, None, stream))

    def greedy():
        _native.check(_native.lib.ctcd_greedy_decode(dec._handle, x.data_ptr(), None, B, T, V, 0, 1, g[0].data_ptr(), g[2].data_ptr(), g[4].data_ptr(), g[5].data_ptr(),
                                                     g[1].data_ptr(), g[3].data_ptr(), stream))

    rows, rlens = k.unsqueeze(0).expand(B, Q, 12).contiguous(), lens.unsqueeze(0).expand(B, Q).contiguous()
    t_kw, t_tr, t_al, t_gr = [], [], [], []
    for i in range(reps + 1):  # (the first pass is not counted)
        t = timed(lambda: keywords(False)), timed(lambda: keywords(True)), wall(lambda: dec.align(x, None, rows, rlens)), timed(greedy)
        if i:
            t_kw.append(t[0]), t_tr.append(t[1]), t_al.append(t[2]), t_gr.append(t[3])
    nbytes = x.numel() * x.element_size()
    rec = dict(equals_host_twin_on_item_0=same, kernel=dec.last_keyword_kernel(), input_bytes=nbytes, keywords_ms=med(t_kw), keywords_with_traces_ms=med(t_tr),
               align_call_ms=med(t_al), greedy_kernels_ms=med(t_gr))
    rec["keywords_input_TBps"] = round(nbytes / (rec["keywords_ms"]["median"] * 1e-3) / 1e12, 4)
    rec["keywords_over_align_call"] = round(rec["keywords_ms"]["median"] / rec["align_call_ms"]["median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keywords.json"))
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "method": " ".join(__doc__.split("\n\n")[2].split())}
    for w in WORKLOADS:
        if only and w["name"] not in only:
            continue
        res[w["name"]] = {}
        for kind in ("transcript", "random"):
            for Q in QS:
                key = "%s_Q%d" % (kind, Q)
                res[w["name"]][key] = probe(w, kind, Q, a.reps)
                print(w["name"], key, json.dumps(res[w["name"]][key]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
