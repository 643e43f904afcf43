#!/usr/bin/env python3
"""What long posteriors (``CTCBeamDecoder.set_long_posteriors``) cost, per band and block, in one process, medians.

    python tools/long_posteriors_probe.py [--reps N] [--only NAME[,NAME]] [--out profiles/long_posteriors.json]

Workloads, random log-softmax rows over V = 29 and random labels, those of tools/long_rows_probe.py: `chapter` (B 1, R 1, T 30000,
L 10000: one workgroup), `corpus` (B 64, R 1, T 8192, L 2900 .. 3100: a workgroup per row, the scratch budget raised to 16 GiB so that
every row has a slot at every band) and `limit_row` (one row of S = 4095 at T 8192: the register kernel of 16 states per lane with
the mode off, next to bands 256 and 1024).  Per (workload, band, block): ctcd_ctc_posteriors into tensors allocated beforehand, between
two HIP events, after one untimed call; next to it, per band, the banded ctcd_ctc_loglik (set_long_rows at the same band) on the same
rows in the same session, and their ratio.  Before anything is timed the outputs of all bands and blocks of a workload are compared
bit for bit, and the log-likelihoods with ctcd_ctc_loglik's."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

V = 29
WORKLOADS = [dict(name="chapter", B=1, T=30000, L=(10000, 10000), bands=[256, 1024, 4096], blocks=[64, 0, 512]),
             dict(name="corpus", B=64, T=8192, L=(2900, 3100), bands=[256, 1024, 4096], blocks=[32, 0, 256], budget=16 << 30),
             dict(name="limit_row", B=1, T=8192, L=(2047, 2047), bands=[0, 256, 1024], blocks=[32, 0, 256])]


def med(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 4), min=round(xs[0], 4), max=round(xs[-1], 4), n=len(xs))


def timed(call, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def probe(w, reps):
    B, T = w["B"], w["T"]
    g = torch.Generator(device="cuda").manual_seed(4321)
    x = torch.randn((B, T, V), generator=g, device="cuda").log_softmax(-1)
    lens = torch.randint(w["L"][0], w["L"][1] + 1, (B, 1), generator=g, device="cuda", dtype=torch.int32)
    Ls = int(lens.max())
    tok = torch.randint(1, V, (B, 1, Ls), generator=g, device="cuda", dtype=torch.int32)
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=8, log_probs_input=True, device="cuda:0")
    dec.set_posterior_scratch(w.get("budget", 0))
    pk = torch.empty((B, 1, Ls), dtype=torch.int32, device="cuda")
    oc, cf = (torch.empty((B, 1, Ls), dtype=torch.float32, device="cuda") for _ in range(2))
    ll, ll2 = (torch.empty((B, 1), dtype=torch.float32, device="cuda") for _ in range(2))
    status = torch.zeros((B,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    head = (dec._handle, x.data_ptr(), None, B, T, V, 0, 1, tok.data_ptr(), lens.data_ptr(), 1, Ls)
    post = lambda: _native.check(_native.lib.ctcd_ctc_posteriors(*head, pk.data_ptr(), oc.data_ptr(), cf.data_ptr(), ll.data_ptr(), status.data_ptr(), stream))
    loglik = lambda: _native.check(_native.lib.ctcd_ctc_loglik(*head, ll2.data_ptr(), status.data_ptr(), stream))
    configs = [(band, block) for band in w["bands"] for block in (w["blocks"] if band else [0])]
    # every configuration's outputs, bit for bit, before anything is timed (these calls are the warm-up of every kernel timed below)
    first, same = None, True
    for band, block in configs:
        dec.set_long_posteriors(band, block)
        dec.set_long_rows(band)
        post()
        loglik()
        torch.cuda.synchronize()
        got = [t.clone() for t in (pk, oc.view(torch.int32), cf.view(torch.int32), ll.view(torch.int32))]
        first = first or got
        same = same and all(torch.equal(a, b) for a, b in zip(got, first)) and torch.equal(ll.view(torch.int32), ll2.view(torch.int32))
    out = dict(rows=B, T=T, row_labels=dict(min=int(lens.min()), max=Ls), rows_with_alignments=int(torch.isfinite(ll).sum()),
               identical_across_bands_and_blocks=bool(same), status_raised=bool(status.any()))
    for band in w["bands"]:
        dec.set_long_rows(band)
        rec = dict(loglik=dict(kernels_ms=med(timed(loglik, reps)), launched_band=dec.last_long_rows()))
        for block in (w["blocks"] if band else [0]):
            dec.set_long_posteriors(band, block)
            ms = timed(post, reps)
            rec["block_%d" % block] = dict(kernels_ms=med(ms), grid=dec.last_posterior_grid(), launched=list(dec.last_long_posteriors()),
                                           times_loglik=round(statistics.median(ms) / rec["loglik"]["kernels_ms"]["median"], 3))
        out["band_%d" % band] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_posteriors.json"))
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "method": __doc__.split("\n\n")[2]}
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
