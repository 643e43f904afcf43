#!/usr/bin/env python3
"""What ``CTCBeamDecoder.log_likelihood_grad`` costs next to ``label_posteriors`` and ``log_likelihood`` on the same rows, in one process, medians.

    python tools/loglik_grad_probe.py [--reps N] [--only NAME[,NAME]] [--out profiles/loglik_grad.json]

Workloads: the north-star shape (B 256, T 1000, V 29, beam 100) and configs[3]'s shape (B 64, T 500, V 10000, beam 100, cutoff_top_n
40, cutoff_prob 0.99), each at R = 1 and 4 rows per item, on random rows (log-softmax of normal logits: the longest labels) and on
transcript-like rows (three frames in four dominated by the blank, the others by one label: short labels).  Per (workload, rows, R):
the rows of decode_device(..., n_best=R) are fed straight back; the gradient kernels between two HIP events (ctcd_ctc_loglik_grad
into tensors allocated beforehand, rows permuted beforehand, status word zeroed beforehand), the posterior and the log-likelihood
kernels the same way on the same rows, and the whole log_likelihood_grad() call (wall time between synchronisations: the permutes,
the allocations, the status read), all alternated in one loop after one untimed pass.  Before anything is timed loglik is compared
bit for bit with log_likelihood's, a second call with the first, and each frame's sum of grad with the rows that contribute.
The expectation, stated before any run and not measured: about label_posteriors' time, plus one LDS pass over L values per frame,
plus the writes of grad (B x T x V x 4 bytes zeroed once, the touched labels per frame and row after that).
The file also keeps the tolerances of tests/loglik_grad_util.py: the float32 numpy reference against the float64 one on the test
inputs, measured on the CPU, and eight times that."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import loglik_grad_util as gu  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402
from posterior_probe import rows_of  # noqa: E402

WORKLOADS = [dict(name="north_star", B=256, T=1000, V=29, K=100, rows=[1, 4]),
             dict(name="cfg3", B=64, T=500, V=10000, K=100, rows=[1, 4], kw=dict(cutoff_top_n=40, cutoff_prob=0.99))]
KINDS = ["random", "transcript"]


def med(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 4), min=round(xs[0], 4), max=round(xs[-1], 4), n=len(xs))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def probe(w, kind, reps):
    B, T, V, K = w["B"], w["T"], w["V"], w["K"]
    x = rows_of(w, kind)
    kw = dict(beam_width=K, cutoff_top_n=V, log_probs_input=True, device="cuda:0")
    kw.update(w.get("kw", {}))
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], **kw)
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for R in w["rows"]:
        tok, _, _, lens = dec.decode_device(x, n_best=R)
        grad, gll = dec.log_likelihood_grad(x, None, tok, lens)
        again, _ = dec.log_likelihood_grad(x, None, tok, lens)
        ll = dec.log_likelihood(x, None, tok, lens)
        pk, oc, cf, pll = dec.label_posteriors(x, None, tok, lens)
        rows = torch.isfinite(ll).sum(1).float()
        rec = dict(grid=dec.last_posterior_grid(), hypotheses=B * R, grad_mb=round(grad.numel() * 4 / 2 ** 20, 1),
                   row_labels=dict(min=int(lens.min()), median=float(lens.float().median()), max=int(lens.max())),
                   loglik_equals_log_likelihood=bool(torch.equal(gll.view(torch.int32), ll.view(torch.int32))),
                   second_call_equal_bits=bool(torch.equal(grad.view(torch.int32), again.view(torch.int32))),
                   worst_frame_sum_minus_rows=float((grad.double().sum(-1) - rows[:, None]).abs().max()))
        del again
        tok_r, lens_r = tok.permute(1, 0, 2).contiguous(), lens.t().contiguous()
        ones, gll_r = torch.ones((R, B), device="cuda"), torch.empty((R, B), device="cuda")
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")
        L = int(tok.shape[2])

        def grad_kernels():
            _native.check(_native.lib.ctcd_ctc_loglik_grad(dec._handle, x.data_ptr(), None, B, T, V, 0, 1, tok_r.data_ptr(), lens_r.data_ptr(), ones.data_ptr(), R, L,
                                                           grad.data_ptr(), gll_r.data_ptr(), status.data_ptr(), stream))

        def posterior_kernels():
            _native.check(_native.lib.ctcd_ctc_posteriors(dec._handle, x.data_ptr(), None, B, T, V, 0, 1, tok.data_ptr(), lens.data_ptr(), R, L, pk.data_ptr(), oc.data_ptr(),
                                                          cf.data_ptr(), pll.data_ptr(), status.data_ptr(), stream))

        def loglik_kernels():
            _native.check(_native.lib.ctcd_ctc_loglik(dec._handle, x.data_ptr(), None, B, T, V, 0, 1, tok.data_ptr(), lens.data_ptr(), R, L, ll.data_ptr(),
                                                      status.data_ptr(), stream))

        gr, po, lk, wall = [], [], [], []
        for i in range(reps + 1):  # (the first pass is not counted)
            t_gr, t_po, t_lk = timed(grad_kernels), timed(posterior_kernels), timed(loglik_kernels)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.log_likelihood_grad(x, None, tok, lens)
            torch.cuda.synchronize()
            t_wall = (time.perf_counter() - t0) * 1e3
            if i:
                gr.append(t_gr), po.append(t_po), lk.append(t_lk), wall.append(t_wall)
        rec.update(grad_kernels_ms=med(gr), posterior_kernels_ms=med(po), loglik_kernels_ms=med(lk), grad_call_ms=med(wall))
        rec["grad_kernels_over_posterior_kernels"] = round(rec["grad_kernels_ms"]["median"] / rec["posterior_kernels_ms"]["median"], 4)
        rec["grad_kernels_over_loglik_kernels"] = round(rec["grad_kernels_ms"]["median"] / rec["loglik_kernels_ms"]["median"], 4)
        out["R_%d" % R] = rec
        del grad
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loglik_grad.json"))
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "method": " ".join(__doc__.split("\n\n")[2].split()),
           "tolerances": {"measured_on": "CPU, tests/loglik_grad_util.py _measure(): max |float32 reference - float64 reference| per case family",
                          "measured": gu.MEASURED, "bound_x8": gu.BOUND}}
    for w in WORKLOADS:
        if only and w["name"] not in only:
            continue
        res[w["name"]] = {}
        for kind in KINDS:
            res[w["name"]][kind] = probe(w, kind, a.reps)
            print(w["name"], kind, json.dumps(res[w["name"]][kind]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
