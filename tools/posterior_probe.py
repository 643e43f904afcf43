#!/usr/bin/env python3
"""What ``CTCBeamDecoder.label_posteriors`` costs next to ``log_likelihood`` and ``align`` on the same rows and next to the decode it follows, in one process, medians.

    python tools/posterior_probe.py [--reps N] [--only NAME[,NAME]] [--budget-gib G] [--out profiles/posteriors.json]

Workloads: the north-star shape (B 256, T 1000, V 29, beam 100) at R = 1, 10 and 100 rows per item, and configs[3]'s shape (B 64,
T 500, V 10000, beam 100, cutoff_top_n 40, cutoff_prob 0.99) at R = 1; each on random rows (log-softmax of normal logits: the longest
labels) and on transcript-like rows (three frames in four dominated by the blank, the others by one label: short labels).
Per (workload, rows, R): the rows of decode_device(..., n_best=R) are fed straight back; the posterior kernels between two HIP events
(ctcd_ctc_posteriors into tensors allocated beforehand, status word zeroed beforehand), the log-likelihood and the alignment kernels
the same way on the same rows, the whole label_posteriors() call (wall time between synchronisations: allocations, the status read),
the grid and the scratch it stands for, the lengths of the rows, and the decode kernel's own time (set_timing), all alternated in one
loop after one untimed pass.  Before anything is timed the first rows of the first and the last item are compared bit for bit with
the host twin (tests/native/posterior_host.cpp), and the fourth output with log_likelihood's on every row."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import posterior_util as pu  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

WORKLOADS = [dict(name="north_star", B=256, T=1000, V=29, K=100, rows=[1, 10, 100]),
             dict(name="cfg3", B=64, T=500, V=10000, K=100, rows=[1], kw=dict(cutoff_top_n=40, cutoff_prob=0.99))]
KINDS = ["random", "transcript"]


def rows_of(w, kind):
    B, T, V = w["B"], w["T"], w["V"]
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.empty((B, T, V), device="cuda")
    for b in range(B):  # (row by row: the logits of configs[3] are 1.28 GB)
        z = torch.randn((T, V), generator=g, device="cuda")
        if kind == "transcript":
            top = torch.randint(1, V, (T,), generator=g, device="cuda")
            top[torch.rand((T,), generator=g, device="cuda") < 0.75] = 0
            z[torch.arange(T, device="cuda"), top] += 8.0
        x[b] = z.log_softmax(-1)
    return x


def med(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 4), min=round(xs[0], 4), max=round(xs[-1], 4), n=len(xs))


def probe(w, kind, reps, budget_gib=0.0):
    B, T, V, K = w["B"], w["T"], w["V"], w["K"]
    x = rows_of(w, kind)
    kw = dict(beam_width=K, cutoff_top_n=V, log_probs_input=True, device="cuda:0")
    kw.update(w.get("kw", {}))
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], **kw)
    dec.set_timing(True)
    stream = torch.cuda.current_stream().cuda_stream
    out = {}
    for R in w["rows"]:
        tok, _, _, lens = dec.decode_device(x, n_best=R)
        pk, oc, cf, pll = dec.label_posteriors(x, None, tok, lens)
        ll = dec.log_likelihood(x, None, tok, lens)
        st, en, sc = dec.align(x, None, tok, lens)
        live = torch.arange(T, device="cuda")[None, None, :] < lens[:, :, None]
        grid = dec.last_posterior_grid()
        rec = dict(grid=grid, scratch_mb=round(grid * pu.host_slot_bytes(T, T) / 2 ** 20, 1), loglik_grid=dec.last_loglik_grid(), align_grid=dec.last_align_grid(),
                   hypotheses=B * R, row_labels=dict(min=int(lens.min()), median=float(lens.float().median()), max=int(lens.max())),
                   finite=int(torch.isfinite(pll).sum()), loglik_equals_log_likelihood=bool(torch.equal(pll.view(torch.int32), ll.view(torch.int32))),
                   peaks_inside_align_spans=float(((pk >= st) & (pk <= en))[live].float().mean()) if bool(live.any()) else 1.0,
                   confidence=dict(min=float(cf[live].min()), median=float(cf[live].median()), max=float(cf[live].max())) if bool(live.any()) else {},
                   occupancy=dict(min=float(oc[live].min()), median=float(oc[live].median()), max=float(oc[live].max())) if bool(live.any()) else {})
        same = True
        for b in (0, B - 1):  # the first rows of the first and the last item against the host twin
            r = min(R, 2)
            c_tok, c_lens = tok[b:b + 1, :r].cpu().numpy(), lens[b:b + 1, :r].cpu().numpy()
            want = pu.host_posteriors(x[b:b + 1].cpu().numpy(), None, c_tok, c_lens, 0)
            for k, got in zip(pu.KEYS, (pk, oc, cf, pll)):
                same = same and np.array_equal(want[k].view(np.uint32), got[b:b + 1, :r].cpu().numpy().view(np.uint32))
        rec["equals_host_twin_on_sampled_rows"] = bool(same)
        status = torch.zeros((B,), dtype=torch.int32, device="cuda")

        def posterior_kernels():
            _native.check(_native.lib.ctcd_ctc_posteriors(dec._handle, x.data_ptr(), None, B, T, V, 0, 1, tok.data_ptr(), lens.data_ptr(), R, T, pk.data_ptr(), oc.data_ptr(),
                                                          cf.data_ptr(), pll.data_ptr(), status.data_ptr(), stream))

        def loglik_kernels():
            _native.check(_native.lib.ctcd_ctc_loglik(dec._handle, x.data_ptr(), None, B, T, V, 0, 1, tok.data_ptr(), lens.data_ptr(), R, T, ll.data_ptr(),
                                                      status.data_ptr(), stream))

        def align_kernels():
            _native.check(_native.lib.ctcd_ctc_align(dec._handle, x.data_ptr(), None, B, T, V, 0, 1, tok.data_ptr(), lens.data_ptr(), R, T, st.data_ptr(), en.data_ptr(),
                                                     sc.data_ptr(), status.data_ptr(), stream))

        def timed(fn):
            a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b_.record()
            b_.synchronize()
            return a.elapsed_time(b_)

        po, lk, al, wall, dk = [], [], [], [], []
        for i in range(reps + 1):  # (the first pass is not counted)
            t_po, t_lk, t_al = timed(posterior_kernels), timed(loglik_kernels), timed(align_kernels)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.label_posteriors(x, None, tok, lens)
            torch.cuda.synchronize()
            t_wall = (time.perf_counter() - t0) * 1e3
            dec.decode_device(x, n_best=R)
            if i:
                po.append(t_po), lk.append(t_lk), al.append(t_al), wall.append(t_wall), dk.append(dec.last_kernel_ms())
        rec.update(posterior_kernels_ms=med(po), loglik_kernels_ms=med(lk), align_kernels_ms=med(al), posterior_call_ms=med(wall), decode_kernel_ms=med(dk))
        for other in ("loglik_kernels", "align_kernels", "decode_kernel"):
            rec["posterior_kernels_over_" + other] = round(rec["posterior_kernels_ms"]["median"] / rec[other + "_ms"]["median"], 4)
        if budget_gib and B * R > grid:  # the same kernels with a budget that pays for more slots than the default's
            dec.set_posterior_scratch(int(budget_gib * 2 ** 30))
            timed(posterior_kernels)
            rec["at_budget_gib_%g" % budget_gib] = dict(posterior_kernels_ms=med([timed(posterior_kernels) for _ in range(reps)]), grid=dec.last_posterior_grid())
            dec.set_posterior_scratch(0)
        out["R_%d" % R] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--budget-gib", type=float, default=0.0, help="also time the kernels with set_posterior_scratch at this many GiB, where the default binds the grid")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posteriors.json"))
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "method": " ".join(__doc__.split("\n\n")[2].split())}
    for w in WORKLOADS:
        if only and w["name"] not in only:
            continue
        res[w["name"]] = {}
        for kind in KINDS:
            res[w["name"]][kind] = probe(w, kind, a.reps, a.budget_gib)
            print(w["name"], kind, json.dumps(res[w["name"]][kind]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
