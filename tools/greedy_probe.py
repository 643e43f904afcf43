#!/usr/bin/env python3
"""What ``CTCBeamDecoder.greedy_decode_device`` costs next to the beam route on the same rows, in one process, medians.

    python tools/greedy_probe.py [--reps N] [--only NAME[,NAME]] [--out profiles/greedy.json]

Workloads: the north-star shape (B 256, T 1000, V 29, beam 100) and configs[3]'s shape (B 64, T 500, V 10000, beam 100, cutoff_top_n
40, cutoff_prob 0.99); each as probabilities, log-probabilities and raw logits (log_input 0 / 1 / 2), float32 and bfloat16.
Per (workload, mode, dtype): the two greedy kernels between two HIP events (ctcd_greedy_decode into tensors allocated beforehand), the
bytes of the input over that time, the whole greedy_decode_device() call (wall time between synchronisations: allocations included),
and on the same rows the decode_device() call (wall time), its decode kernel and -- where the configuration prunes -- its prune pass
(set_timing; for raw logits the fused-logits prune), all alternated in one loop after one untimed pass.  Before anything is timed the
first and the last item are compared bit for bit with the host twin (tests/native/greedy_host.cpp)."""
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

import greedy_util as gu  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

WORKLOADS = [dict(name="north_star", B=256, T=1000, V=29, K=100),
             dict(name="cfg3", B=64, T=500, V=10000, K=100, kw=dict(cutoff_top_n=40, cutoff_prob=0.99))]
MODES = {0: "probabilities", 1: "log_probabilities", 2: "logits"}
DTYPES = {"float32": (torch.float32, 0), "bfloat16": (torch.bfloat16, 2)}


def rows_of(w, mode, dtype):
    """Transcript-like rows: three frames in four dominated by the blank, the others by one label."""
    B, T, V = w["B"], w["T"], w["V"]
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.empty((B, T, V), device="cuda", dtype=dtype)
    for b in range(B):  # (row by row: the logits of configs[3] are 1.28 GB)
        z = torch.randn((T, V), generator=g, device="cuda")
        top = torch.randint(1, V, (T,), generator=g, device="cuda")
        top[torch.rand((T,), generator=g, device="cuda") < 0.75] = 0
        z[torch.arange(T, device="cuda"), top] += 8.0
        x[b] = (z if mode == 2 else (z.log_softmax(-1) if mode == 1 else z.softmax(-1))).to(dtype)
    return x


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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def probe(w, mode, dtype_name, reps):
    B, T, V, K = w["B"], w["T"], w["V"], w["K"]
    dtype, code = DTYPES[dtype_name]
    x = rows_of(w, mode, dtype)
    kw = dict(beam_width=K, cutoff_top_n=V, log_probs_input=mode == 1, logits_input=mode == 2, device="cuda:0")
    kw.update(w.get("kw", {}))
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], **kw)
    dec.set_timing(True)
    stream = torch.cuda.current_stream().cuda_stream
    tok, sc, st, lens, en, ls = dec.greedy_decode_device(x, details=True)
    same = True
    for b in (0, B - 1):  # the first and the last item against the host twin
        xb = x[b:b + 1].cpu()
        stored = xb.numpy() if code == 0 else xb.view(torch.int16).numpy().view(np.uint16)
        want = gu.host_decode(stored, code, None, 0, mode)
        got = dict(tokens=tok[b:b + 1, 0].cpu().numpy(), starts=st[b:b + 1, 0].cpu().numpy(), ends=en[b:b + 1, 0].cpu().numpy(),
                   label_scores=ls[b:b + 1, 0].cpu().numpy(), scores=sc[b:b + 1, 0].cpu().numpy(), lens=lens[b:b + 1, 0].cpu().numpy())
        try:
            gu.assert_same(got, want, "item %d" % b)
        except AssertionError as e:
            print("MISMATCH", e, flush=True)
            same = False
    nbytes = x.numel() * x.element_size()
    rec = dict(equals_host_twin_on_sampled_items=bool(same), input_bytes=nbytes,
               labels=dict(min=int(lens.min()), median=float(lens.float().median()), max=int(lens.max())))

    def greedy_kernels():
        _native.check(_native.lib.ctcd_greedy_decode(dec._handle, x.data_ptr(), None, B, T, V, 0, mode, tok.data_ptr(), st.data_ptr(), en.data_ptr(), ls.data_ptr(),
                                                     sc.data_ptr(), lens.data_ptr(), stream))

    gk, gc, dc, dk, pk = [], [], [], [], []
    for i in range(reps + 1):  # (the first pass is not counted)
        t_gk = timed(greedy_kernels)
        t_gc = wall(lambda: dec.greedy_decode_device(x))
        t_dc = wall(lambda: dec.decode_device(x))
        if i:
            gk.append(t_gk), gc.append(t_gc), dc.append(t_dc), dk.append(dec.last_kernel_ms())
            try:
                pk.append(dec.last_prune_ms())
            except Exception:  # (no prune pass in this configuration)
                pass
    rec.update(greedy_kernels_ms=med(gk), greedy_call_ms=med(gc), decode_call_ms=med(dc), decode_kernel_ms=med(dk), prune_ms=med(pk) if pk else None)
    rec["greedy_kernels_input_TBps"] = round(nbytes / (rec["greedy_kernels_ms"]["median"] * 1e-3) / 1e12, 3)
    if pk:
        rec["prune_input_TBps"] = round(nbytes / (rec["prune_ms"]["median"] * 1e-3) / 1e12, 3)
        rec["greedy_kernels_over_prune"] = round(rec["greedy_kernels_ms"]["median"] / rec["prune_ms"]["median"], 4)
    rec["greedy_call_over_decode_call"] = round(rec["greedy_call_ms"]["median"] / rec["decode_call_ms"]["median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy.json"))
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "method": " ".join(__doc__.split("\n\n")[2].split())}
    for w in WORKLOADS:
        if only and w["name"] not in only:
            continue
        res[w["name"]] = {}
        for mode, mname in MODES.items():
            for dname in DTYPES:
                key = "%s_%s" % (mname, dname)
                res[w["name"]][key] = probe(w, mode, dname, a.reps)
                print(w["name"], key, json.dumps(res[w["name"]][key]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
