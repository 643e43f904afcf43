#!/usr/bin/env python3
"""What ``n_best`` saves on the one-shot routes: n_best None against 1 and 10, interleaved in one process, medians.

    python tools/nbest_probe.py [--reps N] [--only NAME[,NAME]] [--out profiles/nbest.json]

Workloads: the north-star shape (B 256, T 1000, V 29, beam 100, random rows), configs[3]'s shape (B 64, T 500, V 10000, beam 100,
cutoff_top_n 40, cutoff_prob 0.99) and configs[4]'s per-GPU shape (B 128, T 1500, V 29, beam 100) with the built-in scorer over
tests/data/test.arpa on transcript-like rows.
Per (workload, setting): the whole decode() call and the whole decode_device call (wall time between synchronisations, input in HBM),
the decode kernel's own time (set_timing), the peak of torch's device allocations over one decode_device call, and the bytes of the
page-locked result tensors decode() allocates.  On the records of one decode_compact call: the n-best expansion kernel between two HIP
events (ctcd_expand_compact_nbest, no status word) next to expand_compact_kernel (ctcd_expand_compact) into tensors allocated
beforehand.  Before anything is timed every n-best result is compared bit for bit with rows [:, :n] of the full call's."""
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

import bench  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

LABELS29 = ["_", "'", " "] + [chr(ord("a") + i) for i in range(26)]
ARPA = os.path.join(ROOT, "tests", "data", "test.arpa")
WORKLOADS = [dict(name="north_star", B=256, T=1000, V=29, K=100),
             dict(name="cfg3", B=64, T=500, V=10000, K=100, kw=dict(cutoff_top_n=40, cutoff_prob=0.99)),
             dict(name="cfg4_per_gpu_lm", B=128, T=1500, V=29, K=100, lm=True)]
SETTINGS = [None, 1, 10]


def rows(w):
    B, T, V = w["B"], w["T"], w["V"]
    if w.get("lm"):
        return bench.synth_transcript_rows(torch, B, T, LABELS29, bench.arpa_unigrams(ARPA), 1234).cuda().contiguous()
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.empty((B, T, V), device="cuda")
    for b in range(B):  # (row by row: the logits of configs[3] are 1.28 GB)
        x[b] = torch.randn((T, V), generator=g, device="cuda").log_softmax(-1)
    return x


def make(w):
    V = w["V"]
    kw = dict(beam_width=w["K"], cutoff_top_n=V, log_probs_input=True, device="cuda:0")
    kw.update(w.get("kw", {}))
    if w.get("lm"):
        kw.update(model_path=ARPA, alpha=0.5, beta=1.0)
    dec = ctcdecode_amd.CTCBeamDecoder(LABELS29 if V == 29 else [str(i) for i in range(V)], **kw)
    dec.set_timing(True)
    return dec


def med(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 4), min=round(xs[0], 4), max=round(xs[-1], 4), n=len(xs))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def same_slices(res, full, n):
    """rows [:, :n] of the full call on the region it defines, and zeros elsewhere"""
    out, sc, ts, ln = (t.cpu().numpy() for t in res)
    fout, fsc, fts, fln = (t.cpu().numpy()[:, :n] for t in full)
    if not (np.array_equal(ln, fln) and np.array_equal(sc.view(np.uint32), fsc.view(np.uint32))):
        return False
    mask = np.arange(out.shape[2])[None, None, :] < ln[:, :, None]
    return bool(np.array_equal(out * mask, fout * mask) and np.array_equal(ts * mask, fts * mask) and not (out * ~mask).any() and not (ts * ~mask).any())


def probe(w, reps):
    B, T, K = w["B"], w["T"], w["K"]
    x = rows(w)
    dec = make(w)
    full = dec.decode_device(x)
    out = {}
    for n in SETTINGS:  # warm-up, and the comparisons
        rec = {}
        if n is not None:
            rec["decode_device_equals_full_slices"] = same_slices(dec.decode_device(x, n_best=n), full, n)
            rec["decode_equals_full_slices"] = same_slices(dec.decode(x, n_best=n), full, n)
        else:
            dec.decode(x)
        R = K if n is None else n
        rec["page_locked_result_bytes"] = 2 * B * R * T * 4 + 2 * B * R * 4
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        dec.decode_device(x, n_best=n)
        torch.cuda.synchronize()
        rec["torch_peak_bytes_over_call"] = int(torch.cuda.max_memory_allocated() - base)
        out[n] = rec
    # the two expansion kernels on the same records
    hdr, ent, labels, _, _ = dec.decode_compact(x)
    stream = torch.cuda.current_stream().cuda_stream
    bufs = {n: (torch.empty((B, K if n is None else n, T), dtype=torch.int32, device="cuda"), torch.empty((B, K if n is None else n, T), dtype=torch.int32, device="cuda"))
            for n in SETTINGS}

    def expand(n):
        tok, ts = bufs[n]
        if n is None:
            _native.check(_native.lib.ctcd_expand_compact(dec._handle, hdr.data_ptr(), ent.data_ptr(), labels.data_ptr(), B, K, T, tok.data_ptr(), ts.data_ptr(), stream))
        else:
            _native.check(_native.lib.ctcd_expand_compact_nbest(dec._handle, hdr.data_ptr(), ent.data_ptr(), labels.data_ptr(), int(labels.numel()), B, K, T, n,
                                                                tok.data_ptr(), ts.data_ptr(), None, stream))

    for n in SETTINGS:
        expand(n)
    torch.cuda.synchronize()
    for n in SETTINGS[1:]:
        out[n]["expansion_equals_full_expansion_rows"] = bool(torch.equal(bufs[n][0], bufs[None][0][:, :n]) and torch.equal(bufs[n][1], bufs[None][1][:, :n]))
    t = {n: dict(host_call=[], device_call=[], kernel=[], expansion=[]) for n in SETTINGS}
    for _ in range(reps):
        for n in SETTINGS:
            t[n]["device_call"].append(wall_ms(lambda: dec.decode_device(x, n_best=n))[0])
            t[n]["kernel"].append(dec.last_kernel_ms())
            t[n]["host_call"].append(wall_ms(lambda: dec.decode(x, n_best=n))[0])
            t[n]["expansion"].append(event_ms(lambda: expand(n)))
    for n in SETTINGS:
        for k, v in t[n].items():
            out[n][k + "_ms"] = med(v)
    kern = out[None]["kernel_ms"]["median"]
    for n in SETTINGS:
        out[n]["host_call_over_decode_kernel_ms"] = round(out[n]["host_call_ms"]["median"] - kern, 4)
        out[n]["device_call_over_decode_kernel_ms"] = round(out[n]["device_call_ms"]["median"] - kern, 4)
        out[n]["expansion_share_of_full_expansion"] = round(out[n]["expansion_ms"]["median"] / out[None]["expansion_ms"]["median"], 4)
    return {"full" if n is None else "n_best_%d" % n: v for n, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nbest.json"))
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
