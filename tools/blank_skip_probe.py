#!/usr/bin/env python3
"""What the blank-frame filter (CTCBeamDecoder(blank_skip=thr)) costs and saves: off against thr = 0.999 / 0.99 / 0.9, interleaved in
one process, HIP events, medians.

    python tools/blank_skip_probe.py [--reps N] [--only NAME[,NAME]] [--no-gather] [--out profiles/blank_skip.json]

Shapes: the north-star shape (B 256, T 1000, V 29, beam 100) and configs[4]'s per-GPU shape (B 128, T 1500, V 29, beam 100, no LM).
Rows: blank-dominated (+6 on the blank logit), transcript-like (bench.synth_transcript_rows over tests/data/test.arpa's words) and
random (log-softmax of N(0,1) logits: nothing to skip -- the filter costs a copy and saves nothing).
Per (shape, rows, setting): the kept share; the filter's own time (skip_blank_frames between two events), split into the scan -- the
same call with a bound every frame exceeds, whose gather workgroups leave at once -- and the gather (the difference); the decode
kernel's time (set_timing); the whole decode_device call and the whole decode() call (wall time between synchronisations), and the
decode_device call again with length order.  Before anything is timed, decode_device and decode() with the filter on are compared bit
for bit, and length order with batch order.
The gather alone at configs[3]'s shape (B 64, T 500, V 10000: 1.28 GB of float32 rows, every row kept) in float32 and bfloat16: GB/s
read + written, to set next to the 8 TB/s roofline and the prune pass's 4.5 TB/s."""
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

SHAPES = [dict(name="north_star", B=256, T=1000, V=29, K=100), dict(name="cfg4_per_gpu", B=128, T=1500, V=29, K=100)]
KINDS = ["blank", "transcript", "random"]
SETTINGS = [None, 0.999, 0.99, 0.9]
LABELS29 = ["_", "'", " "] + [chr(ord("a") + i) for i in range(26)]


def rows(kind, B, T, V, seed):
    if kind == "transcript":
        arpa = os.path.join(ROOT, "tests", "data", "test.arpa")
        return bench.synth_transcript_rows(torch, B, T, LABELS29, bench.arpa_unigrams(arpa), seed).cuda().contiguous()
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((B, T, V), generator=g, device="cuda")
    if kind == "blank":
        x[:, :, 0] += 6.0
    return x.log_softmax(-1).contiguous()


def med(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 4), min=round(xs[0], 4), max=round(xs[-1], 4), n=len(xs))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def same_bits(a, b):
    for u, v in zip(a, b):
        u, v = u.cpu().numpy(), v.cpu().numpy()
        if u.dtype == np.float32:
            u, v = u.view(np.uint32), v.view(np.uint32)
        if not np.array_equal(u, v):
            return False
    return True


def make(V, K, thr):
    dec = ctcdecode_amd.CTCBeamDecoder(LABELS29 if V == 29 else [str(i) for i in range(V)], beam_width=K, cutoff_top_n=V, log_probs_input=True,
                                       device="cuda:0", blank_skip=thr)
    dec.set_timing(True)
    return dec


def probe(shape, kind, reps):
    B, T, V, K = shape["B"], shape["T"], shape["V"], shape["K"]
    x = rows(kind, B, T, V, 1234)
    decs = {thr: make(V, K, thr) for thr in SETTINGS}
    scan_only = make(V, K, 1e-30)  # log(1e-30) is below every log-probability these rows hold: every frame is skipped
    out = {}
    for thr, dec in decs.items():  # warm-up, and the comparisons
        a = dec.decode_device(x)
        rec = {"decode_equals_decode_device": same_bits(a, dec.decode(x))}
        dec.set_launch_order("length")
        rec["length_order_equals_batch_order"] = same_bits(a, dec.decode_device(x))
        dec.set_launch_order("batch")
        if thr is not None:
            considered, kept = dec.last_blank_skip()
            rec["kept_share"] = round(kept / max(considered, 1), 4)
        out[thr] = rec
        del a
    scan_only.skip_blank_frames(x)
    assert scan_only.last_blank_skip()[1] == 0
    t = {thr: dict(filter=[], scan=[], kernel=[], device_call=[], device_call_length=[], host_call=[]) for thr in SETTINGS}
    for _ in range(reps):
        for thr, dec in decs.items():
            if thr is not None:
                t[thr]["filter"].append(event_ms(lambda: dec.skip_blank_frames(x))[0])
                t[thr]["scan"].append(event_ms(lambda: scan_only.skip_blank_frames(x))[0])
            t[thr]["device_call"].append(wall_ms(lambda: dec.decode_device(x))[0])
            t[thr]["kernel"].append(dec.last_kernel_ms())
            dec.set_launch_order("length")
            t[thr]["device_call_length"].append(wall_ms(lambda: dec.decode_device(x))[0])
            dec.set_launch_order("batch")
            t[thr]["host_call"].append(wall_ms(lambda: dec.decode(x))[0])
    for thr in SETTINGS:
        rec = out[thr]
        for k, v in t[thr].items():
            if v:
                rec[k + "_ms"] = med(v)
        if thr is not None:
            rec["gather_ms_median"] = round(rec["filter_ms"]["median"] - rec["scan_ms"]["median"], 4)
            off = out[None]
            rec["decode_kernel_saved_ms"] = round(off["kernel_ms"]["median"] - rec["kernel_ms"]["median"], 4)
            rec["device_call_saved_ms"] = round(off["device_call_ms"]["median"] - rec["device_call_ms"]["median"], 4)
    return {"off" if k is None else "thr_%g" % k: v for k, v in out.items()}


def gather_probe(reps):
    """Every row kept (random rows, thr 0.999): the gather moves the whole input once in, once out."""
    B, T, V = 64, 500, 10000
    res = {}
    for name, dtype in (("float32", torch.float32), ("bfloat16", torch.bfloat16)):
        g = torch.Generator(device="cuda").manual_seed(7)
        x = torch.empty((B, T, V), dtype=dtype, device="cuda")
        for b in range(B):
            x[b] = torch.randn((T, V), generator=g, device="cuda").log_softmax(-1).to(dtype)
        dec = make(V, 8, 0.999)
        scan_only = make(V, 8, 1e-30)
        dec.skip_blank_frames(x)
        considered, kept = dec.last_blank_skip()
        scan_only.skip_blank_frames(x)
        f, s = [], []
        for _ in range(reps):
            f.append(event_ms(lambda: dec.skip_blank_frames(x))[0])
            s.append(event_ms(lambda: scan_only.skip_blank_frames(x))[0])
        gms = statistics.median(f) - statistics.median(s)
        nbytes = kept * V * x.element_size()
        res[name] = dict(kept_share=round(kept / considered, 4), bytes_in=nbytes, filter_ms=med(f), scan_ms=med(s), gather_ms_median=round(gms, 4),
                         gather_GBps_read_plus_written=round(2 * nbytes / (gms * 1e-3) / 1e9, 1))
        del x
    res["note"] = ("filter_ms includes the allocation of the filtered copy by the caching allocator; roofline 8000 GB/s, the prune pass of configs[3] "
                   "reads at about 4500 GB/s")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blank_skip.json"))
    a = ap.parse_args()
    only = [s for s in a.only.split(",") if s]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "method": __doc__.split("\n\n")[2]}
    for shape in SHAPES:
        if only and shape["name"] not in only:
            continue
        for kind in KINDS:
            key = "%s/%s" % (shape["name"], kind)
            res[key] = probe(shape, kind, a.reps)
            print(key, json.dumps(res[key]), flush=True)
    if not a.no_gather and not only:
        res["cfg3_gather"] = gather_probe(a.reps)
        print("cfg3_gather", json.dumps(res["cfg3_gather"]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
