#!/usr/bin/env python3
"""bf16 input, two routes, one process, interleaved: TODAY's (x.float() on the device, then the float32 decode) against the NATIVE one
(the bf16 tensor handed to the library: the pre-pass kernels widen in registers), outputs compared bit for bit.  Per route: the cast
(device events around x.float()), the prune fast pass (ctcd_last_prune_ms), the replay of the flagged frames behind it
(ctcd_last_resolve_ms: prune_resolve_kernel), the decode kernel (ctcd_last_kernel_ms), the rest of the call (memsets, launch gaps), the
flagged-frame count and the peak torch allocation over the call.  Shapes: BASELINE.json configs[3] (B=64, T=500, V=10000, beam 100, cutoff_top_n 40) with log-probabilities
and with logits at cutoff_prob 0.99 and 0.5; configs[1] (B=256, T=1000, V=29, beam 100) with log-probabilities.  The bf16 rows are a
seeded float32 source put through log_softmax in float32 (or left as logits) and rounded.
    python tools/half_input_probe.py [--reps 5] [--out profiles/half_input_probe.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import ctcdecode_amd
import ctcdecode_amd._native as n


def one(dec, x, native):
    """One timed call; returns (outputs on the host, timings)."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ev[0].record()
    y = x if native else x.float()
    ev[1].record()
    out = dec.decode_device(y, check=False)
    ev[2].record()
    torch.cuda.synchronize()
    n.check(n.lib.ctcd_check_status(dec._handle, x.shape[0]))
    pruned = dec.cutoff_top_n < x.shape[2]
    t = dict(cast_ms=ev[0].elapsed_time(ev[1]), call_ms=ev[1].elapsed_time(ev[2]), prune_fast_ms=dec.last_prune_ms() if pruned else 0.0,
             resolve_ms=dec.last_resolve_ms() if pruned else 0.0, decode_kernel_ms=dec.last_kernel_ms(), flagged=int(n.lib.ctcd_last_prune_flagged_rows(dec._handle)),
             peak_alloc_mb=(torch.cuda.max_memory_allocated() - base) / 2**20, input_dtype=int(n.lib.ctcd_last_input_dtype(dec._handle)))
    t["rest_ms"] = t["call_ms"] - t["prune_fast_ms"] - t["resolve_ms"] - t["decode_kernel_ms"]
    t["total_ms"] = t["cast_ms"] + t["call_ms"]
    del y
    return [o.cpu().numpy() for o in out], t


def shape(name, B, T, V, K, top_n, cp, kind, reps):
    g = torch.Generator().manual_seed(3)
    src = torch.randn((B, T, V), generator=g)
    if kind == "logp":
        src = src.log_softmax(-1)
    x = src.to(torch.bfloat16).cuda()
    del src
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], cutoff_top_n=top_n, cutoff_prob=cp, beam_width=K, log_probs_input=kind == "logp",
                                       logits_input=kind == "logits", device="cuda:0")
    dec.set_timing(True)
    runs = {"today": [], "native": []}
    outs = {}
    for r in range(reps + 1):  # (today's route first in every round; round 0 is the warm-up)
        for route in ("today", "native"):
            o, t = one(dec, x, route == "native")
            outs[route] = o
            if r:
                runs[route].append(t)
    same = all((a.view("int32") == b.view("int32")).all() if a.dtype.kind == "f" else (a == b).all() for a, b in zip(outs["today"], outs["native"]))
    res = {"shape": dict(B=B, T=T, V=V, beam=K, cutoff_top_n=top_n, cutoff_prob=cp, input=kind + " bf16"), "identical": bool(same)}
    for route, ts in runs.items():
        res[route] = {k: (round(statistics.median([t[k] for t in ts]), 4) if isinstance(ts[0][k], float) else ts[0][k]) for k in ts[0]}
    res["native_total_below_today_by_ms"] = round(res["today"]["total_ms"] - res["native"]["total_ms"], 4)
    print(name, json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="configs[3] log-probabilities at 0.99 only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    plan = [("configs[3] logp 0.99", 64, 500, 10000, 100, 40, 0.99, "logp")]
    if not a.quick:
        plan += [("configs[3] logp 0.5", 64, 500, 10000, 100, 40, 0.5, "logp"), ("configs[3] logits 0.99", 64, 500, 10000, 100, 40, 0.99, "logits"),
                 ("configs[3] logits 0.5", 64, 500, 10000, 100, 40, 0.5, "logits"), ("configs[1] logp", 256, 1000, 29, 100, 29, 1.0, "logp")]
    out = {name: shape(name, *args, reps=a.reps) for name, *args in plan}
    out["device"] = torch.cuda.get_device_name(0)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
