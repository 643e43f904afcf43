#!/usr/bin/env python3
"""Launch order on ragged batches: batch order against length order (ctcd_set_launch_order), interleaved A B A B in one process.

    python tools/ragged_probe.py [--reps N] [--only NAME[,NAME]] [--out profiles/ragged_order.json]
    python tools/ragged_probe.py --order-pass     (tiny decodes at B = 1024 / 16384 / 20000 for a kernel trace of the order pass alone)

Per shape: one decoder, the same rows and lengths for both orders; the outputs of the two orders are compared bit for bit (scores as
uint32) before anything is timed.  Each rep times one launch per order: the kernel time (set_timing / last_kernel_ms; with length order
it includes the order pass) and the wall time of decode_device between two synchronisations.  Shapes: configs[1]'s class (T 1000,
V 29, beam 100) at B 256 / 1024 / 2048 with equal lengths and with lengths uniform in [T/4, T] (fixed seed); the wide-beam class
(beam 500, T 2000) at B 512, ragged; configs[3]'s pruned class (V 10000, cutoff_top_n 40, cutoff_prob 0.99, beam 100, T 500) at
B 1024, ragged."""
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

import ctcdecode_amd  # noqa: E402

SHAPES = [
    dict(name="cfg1_B256_equal", B=256, T=1000, V=29, K=100, ragged=False),
    dict(name="cfg1_B256_ragged", B=256, T=1000, V=29, K=100, ragged=True),
    dict(name="cfg1_B1024_equal", B=1024, T=1000, V=29, K=100, ragged=False),
    dict(name="cfg1_B1024_ragged", B=1024, T=1000, V=29, K=100, ragged=True),
    dict(name="cfg1_B2048_equal", B=2048, T=1000, V=29, K=100, ragged=False),
    dict(name="cfg1_B2048_ragged", B=2048, T=1000, V=29, K=100, ragged=True),
    dict(name="wide_B512_ragged", B=512, T=2000, V=29, K=500, ragged=True, reps=3),
    dict(name="cfg3_B1024_ragged", B=1024, T=500, V=10000, K=100, top_n=40, cutoff_prob=0.99, ragged=True),
]


def rows(B, T, V, seed):
    """log_softmax of N(0, 1) logits, made on the device in slices (configs[3]'s class is 20 GB of rows)."""
    out = torch.empty((B, T, V), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(seed)
    step = max(1, (1 << 28) // (T * V))
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        out[b0:b1] = torch.randn((b1 - b0, T, V), generator=g, device="cuda").log_softmax(-1)
    return out


def lengths(B, T, ragged, seed):
    if not ragged:
        return np.full((B,), T, np.int32)
    return np.random.default_rng(seed).integers(T // 4, T + 1, size=B).astype(np.int32)


def same_bits(a, b):
    for u, v in zip(a, b):
        u, v = u.cpu().numpy(), v.cpu().numpy()
        if u.dtype == np.float32:
            u, v = u.view(np.uint32), v.view(np.uint32)
        if not np.array_equal(u, v):
            return False
    return True


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 4), min=round(xs[0], 4), max=round(xs[-1], 4), n=len(xs))


def probe(shape, reps):
    B, T, V, K = shape["B"], shape["T"], shape["V"], shape["K"]
    probs = rows(B, T, V, 1234)
    lens = lengths(B, T, shape["ragged"], 4321)
    sl = torch.from_numpy(lens).cuda()
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=K, cutoff_top_n=shape.get("top_n", 40),
                                       cutoff_prob=shape.get("cutoff_prob", 1.0), log_probs_input=True, device="cuda:0")
    dec.set_timing(True)
    outs = {}
    for mode in ("batch", "length"):  # warm-up launch of each order, checked, and the outputs kept for the comparison
        dec.set_launch_order(mode)
        outs[mode] = dec.decode_device(probs, sl)
    identical = same_bits(outs["batch"], outs["length"])
    order = dec.last_launch_order()
    del outs
    kern = {"batch": [], "length": []}
    wall = {"batch": [], "length": []}
    for _ in range(reps):
        for mode in ("batch", "length"):
            dec.set_launch_order(mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dec.decode_device(probs, sl, check=False)
            torch.cuda.synchronize()
            wall[mode].append(1e3 * (time.perf_counter() - t0))
            kern[mode].append(dec.last_kernel_ms())
    res = dict(shape={k: v for k, v in shape.items() if k != "reps"}, layout=dec.last_layout(), bit_identical=identical,
               order_nontrivial=bool(order is not None and not np.array_equal(order, np.arange(B))),
               frames=int(lens.sum()), kernel_ms={m: stats(v) for m, v in kern.items()}, wall_ms={m: stats(v) for m, v in wall.items()})
    mb, ml = res["wall_ms"]["batch"]["median"], res["wall_ms"]["length"]["median"]
    res["utt_per_s"] = {"batch": round(B / mb * 1e3, 1), "length": round(B / ml * 1e3, 1)}
    res["speedup_wall"] = round(mb / ml, 3)
    res["speedup_kernel"] = round(res["kernel_ms"]["batch"]["median"] / res["kernel_ms"]["length"]["median"], 3)
    # (the runs of each order spread over this range; a gain inside the other order's range is not a gain)
    res["spread_wall_pct"] = {m: round(100.0 * (s["max"] - s["min"]) / s["median"], 2) for m, s in res["wall_ms"].items()}
    del probs
    torch.cuda.empty_cache()
    return res


def order_pass():
    """Tiny decodes (T 4, V 3, beam 1) under length order: what a kernel trace of this process shows for launch_order_*_kernel."""
    for B in (1024, 16384, 20000):
        probs = rows(B, 4, 3, 5)
        sl = torch.from_numpy(np.random.default_rng(B).integers(0, 5, size=B).astype(np.int32)).cuda()
        dec = ctcdecode_amd.CTCBeamDecoder(["_", "a", "b"], beam_width=1, log_probs_input=True, device="cuda:0")
        dec.set_launch_order("length")
        for _ in range(20):
            dec.decode_device(probs, sl, check=False)
        dec.decode_device(probs, sl)
        print("order pass: B=%d done" % B, flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_order.json"))
    ap.add_argument("--order-pass", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    if a.order_pass:
        order_pass()
        return
    want = set(a.only.split(",")) if a.only else None
    results = []
    print("%-20s %6s %5s %12s %12s %8s %12s %12s %8s %s" % ("shape", "layout", "bits", "batch ms", "length ms", "x wall", "batch kern", "length kern",
                                                          "x kern", "spread % (b/l)"))
    for s in SHAPES:
        if want and s["name"] not in want:
            continue
        r = probe(s, s.get("reps", a.reps))
        results.append(r)
        print("%-20s %6d %5s %12.3f %12.3f %8.3f %12.3f %12.3f %8.3f %s / %s" % (
            s["name"], r["layout"], "same" if r["bit_identical"] else "DIFF", r["wall_ms"]["batch"]["median"], r["wall_ms"]["length"]["median"],
            r["speedup_wall"], r["kernel_ms"]["batch"]["median"], r["kernel_ms"]["length"]["median"], r["speedup_kernel"],
            r["spread_wall_pct"]["batch"], r["spread_wall_pct"]["length"]), flush=True)
    doc = dict(tool="tools/ragged_probe.py", device=torch.cuda.get_device_name(0), reps=a.reps, results=results)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)
    if not all(r["bit_identical"] for r in results):
        sys.exit("the two orders' outputs differ")


if __name__ == "__main__":
    main()
