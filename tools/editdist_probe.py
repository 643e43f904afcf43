#!/usr/bin/env python3
"""What ``CTCBeamDecoder.edit_distance`` costs at the north-star shape, in one process, medians.

    python tools/editdist_probe.py [--reps N] [--out profiles/editdist.json]

Rows: B 256 items of R 100 rows, L = T = 1000, V 29.  "transcript": the rows of an item are edits of one base row of 230 .. 270 labels
(one label in twenty redrawn, dropped or doubled), as the rows of a beam are; "random": independent rows of 250 .. 900 random labels.
Per kind: the kernel between two HIP events (ctcd_edit_distance into a tensor allocated beforehand) for 1 / 10 / 100 rows against one
reference per item, and pairwise over 10 and 100 rows; the pairs per second and the DP cells per second that follow; the whole
edit_distance() call (wall time between synchronisations: allocation and the status read included); ``mbr_select`` on 100 rows.  For
scale: ``log_likelihood`` of the same transcript rows against random log-probability rows (wall time), and the numpy dynamic programme
of tests/editdist_util.py on one pair.  Before anything is timed, sampled pairs of every launch are compared with the host twin
(tests/native/editdist_host.cpp)."""
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

import editdist_util as eu  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

B, R, L, V = 256, 100, 1000, 29


def make_rows(kind, rng):
    x = np.zeros((B, R + 1, L), np.int32)  # (row R: the item's reference)
    lens = np.zeros((B, R + 1), np.int32)
    for b in range(B):
        base = rng.integers(1, V, int(rng.integers(230, 271)))
        for i in range(R + 1):
            if kind == "random":
                row = rng.integers(1, V, int(rng.integers(250, 901)))
            else:
                u = rng.random(len(base))
                row = np.where(u < 0.02, rng.integers(1, V, len(base)), base)
                row = np.repeat(row, np.where(u > 0.985, 2, np.where(u > 0.97, 0, 1)))
            x[b, i, :len(row)], lens[b, i] = row, len(row)
    return x, lens


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


def sampled_equal(D, x, xl, y, yl, rng, n=24):
    """n sampled entries of D against the host twin."""
    D = D.cpu().numpy()
    ok = True
    for _ in range(n):
        b, i, j = int(rng.integers(D.shape[0])), int(rng.integers(D.shape[1])), int(rng.integers(D.shape[2]))
        want = eu.host_pair(x[b, i, :xl[b, i]], y[b, j, :yl[b, j]])
        if D[b, i, j] != want:
            print("MISMATCH", (b, i, j), int(D[b, i, j]), want, flush=True)
            ok = False
    return ok


def probe_kind(dec, kind, reps, rng):
    x_np, lens_np = make_rows(kind, rng)
    rows, lens = torch.from_numpy(x_np).cuda(), torch.from_numpy(lens_np).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    rec = dict(labels=dict(min=int(lens_np.min()), median=float(np.median(lens_np)), max=int(lens_np.max())))
    ref, ref_lens = rows[:, R:].contiguous(), lens[:, R:].contiguous()
    for r in (1, 10, 100):
        for pairwise in (False, True):
            if pairwise and r == 1:
                continue
            x, xl = rows[:, :r].contiguous(), lens[:, :r].contiguous()
            q = r if pairwise else 1
            out = torch.empty((B, r, q), dtype=torch.int32, device="cuda")
            D = dec.edit_distance(x, xl) if pairwise else dec.edit_distance(x, xl, ref, ref_lens)
            same = sampled_equal(D, x_np[:, :r], lens_np[:, :r], x_np[:, :r] if pairwise else x_np[:, R:], lens_np[:, :r] if pairwise else lens_np[:, R:], rng)

            def kernel():
                _native.check(_native.lib.ctcd_edit_distance(dec._handle, x.data_ptr(), xl.data_ptr(), B, r, L, None if pairwise else ref.data_ptr(),
                                                             None if pairwise else ref_lens.data_ptr(), q, L, out.data_ptr(), None, stream))

            def call():
                return dec.edit_distance(x, xl) if pairwise else dec.edit_distance(x, xl, ref, ref_lens)

            tk, tc = [], []
            for k in range(reps + 1):  # (the first pass is not counted)
                a, c = timed(kernel), wall(call)
                if k:
                    tk.append(a), tc.append(c)
            pairs = dec.last_edit_pairs()
            ln = lens_np[:, :r].astype(np.int64)
            if pairwise:
                cells = int(sum(int(ln[b, i]) * int(ln[b, i + 1:].sum()) for b in range(B) for i in range(r)))
            else:
                cells = int((ln * lens_np[:, R:].astype(np.int64)).sum())
            e = dict(equals_host_twin_on_sampled_pairs=bool(same), pairs=pairs, cells=cells, kernel_ms=med(tk), call_ms=med(tc))
            e["pairs_per_s"] = round(pairs / (e["kernel_ms"]["median"] * 1e-3))
            e["gcells_per_s"] = round(cells / (e["kernel_ms"]["median"] * 1e-3) / 1e9, 2)
            rec["%s_%d" % ("pairwise" if pairwise else "rows_vs_reference", r)] = e
            print(kind, "pairwise" if pairwise else "vs_reference", r, json.dumps(e), flush=True)
    x, xl = rows[:, :R].contiguous(), lens[:, :R].contiguous()
    lw = torch.from_numpy(-10.0 * rng.random((B, R))).cuda()
    rec["mbr_select_100_call_ms"] = med([wall(lambda: dec.mbr_select(x, xl, lw)) for _ in range(reps + 1)][1:])
    if kind == "transcript":
        g = torch.Generator(device="cuda").manual_seed(1234)
        lp = torch.randn((B, L, V), generator=g, device="cuda").log_softmax(-1)
        rec["log_likelihood_100_call_ms"] = med([wall(lambda: dec.log_likelihood(lp, None, x, xl)) for _ in range(reps + 1)][1:])
    a, b = x_np[0, 0, :lens_np[0, 0]], x_np[0, 1, :lens_np[0, 1]]
    t0 = time.perf_counter()
    d = eu.lev(a, b)
    rec["numpy_one_pair_ms"] = dict(ms=round((time.perf_counter() - t0) * 1e3, 3), lengths=[len(a), len(b)], distance=d)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "editdist.json"))
    a = ap.parse_args()
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=R, log_probs_input=True, device="cuda:0")
    rng = np.random.default_rng(20241021)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "shape": dict(B=B, R=R, L=L, V=V), "method": " ".join(__doc__.split("\n\n")[2].split())}
    for kind in ("transcript", "random"):
        res[kind] = probe_kind(dec, kind, a.reps, rng)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
