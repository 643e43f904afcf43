#!/usr/bin/env python3
"""What the long edit pairs (``CTCBeamDecoder.set_edit_long``) cost, in one process on one device, medians of ``--reps`` launches.

    python tools/editlong_probe.py [--reps 7] [--out profiles/edit_long.json]

Timed between two HIP events around the C entry point, outputs allocated beforehand, one warm-up launch per shape:
  * one pair of 30000 x 30000 tokens at 2 / 4 / 8 / 16 waves, distance and counts;
  * 64 pairs of 6000 x 6000, likewise;
  * the yardstick: the per-wave kernel (mode off) on pairs of 2048 x 30000 -- one pair, a wave alone on the device, and 2048 pairs, the
    usual grid full -- as cells per second per wave.
The long kernel's cells per second per wave (cells / time / waves of the workgroups at work) are reported as a ratio to the lone wave's:
what tiles, hand-offs and barriers cost.  Before anything is timed the 6000 x 6000 results are compared across the widths and, one pair,
with ``editdist_util.lev``."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import editdist_util as eu  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

WAVES = (2, 4, 8, 16)


def rows(rng, B, n, m):
    """B pairs over 4 symbols that share material (a tenth of the positions redrawn)."""
    src = rng.integers(0, 4, (B, max(n, m))).astype(np.int32)
    noisy = lambda k: np.where(rng.random((B, k)) < 0.1, rng.integers(0, 4, (B, k)), src[:, :k]).astype(np.int32)  # noqa: E731
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return dev(noisy(n)[:, None]), dev(np.full((B, 1), n, np.int32)), dev(noisy(m)[:, None]), dev(np.full((B, 1), m, np.int32))


def timed(dec, fn, t, words, reps):
    """-> (median ms, output) of fn over the tensors t."""
    x, xl, y, yl = t
    (B, R, L), (Q, Lq) = x.shape, y.shape[1:]
    out = torch.zeros((B, R, Q) + words, dtype=torch.int32, device="cuda")
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = []
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(dec._handle, x.data_ptr(), xl.data_ptr(), B, R, L, y.data_ptr(), yl.data_ptr(), Q, Lq, out.data_ptr(), st.data_ptr(), stream)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0 and not st.any(), _native.lib.ctcd_last_error()
        if k:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_long.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the device"
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(8)], blank_id=0, beam_width=16, log_probs_input=True)
    rng = np.random.default_rng(20261126)
    kernels = (("distance", _native.lib.ctcd_edit_distance, ()), ("counts", _native.lib.ctcd_edit_counts, (4,)))
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "unit": "ms, median", "long": [], "yardstick": []}
    # the yardstick first: the per-wave kernel, mode off
    for B in (1, 2048):
        t = rows(rng, B, 2048, 30000)
        for name, fn, words in kernels:
            ms, _ = timed(dec, fn, t, words, args.reps)
            res["yardstick"].append(dict(kernel=name, pairs=B, n=2048, m=30000, ms=ms, cells_per_s_per_wave=2048 * 30000 / (ms * 1e-3)))
    lone = {r["kernel"]: r["cells_per_s_per_wave"] for r in res["yardstick"] if r["pairs"] == 1}
    for B, n in ((1, 30000), (64, 6000)):
        t = rows(rng, B, n, n)
        first = {}
        for W in WAVES:
            dec.set_edit_long(W)
            for name, fn, words in kernels:
                ms, out = timed(dec, fn, t, words, args.reps)
                assert dec.last_edit_long() == B
                assert (first.setdefault(name, out) == out).all(), "the width changed a result"
                rate = B * n * n / (ms * 1e-3) / (W * min(B, dec.last_edit_slots()))
                res["long"].append(dict(kernel=name, pairs=B, n=n, m=n, waves=W, workgroups=dec.last_edit_slots(), ms=ms, cells_per_s=B * n * n / (ms * 1e-3),
                                        cells_per_s_per_wave=rate, ratio_to_lone_wave=rate / lone[name]))
        if n == 6000:
            a, b = t[0][0, 0].cpu().numpy(), t[2][0, 0].cpu().numpy()
            assert first["distance"][0, 0, 0] == eu.lev(a, b) == first["counts"][0, 0, 0, 1:].sum()
        dec.set_edit_long(0)
    single = [r for r in res["long"] if r["pairs"] == 1 and r["kernel"] == "distance"]
    res["fastest_waves_single_pair"] = min(single, key=lambda r: r["ms"])["waves"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    for r in res["yardstick"] + res["long"]:
        print(json.dumps(r))
    print("fastest on the single long pair: %d waves" % res["fastest_waves_single_pair"])


if __name__ == "__main__":
    main()
