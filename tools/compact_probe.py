#!/usr/bin/env python3
"""What compacting live streams costs and saves (OnlineCTCBeamDecoder.compact / the ctc_stream_compact_* kernels):
python tools/compact_probe.py [--out profiles/stream_compact.json]

256 streams, 29 labels, beam 100, fed 50 frames at a time (the README's streaming row).
(a) At stream ages 250, 1000 and 4000 frames: one compact() of all streams -- the FIRST one at that age (the pools are full of dead
    nodes: one sample) and 30 repeats directly after it (the same live set out of an already compact pool) -- as device time (HIP events
    around the call, the host's sizing step between its kernels included) and wall time, next to the live nodes per stream and to
    the same session's 50-frame chunk calls.
(b) A 20 000-frame run with compact_pool_above=1 against the same run without it, interleaved in one session: wall time per frame.
(c) The peak of the streams' summed ctcd_stream_bytes in both runs."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import ctcdecode_amd

B, V, K, CHUNK = 256, 29, 100, 50
AGES = (250, 1000, 4000)
REPS = 30
LONG_T, LONG_BLOCK, LONG_PAIRS = 20000, 2000, 3


def inputs(kind, seed, T):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    if kind == "blank_dominated":
        x[:, :, 0] += np.float32(4.0)
    return torch.from_numpy(x).log_softmax(-1)


def mm(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4), n=len(v))


def timed(fn):
    """-> (device ms between two events around fn, wall ms)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3


def ages(kind, seed, dev):
    T = max(AGES)
    lp = inputs(kind, seed, T).to(dev)
    rows, chunk_ms = [], []
    # a fresh set of streams per age: the first compaction at that age meets pools nobody has compacted
    for age in AGES:
        dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device=dev)
        states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
        for c in range(age // CHUNK):
            d, _ = timed(lambda: dec.decode(lp[:, c * CHUNK:(c + 1) * CHUNK], states, [False] * B, check=False))
            if age == max(AGES) and c > 0 and (c + 1) * CHUNK not in (1050, 2050):  # (not the calls that double the pools)
                chunk_ms.append(d)
        before = sum(s.nbytes for s in states)
        live = []
        first = timed(lambda: live.extend(dec.compact(states)))
        rep = [timed(lambda: dec.compact(states)) for _ in range(REPS)]
        rows.append(dict(input=kind, age=age, live_nodes_per_stream=mm(live), pool_bound_before=age * K + 1,
                         first_compact_device_ms=round(first[0], 4), first_compact_wall_ms=round(first[1], 4),
                         repeat_compact_device_ms=mm([r[0] for r in rep]), repeat_compact_wall_ms=mm([r[1] for r in rep]),
                         bytes_before=before, bytes_after=sum(s.nbytes for s in states)))
        del states, dec
    return rows, dict(input=kind, chunk_call_device_ms=mm(chunk_ms))


def long_run(lp, dev, above):
    dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device=dev,
                                             compact_pool_above=above)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    peak = 0
    per_block = LONG_BLOCK // CHUNK
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for c in range(LONG_T // CHUNK):
        lo = (c % per_block) * CHUNK
        dec.decode(lp[:, lo:lo + CHUNK], states, [False] * B, check=False)
        if c % 20 == 19:
            peak = max(peak, sum(s.nbytes for s in states))
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    peak = max(peak, sum(s.nbytes for s in states))
    return wall * 1e6 / LONG_T, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_compact.json"))
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    table, chunks, longs = [], [], []
    for i, kind in enumerate(("random", "blank_dominated")):
        rows, ch = ages(kind, 5321 + i, dev)
        table += rows
        chunks.append(ch)
    def dump():
        out = dict(what="256 streams, V 29, beam 100, 50-frame chunks; compact() of all streams", device=torch.cuda.get_device_name(0), reps=REPS,
                   compactions=table, same_session_chunk_calls=chunks, long_runs=longs)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)

    dump()  # (the long runs take most of the time: what is measured so far is on disk before they start)
    if not args.skip_long:
        for i, kind in enumerate(("random", "blank_dominated")):
            lp = inputs(kind, 6321 + i, LONG_BLOCK).to(dev)  # (the run feeds this block of frames ten times over)
            on, off, peak_on, peak_off = [], [], 0, 0
            for _ in range(LONG_PAIRS):
                us, pk = long_run(lp, dev, 1)
                on.append(us)
                peak_on = max(peak_on, pk)
                us, pk = long_run(lp, dev, None)
                off.append(us)
                peak_off = max(peak_off, pk)
            longs.append(dict(input=kind, frames=LONG_T, wall_us_per_frame_policy_on=mm(on), wall_us_per_frame_policy_off=mm(off),
                              peak_stream_bytes_policy_on=peak_on, peak_stream_bytes_policy_off=peak_off))
            dump()
    for r in table:
        print("%-16s age %4d live %s first %.3f / %.3f ms (device / wall)  repeat device %s wall %s  bytes %d -> %d" % (
            r["input"], r["age"], r["live_nodes_per_stream"], r["first_compact_device_ms"], r["first_compact_wall_ms"], r["repeat_compact_device_ms"],
            r["repeat_compact_wall_ms"], r["bytes_before"], r["bytes_after"]))
    print(json.dumps(chunks))
    print(json.dumps(longs))


if __name__ == "__main__":
    main()
