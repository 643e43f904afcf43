#!/usr/bin/env python3
"""What committing live streams' final labels costs (OnlineCTCBeamDecoder.commit / the ctc_stream_commit_* kernels):
python tools/commit_probe.py [--out profiles/stream_commit.json]

256 streams, 29 labels, beam 100, fed 50 frames at a time (the README's streaming row).  At stream ages 250, 1000 and 4000 frames, on
two sets of streams fed the same rows in the same session: one commit() of all streams of the one set -- the FIRST one at that age
(the pools are full of dead nodes and hold the whole trunk: one sample) -- next to one compact() of all streams of the other set, as
device time (HIP events around the call, the host's sizing step between its kernels included) and wall time; then REPS repeats of
each directly after (nothing new to commit: the same live set out of an already compact pool); the labels committed and the nodes
kept per stream, and the same session's 50-frame chunk calls.  No target: the comparison is compact() at the same age."""
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
REPS = 10


def inputs(kind, seed, T):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    if kind == "blank_dominated":
        x[:, :, 0] += np.float32(4.0)
    if kind == "transcript_like":  # a label or the blank dominates for a few frames, mostly with a sharp peak
        for b in range(B):
            t = 0
            while t < T:
                n = int(rng.integers(1, 6))
                c = 0 if rng.random() < 0.5 else int(rng.integers(0, V))
                x[b, t:t + n, c] += np.float32(1.0 if rng.random() < 0.4 else 20.0)
                t += n
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
    lp = inputs(kind, seed, max(AGES)).to(dev)
    rows, chunk_ms = [], []
    for age in AGES:  # fresh streams per age: the first call at that age meets pools nobody has touched
        dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device=dev)
        sets = [[ctcdecode_amd.DecoderState(dec) for _ in range(B)] for _ in range(2)]
        for c in range(age // CHUNK):
            for states in sets:
                d, _ = timed(lambda: dec.decode(lp[:, c * CHUNK:(c + 1) * CHUNK], states, [False] * B, check=False))
                if age == max(AGES) and c > 0 and (c + 1) * CHUNK not in (1050, 2050):  # (not the calls that double the pools)
                    chunk_ms.append(d)
        got, live = [], []
        before = [sum(s.nbytes for s in states) for states in sets]
        first_commit = timed(lambda: got.extend(dec.commit(sets[0])))
        first_compact = timed(lambda: live.extend(dec.compact(sets[1])))
        rep_commit = [timed(lambda: dec.commit(sets[0])) for _ in range(REPS)]
        rep_compact = [timed(lambda: dec.compact(sets[1])) for _ in range(REPS)]
        rows.append(dict(input=kind, age=age, labels_committed_per_stream=mm([len(t) for t, _ in got]),
                         nodes_kept_per_stream_commit=mm([s.pool_nodes for s in sets[0]]), nodes_kept_per_stream_compact=mm(live),
                         first_commit_device_ms=round(first_commit[0], 4), first_commit_wall_ms=round(first_commit[1], 4),
                         first_compact_device_ms=round(first_compact[0], 4), first_compact_wall_ms=round(first_compact[1], 4),
                         repeat_commit_device_ms=mm([r[0] for r in rep_commit]), repeat_commit_wall_ms=mm([r[1] for r in rep_commit]),
                         repeat_compact_device_ms=mm([r[0] for r in rep_compact]), repeat_compact_wall_ms=mm([r[1] for r in rep_compact]),
                         bytes_before=before, bytes_after=[sum(s.nbytes for s in states) for states in sets]))
        del sets, dec
    return rows, dict(input=kind, chunk_call_device_ms=mm(chunk_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_commit.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    table, chunks = [], []
    for i, kind in enumerate(("random", "blank_dominated", "transcript_like")):
        rows, ch = ages(kind, 7321 + i, dev)
        table += rows
        chunks.append(ch)
        out = dict(what="256 streams, V 29, beam 100, 50-frame chunks; commit() of all streams of one set next to compact() of all streams of a "
                        "second set fed the same rows; the commit runs first and pays the one allocation of the scratch buffer both calls share", device=torch.cuda.get_device_name(0), reps=REPS, commits=table, same_session_chunk_calls=chunks)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for r in table:
        print("%-16s age %4d committed %s  first commit %.3f / %.3f ms, first compact %.3f / %.3f ms (device / wall)  repeat commit %s compact %s" % (
            r["input"], r["age"], r["labels_committed_per_stream"], r["first_commit_device_ms"], r["first_commit_wall_ms"],
            r["first_compact_device_ms"], r["first_compact_wall_ms"], r["repeat_commit_device_ms"], r["repeat_compact_device_ms"]))
    print(json.dumps(chunks))


if __name__ == "__main__":
    main()
