#!/usr/bin/env python3
"""What taking live streams off the GPU and putting them back costs (OnlineCTCBeamDecoder.save / restore: the compaction, then
ctc_stream_export_kernel and one copy to the host / one copy from the host, then ctc_stream_import_kernel):
python tools/snapshot_probe.py [--out profiles/stream_snapshot.json]

256 streams, 29 labels, beam 100, fed 50 frames at a time (the README's streaming row).  At stream ages 250, 1000 and 4000 frames, on
two sets of streams fed the same rows in the same session: one save() of all streams of the one set -- the FIRST one at that age (the
pools are full of dead nodes: the save's compaction does the work a compact() would) -- next to one compact() of all streams of the
twin set, then one restore() of the images into a second decoder, as device time (HIP events around the call, the host's steps
between its kernels included) and wall time; then REPS repeats of each directly after (an already compact pool; the restored streams
of a repeat are dropped before the next); the image bytes per stream next to DecoderState.nbytes before the save.  No target: the
comparison is compact() at the same age."""
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
    rows = []
    for age in AGES:  # fresh streams per age: the first call at that age meets pools nobody has touched
        mk = lambda: ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device=dev)  # noqa: E731
        dec, dec2 = mk(), mk()
        sets = [[ctcdecode_amd.DecoderState(dec) for _ in range(B)] for _ in range(2)]
        for c in range(age // CHUNK):
            for states in sets:
                dec.decode(lp[:, c * CHUNK:(c + 1) * CHUNK], states, [False] * B, check=False)
        before = [s.nbytes for s in sets[0]]
        blobs, live, back = [], [], []
        first_save = timed(lambda: blobs.extend(dec.save(sets[0])))
        first_compact = timed(lambda: live.extend(dec.compact(sets[1])))
        first_restore = timed(lambda: back.extend(dec2.restore(blobs)))
        del back[:]
        rep_save = [timed(lambda: dec.save(sets[0])) for _ in range(REPS)]
        rep_compact = [timed(lambda: dec.compact(sets[1])) for _ in range(REPS)]
        rep_restore = []
        for _ in range(REPS):
            rep_restore.append(timed(lambda: back.extend(dec2.restore(blobs))))
            del back[:]
        rows.append(dict(input=kind, age=age, image_bytes_per_stream=mm([int(b.numel()) for b in blobs]), block_bytes_per_stream_before=mm(before),
                         block_bytes_per_stream_after=mm([s.nbytes for s in sets[0]]), nodes_kept_per_stream=mm(live),
                         first_save_device_ms=round(first_save[0], 4), first_save_wall_ms=round(first_save[1], 4),
                         first_compact_device_ms=round(first_compact[0], 4), first_compact_wall_ms=round(first_compact[1], 4),
                         first_restore_device_ms=round(first_restore[0], 4), first_restore_wall_ms=round(first_restore[1], 4),
                         repeat_save_device_ms=mm([r[0] for r in rep_save]), repeat_save_wall_ms=mm([r[1] for r in rep_save]),
                         repeat_compact_device_ms=mm([r[0] for r in rep_compact]), repeat_compact_wall_ms=mm([r[1] for r in rep_compact]),
                         repeat_restore_device_ms=mm([r[0] for r in rep_restore]), repeat_restore_wall_ms=mm([r[1] for r in rep_restore])))
        del sets, dec, dec2, blobs
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_snapshot.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    table = []
    for i, kind in enumerate(("random", "blank_dominated", "transcript_like")):
        table += ages(kind, 7321 + i, dev)
        out = dict(what="256 streams, V 29, beam 100, 50-frame chunks; save() of all streams of one set next to compact() of all streams of a "
                        "twin set fed the same rows, then restore() of the images into a second decoder; the save runs first and pays the one "
                        "allocation of the scratch buffer the calls share", device=torch.cuda.get_device_name(0), reps=REPS, snapshots=table)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    for r in table:
        print("%-16s age %4d image %s B of %s B  first save %.3f / %.3f ms, compact %.3f / %.3f ms, restore %.3f / %.3f ms (device / wall)  repeat save %s compact %s restore %s" % (
            r["input"], r["age"], r["image_bytes_per_stream"]["median"], r["block_bytes_per_stream_before"]["median"], r["first_save_device_ms"],
            r["first_save_wall_ms"], r["first_compact_device_ms"], r["first_compact_wall_ms"], r["first_restore_device_ms"], r["first_restore_wall_ms"],
            r["repeat_save_wall_ms"]["median"], r["repeat_compact_wall_ms"]["median"], r["repeat_restore_wall_ms"]["median"]))


if __name__ == "__main__":
    main()
