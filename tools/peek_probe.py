#!/usr/bin/env python3
"""What a peek costs (OnlineCTCBeamDecoder.peek / ctc_stream_peek_kernel):  python tools/peek_probe.py [--out profiles/stream_peek.json]

256 streams, 29 labels, beam 100, fed 50 frames at a time (the README's streaming row) and peeked after every chunk with n_best = 1.
At stream ages 250, 500 and 1000 frames: the device time of one peek (HIP events around ctcd_stream_peek: its argument copy, the
status clear and the kernel), min / median over repeats in one process, for since = 0 and since = the last stable_len, next to the
labels it reports (n_best x (len - since), summed over the streams); and the wall time of peek() to CPU tensors.  To be read against
two figures of the same session: the device time of the 50-frame chunk calls and the wall time of the call that ends the streams."""
import argparse
import ctypes
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
from ctcdecode_amd import _native

B, V, K, CHUNK, T = 256, 29, 100, 50, 1000
T_IN = T + CHUNK  # the call that ends the streams feeds one more chunk, as a serving loop's last call does
AGES = (250, 500, 1000)
REPS = 30


def inputs(kind, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T_IN, V)).astype(np.float32)
    if kind == "blank_dominated":
        x[:, :, 0] += np.float32(4.0)
    elif kind == "peaky":  # a label or the blank dominates for a few frames; most stretches sharply, some faintly
        for b in range(B):
            t = 0
            while t < T_IN:
                n = int(rng.integers(1, 6))
                c = 0 if rng.random() < 0.5 else int(rng.integers(0, V))
                x[b, t:t + n, c] += np.float32(1.0 if rng.random() < 0.4 else 20.0)
                t += n
    return torch.from_numpy(x).log_softmax(-1)


def mm(v):
    return dict(min=round(min(v), 4), median=round(statistics.median(v), 4), max=round(max(v), 4), n=len(v))


def device_ms(fn, reps=REPS):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def run(kind, seed, dev):
    lp = inputs(kind, seed).to(dev)
    dec = ctcdecode_amd.OnlineCTCBeamDecoder([str(i) for i in range(V)], beam_width=K, blank_id=0, log_probs_input=True, device=dev)
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    ptrs = (ctypes.c_void_p * B)(*[s.state.value for s in states])
    stream = torch.cuda.current_stream(dev).cuda_stream
    tok = torch.empty((B, 1, T), dtype=torch.int32, device=dev)
    ts = torch.empty((B, 1, T), dtype=torch.int32, device=dev)
    sc = torch.empty((B, 1), dtype=torch.float32, device=dev)
    ln = torch.empty((B, 1), dtype=torch.int32, device=dev)
    nres = torch.empty((B,), dtype=torch.int32, device=dev)
    stable = torch.empty((B,), dtype=torch.int32, device=dev)

    def raw_peek(since, L_cap):
        since_c = (ctypes.c_int32 * B)(*since) if since is not None else None
        _native.check(_native.lib.ctcd_stream_peek(dec._handle, ptrs, B, 1, since_c, tok.data_ptr(), ts.data_ptr(), L_cap, sc.data_ptr(), ln.data_ptr(),
                                                   nres.data_ptr(), stable.data_ptr(), stream))

    chunk_ms, rows, last_stable = [], [], [0] * B
    for c in range(T // CHUNK):
        age = (c + 1) * CHUNK
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dec.decode(lp[:, c * CHUNK:age], states, [False] * B, check=False)
        e1.record()
        e1.synchronize()
        chunk_ms.append(e0.elapsed_time(e1))
        res = dec.peek(states, n_best=1, since=last_stable)  # the peek a client makes after every chunk
        if age in AGES:
            for mode in ("since=0", "since=stable_len"):
                since = [0] * B if mode == "since=0" else last_stable
                L_cap = max(age - s for s in since)
                raw_peek(since, L_cap)
                _native.check(_native.lib.ctcd_check_status(dec._handle, 0))
                labels = int((ln[:, 0].cpu() - torch.tensor(since, dtype=torch.int32)).clamp(min=0).sum())
                dev_ms = device_ms(lambda: raw_peek(since, L_cap))
                _native.check(_native.lib.ctcd_check_status(dec._handle, 0))
                torch.cuda.synchronize(dev)
                wall = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    dec.peek(states, n_best=1, since=since)
                    wall.append((time.perf_counter() - t0) * 1e3)
                rows.append(dict(input=kind, age=age, mode=mode, labels_reported=labels, mean_tail=round(labels / B, 1),
                                 peek_device_ms=mm(dev_ms), peek_wall_ms=mm(wall)))
        last_stable = [int(v) for v in res[4]]
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    dec.decode(lp[:, T:T_IN], states, [True] * B)
    end_ms = (time.perf_counter() - t0) * 1e3
    return rows, chunk_ms, end_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_peek.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    table, chunks, ends = [], [], []
    for i, kind in enumerate(("random", "blank_dominated", "peaky")):
        rows, chunk_ms, end_ms = run(kind, 4321 + i, dev)
        table += rows
        chunks.append(dict(input=kind, chunk_call_device_ms=mm(chunk_ms[1:])))  # (the first call allocates)
        ends.append(dict(input=kind, end_call_wall_ms=round(end_ms, 3)))
    out = dict(what="256 streams, V 29, beam 100, 50-frame chunks, peek with n_best = 1 after every chunk", device=torch.cuda.get_device_name(0),
               reps=REPS, peeks=table, same_session_chunk_calls=chunks, same_session_end_calls=ends)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    for r in table:
        print("%-16s age %4d %-16s labels %6d  device ms %s  wall ms %s" % (r["input"], r["age"], r["mode"], r["labels_reported"],
                                                                           r["peek_device_ms"], r["peek_wall_ms"]))
    print(json.dumps(chunks))
    print(json.dumps(ends))


if __name__ == "__main__":
    main()
