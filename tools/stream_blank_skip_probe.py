#!/usr/bin/env python3
"""What the blank-frame filter of live streams (OnlineCTCBeamDecoder.set_blank_skip(thr)) costs and saves: off against thr = 0.9 / 0.99,
interleaved in one process, medians over the chunk calls of whole streams.

    python tools/stream_blank_skip_probe.py [--reps N] [--frames T] [--out profiles/stream_blank_skip.json]

256 streams, V 29, beam 100, 1000 frames each, fed in 50- and in 200-frame chunks (decode(..., check=False); the last call ends the
streams and is reported apart).  Rows: blank-dominated (+6 on the blank logit), transcript-like (bench.synth_transcript_rows over
tests/data/test.arpa's words) and random (log-softmax of N(0,1) logits: nothing to skip).  Per (chunk, rows, setting) and chunk call:
the wall time between two device synchronisations; the filter (log-softmax, scan, gather) by HIP events; the host's wait for the kept
counts; the decode kernel by set_timing; at a stream's end the remap by HIP events; the kept share; and, when the streams end, the
bytes of a stream's frame map next to the bytes of its block.  Before anything is timed the filtered stream's end is compared bit for
bit with the one-shot CTCBeamDecoder(blank_skip=thr).decode of the same rows."""
import argparse
import ctypes
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

B, V, K = 256, 29, 100
KINDS = ["blank", "transcript", "random"]
SETTINGS = [None, 0.9, 0.99]
CHUNKS = [50, 200]
LABELS29 = ["_", "'", " "] + [chr(ord("a") + i) for i in range(26)]


def rows(kind, T, seed):
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


def make(thr):
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(LABELS29, beam_width=K, cutoff_top_n=V, log_probs_input=True, device="cuda:0")
    dec.set_blank_skip(thr)
    _native.check(_native.lib.ctcd_set_timing(dec._handle, 1))
    return dec


def kernel_ms(dec):
    ms = ctypes.c_float(0)
    _native.check(_native.lib.ctcd_last_kernel_ms(dec._handle, ctypes.byref(ms)))
    return float(ms.value)


def skip_ms(dec):
    f, w, r = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0)
    _native.check(_native.lib.ctcd_last_stream_blank_skip_ms(dec._handle, ctypes.byref(f), ctypes.byref(w), ctypes.byref(r)))
    return float(f.value), float(w.value), float(r.value)


def stream(dec, x, chunk, t=None):
    """One batch of streams from first chunk to end; t: lists to append the per-call figures to."""
    T = x.shape[1]
    states = [ctcdecode_amd.DecoderState(dec) for _ in range(B)]
    out = None
    kept = considered = 0
    for a in range(0, T, chunk):
        last = a + chunk >= T
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = dec.decode(x[:, a:a + chunk], states, [last] * B, check=False)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if dec._blank_skip is not None:
            c, k = dec.last_blank_skip()
            considered, kept = considered + c, kept + k
        if t is not None:
            t["end_call" if last else "chunk_call"].append(ms)
            if not last:
                t["kernel"].append(kernel_ms(dec))
            if dec._blank_skip is not None:
                f, w, r = skip_ms(dec)
                if not last:
                    t["filter"].append(f)
                    t["wait"].append(w)
                else:
                    t["end_remap"].append(r)
    sizes = dict(map_bytes=int(_native.lib.ctcd_stream_map_bytes(states[0].state)), block_bytes=states[0].nbytes, frames=states[0].frames,
                 frames_seen=states[0].frames_seen)
    return out, (kept / considered if considered else None), sizes


def same_bits(a, b):
    for u, v in zip(a, b):
        u, v = u.cpu().numpy(), v.cpu().numpy()
        if u.dtype == np.float32:
            u, v = u.view(np.uint32), v.view(np.uint32)
        if u.shape != v.shape or not np.array_equal(u, v):
            return False
    return True


def probe(kind, chunk, T, reps):
    x = rows(kind, T, 1234)
    decs = {thr: make(thr) for thr in SETTINGS}
    out = {}
    for thr, dec in decs.items():  # warm-up, and the comparison with the one-shot class
        res, share, sizes = stream(dec, x, chunk)
        rec = dict(sizes)
        if thr is not None:
            one = ctcdecode_amd.CTCBeamDecoder(LABELS29, beam_width=K, cutoff_top_n=V, log_probs_input=True, device="cuda:0", blank_skip=thr)
            tok, sc, ts, ln = one.decode(x)
            R, L = res[0].shape[1], res[0].shape[2]
            rec["equals_one_shot"] = same_bits(res, (tok[:, :R, :L], sc, ts[:, :R, :L], ln))
            rec["kept_share"] = round(share, 4)
            del one
        out[thr] = rec
    t = {thr: dict(chunk_call=[], end_call=[], kernel=[], filter=[], wait=[], end_remap=[]) for thr in SETTINGS}
    for _ in range(reps):
        for thr, dec in decs.items():
            stream(dec, x, chunk, t[thr])
    for thr in SETTINGS:
        rec = out[thr]
        for k, v in t[thr].items():
            if v:
                rec[k + "_ms"] = med(v)
        if thr is not None:
            off = out[None]
            rec["chunk_call_saved_ms"] = round(off["chunk_call_ms"]["median"] - rec["chunk_call_ms"]["median"], 4)
            rec["decode_kernel_saved_ms"] = round(off["kernel_ms"]["median"] - rec["kernel_ms"]["median"], 4)
    return {"off" if k is None else "thr_%g" % k: v for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_blank_skip.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "streams": B, "labels": V, "beam": K, "frames": a.frames,
           "method": " ".join(__doc__.split("\n\n")[2].split())}
    for chunk in CHUNKS:
        for kind in KINDS:
            key = "chunk_%d/%s" % (chunk, kind)
            res[key] = probe(kind, chunk, a.frames, a.reps)
            print(key, json.dumps(res[key]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
