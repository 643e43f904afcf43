#!/usr/bin/env python3
"""What a chunk call of the greedy decode of live streams costs, next to its floor and to the beam stream, in one process, medians.

    python tools/greedy_stream_probe.py [--reps N] [--out profiles/greedy_stream.json]

256 streams, V 29, chunks of 50 and 200 frames, float32 and bfloat16, log-probabilities and raw logits.  Per combination, on the same
[256, Tc, 29] tensor and alternated in one loop after one untimed pass, each a wall time between synchronisations (allocations
included): OnlineCTCBeamDecoder.greedy_decode_device (the chunk call: one staged upload, the argmax pass, the stream collapse kernel),
with the time of the same call between two HIP events, and the native entry point alone (ctcd_greedy_stream_decode into tensors
allocated beforehand) between two HIP events next to ctcd_greedy_decode measured the same way; CTCBeamDecoder.greedy_decode_device
(the one-shot call: the same argmax pass, no upload -- the floor); the beam stream's chunk call OnlineCTCBeamDecoder.decode(check=False) at beam 100 on streams of the
same age; and peek() of those streams.  Before anything is timed the first chunk of fresh streams is compared with the one-shot call:
equal labels, start frames, counts and score bits."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

B, V, K = 256, 29, 100
CHUNKS = (50, 200)
MODES = {1: "log_probabilities", 2: "logits"}
DTYPES = {"float32": torch.float32, "bfloat16": torch.bfloat16}


def rows_of(Tc, mode, dtype):
    """Transcript-like rows: three frames in four dominated by the blank, the others by one label."""
    g = torch.Generator(device="cuda").manual_seed(1234)
    z = torch.randn((B, Tc, V), generator=g, device="cuda")
    top = torch.randint(1, V, (B, Tc), generator=g, device="cuda")
    top[torch.rand((B, Tc), generator=g, device="cuda") < 0.75] = 0
    z.scatter_add_(2, top.unsqueeze(-1), torch.full((B, Tc, 1), 8.0, device="cuda"))
    return (z if mode == 2 else z.log_softmax(-1)).to(dtype).contiguous()


def med(xs):
    xs = sorted(xs)
    return dict(median=round(statistics.median(xs), 4), min=round(xs[0], 4), max=round(xs[-1], 4), n=len(xs))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def probe(Tc, mode, dtype, reps):
    x = rows_of(Tc, mode, dtype)
    labels = [str(i) for i in range(V)]
    kw = dict(beam_width=K, cutoff_top_n=V, log_probs_input=mode == 1, logits_input=mode == 2, device="cuda:0")
    online = ctcdecode_amd.OnlineCTCBeamDecoder(labels, **kw)
    one = ctcdecode_amd.CTCBeamDecoder(labels, **kw)
    gstates = [ctcdecode_amd.GreedyState(online) for _ in range(B)]
    bstates = [ctcdecode_amd.DecoderState(online) for _ in range(B)]
    go_on = [False] * B
    tok, sc, st, lens = online.greedy_decode_device(x, gstates, go_on)
    tok1, sc1, st1, lens1 = one.greedy_decode_device(x)
    cols = torch.arange(Tc, device="cuda")[None, None, :] < lens[:, :, None]  # (a label the chunk's last frame leaves open is emitted too)
    same = bool(torch.equal(lens, lens1) and torch.equal(tok * cols, tok1 * cols) and torch.equal(st * cols, st1 * cols) and
                torch.equal(sc.view(torch.int32), sc1.view(torch.int32)))
    rec = dict(first_chunk_equals_one_shot=same, input_bytes=x.numel() * x.element_size())
    # the two native entry points alone, into the tensors above, between two HIP events: what the Python layer adds is the difference
    stream = torch.cuda.current_stream().cuda_stream
    ptrs = (ctypes.c_void_p * B)(*[s._handle.value for s in gstates])
    flags = (ctypes.c_ubyte * B)()

    def native_stream():
        _native.check(_native.lib.ctcd_greedy_stream_decode(online._handle, ptrs, flags, x.data_ptr(), None, B, Tc, V, 0, mode, tok.data_ptr(), st.data_ptr(), None,
                                                            None, None, sc.data_ptr(), lens.data_ptr(), stream))

    def native_one_shot():
        _native.check(_native.lib.ctcd_greedy_decode(one._handle, x.data_ptr(), None, B, Tc, V, 0, mode, tok1.data_ptr(), st1.data_ptr(), None, None, sc1.data_ptr(),
                                                     lens1.data_ptr(), stream))

    gs, gs_dev, g1, bs, pk, ns, n1 = [], [], [], [], [], [], []
    for i in range(reps + 1):  # (the first pass is not counted)
        t_ns = timed(native_stream)
        t_n1 = timed(native_one_shot)
        t_gs = wall(lambda: online.greedy_decode_device(x, gstates, go_on))
        t_dev = timed(lambda: online.greedy_decode_device(x, gstates, go_on))
        t_g1 = wall(lambda: one.greedy_decode_device(x))
        t_bs = wall(lambda: online.decode(x, bstates, go_on, check=False))
        t_pk = wall(lambda: online.peek(bstates))
        if i:
            ns.append(t_ns), n1.append(t_n1), gs.append(t_gs), gs_dev.append(t_dev), g1.append(t_g1), bs.append(t_bs), pk.append(t_pk)
    rec.update(greedy_stream_native_ms=med(ns), greedy_one_shot_native_ms=med(n1), greedy_stream_call_ms=med(gs), greedy_stream_call_device_ms=med(gs_dev), greedy_one_shot_call_ms=med(g1), beam_stream_call_ms=med(bs),
               beam_stream_peek_ms=med(pk), frames_per_stream_at_the_end=gstates[0].info()["frames"])
    rec["beam_stream_peek_over_greedy_stream"] = round(rec["beam_stream_peek_ms"]["median"] / rec["greedy_stream_call_ms"]["median"], 4)
    rec["greedy_stream_over_one_shot"] = round(rec["greedy_stream_call_ms"]["median"] / rec["greedy_one_shot_call_ms"]["median"], 4)
    rec["greedy_stream_over_beam_stream"] = round(rec["greedy_stream_call_ms"]["median"] / rec["beam_stream_call_ms"]["median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "greedy_stream.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "streams": B, "labels": V, "beam_of_the_beam_stream": K,
           "method": " ".join(__doc__.split("\n\n")[2].split())}
    for Tc in CHUNKS:
        for mode, mname in MODES.items():
            for dname, dtype in DTYPES.items():
                key = "chunk_%d_%s_%s" % (Tc, mname, dname)
                res[key] = probe(Tc, mode, dtype, a.reps)
                print(key, json.dumps(res[key]), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
