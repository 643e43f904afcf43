#!/usr/bin/env python3
"""What a chunk call of the keyword search of live streams (``KeywordState`` / ``OnlineCTCBeamDecoder.find_keywords``) costs, next to
what a caller has without it, in one process, medians.

    python tools/keyword_stream_probe.py [--reps N] [--out profiles/keyword_stream.json]

256 streams, V 29, float32 log-probabilities, transcript-like rows; Q = 1, 16 and 256 keywords of 4 - 12 labels; chunks of 50 and 200
frames.  Per (Q, chunk), alternated in one loop after one untimed pass, each into tensors allocated beforehand, between two HIP events
(``_ms``) and as the call's wall time between synchronisations (``_wall_ms``): ctcd_keyword_stream_find on the chunk (one launch: the
staged route); ctcd_ctc_keywords on the same chunk tensor (two launches: the floor a stream call is held against); ctcd_ctc_keywords
on 1000 frames (what a caller does today at stream age 1000: everything so far again); ctcd_greedy_stream_decode on the chunk.  The
gathered route (two launches) is probed at 64 streams, V 10000, Q 16.  Medians of 7.  Before anything is timed the streams' running
result after two chunks is compared bit for bit with the one-shot call on their concatenation."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import keyword_util as ku  # noqa: E402
from greedy_probe import med, rows_of, timed, wall  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

AGE = 1000


def probe(B, V, Q, Tc, reps):
    x = rows_of(dict(B=B, T=AGE if V <= 128 else 2 * Tc, V=V), 1, torch.float32)
    chunk = x[:, :Tc].contiguous()
    rng = np.random.default_rng(Q)
    kws = [ku._keyword(rng, int(rng.integers(4, 13)), V, 0) for _ in range(Q)]
    k, lens = (torch.from_numpy(a) for a in ku.kw_tensors(kws, 12))
    labels = [str(i) for i in range(V)]
    one = ctcdecode_amd.CTCBeamDecoder(labels, log_probs_input=True, device="cuda:0")
    dec = ctcdecode_amd.OnlineCTCBeamDecoder(labels, log_probs_input=True, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    # ---- two chunks against the one-shot call on their concatenation
    states = [ctcdecode_amd.KeywordState(dec, k, lens) for _ in range(B)]
    dec.find_keywords(chunk, states, [False] * B)
    got = dec.find_keywords(x[:, Tc:2 * Tc].contiguous(), states, [False] * B)
    want = one.find_keywords(x[:, :2 * Tc].contiguous(), None, k.cuda(), lens.cuda())
    same = all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want))
    if not same:
        print("MISMATCH B %d V %d Q %d Tc %d" % (B, V, Q, Tc), flush=True)

    # ---- the four calls, on tensors allocated beforehand
    f32, i32 = (lambda *s: torch.empty(s, dtype=torch.float32, device="cuda")), (lambda *s: torch.empty(s, dtype=torch.int32, device="cuda"))
    o3, kd, ld = [f32(B, Q), i32(B, Q), i32(B, Q)], k.cuda(), lens.cuda()
    ptrs = (ctypes.c_void_p * B)(*[st._handle.value for st in states])
    no_eos = (ctypes.c_ubyte * B)()
    gstates = [ctcdecode_amd.GreedyState(dec) for _ in range(B)]
    gptrs = (ctypes.c_void_p * B)(*[st._handle.value for st in gstates])
    g = [i32(B, Tc), i32(B, Tc), f32(B), i32(B)]

    def stream_call():
        _native.check(_native.lib.ctcd_keyword_stream_find(dec._handle, ptrs, no_eos, chunk.data_ptr(), None, B, Tc, V, 0, 1, *[o.data_ptr() for o in o3],
                                                           None, None, None, None, None, None, stream))

    def one_shot(rows):
        _native.check(_native.lib.ctcd_ctc_keywords(one._handle, rows.data_ptr(), None, B, rows.shape[1], V, 0, 1, kd.data_ptr(), ld.data_ptr(), Q, 12,
                                                    *[o.data_ptr() for o in o3], None, None, None, stream))

    def greedy_call():
        _native.check(_native.lib.ctcd_greedy_stream_decode(dec._handle, gptrs, no_eos, chunk.data_ptr(), None, B, Tc, V, 0, 1, g[0].data_ptr(), g[1].data_ptr(),
                                                            None, None, None, g[2].data_ptr(), g[3].data_ptr(), stream))

    calls = dict(stream_chunk=stream_call, one_shot_chunk=lambda: one_shot(chunk), greedy_stream_chunk=greedy_call)
    if V <= 128:
        calls["one_shot_age_%d" % AGE] = lambda: one_shot(x)
    t = {n + s: [] for n in calls for s in ("_ms", "_wall_ms")}
    for i in range(reps + 1):  # (the first pass is not counted)
        for n, fn in calls.items():
            a, b = timed(fn), wall(fn)
            if i:
                t[n + "_ms"].append(a), t[n + "_wall_ms"].append(b)
    rec = {n: med(v) for n, v in t.items()}
    rec.update(equals_one_shot_after_two_chunks=same, kernel=dec.last_keyword_kernel(), state_bytes_per_stream=32 + Q * 16 + Q * 16 * 16)
    rec["stream_over_one_shot_chunk"] = round(rec["stream_chunk_ms"]["median"] / rec["one_shot_chunk_ms"]["median"], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyword_stream.json"))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "method": " ".join(__doc__.split("\n\n")[2].split())}
    for B, V, Q, Tc in [(256, 29, Q, Tc) for Q in (1, 16, 256) for Tc in (50, 200)] + [(64, 10000, 16, 50)]:
        key = "B%d_V%d_Q%d_Tc%d" % (B, V, Q, Tc)
        res[key] = probe(B, V, Q, Tc, a.reps)
        print(key, json.dumps(res[key]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
