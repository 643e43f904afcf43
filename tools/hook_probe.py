#!/usr/bin/env python3
"""The scorer hook's cost (bench.py time_scorer_hook) and the two-launches-in-flight rule (bench.py time_inflight) on their own.
    python tools/hook_probe.py [--big] [--inflight] [--threads=1 --threads=4 ...]
    python tools/hook_probe.py --forms [--big]: the four forms of the callback (native / Python, per window / batched) at the configs[4]
    shape on transcript-like rows, cold and warm, and the queued pairs per distinct window with the device filter off and on."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
import ctcdecode_amd  # noqa: E402

dev = torch.device("cuda", 0)
labels = ["_", "'", " "] + [chr(ord("a") + i) for i in range(26)]
arpa = os.path.join(ROOT, "tests", "data", "test.arpa")
if "--inflight" in sys.argv:
    lp128 = bench.synth_rows(torch, 128, 1500, 29, 7).to(dev)
    for name, kw in (("no LM", {}), ("test.arpa", dict(model_path=arpa, alpha=0.5, beta=1.0))):
        one = bench.time_inflight(torch, ctcdecode_amd, dev, lp128, labels, 100, 1, **kw)
        two = bench.time_inflight(torch, ctcdecode_amd, dev, lp128, labels, 100, 2, **kw)
        print("128 utterances x 1500 frames, %s: one in flight %.3f ms/batch (%.0f utt/s), two in flight %.3f ms/batch (%.0f utt/s)" % (name, one * 1e3, 128 / one, two * 1e3, 128 / two))
    lp256 = bench.synth_rows(torch, 256, 1000, 29, 1234).to(dev)
    for k in (1, 2, 3):
        dt = bench.time_inflight(torch, ctcdecode_amd, dev, lp256, [str(i) for i in range(29)], 100, k, steps=20)
        print("headline batch, default build, %d in flight: %.3f ms/batch (%.0f utt/s)" % (k, dt * 1e3, 256 / dt))


def forms(arpa, B=128, T=1500, K=100, alpha=0.5, beta=1.0):
    """Cold (fresh scorer) and warm decodes through each form of the callback, the built-in tables of `arpa` behind it; every result is
    checked against the built-in path."""
    import ctypes
    import time

    n = ctcdecode_amd._native
    V = len(labels)
    voc = bench.arpa_unigrams(arpa)
    x = bench.synth_transcript_rows(torch, B, T, labels, [w for w in voc if w not in ("<s>", "</s>", "<unk>")], 7).to(dev)
    arr = (ctypes.c_char_p * V)(*[w.encode("utf-8") for w in labels])
    inner = ctypes.c_void_p()
    n.check(n.lib.ctcd_scorer_create(ctypes.byref(inner), 0.0, 0.0, arpa.encode(), arr, V, 0))
    order = int(n.lib.ctcd_scorer_max_order(inner))

    def py_one(words):
        a = (ctypes.c_char_p * len(words))(*[w.encode("utf-8") for w in words])
        p = ctypes.c_float()
        rc = n.lib.ctcd_scorer_cond_log10(inner, a, len(words), ctypes.byref(p))
        return None if rc else p.value

    memo = {}

    def py_batch(windows):
        return [py_one(w) for w in windows]

    def recording(windows):  # (fills the dict of the "over a dict" row in an untimed decode)
        r = py_batch(windows)
        memo.update(zip(windows, r))
        return r

    makers = {
        "native per-window": lambda: ctcdecode_amd.CallbackScorer.from_c(ctypes.cast(n.lib.ctcd_scorer_cond_log10, ctypes.c_void_p).value, inner.value, voc, order, labels,
                                                                         alpha=alpha, beta=beta),
        "Python per-window": lambda: ctcdecode_amd.CallbackScorer(py_one, voc, order, labels, alpha=alpha, beta=beta),
        "Python batched": lambda: ctcdecode_amd.CallbackScorer.batched(py_batch, voc, order, labels, alpha=alpha, beta=beta),
        # (the answers of the run above from a dict: what the batched hook itself costs a Python callable)
        "Python batched over a dict": lambda: ctcdecode_amd.CallbackScorer.batched(lambda ws: [memo[w] for w in ws], voc, order, labels, alpha=alpha, beta=beta),
        "native batched": lambda: ctcdecode_amd.CallbackScorer.from_c_batch(ctypes.cast(n.lib.ctcd_scorer_cond_log10_batch, ctypes.c_void_p).value, inner.value, voc, order,
                                                                           labels, alpha=alpha, beta=beta),
    }
    out = {"model": os.path.basename(arpa), "shape": [B, T, K]}
    try:
        ref = ctcdecode_amd.CTCBeamDecoder(labels, model_path=arpa, alpha=alpha, beta=beta, cutoff_top_n=V, beam_width=K, log_probs_input=True)
        want = ref.decode_device(x, None)
        for name, make in makers.items():
            if name == "Python batched over a dict":
                rec = ctcdecode_amd.CallbackScorer.batched(recording, voc, order, labels, alpha=alpha, beta=beta)
                ctcdecode_amd.CTCBeamDecoder(labels, scorer=rec, cutoff_top_n=V, beam_width=K, log_probs_input=True).decode_device(x, None)
                del rec
            for filt in ((False, True) if name == "native per-window" else (True,)):
                sc = make()
                dec = ctcdecode_amd.CTCBeamDecoder(labels, scorer=sc, cutoff_top_n=V, beam_width=K, log_probs_input=True)
                dec.set_scorer_filter(filt)
                row = {}
                for phase in ("cold", "warm"):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    got = dec.decode_device(x, None)
                    torch.cuda.synchronize(); dt = time.perf_counter() - t0
                    q, d, r = dec.last_scorer_pairs()
                    row[phase] = {"ms": round(dt * 1e3, 1), "equals_built_in": all(bool(torch.equal(a, b)) for a, b in zip(got, want)),
                                  "queued_pairs": q, "distinct_windows": d, "repeats_same_item": r, "pairs_per_window": round(q / d, 3) if d else None}
                row["callback_calls"], row["callback_batches"] = sc.callback_calls(), sc.callback_batches()
                out[name + ("" if filt else ", device filter off")] = row
                del dec, sc
    finally:
        n.lib.ctcd_scorer_destroy(inner)
    return out


if "--forms" in sys.argv:
    print(json.dumps(forms(arpa), indent=1))
    if "--big" in sys.argv:
        import importlib.util
        import tempfile

        spec = importlib.util.spec_from_file_location("make_big_lm", os.path.join(ROOT, "tools", "make_big_lm.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        big = os.path.join(tempfile.gettempdir(), "ctcd_big_words_50k.arpa")
        if not os.path.exists(big):
            mod.make(big)
        print(json.dumps(forms(big), indent=1))
    sys.exit(0)
threads = [int(a.split("=")[1]) for a in sys.argv if a.startswith("--threads=")] or [1]
for th in threads:
    print(json.dumps(bench.time_scorer_hook(torch, ctcdecode_amd, dev, arpa, labels, threads=th), indent=1))
    print(json.dumps(bench.time_scorer_hook(torch, ctcdecode_amd, dev, arpa, labels, transcripts=True, threads=th), indent=1))
if "--big" in sys.argv:
    import importlib.util
    import tempfile

    spec = importlib.util.spec_from_file_location("make_big_lm", os.path.join(ROOT, "tools", "make_big_lm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    big = os.path.join(tempfile.gettempdir(), "ctcd_big_words_50k.arpa")
    if not os.path.exists(big):
        mod.make(big)
    for th in threads:
        print(json.dumps(bench.time_scorer_hook(torch, ctcdecode_amd, dev, big, labels, transcripts=True, threads=th), indent=1))
