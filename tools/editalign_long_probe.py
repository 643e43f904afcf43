#!/usr/bin/env python3
"""What the alignment of long edit pairs (``edit_align`` with ``set_edit_long`` on) costs, in one process on one device, medians of
``--reps`` launches.

    python tools/editalign_long_probe.py [--reps 7] [--out profiles/edit_align_long.json]

Timed between two HIP events around the C entry point, outputs allocated beforehand, one warm-up launch per shape and width:
  * one pair of 30000 x 30000 tokens at 2 / 4 / 8 / 16 waves;
  * 64 pairs of 6000 x 6000, likewise;
each next to ``edit_counts`` with the mode on, on the same tensors in the same session: that is the forward pass alone (without the
checkpoints), and the ratio is the price of the checkpoints and the walk.  Before a shape is timed its maps are compared across the
widths, and the first pair's maps and counts with the host twin (tests/native/editalign_long_host.cpp), which also says how many blocks
the walk swept again."""
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

import editalign_long_util as au  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402

WAVES = (2, 4, 8, 16)


def rows(rng, B, n, m):
    """B pairs over 4 symbols that share material (a tenth of the positions redrawn)."""
    src = rng.integers(0, 4, (B, max(n, m))).astype(np.int32)
    noisy = lambda k: np.where(rng.random((B, k)) < 0.1, rng.integers(0, 4, (B, k)), src[:, :k]).astype(np.int32)  # noqa: E731
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return dev(noisy(n)[:, None]), dev(np.full((B, 1), n, np.int32)), dev(noisy(m)[:, None]), dev(np.full((B, 1), m, np.int32))


def timed(dec, t, align, reps):
    """-> (median ms, outputs) of ctcd_edit_align or ctcd_edit_counts over the tensors t."""
    x, xl, y, yl = t
    (B, R, L), (Q, Lq) = x.shape, y.shape[1:]
    outs = [torch.zeros((B, R, Q, w), dtype=torch.int32, device="cuda") for w in ((L, Lq, 4) if align else (4,))]
    st = torch.zeros((B,), dtype=torch.int32, device="cuda")
    fn = _native.lib.ctcd_edit_align if align else _native.lib.ctcd_edit_counts
    stream = torch.cuda.current_stream().cuda_stream
    ms = []
    for k in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn(dec._handle, x.data_ptr(), xl.data_ptr(), B, R, L, y.data_ptr(), yl.data_ptr(), Q, Lq, *[o.data_ptr() for o in outs], st.data_ptr(), stream)
        e1.record()
        torch.cuda.synchronize()
        assert rc == 0 and not st.any(), _native.lib.ctcd_last_error()
        if k:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), [o.cpu().numpy() for o in outs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_align_long.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the device"
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(8)], blank_id=0, beam_width=16, log_probs_input=True)
    rng = np.random.default_rng(20261126)
    res = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "unit": "ms, median", "shapes": []}
    for B, n in ((1, 30000), (64, 6000)):
        t = rows(rng, B, n, n)
        twin_x, twin_y, twin_counts, blocks, slot = au.host_pair(t[0][0, 0].cpu().numpy(), t[2][0, 0].cpu().numpy(), 2)
        shape = dict(pairs=B, n=n, m=n, slot_bytes=slot, full_matrix_bytes=n * n // 4, blocks_reswept_first_pair=blocks, widths=[])
        first = None
        for W in WAVES:
            dec.set_edit_long(W)
            ms, outs = timed(dec, t, True, args.reps)
            assert dec.last_edit_long() == B
            groups = dec.last_edit_slots()
            first = first or outs
            assert all((a == b).all() for a, b in zip(first, outs)), "the width changed a result"
            ms_counts, counts = timed(dec, t, False, args.reps)
            assert (counts[0] == outs[2]).all()
            shape["widths"].append(dict(waves=W, workgroups=groups, align_ms=ms, counts_ms=ms_counts, ratio=ms / ms_counts))
        assert (first[0][0, 0, 0] == twin_x).all() and (first[1][0, 0, 0] == twin_y).all() and tuple(first[2][0, 0, 0]) == twin_counts, "the twin disagrees"
        res["shapes"].append(shape)
        dec.set_edit_long(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
