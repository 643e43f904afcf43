#!/usr/bin/env python3
"""What ``CTCBeamDecoder.edit_counts`` and ``edit_align`` cost next to ``edit_distance``, in one process, medians.

    python tools/editops_probe.py [--reps N] [--out profiles/editops.json]

Rows: those of tools/editdist_probe.py -- B 256 items of up to 100 rows, L = 1000; "transcript": edits of one base row of 230 .. 270
labels per item; "random": independent rows of 250 .. 900 labels.  Per kind, each kernel between two HIP events, into tensors
allocated beforehand: ctcd_edit_counts next to the unchanged ctcd_edit_distance on the same tensors for 1 / 10 / 100 rows against one
reference per item and pairwise over 100 rows; ctcd_edit_align for 1 and 10 rows against one reference each next to ctcd_edit_counts on
the same rows, with the slot size, the slots and the grid it ran with at the default scratch budget.  The sweep's and the walk's share
of edit_align are not timed apart inside the kernel: what is recorded is edit_counts' time on the same rows and grid -- the sweep
without direction stores -- and the remainder, which is the direction stores, the -1 fill and the walk.  Before anything is timed,
sampled pairs of every launch are compared with the host twin (tests/native/editops_host.cpp)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import editops_util as ou  # noqa: E402
import ctcdecode_amd  # noqa: E402
from ctcdecode_amd import _native  # noqa: E402
from editdist_probe import B, L, R, V, make_rows, med, timed  # noqa: E402

# hipcc -Rpass-analysis=kernel-resource-usage for gfx950 (python ctcdecode_amd/_build.py --force prints it): copied here by hand, it is not
# measured by this tool.  The align kernel's scratch is three spilled 32-bit values, stored in the prologue and reloaded once per pair
# outside the sweep and walk loops; no lane array of either kernel is in scratch.
COMPILER_REPORT = {
    "edit_counts_kernel": dict(vgprs=256, agprs=0, sgprs=106, sgpr_spills=17, vgpr_spills=0, scratch_bytes_per_lane=0, lds_bytes=0, waves_per_simd=2),
    "edit_align_kernel": dict(vgprs=256, agprs=0, sgprs=106, sgpr_spills=12, vgpr_spills=3, scratch_bytes_per_lane=16, lds_bytes=0, waves_per_simd=2),
    "edit_distance_kernel": dict(vgprs=190, agprs=0, sgprs=106, sgpr_spills=15, vgpr_spills=0, scratch_bytes_per_lane=0, lds_bytes=0, waves_per_simd=2),
}


def sampled_equal(outs, x, xl, y, yl, rng, pairwise, n=12):
    """n sampled pairs of a launch against the host twin: counts, and maps where the launch has them."""
    outs = [o.cpu().numpy() for o in outs]
    ok = True
    for _ in range(n):
        b, i, j = int(rng.integers(outs[0].shape[0])), int(rng.integers(outs[0].shape[1])), int(rng.integers(outs[0].shape[2]))
        if pairwise and i == j:
            continue
        lx, ly = int(xl[b, i]), int(yl[b, j])
        cnt, xm, ym = ou.host_pair_align(x[b, i, :lx], y[b, j, :ly])
        same = tuple(outs[-1][b, i, j]) == cnt
        if len(outs) == 3:
            same = same and outs[0][b, i, j, :lx].tolist() == xm and outs[1][b, i, j, :ly].tolist() == ym
        if not same:
            print("MISMATCH", (b, i, j), flush=True)
            ok = False
    return ok


def probe_kind(dec, kind, reps, rng):
    x_np, lens_np = make_rows(kind, rng)
    rows, lens = torch.from_numpy(x_np).cuda(), torch.from_numpy(lens_np).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    rec = dict(labels=dict(min=int(lens_np.min()), median=float(np.median(lens_np)), max=int(lens_np.max())))
    ref, ref_lens = rows[:, R:].contiguous(), lens[:, R:].contiguous()
    lib = _native.lib
    for r, pairwise in ((1, False), (10, False), (100, False), (100, True)):
        x, xl = rows[:, :r].contiguous(), lens[:, :r].contiguous()
        q = r if pairwise else 1
        dist = torch.empty((B, r, q), dtype=torch.int32, device="cuda")
        cnt = torch.empty((B, r, q, 4), dtype=torch.int32, device="cuda")
        y_args = (None, None) if pairwise else (ref.data_ptr(), ref_lens.data_ptr())
        got = dec.edit_counts(x, xl) if pairwise else dec.edit_counts(x, xl, ref, ref_lens)
        same = sampled_equal([got], x_np[:, :r], lens_np[:, :r], x_np[:, :r] if pairwise else x_np[:, R:], lens_np[:, :r] if pairwise else lens_np[:, R:], rng, pairwise)

        def distance():
            _native.check(lib.ctcd_edit_distance(dec._handle, x.data_ptr(), xl.data_ptr(), B, r, L, *y_args, q, L, dist.data_ptr(), None, stream))

        def counts():
            _native.check(lib.ctcd_edit_counts(dec._handle, x.data_ptr(), xl.data_ptr(), B, r, L, *y_args, q, L, cnt.data_ptr(), None, stream))

        td, tc = [], []
        for k in range(reps + 1):  # (the first pass is not counted)
            a, c = timed(distance), timed(counts)
            if k:
                td.append(a), tc.append(c)
        consistent = bool((cnt[..., 1:].sum(-1) == dist).all().item())
        e = dict(equals_host_twin_on_sampled_pairs=bool(same), counts_sum_to_the_distance=consistent, pairs=dec.last_edit_pairs(), edit_distance_ms=med(td),
                 edit_counts_ms=med(tc))
        e["counts_over_distance"] = round(e["edit_counts_ms"]["median"] / e["edit_distance_ms"]["median"], 3)
        rec["%s_%d" % ("pairwise" if pairwise else "rows_vs_reference", r)] = e
        print(kind, "pairwise" if pairwise else "vs_reference", r, json.dumps(e), flush=True)
    for r in (1, 10):
        x, xl = rows[:, :r].contiguous(), lens[:, :r].contiguous()
        xm = torch.empty((B, r, 1, L), dtype=torch.int32, device="cuda")
        ym = torch.empty((B, r, 1, L), dtype=torch.int32, device="cuda")
        cnt = torch.empty((B, r, 1, 4), dtype=torch.int32, device="cuda")
        same = sampled_equal(dec.edit_align(x, xl, ref, ref_lens), x_np[:, :r], lens_np[:, :r], x_np[:, R:], lens_np[:, R:], rng, False)

        def align():
            _native.check(lib.ctcd_edit_align(dec._handle, x.data_ptr(), xl.data_ptr(), B, r, L, ref.data_ptr(), ref_lens.data_ptr(), 1, L, xm.data_ptr(), ym.data_ptr(),
                                              cnt.data_ptr(), None, stream))

        def counts():
            _native.check(lib.ctcd_edit_counts(dec._handle, x.data_ptr(), xl.data_ptr(), B, r, L, ref.data_ptr(), ref_lens.data_ptr(), 1, L, cnt.data_ptr(), None, stream))

        ta, tc = [], []
        for k in range(reps + 1):
            c, a = timed(counts), timed(align)
            if k:
                ta.append(a), tc.append(c)
        e = dict(equals_host_twin_on_sampled_pairs=bool(same), pairs=dec.last_edit_pairs(), slots=dec.last_edit_slots(), grid=dec.last_edit_grid(),
                 slot_bytes=ou.host_slot_bytes(L, L), edit_align_ms=med(ta), edit_counts_ms=med(tc))
        e["sweep_share_as_edit_counts_over_edit_align"] = round(e["edit_counts_ms"]["median"] / e["edit_align_ms"]["median"], 3)
        e["stores_fill_and_walk_share"] = round(1.0 - e["sweep_share_as_edit_counts_over_edit_align"], 3)
        rec["align_rows_vs_reference_%d" % r] = e
        print(kind, "align", r, json.dumps(e), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "editops.json"))
    a = ap.parse_args()
    dec = ctcdecode_amd.CTCBeamDecoder([str(i) for i in range(V)], beam_width=R, log_probs_input=True, device="cuda:0")
    rng = np.random.default_rng(20261021)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "shape": dict(B=B, R=R, L=L, V=V), "method": " ".join(__doc__.split("\n\n")[2].split()),
           "compiler_report": COMPILER_REPORT}
    for kind in ("transcript", "random"):
        res[kind] = probe_kind(dec, kind, a.reps, rng)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
