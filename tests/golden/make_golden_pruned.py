#!/usr/bin/env python3
"""Generate tests/golden/live/pruned_rows.json: for every case of tests/test_oracle.py's per-frame prune comparison, the sha256 of its
inputs and of the REAL reference's get_pruned_log_probs output (oracle/_ref/libctcref.so: counts, labels, values), so that the test
compares the restatement with the reference also where oracle/_ref is not built.  Runs only where the reference checkout exists."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_util as ou  # noqa: E402
import test_oracle as to  # noqa: E402

if __name__ == "__main__":
    assert ou.have_reference(), "oracle/_ref is not built"
    out = {}
    for name, x, cp, top_n, li in to._prune_cases():
        want = ou.pruned_rows(x, cp, top_n, li, which="reference")
        out[name] = [to._digest(x, np.float64(cp), np.int32(top_n), np.int32(li)), to._digest(*want)]
    with open(to.PRUNE_DIGESTS, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(out), "cases ->", to.PRUNE_DIGESTS)
