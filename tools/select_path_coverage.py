#!/usr/bin/env python3
"""Which paths of the select the kernel matrix's inputs take, per case, from the host twin alone (one thread, instantiated as each
case's own class: tests/select_path_util.py host_env).

    python tools/select_path_coverage.py [--write]

Scorer cases decode select_path_inputs, scorer-free cases km.inputs; the unpruned callback cases are counted a second time through the
scorer hook's twin (`hook`: a frame that parks on a miss and is run again is counted again).  Prints case id -> counters of
beam_core.h enum Event; --write also stores the table as profiles/select_path_coverage.json, which tests/test_select_paths.py
compares with what it measures."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
TABLE = os.path.join(ROOT, "profiles", "select_path_coverage.json")


def measure():
    import kernel_matrix_util as km
    import select_path_util as sp
    from test_lm import make_wide_label_lm

    def setenv(k, v):
        os.environ[k] = v

    def delenv(k):
        os.environ.pop(k, None)

    table = {"inputs": {"scorer": "select_path_inputs", "scorer_free": "km.inputs"}, "left_out": sp.LEFT_OUT, "scorer": {}, "hook": {}, "scorer_free": {}}
    with tempfile.TemporaryDirectory() as tmp:
        wide99 = make_wide_label_lm(tmp)
        for c in sp.scorer_cases():
            lm = km.lm_spec(c, *wide99)
            lp, sl = sp.select_path_inputs(c, lm[1])
            sp.set_host_env(c, setenv, delenv)
            table["scorer"][km.case_id(c)] = sp.counted(lambda: sp.host_decode(c, lp, sl, lm))[1]
            if c["callback"] and not sp.is_pruned(c):
                table["hook"][km.case_id(c)] = sp.counted(lambda: sp.host_decode(c, lp, sl, lm, callback=True))[1]
        for c in sp.scorer_free_cases():
            lp, sl = km.inputs(c)
            sp.set_host_env(c, setenv, delenv)
            table["scorer_free"][km.case_id(c)] = sp.counted(lambda: sp.host_decode(c, lp, sl, None))[1]
    for k in sp.HOST_SWITCHES:
        delenv(k)
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--write", action="store_true", help="store the table as profiles/select_path_coverage.json")
    a = ap.parse_args()
    table = measure()
    names = None
    for group in ("scorer", "hook", "scorer_free"):
        print("%s cases (%d)" % (group, len(table[group])))
        for cid, cnt in table[group].items():
            names = names or list(cnt)
            print("  %-24s %s" % (cid, " ".join("%s=%d" % (n[3:].lower(), cnt[n]) for n in names)))
    if a.write:
        with open(TABLE, "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", os.path.relpath(TABLE, ROOT))


if __name__ == "__main__":
    main()
