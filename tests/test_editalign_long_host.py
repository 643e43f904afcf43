"""The long alignments' host code (ctcdecode_amd/csrc/editlong.h "Alignments") on the CPU: the sequential twin, through a buffer of exactly
the slot's size, against the references of tests/editalign_long_util.py at the GPU tests' cases."""
import subprocess

import editalign_long_util as au
import editlong_util as lu
import editops_util as ou
import numpy as np
import pytest


@pytest.mark.parametrize("name", au.CASES)
def test_the_twin_equals_the_references(name):
    sizes = []
    for x, y, xm, ym in au.pairs(name):
        got_x, got_y, counts, blocks, nbytes = au.host_pair(x, y, au.CASES[name])
        assert (got_x == xm).all() and (got_y == ym).all(), (len(x), len(y))
        assert counts == lu.host_pair(x, y, au.CASES[name], True) == ou.counts_from_maps(got_x, got_y, x, y, len(x), len(y))
        ou.check_maps(got_x, got_y, len(x), len(y))
        sizes.append((blocks, nbytes))
    # blocks: the corner's one cell, then one per band.  Bytes: 3 x 4098 | 4 x 6146 column keys, 4 x 3 x 2048 | 6 x 4 x 2048 row keys, 512 KiB
    assert name != "corners" or sizes == [(5, 819456), (7, 1114368)]


def test_sanitizer_driver_runs_clean(tmp_path):
    """The twin with its own main under ASan + UBSan over the first two case groups in both roles: the slot is a buffer of exactly its size."""
    files = []
    for name, (x, y, xm, ym) in ((n, p) for n in ("four symbols", "four symbols/swap", "corners") for p in au.pairs(n)):
        files.append(str(tmp_path / ("%d.bin" % len(files))))
        with open(files[-1], "wb") as f:
            f.write(b"".join(a.astype("<i4").tobytes() for a in (np.asarray([len(x), len(y), au.CASES[name]]), x, y, xm, ym)))
    exe = str(tmp_path / "editalign_long_host_main")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-DEDITALIGN_LONG_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", au.SRC, "-o", exe], check=True)
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "%d checks, 0 failures" % len(files) in r.stdout, r.stdout[-4000:]
