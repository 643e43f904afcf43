"""What the long-alignment tests share (ctcdecode_amd/csrc/editlong.h "Alignments"): the cases of the CPU and the GPU tests with their
references (``editops_util.align_ref`` up to 4400 tokens, closed forms beyond) and the twin of tests/native/editalign_long_host.cpp."""
import ctypes
import os
import subprocess

import editdist_util as eu
import editlong_util as lu
import editops_util as ou
import numpy as np

SRC = os.path.join(eu.NATIVE, "editalign_long_host.cpp")
# name -> waves.  Every case is a list of (x, y, x_to_y, y_to_x); "/swap" runs it with the rows exchanged (x the streamed row).
CASES = {"four symbols": 2, "four symbols/swap": 2, "corners": 2, "runs along a checkpoint": 4, "disjoint": 2, "disjoint/swap": 2, "beyond the packed key": 2}


def _ref(x, y):
    _, _, xm, ym = ou.align_ref(x, y)
    return x, y, np.asarray(xm, np.int32), np.asarray(ym, np.int32)


def _make(name):
    rng = np.random.default_rng(eu.hash_name("align long " + name))
    ident = lambda n: np.arange(n, dtype=np.int32)  # noqa: E731
    if name == "four symbols":  # many ties and S > 0: strips around the tile edge against streamed rows around the strip's length
        sizes = [(n, m) for n in (2049, 4096, 4097) for m in (n, n + 1, n + 200)] + [(2049, 3073)]
        return [_ref(*eu.related_rows(rng, n, m, 4)) for n, m in sizes]
    if name == "corners":  # equal rows: the identity, through cells (2048, 2048), (4096, 4096); 6145: a tile whose left edge crossed a round
        return [((ident(n) * 7 % 5).astype(np.int32),) * 2 + (ident(n),) * 2 for n in (4097, 6145)]
    if name == "runs along a checkpoint":  # 100 unpartnered tokens across column / row 2048 (cut at 2000) and row / column 1024 (cut at 1000)
        x = ident(4200) + 10
        cuts = [np.delete(x, np.arange(cut, cut + 100)) for cut in (2000, 1000)]
        return [_ref(*p) for y in cuts for p in ((x, y), (y, x))]
    if name == "disjoint":  # D = 12545, S = 6145 > 4095: x[lx - 1 - t] stands against y[ly - 1 - t], the first ly - lx of y against nothing
        lx, ly = 6145, 12545
        return [(rng.integers(0, 2, lx).astype(np.int32), rng.integers(2, 4, ly).astype(np.int32), ident(lx) + (ly - lx), np.maximum(ident(ly) - (ly - lx), -1))]
    ly = 262145  # "beyond the packed key": three tokens, the reference's last three
    y = rng.integers(0, 4, ly).astype(np.int32)
    return [(y[-3:].copy(), y, ident(3) + (ly - 3), np.maximum(ident(ly) - (ly - 3), -1))]


def pairs(name):
    base = eu.cached(("align long", name.split("/")[0]), lambda: _make(name.split("/")[0]))
    if name == "four symbols/swap":  # (insertions come before deletions: the walk is not its own mirror image)
        return eu.cached(("align long", name), lambda: [_ref(y, x) for x, y, _, _ in base])
    return [(y, x, ym, xm) for x, y, xm, ym in base] if name.endswith("/swap") else base


def mixed_case():
    """B = 2: item 0 has rows of 0 .. 4300 against references of 0 .. 4400 tokens, item 1 the same with a bad length.  -> dict(x, x_lens,
    y, y_lens, xm, ym, counts), the expectation as ``editops_util.reference`` states it; four of the pairs are long."""
    rng = np.random.default_rng(eu.hash_name("align long mixed"))
    src = rng.integers(0, 4, 4400).astype(np.int32)
    noisy = lambda lens: eu.pack_rows([np.where(rng.random(k) < 0.15, rng.integers(0, 4, k), src[:k]).astype(np.int32) for k in lens])  # noqa: E731
    (x, xl), (y, yl) = noisy((0, 300, 2049, 4300)), noisy((0, 2048, 2049, 4400))
    c = dict(x=np.stack([x, x]), x_lens=np.stack([xl, xl]), y=np.stack([y, y]), y_lens=np.stack([yl, yl]))
    c["x_lens"][1, 1] = 4301
    c["counts"], c["xm"], c["ym"], _ = ou.case_reference(c, maps=True)
    return c


def limits_case():  # the six long pairs of ``editlong_util.strip_case(2049)`` with their maps
    c = lu.strip_case(2049)
    return [_ref(c["x"][k, 0, :c["x_lens"][k, 0]], c["y"][k, 0, :c["y_lens"][k, 0]]) for k in range(len(c["dist"]))]


def host_pair(x, y, W):
    """The twin, built once a session.  -> (x_to_y, y_to_x, counts (H, S, Del, I), the blocks the walk swept again, the slot's bytes)"""
    def make():
        so = os.path.join(eu.ROOT, "oracle", "_build", "libctcedit_align_long_host.so")
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", SRC, "-o", "%s.%d.tmp" % (so, os.getpid())], check=True)
        os.replace("%s.%d.tmp" % (so, os.getpid()), so)
        return ctypes.CDLL(so)
    x, y = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(y, np.int32)
    xm, ym, out = np.full(len(x), eu.SENTINEL, np.int32), np.full(len(y), eu.SENTINEL, np.int32), np.zeros(6, np.int32)
    eu.cached("align long lib", make).ctcedit_align_long_host_pair(eu._ptr(x), len(x), eu._ptr(y), len(y), W, eu._ptr(xm), eu._ptr(ym), eu._ptr(out))
    return xm, ym, tuple(int(v) for v in out[:4]), int(out[4]), int(out[5])
