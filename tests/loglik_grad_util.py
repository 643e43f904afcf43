"""What tests/test_gpu_loglik_grad.py needs: a plain numpy CTC forward-backward in log space (``dtype``: the precision it runs in), the
gradient it gives for weighted rows, and builders of transcript-like inputs -- the row's own alignment made likely, so that the
reference is well conditioned (``python tests/loglik_grad_util.py`` checks that and measures the tolerances below on the CPU)."""
import functools

import numpy as np

BAD_ROW = 8  # CTCD_ALIGN_BAD_ROW

# The greatest |float32 run - float64 run| of THIS FILE's reference on exactly the test inputs, per case family, measured on the CPU
# by `python tests/loglik_grad_util.py` (profiles/loglik_grad.json keeps the figures).  The device gets eight times that: its float32
# log-sum-exp orders its operations differently from numpy's and is not expected to be less accurate.
MEASURED = {"rows_V5": 2.8610e-05, "rows_V300": 2.0862e-05, "mixed": 4.0771e-05, "edges": 3.8586e-06,
            "modes_logp": 6.2704e-06, "modes_prob": 5.6131e-03, "modes_logits": 3.5769e-06}
BOUND = {k: 8.0 * v for k, v in MEASURED.items()}


def lse(xs, dtype):
    m = np.maximum.reduce(xs)
    ms = np.where(np.isfinite(m), m, 0).astype(dtype)
    with np.errstate(divide="ignore"):
        return (ms + np.log(sum(np.exp(x - ms) for x in xs))).astype(dtype)


def forward_backward(lp, y, blank, dtype=np.float64):
    """lp [n, V] log-probabilities, y the labels.  -> (ll, G [n, V]): the log-likelihood and its derivative to lp, in ``dtype``;
    (-inf, zeros) if no alignment fits."""
    lp = np.asarray(lp, dtype)
    n, L = lp.shape[0], len(y)
    S, ninf = 2 * L + 1, dtype(-np.inf)
    G = np.zeros(lp.shape, dtype)
    if n == 0 or L > n:
        return (dtype(0) if n == 0 and L == 0 else ninf), G
    z = np.full(S, blank)
    z[1::2] = y
    skip = np.zeros(S, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    e = lp[:, z]

    def shift(v, k):
        return np.concatenate([np.full(k, ninf, dtype), v[:-k]]) if k < len(v) else np.full(len(v), ninf, dtype)

    a = np.full((n, S), ninf, dtype)
    a[0, :2] = e[0, :2]
    for t in range(1, n):
        a[t] = e[t] + lse([a[t - 1], shift(a[t - 1], 1), np.where(skip, shift(a[t - 1], 2), ninf)], dtype)
    b = np.full((n, S), ninf, dtype)
    b[n - 1, -2:] = e[n - 1, -2:]
    skip2 = np.concatenate([skip[2:], [False, False]])[:S]  # (state s may move on to s + 2 where s + 2 may be entered from s)
    for t in range(n - 2, -1, -1):
        r = b[t + 1][::-1]  # (the shifts are towards higher states: done on the reversed row)
        b[t] = e[t] + lse([b[t + 1], shift(r, 1)[::-1], np.where(skip2, shift(r, 2)[::-1], ninf)], dtype)
    ll = lse([a[n - 1, S - 1], a[n - 1, S - 2] if L else ninf], dtype)
    if not np.isfinite(ll):
        return ninf, G
    with np.errstate(invalid="ignore"):
        x = (a + b) - e - ll
    g = np.where(np.isfinite(x), np.exp(np.where(np.isfinite(x), x, 0)), 0).astype(dtype)
    np.add.at(G.T, z, g.T)
    return ll, G


def row_ok(y, length, L_stride, V, blank):
    return 0 <= length <= L_stride and all(0 <= c < V and c != blank for c in y[:max(length, 0)])


def reference(lp, seq_lens, tokens, lens, weights, blank, dtype=np.float64):
    """-> dict(grad [B, T, V], loglik [B, R], weight_sum [B]: the weights of the rows that contribute, status [B])."""
    B, T, V = lp.shape
    R, Ls = tokens.shape[1:]
    out = dict(grad=np.zeros((B, T, V), dtype), loglik=np.zeros((B, R), dtype), weight_sum=np.zeros(B), status=np.zeros(B, np.int32))
    for b in range(B):
        n = T if seq_lens is None else int(min(max(seq_lens[b], 0), T))
        for r in range(R):
            if not row_ok(tokens[b, r], lens[b, r], Ls, V, blank):
                out["status"][b] = BAD_ROW
                continue
            ll, G = forward_backward(lp[b, :n], tokens[b, r, :lens[b, r]], blank, dtype)
            out["loglik"][b, r] = ll
            if np.isfinite(ll) and n > 0:
                out["grad"][b, :n] += dtype(weights[b, r]) * G
                out["weight_sum"][b] += weights[b, r]
    return out


def mode_gradient(x, mode, seq_lens, tokens, lens, weights, blank, dtype=np.float64):
    """d sum_r w ll / d x for the input x of a decoder in ``mode`` ("logp", "prob", "logits"), everything in ``dtype``."""
    x = np.asarray(x, dtype)
    if mode == "logits":
        m = x.max(-1, keepdims=True)
        lp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(dtype)
    else:
        with np.errstate(divide="ignore"):
            lp = np.log(x).astype(dtype) if mode == "prob" else x
    ref = reference(lp, seq_lens, tokens, lens, weights, blank, dtype)
    g = ref["grad"]
    if mode == "logits":
        g = g - np.exp(lp) * g.sum(-1, keepdims=True)
    elif mode == "prob":
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(g != 0, g / x, 0)
    return dict(ref, grad=g.astype(dtype))


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def _labels(rng, L, V, blank, room):
    """L labels; at most ``room`` of them repeat their neighbour (each such pair needs a frame for its separating blank)."""
    others = [c for c in range(V) if c != blank]
    y = []
    for i in range(L):
        c = others[rng.integers(len(others))]
        if y and c == y[-1]:
            if room > 0:
                room -= 1
            else:
                c = others[(others.index(c) + 1 + rng.integers(len(others) - 1)) % len(others)]
        y.append(c)
    return y


def _alignment(rng, y, n, blank):
    """One alignment of y over n frames: a frame per label, the separating blanks, the other frames as blanks and as a second frame
    of a label (no more: rows 1 and 2 of a case lose a label's frames, and their log-likelihood is to stay far above -80)."""
    units = []
    for i, c in enumerate(y):
        units.append(([blank] if i and c == y[i - 1] else []) + [c])
    units.append([])
    for _ in range(n - sum(len(u) for u in units)):
        k = rng.integers(len(units))
        if units[k] and units[k].count(units[k][-1]) == 1 and rng.integers(2):
            units[k].append(units[k][-1])
        else:
            units[k].insert(0, blank)
    return [c for u in units for c in u]


def transcript_case(seed, T, V, Ls, R, seq_lens=None, blank=0, bonus=6.0):
    """Items with rows of Ls[b] labels over seq_lens[b] (default T) frames: logits = noise + ``bonus`` + log V (the alignment as likely
    at every vocabulary) on an alignment of row 0; row 1 substitutes one label of row 0, row 2 drops its last.
    -> dict(x: the logits, float64; tokens, lens, seq_lens, blank)."""
    rng = np.random.default_rng(seed)
    bonus = bonus + np.log(V)
    B = len(Ls)
    ns = [T] * B if seq_lens is None else list(seq_lens)
    x = rng.normal(0.0, 1.0, (B, T, V))
    tokens, lens = np.zeros((B, R, max(max(Ls), 1)), np.int32), np.zeros((B, R), np.int32)
    for b, (L, n) in enumerate(zip(Ls, ns)):
        y = _labels(rng, L, V, blank, min(4, (n - L) // 2))
        path = _alignment(rng, y, n, blank)
        if len(path) == n:  # (an item too short for its row gets no alignment)
            x[b, np.arange(n), path] += bonus
        rows = [y, list(y), y[:-1]]
        if L:
            i = int(rng.integers(L))
            near = {blank, y[i]} | {y[j] for j in (i - 1, i + 1) if 0 <= j < L}
            rows[1][i] = next(c for c in range(V) if c not in near)
        for r in range(R):
            lens[b, r] = len(rows[r])
            tokens[b, r, :len(rows[r])] = rows[r]
    return dict(x=x, tokens=tokens, lens=lens, seq_lens=np.asarray(ns, np.int32), blank=blank)


def log_softmax32(x):
    m = x.max(-1, keepdims=True)
    return (x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))).astype(np.float32)


WEIGHTS = (1.5, -2.0, 0.0)
ROW_LS = (31, 32, 127, 128, 511, 512)  # S = 63, 65, 255, 257, 1023, 1025
MIXED_LS = (31, 20, 5, 31, 32, 127, 511, 512)  # a group of four one-wave rows, then one row of each other class


@functools.lru_cache(maxsize=None)
def rows_case(L, V, R):
    """Two items of L and L - 3 labels in L + 8 and L + 2 frames, log-probabilities in float32, and the float64 reference."""
    c = transcript_case(1000 * L + V + R, L + 8, V, (L, L - 3), R, seq_lens=(L + 8, L + 2))
    return _with_reference(c, R)


@functools.lru_cache(maxsize=None)
def mixed_case():
    c = transcript_case(77, 520, 300, MIXED_LS, 3, seq_lens=(40, 520, 9, 33, 41, 140, 520, 517))
    return _with_reference(c, 3)


def _with_reference(c, R):
    c["lp"] = log_softmax32(c["x"])
    c["weights"] = np.tile(np.asarray(WEIGHTS[:R], np.float32), (len(c["lens"]), 1))
    c["ref"] = reference(c["lp"].astype(np.float64), c["seq_lens"], c["tokens"], c["lens"], c["weights"], c["blank"])
    return c


@functools.lru_cache(maxsize=None)
def edges_case():
    """Item by item: no frames; one frame; a row longer than its item; an empty row; a repeated label; a whole frame of -inf; and
    in row 1 of every item an ordinary transcript.  V = 6, T = 12, blank = 2."""
    T, V, blank = 12, 6, 2
    c = transcript_case(5, T, V, (3, 1, 3, 3, 3, 3), 2, seq_lens=(0, 1, 3, 12, 12, 12), blank=blank, bonus=3.0)
    tok, lens = c["tokens"], c["lens"]
    tok[:, 1], lens[:, 1] = tok[:, 0], lens[:, 0]  # (row 0 of each item is overwritten below; its transcript stays as row 1)
    tok = np.concatenate([tok, np.zeros((6, 2, 2), np.int32)], axis=2)
    tok[2, 0, :5], lens[2, 0] = (0, 1, 3, 4, 5), 5
    lens[3, 0] = 0
    tok[4, 0, :3], lens[4, 0] = (4, 4, 1), 3
    c["tokens"], c["lp"] = tok, log_softmax32(c["x"])
    c["lp"][5, 4, :] = -np.inf
    c["weights"] = np.tile(np.asarray((1.0, 0.5), np.float32), (6, 1))
    c["ref"] = reference(c["lp"].astype(np.float64), c["seq_lens"], tok, lens, c["weights"], blank)
    return c


@functools.lru_cache(maxsize=None)
def modes_case():
    """B = 3, T = 40, L <= 12, V = 29, two rows per item: the logits (float64); the tests round them to the element type."""
    return transcript_case(9, 40, 29, (12, 7, 1), 2, seq_lens=(40, 31, 40), bonus=4.0)


def mode_input(x64, mode, np_round):
    """The tensor a decoder in ``mode`` is given, rounded to the element type by ``np_round`` (float64 -> float64 values of that
    type): the logits, their softmax or their log-softmax."""
    lp = x64 - (x64.max(-1, keepdims=True) + np.log(np.exp(x64 - x64.max(-1, keepdims=True)).sum(-1, keepdims=True)))
    return np_round({"logits": x64, "prob": np.exp(lp), "logp": lp}[mode])


def _measure():
    """The float32 reference against the float64 one on every test input, per family; and the conditioning check: every finite
    log-likelihood, and with it every a and b on an alignment that counts, stays far inside (-80, 0], where e80 does not cut."""
    import json
    import torch

    def dev(c, **kw):
        r32 = reference(c["lp"], c["seq_lens"], c["tokens"], c["lens"], c["weights"], c["blank"], np.float32)
        assert np.all(np.abs(c["ref"]["loglik"][np.isfinite(c["ref"]["loglik"])]) < 80.0), "a log-likelihood near the float32 exp range"
        return float(np.abs(r32["grad"].astype(np.float64) - c["ref"]["grad"]).max())

    out = {k: 0.0 for k in MEASURED}
    for L in ROW_LS:
        for V in (5, 300):
            for R in (1, 3):
                out["rows_V%d" % V] = max(out["rows_V%d" % V], dev(rows_case(L, V, R)))
    out["mixed"], out["edges"] = dev(mixed_case()), dev(edges_case())
    c = modes_case()
    ones = np.ones(c["lens"].shape, np.float32)
    for mode in ("logp", "prob", "logits"):
        for dt in (torch.float32, torch.float16, torch.bfloat16):
            x = mode_input(c["x"], mode, lambda v: torch.from_numpy(v).to(dt).double().numpy())
            r64 = mode_gradient(x, mode, c["seq_lens"], c["tokens"], c["lens"], ones, c["blank"])
            r32 = mode_gradient(x.astype(np.float32), mode, c["seq_lens"], c["tokens"], c["lens"], ones, c["blank"], np.float32)
            out["modes_" + mode] = max(out["modes_" + mode], float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max()))
    print(json.dumps({"measured_f32_vs_f64": out, "bound_x8": {k: 8 * v for k, v in out.items()}}, indent=1))


if __name__ == "__main__":
    _measure()
